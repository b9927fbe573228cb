// What a launch of rs_raster_kernel (raster.hip) is given, for the two drivers that fill key images with it: the rasteriser's
// own (raster.hip) and the shading pass behind it (raster_shade.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "raster_fragment.h"

namespace vcy {
namespace rs {

typedef unsigned long long u64;

struct Target {  // one per view of a launch, in device memory, beside its View
  u64* keys;
  float* depth;         // any of the three outputs may be null
  int32_t* face;
  u64* hits;
  const uint8_t* mask;  // null unless the agreement is counted
};

struct Launch {
  int64_t n_faces;
  const float* vtx;
  const int32_t* faces;
  const View* views;
  const Target* targets;
  int n_views;
  long long wide;   // "rasterwide"
  u64* dropped;     // 2 per view
  u64* counts;      // 3 per view (agreement)
};

// rs_raster_kernel over the faces of L on `stream` (no launch for a mesh without faces); the key images are filled by the
// caller.  raster.hip
hipError_t launch_raster(const Launch& L, hipStream_t stream);

}  // namespace rs
}  // namespace vcy
