// The depth carve's arithmetic of one (voxel, view) pair -- the section "carve from depth images" of vacancy_hip.h, steps
// 1 to 7 -- in ONE function, dp::add_view, compiled for the kernel (carve_depth.hip) and for the serial host function
// (carve_depth_host.hip).  Projection, ROI test and nearest pixel are view_distance<> of carve_common.h term for term, the
// update is fuse<> of the same header; the library's flags (no FMA contraction, correctly rounded division, denormals kept)
// make host and device agree to the bit.
#pragma once

#include <cmath>
#include <cstdint>

#include "vacancy_hip.h"

#if defined(__HIPCC__)
#define VCY_DP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define VCY_DP_FN inline
#endif

namespace vcy {
namespace dp {

constexpr int kMaxViewsPerLaunch = 64;

struct View {  // one per view of a launch, in device memory (the host function: one per view of the call)
  float r[3][3], t[3];  // w2c
  float fx, fy, cx, cy;
  float rx0f, ry0f, rx1f, ry1f;  // (float)int, as the carve compares
  int rx0, ry0, rx1, ry1;
  int width, ortho;
  const float* depth;
};

inline void fill_view(const vcy_view& in, const float* depth, View* v) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) v->r[i][j] = in.w2c[4 * i + j];
    v->t[i] = in.w2c[4 * i + 3];
  }
  v->fx = in.fx, v->fy = in.fy, v->cx = in.cx, v->cy = in.cy;
  v->rx0 = in.roi_min[0], v->ry0 = in.roi_min[1], v->rx1 = in.roi_max[0], v->ry1 = in.roi_max[1];
  v->rx0f = (float)in.roi_min[0], v->ry0f = (float)in.roi_min[1];
  v->rx1f = (float)in.roi_max[0], v->ry1f = (float)in.roi_max[1];
  v->width = in.width;
  v->ortho = in.is_ortho ? 1 : 0;
  v->depth = depth;
}

// band finite and > 0 with a finite reciprocal (written so that a NaN fails)
inline bool band_ok(float band) { return band > 0.0f && std::isfinite(band) && std::isfinite(1.0f / band); }

VCY_DP_FN int imax(int a, int b) { return a > b ? a : b; }
VCY_DP_FN int imin(int a, int b) { return a < b ? a : b; }

// The one tap.  On the device the pointer comes out of a view record in memory, so the compiler cannot know its address
// space and would emit a flat load; the images are device allocations, and saying so gives a global load.
VCY_DP_FN float depth_tap(const float* depth, int64_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ((const __attribute__((address_space(1))) float*)depth)[at];
#else
  return depth[at];
#endif
}

// Steps 1 - 7 for one view on the running state (sdf, n) of the voxel at (px, py, pz).  True when the state changed.
template <int UPDATE>
VCY_DP_FN bool add_view(const View& v, float px, float py, float pz, float inv_band, int max_update_num, float weight,
                        float& sdf, int& n) {
  if (n > max_update_num) return false;  // 1. voxel_carver.cc:447-450, on the running count
  float pc[3];                           // 2.
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float c0 = v.r[i][0] * px;
    const float c1 = v.r[i][1] * py;
    const float c2 = v.r[i][2] * pz;
    pc[i] = v.t[i] + (c0 + (c1 + c2));
  }
  if (pc[2] < 0.0f) return false;
  float u, w;
  if (v.ortho) {
    u = pc[0];
    w = pc[1];
  } else {
    u = v.fx / pc[2] * pc[0] + v.cx;
    w = v.fy / pc[2] * pc[1] + v.cy;
  }
  const bool inside = u >= v.rx0f && w >= v.ry0f && u <= v.rx1f && w <= v.ry1f;  // 3. (NaN: outside)
  if (!inside) return false;
  int xi = (int)roundf(u);  // 4.
  int yi = (int)roundf(w);
  xi = imax(xi, v.rx0);
  yi = imax(yi, v.ry0);
  xi = imin(xi, v.rx1);
  yi = imin(yi, v.ry1);
  const float z = depth_tap(v.depth, (int64_t)v.width * yi + xi);
  if (!(z > 0.0f)) return false;  // 5. (NaN, 0, negative: no measurement; +inf passes)
  const float e = z - pc[2];      // 6.
  float d = e * inv_band;
  if (d > 1.0f) d = 1.0f;
  if (!(d >= -1.0f)) return false;  // (NaN; more than one band behind the surface: occluded)
  if (n < 1) {                      // 7. first touch, voxel_carver.cc:482-486
    sdf = d;
    n = 1;
    return true;
  }
  if (UPDATE == VCY_UPDATE_MAX) {  // UpdateVoxelMax, :78-86
    if (d > sdf) {
      sdf = d;
      n = n + 1;
      return true;
    }
    return false;
  }
  // UpdateVoxelWeightedAverage, :88-95
  const float inv_denom = 1.0f / (weight * (float)(n + 1));
  sdf = (weight * (float)n * sdf + weight * d) * inv_denom;
  n = n + 1;
  return true;
}

}  // namespace dp
}  // namespace vcy
