// What the device path (distance.hip) and the serial host function (distance_host.hip) of the section "distance field of
// the hull" of vacancy_hip.h share: the cap, the argument check and the ONE place the metric value is computed.  Host code
// only: the kernel does not evaluate phi, it looks it up in the table phi_table() built here and uploaded, so the float
// bits of the two paths cannot differ.  Every user is built with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "host_shared.h"

namespace vcy {
namespace df {

constexpr int kMaxRadius = 127;  // the row distance fits 7 bits, 2 * 127^2 + 1 fits 15

inline int far_of(int radius) { return radius * radius + 1; }

// phi of a capped squared distance d2c in [0, R*R] (exact as a float): one rounding per operation
inline float phi_of(int d2c, float resolution) {
  const float root = sqrtf((float)d2c);
  const float shifted = root - 0.5f;
  return shifted * resolution;
}

// phi_of for every d2c in [0, R*R]; a field value (1 .. FAR) is looked up at min(d2, R*R)
inline std::vector<float> phi_table(int radius, float resolution) {
  std::vector<float> t((size_t)radius * radius + 1);
  for (int i = 0; i <= radius * radius; ++i) t[(size_t)i] = phi_of(i, resolution);
  return t;
}

inline int check_radius(const char* who, int radius) {
  if (radius >= 1 && radius <= kMaxRadius) return VCY_OK;
  set_error("%s: radius %d is outside [1, %d]", who, radius, kMaxRadius);
  return VCY_ERR_INVALID_ARG;
}

// The planes of its neighbours a slab [z_begin, z_end) of nz slices needs at either end: min(R, what the grid has there)
inline int halo_below(int radius, int z_begin) { return radius < z_begin ? radius : z_begin; }
inline int halo_above(int radius, int z_end, int nz) { return radius < nz - z_end ? radius : nz - z_end; }

// ... and the finishing calls' check of what they were handed
inline int check_halo(const char* who, int radius, int z_begin, int z_end, int nz, int n_below, int n_above, const void* below,
                      const void* above) {
  const int want_below = halo_below(radius, z_begin), want_above = halo_above(radius, z_end, nz);
  if (n_below != want_below || n_above != want_above) {
    set_error("%s: %d planes below and %d above; the slab [%d, %d) of %d slices needs %d and %d at radius %d", who, n_below,
              n_above, z_begin, z_end, nz, want_below, want_above, radius);
    return VCY_ERR_INVALID_ARG;
  }
  if ((n_below > 0 && !below) || (n_above > 0 && !above)) {
    set_error("%s: null pointer", who);
    return VCY_ERR_INVALID_ARG;
  }
  return VCY_OK;
}

}  // namespace df
}  // namespace vcy
