// The three host rules a grid cut into z-slabs shares between its front ends, stated once: the plan and the tie rule of
// the closing (vcy_close_hull_plan), which components stay (vcy_select_components_host, vcy_keep_components) and which
// planes a slab's z pass gets from its neighbours (vcy_distance_halo_host).  Plain functions on plain arguments: no HIP,
// no context, no error text, nothing kept -- the C-ABI entries (distance_host.hip, components.hip) are wrappers that add
// the argument checks' words.  tests/slab_rules_host_check.cpp states what each rule gives, also under host sanitizers.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "vacancy_hip.h"  // vcy_component

namespace vcy {
namespace slab {

// ---- the closing (vacancy_hip.h, "Closing the hull") ---------------------------------------------------------------------
enum ClosePlan { kCloseOk = 0, kCloseOutOfRange, kCloseTies };

// r = radius_voxels * resolution in world units and the transform's radius R = ceil(radius_voxels) + 2, for
// 0 < radius_voxels and R <= 127.  kCloseTies, with *tie_square = (radius_voxels + 0.5)^2, when that is an integer that is
// a sum of three squares: voxels then sit exactly on the thresholds of the growing and of the shrinking step.
inline ClosePlan close_hull_plan(double radius_voxels, float resolution, double* r, int* big_r, long long* tie_square) {
  const double rv = radius_voxels;
  if (!(rv > 0.0) || rv > 125.0) return kCloseOutOfRange;  // (R > 127, asked before the conversion: a NaN has no R)
  const double t = (rv + 0.5) * (rv + 0.5);
  const double nearest = std::floor(t + 0.5);
  if (std::fabs(t - nearest) <= 1e-9 * t) {
    long long m = static_cast<long long>(nearest);
    while (m % 4 == 0) m /= 4;
    if (m % 8 != 7) {  // Legendre: a sum of three squares, so a squared voxel distance
      *tie_square = static_cast<long long>(nearest);
      return kCloseTies;
    }
  }
  *r = rv * static_cast<double>(resolution);
  *big_r = static_cast<int>(std::ceil(rv)) + 2;
  return kCloseOk;
}

// ---- which components stay (vacancy_hip.h, vcy_keep_components) ----------------------------------------------------------
// `comps` in the order of vcy_label_components.  removed[i] = 1 unless (keep_largest <= 0 or i < keep_largest) and
// n_voxels >= min_voxels; the counts of what went.
inline void select_components(const vcy_component* comps, int64_t n, int keep_largest, int64_t min_voxels, uint8_t* removed,
                              int64_t* n_removed, int64_t* voxels_removed) {
  *n_removed = *voxels_removed = 0;
  for (int64_t i = 0; i < n; ++i) {
    const bool keep = (keep_largest <= 0 || i < (int64_t)keep_largest) && comps[i].n_voxels >= min_voxels;
    removed[i] = keep ? 0 : 1;
    if (!keep) ++*n_removed, *voxels_removed += comps[i].n_voxels;
  }
}

// ... and the slabs' pieces that go with them: piece_removed[k] = 1 iff piece_global[k], the merged label of piece k
// (vcy_merge_components_host), is the label of a removed component.  (One transient list of the removed labels.)
inline void select_pieces(const vcy_component* comps, int64_t n, const uint8_t* removed, const int64_t* piece_global,
                          int64_t n_pieces, uint8_t* piece_removed) {
  std::vector<int64_t> gone;  // merged labels, ascending
  for (int64_t i = 0; i < n; ++i)
    if (removed[i]) gone.push_back(comps[i].label);
  std::sort(gone.begin(), gone.end());
  for (int64_t k = 0; k < n_pieces; ++k) piece_removed[k] = std::binary_search(gone.begin(), gone.end(), piece_global[k]) ? 1 : 0;
}

// ---- the seam planes of the distance field (vacancy_hip.h, the z-slab form, step 2) --------------------------------------
enum Halo { kHaloOk = 0, kHaloBadArgument, kHaloBadBounds, kHaloBadSlab, kHaloMissingEdge };

// The slabs [bounds[s], bounds[s + 1]) of a grid of nz = bounds[n_slabs] slices; bottoms[s] / tops[s]: the lowest / highest
// min(radius, own slices) planes of slab s, `plane` uint16 each, in ascending z.  For slab [z0, z1): the planes of the
// global slices [z0 - *n_below, z0) into `below` and [z1, z1 + *n_above) into `above`, *n_below = min(radius, z0),
// *n_above = min(radius, nz - z1), from as many neighbours as that takes -- a slab thinner than the radius passes its
// neighbours' planes on.  A pointer nobody reads may be null: a buffer whose count is 0, the edges of a slab out of reach.
inline Halo distance_halo(int n_slabs, const int32_t* bounds, int radius, size_t plane, const uint16_t* const* bottoms,
                          const uint16_t* const* tops, int slab, uint16_t* below, uint16_t* above, int* n_below, int* n_above) {
  if (n_slabs < 1 || !bounds || radius < 1 || plane < 1 || !n_below || !n_above) return kHaloBadArgument;
  if (bounds[0] != 0) return kHaloBadBounds;
  for (int s = 0; s < n_slabs; ++s)
    if (bounds[s + 1] <= bounds[s]) return kHaloBadBounds;
  if (slab < 0 || slab >= n_slabs) return kHaloBadSlab;
  const int nz = bounds[n_slabs], z0 = bounds[slab], z1 = bounds[slab + 1];
  *n_below = std::min(radius, z0), *n_above = std::min(radius, nz - z1);
  if ((*n_below && !below) || (*n_above && !above)) return kHaloBadArgument;
  auto edge = [&](int s) { return std::min(radius, bounds[s + 1] - bounds[s]); };
  // the plane of the global slice z, which lies below (from the owner's top planes) or above (bottom planes) the asker
  auto plane_of = [&](int z, bool from_top) -> const uint16_t* {
    const int j = static_cast<int>(std::upper_bound(bounds, bounds + n_slabs + 1, z) - bounds) - 1;
    const uint16_t* const* edges = from_top ? tops : bottoms;
    if (!edges || !edges[j]) return nullptr;
    return edges[j] + plane * static_cast<size_t>(from_top ? z - (bounds[j + 1] - edge(j)) : z - bounds[j]);
  };
  for (int k = 0; k < *n_below; ++k) {
    const uint16_t* p = plane_of(z0 - *n_below + k, true);
    if (!p) return kHaloMissingEdge;
    std::memcpy(below + plane * k, p, plane * sizeof(uint16_t));
  }
  for (int k = 0; k < *n_above; ++k) {
    const uint16_t* p = plane_of(z1 + k, false);
    if (!p) return kHaloMissingEdge;
    std::memcpy(above + plane * k, p, plane * sizeof(uint16_t));
  }
  return kHaloOk;
}

}  // namespace slab
}  // namespace vcy
