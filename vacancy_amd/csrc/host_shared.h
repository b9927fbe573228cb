// Host arithmetic and argument checks that need neither a context nor the HIP runtime, shared by the translation units
// with device code and the ones without (carve_depth_host.hip, which a stand-alone program compiles under host sanitizers).
// Every user is built with -ffp-contract=off.
#pragma once

#include <cstdint>
#include <limits>

#include "vacancy_hip.h"

namespace vcy {

void set_error(const char* fmt, ...);

// Voxel::pos along one axis, reference voxel_carver.cc:308-326:
//   pos = diff * ((float)i / (float)n) + bb_min + resolution * 0.5f   (left to right)
// Host IEEE arithmetic.  The ONE place the expression lives: the device's axis tables (vcy_create), vcy_axis_positions and
// through it the C++ facade's VoxelGrid, and vcy_carve_depth_host come from here.
inline void axis_positions(float bb_min, float bb_max, float resolution, int n, float* out) {
  const float offset = resolution * 0.5f;
  const float diff = bb_max - bb_min;
  for (int i = 0; i < n; ++i) out[i] = diff * (static_cast<float>(i) / static_cast<float>(n)) + bb_min + offset;
}

inline int dims_from_option(const float bb_min[3], const float bb_max[3], float res, int32_t n[3], bool allow_empty = false) {
  // VoxelGrid::Init, reference voxel_carver.cc:278-301
  if (res < std::numeric_limits<float>::min()) {
    set_error("resolution must be positive %f", res);
    return VCY_ERR_INVALID_ARG;
  }
  if (bb_max[0] <= bb_min[0] || bb_max[1] <= bb_min[1] || bb_max[2] <= bb_min[2]) {
    set_error("input bounding box is invalid");
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = 0; i < 3; ++i) {
    const float diff = bb_max[i] - bb_min[i];
    n[i] = static_cast<int>(diff / res);
  }
  if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0) {
    // The reference accepts a box thinner than one voxel and builds an EMPTY grid (voxel_carver.cc:292-345: the
    // loops do not run, Init returns true); the host container does the same (vcy_compute_dims, VoxelGrid::Init).
    // A device context over no voxels is refused (vcy_create).
    if (allow_empty) return VCY_OK;
    set_error("grid has an empty axis (%d,%d,%d)", n[0], n[1], n[2]);
    return VCY_ERR_INVALID_ARG;
  }
  // The reference refuses more than INT_MAX voxels (32-bit ids, voxel_carver.cc:298-301).
  // Device indices are 64-bit; a single xy slice must still fit 31 bits.
  if ((int64_t)n[0] * n[1] > std::numeric_limits<int>::max()) {
    set_error("too many voxels in one xy slice");
    return VCY_ERR_TOO_MANY_VOXELS;
  }
  return VCY_OK;
}

// The size of an indexed mesh the mesh operators take: vertex ids and corner ids 3 f + j are 32 bits wide in their tables.
// The ONE place the bound lives: vcy_smooth_mesh[_host], vcy_decimate_mesh[_quadric][_host] (their argument checks), the
// extraction chain for the mesh it has just extracted (mesh_chain.hip), and vcy_mesh_index_limits.
inline int mesh_index_limits(const char* who, int64_t n_vertices, int64_t n_faces) {
  constexpr int64_t kMax = std::numeric_limits<int32_t>::max();
  if (n_faces > (kMax - 2) / 3 || n_vertices > kMax) {
    set_error("%s: %lld vertices, %lld faces: corner and vertex ids are 32 bits wide", who, (long long)n_vertices, (long long)n_faces);
    return VCY_ERR_UNSUPPORTED;
  }
  return VCY_OK;
}

// The part of a carve view's checks that needs no context: image size and ROI.
inline int check_view_static(const vcy_view* v) {
  if (!v || v->width <= 0 || v->height <= 0) {
    set_error("invalid view");
    return VCY_ERR_INVALID_ARG;
  }
  // The reference indexes sdf.at() unchecked (assert only); a ROI outside the image is
  // undefined there and rejected here.
  if (v->roi_min[0] < 0 || v->roi_min[1] < 0 || v->roi_max[0] >= v->width ||
      v->roi_max[1] >= v->height || v->roi_min[0] > v->roi_max[0] || v->roi_min[1] > v->roi_max[1]) {
    set_error("ROI [%d,%d]-[%d,%d] outside the %dx%d SDF image", v->roi_min[0], v->roi_min[1],
              v->roi_max[0], v->roi_max[1], v->width, v->height);
    return VCY_ERR_INVALID_ARG;
  }
  return VCY_OK;
}

}  // namespace vcy
