// Internal to libvacancy.so: what the facade's classes hand to the C ABI (include/vacancy_hip.h) -- a Camera with its
// ROI as a vcy_view, a VoxelCarverOption as a vcy_carver_option.  One statement for VoxelCarver and ShardedVoxelCarver.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

#include "vacancy/voxel_carver.h"
#include "vacancy_hip.h"

namespace vacancy {
namespace detail {

inline vcy_view ToView(const Camera& camera, const Eigen::Vector2i& roi_min, const Eigen::Vector2i& roi_max, int width,
                       int height, bool* ok) {
  vcy_view v;
  std::memset(&v, 0, sizeof(v));
  const Eigen::Affine3f w2c = camera.w2c().cast<float>();  // reference voxel_carver.cc:438
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) v.w2c[4 * i + j] = w2c.linear()(i, j);
    v.w2c[4 * i + 3] = w2c.translation()[i];
  }
  // Camera::Project is virtual in the reference (camera.h:39-40, called at voxel_carver.cc:460); the device knows the
  // two projections the reference implements.  Anything else is refused, never projected with fx = fy = 0.
  if (const PinholeCamera* p = dynamic_cast<const PinholeCamera*>(&camera)) {
    v.fx = p->focal_length()[0];
    v.fy = p->focal_length()[1];
    v.cx = p->principal_point()[0];
    v.cy = p->principal_point()[1];
  } else if (dynamic_cast<const OrthoCamera*>(&camera)) {
    v.is_ortho = 1;
  } else {
    *ok = false;
    LOGE("VoxelCarver::Carve unsupported Camera subclass: the HIP path projects PinholeCamera and OrthoCamera only\n");
  }
  v.roi_min[0] = roi_min[0];
  v.roi_min[1] = roi_min[1];
  v.roi_max[0] = roi_max[0];
  v.roi_max[1] = roi_max[1];
  v.width = width;
  v.height = height;
  return v;
}

// the whole image as the ROI
inline vcy_view ToView(const Camera& camera, int width, int height, bool* ok) {
  return ToView(camera, Eigen::Vector2i(0, 0), Eigen::Vector2i(width - 1, height - 1), width, height, ok);
}

inline vcy_carver_option ToC(const VoxelCarverOption& o) {
  vcy_carver_option c;
  std::memset(&c, 0, sizeof(c));
  for (int i = 0; i < 3; ++i) {
    c.bb_max[i] = o.bb_max[i];
    c.bb_min[i] = o.bb_min[i];
  }
  c.resolution = o.resolution;
  c.sdf_minmax_normalize = o.sdf_minmax_normalize ? 1 : 0;
  c.update_option.voxel_update = static_cast<int>(o.update_option.voxel_update);
  c.update_option.sdf_interp = static_cast<int>(o.update_option.sdf_interp);
  c.update_option.update_outside = static_cast<int>(o.update_option.update_outside);
  c.update_option.voxel_max_update_num = o.update_option.voxel_max_update_num;
  c.update_option.voxel_update_weight = o.update_option.voxel_update_weight;
  c.update_option.use_truncation = o.update_option.use_truncation ? 1 : 0;
  c.update_option.truncation_band = o.update_option.truncation_band;
  return c;
}

// CloseHull of both carvers: the plan and the tie rule are the library's (vcy_close_hull_plan; vacancy_hip.h, "Closing
// the hull"), then step(level, R) for the metric field, the field of the hull grown by r, the field of that shrunk by r.
// `step` answers false with *error set.  false with *error set when the radius is refused -- before any step has run --
// or a step fails.
template <typename Step>
inline bool CloseHullSteps(float radius_voxels, double iso_level, float resolution, std::string* error, Step step) {
  double r = 0.0;
  int big_r = 0;
  if (vcy_close_hull_plan(static_cast<double>(radius_voxels), resolution, &r, &big_r) != VCY_OK) {
    *error = vcy_last_error();
    return false;
  }
  const double iso[3] = {iso_level, r, -r};
  for (double level : iso)
    if (!step(level, big_r)) return false;
  return true;
}

// ... on one context that owns the whole grid
inline bool CloseHullOn(vcy_ctx* ctx, float radius_voxels, double iso_level, float resolution, std::string* error) {
  return CloseHullSteps(radius_voxels, iso_level, resolution, error, [ctx, error](double level, int big_r) {
    std::int64_t n = 0;
    if (vcy_redistance(ctx, level, big_r, &n) == VCY_OK) return true;
    *error = vcy_last_error();
    return false;
  });
}

}  // namespace detail
}  // namespace vacancy
