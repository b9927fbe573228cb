// Internal to libvacancy.so: what the facade's classes hand to the C ABI (include/vacancy_hip.h) -- a Camera with its
// ROI as a vcy_view, a VoxelCarverOption as a vcy_carver_option.  One statement for VoxelCarver and ShardedVoxelCarver.
#pragma once

#include <cstring>

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

}  // namespace detail
}  // namespace vacancy
