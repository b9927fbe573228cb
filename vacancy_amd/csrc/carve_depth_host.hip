// The depth carve on the host (vcy_carve_depth_host): the definition of the section "carve from depth images" of
// vacancy_hip.h run serially, voxel by voxel, through the same dp::add_view the kernel of carve_depth.hip is compiled from.
// Host code only -- no GPU, no context, nothing of the HIP runtime --, so a stand-alone program can build it under host
// sanitizers (tests/depth_host_check.cpp, `make depth_host_check`).
#include <cstdint>
#include <vector>

#include "depth_sample.h"
#include "host_shared.h"

using namespace vcy;

namespace {

template <int UPDATE>
void depth_host(const vcy_carver_option& o, const int32_t n[3], int z_begin, int z_end, const std::vector<dp::View>& views,
                float inv_band, float* sdf, int32_t* update_num) {
  std::vector<float> axis[3];
  for (int a = 0; a < 3; ++a) {
    axis[a].resize((size_t)n[a]);
    axis_positions(o.bb_min[a], o.bb_max[a], o.resolution, n[a], axis[a].data());
  }
  const vcy_update_option& u = o.update_option;
  int64_t idx = 0;
  for (int z = z_begin; z < z_end; ++z)
    for (int y = 0; y < n[1]; ++y)
      for (int x = 0; x < n[0]; ++x, ++idx) {
        float s = sdf[idx];
        int cnt = update_num[idx];
        for (const dp::View& v : views)
          dp::add_view<UPDATE>(v, axis[0][(size_t)x], axis[1][(size_t)y], axis[2][(size_t)z], inv_band, u.voxel_max_update_num,
                               u.voxel_update_weight, s, cnt);
        sdf[idx] = s;
        update_num[idx] = cnt;
      }
}

}  // namespace

extern "C" int vcy_carve_depth_host(const vcy_carver_option* option, int z_begin, int z_end, int n_views, const vcy_view* views,
                                    const float* const* depth, float band, float* sdf, int32_t* update_num) {
  if (!dp::band_ok(band)) {
    set_error("depth carve: band = %g must be finite and > 0, with a finite reciprocal", (double)band);
    return VCY_ERR_INVALID_ARG;
  }
  if (n_views < 1) {
    set_error("depth carve: %d views, at least 1 is needed", n_views);
    return VCY_ERR_INVALID_ARG;
  }
  if (!option || !views || !depth || !sdf || !update_num) {
    set_error("depth carve: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  const vcy_update_option& u = option->update_option;
  if (u.voxel_update != VCY_UPDATE_MAX && u.voxel_update != VCY_UPDATE_WEIGHTED_AVERAGE) {
    set_error("unknown enum value in update_option");
    return VCY_ERR_INVALID_ARG;
  }
  int32_t n[3];
  {
    const int rc = dims_from_option(option->bb_min, option->bb_max, option->resolution, n);
    if (rc != VCY_OK) return rc;
  }
  if (z_begin < 0 || z_end > n[2] || z_begin > z_end) {
    set_error("invalid z-slab [%d,%d) for nz=%d", z_begin, z_end, n[2]);
    return VCY_ERR_INVALID_ARG;
  }
  std::vector<dp::View> rec((size_t)n_views);
  for (int i = 0; i < n_views; ++i) {
    if (!depth[i]) {
      set_error("depth carve: null image of view %d", i);
      return VCY_ERR_INVALID_ARG;
    }
    const int rc = check_view_static(&views[i]);
    if (rc != VCY_OK) return rc;
    dp::fill_view(views[i], depth[i], &rec[(size_t)i]);
  }
  const float inv_band = 1.0f / band;
  if (u.voxel_update == VCY_UPDATE_MAX) depth_host<VCY_UPDATE_MAX>(*option, n, z_begin, z_end, rec, inv_band, sdf, update_num);
  else depth_host<VCY_UPDATE_WEIGHTED_AVERAGE>(*option, n, z_begin, z_end, rec, inv_band, sdf, update_num);
  return VCY_OK;
}
