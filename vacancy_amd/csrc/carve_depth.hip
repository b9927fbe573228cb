// K10: the depth carve -- projective TSDF fusion of depth images into the voxel state (vcy_carve_depth_device /
// vcy_carve_depth; no reference counterpart -- the definition is the section "carve from depth images" of vacancy_hip.h,
// restated in numpy in tests/depth_ref.py; the serial host function is carve_depth_host.hip).
//
// One launch per 64 views, one lane per voxel, the view loop inside the lane.  A lane reads its sdf and counter once, keeps
// them in registers across the views and writes them once, and only if a view changed them: the state moves once per
// launch where the per-view kernel moves it once per view.  The view records are read with a wave-uniform index (scalar
// loads), and so is every view's projection model: the branch on it is taken by the whole wave.  The arithmetic of a
// (voxel, view) pair is dp::add_view of depth_sample.h, shared with the host function.
//
// A wave covers 64 consecutive x of one (y, z) row, as carve_view_kernel does: the depth taps of neighbouring lanes fall
// into the same few cache lines, and the loads and stores of the state are whole lines.
#include <algorithm>
#include <vector>

#include "carve_common.h"
#include "depth_sample.h"

namespace vcy {
namespace {

struct DepthLaunch {
  GridParams g;
  const dp::View* views;
  int n_views;
  int segs_per_row;
  float inv_band;
};

template <typename CountT, int UPDATE>
__global__ __launch_bounds__(256) void carve_depth_kernel(DepthLaunch L) {
  const int y = blockIdx.x / L.segs_per_row;
  const int seg = blockIdx.x - y * L.segs_per_row;
  const int x = seg * 256 + threadIdx.x;
  if (x >= L.g.nx) return;
  const int zl = blockIdx.y + blockIdx.z * 65535;
  if (zl >= L.g.nz_local) return;
  const int64_t idx = ((int64_t)zl * L.g.ny + y) * L.g.nx + x;

  CountT* __restrict__ cnt = (CountT*)L.g.cnt;
  int n = (int)cnt[idx];
  if (n > L.g.max_update_num) return;  // (the count only grows: a voxel gated now is gated for every view)
  float sdf = L.g.sdf[idx];
  const float px = L.g.px[x], py = L.g.py[y], pz = L.g.pz[L.g.z0 + zl];
  bool changed = false;
  for (int i = 0; i < L.n_views; ++i)  // (i is uniform: the record is read once per wave)
    changed |= dp::add_view<UPDATE>(L.views[i], px, py, pz, L.inv_band, L.g.max_update_num, L.g.weight, sdf, n);
  if (changed) {
    L.g.sdf[idx] = sdf;
    cnt[idx] = (CountT)n;
  }
}

template <typename CountT>
void launch_depth(const DepthLaunch& L, int update, dim3 grid, hipStream_t stream) {
  if (update == VCY_UPDATE_MAX)
    hipLaunchKernelGGL((carve_depth_kernel<CountT, VCY_UPDATE_MAX>), grid, dim3(256), 0, stream, L);
  else
    hipLaunchKernelGGL((carve_depth_kernel<CountT, VCY_UPDATE_WEIGHTED_AVERAGE>), grid, dim3(256), 0, stream, L);
}

// What both entry points refuse before anything is touched.  Also hands a failure of earlier queued views to this caller
// (check_carve_views).
int depth_check(vcy_ctx* c, int n_views, const vcy_view* views, const void* const* images, float band) {
  if (!dp::band_ok(band)) {
    set_error("depth carve: band = %g must be finite and > 0, with a finite reciprocal", (double)band);
    return VCY_ERR_INVALID_ARG;
  }
  if (n_views < 1) {
    set_error("depth carve: %d views, at least 1 is needed", n_views);
    return VCY_ERR_INVALID_ARG;
  }
  if (!c) {
    set_error("VoxelCarver::CarveDepth voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!views || !images) {
    set_error("depth carve: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_views; ++i)
    if (!images[i]) {
      set_error("depth carve: null image of view %d", i);
      return VCY_ERR_INVALID_ARG;
    }
  return check_carve_views(c, n_views, views);
}

// The launches and the bookkeeping of the state; the arguments have passed depth_check and the images are on the context's
// device.
int depth_run(vcy_ctx* c, int n_views, const vcy_view* views, const float* const* depth_dev, float band) {
  VCY_HIP_CHECK(hipSetDevice(c->device));
  // views queued by earlier calls are applied (and their failure reported) first
  { const int rcf = flush_pending(c, true); if (rcf != VCY_OK) return rcf; }
  DepthLaunch L;
  dim3 grid;
  { const int rcg = voxel_lane_grid(c, &L.segs_per_row, &grid); if (rcg != VCY_OK) return rcg; }
  const vcy_update_option& u = c->opt.update_option;
  std::vector<dp::View> rec((size_t)n_views);
  for (int i = 0; i < n_views; ++i) dp::fill_view(views[i], depth_dev[i], &rec[(size_t)i]);
  DeviceBuf<dp::View> d_rec;
  VCY_HIP_CHECK(d_rec.alloc(sizeof(dp::View) * (size_t)n_views));
  VCY_HIP_CHECK(hipMemcpyAsync(d_rec, rec.data(), sizeof(dp::View) * (size_t)n_views, hipMemcpyHostToDevice, c->stream));
  const int n_chunks = (n_views + dp::kMaxViewsPerLaunch - 1) / dp::kMaxViewsPerLaunch;
  if (c->ev_dp.size() < 2 * (size_t)n_chunks) c->ev_dp.resize(2 * (size_t)n_chunks);
  for (int k = 0; k < 2 * n_chunks; ++k) VCY_HIP_CHECK(c->ev_dp[(size_t)k].ensure());

  // from here on the state is the call's (this kernel does not keep the brick minima)
  const int64_t before = c->st.views_carved;
  c->st.written(StateWrite::depth(n_views));
  { const int rcm = materialize(c); if (rcm != VCY_OK) return rcm; }
  L.g = slab_grid_params(c);  // (L.g.cnt again per launch below: ensure_count_width may widen between two)
  L.inv_band = 1.0f / band;

  int chunks_run = 0;
  for (int first = 0; first < n_views; first += dp::kMaxViewsPerLaunch, ++chunks_run) {
    const int m = std::min(dp::kMaxViewsPerLaunch, n_views - first);
    // (update_num <= views applied)
    { const int rcw = ensure_count_width(c, before + first + m); if (rcw != VCY_OK) return rcw; }
    L.g.cnt = c->owned_slab_cnt();
    L.views = d_rec + first;
    L.n_views = m;
    VCY_HIP_CHECK(hipEventRecord(c->ev_dp[2 * (size_t)chunks_run], c->stream));
    if (c->cnt_bytes == 1) launch_depth<uint8_t>(L, u.voxel_update, grid, c->stream);
    else if (c->cnt_bytes == 2) launch_depth<uint16_t>(L, u.voxel_update, grid, c->stream);
    else launch_depth<uint32_t>(L, u.voxel_update, grid, c->stream);
    VCY_HIP_CHECK(hipGetLastError());
    VCY_HIP_CHECK(hipEventRecord(c->ev_dp[2 * (size_t)chunks_run + 1], c->stream));
  }
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));  // (the view records and the caller's images go with this call)
  float total = 0.0f;
  for (int k = 0; k < chunks_run; ++k) {
    float ms = 0.0f;
    VCY_HIP_CHECK(hipEventElapsedTime(&ms, c->ev_dp[2 * (size_t)k], c->ev_dp[2 * (size_t)k + 1]));
    total += ms;
  }
  c->last_depth_device_ms = total;
  return VCY_OK;
}

}  // namespace
}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_carve_depth_device(vcy_ctx* c, int n_views, const vcy_view* views, const float* const* depth_device, float band) {
  const int rc = depth_check(c, n_views, views, (const void* const*)depth_device, band);
  if (rc != VCY_OK) return rc;
  return depth_run(c, n_views, views, depth_device, band);
}

int vcy_carve_depth(vcy_ctx* c, int n_views, const vcy_view* views, const float* const* depth_host, float band) {
  const int rc = depth_check(c, n_views, views, (const void* const*)depth_host, band);
  if (rc != VCY_OK) return rc;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  DeviceBuf<char> d_images;
  std::vector<float*> images;
  { const int rca = alloc_view_images("depth carve", "depth", n_views, views, &d_images, &images); if (rca != VCY_OK) return rca; }
  for (int i = 0; i < n_views; ++i)
    VCY_HIP_CHECK(hipMemcpyAsync(images[(size_t)i], depth_host[i], sizeof(float) * (size_t)views[i].width * views[i].height,
                                 hipMemcpyHostToDevice, c->stream));
  return depth_run(c, n_views, views, images.data(), band);
}

int vcy_last_depth_ms(const vcy_ctx* c, float* device_ms) {
  if (!c || !device_ms) return VCY_ERR_INVALID_ARG;
  *device_ms = c->last_depth_device_ms;
  return VCY_OK;
}

}  // extern "C"
