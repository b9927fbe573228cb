// The robust carve: per voxel the (m + 1)-th largest sample over ALL views of the call instead of the largest, so that a
// voxel is carved only when more than m views say "outside" (vcy_carve_robust_device / _silhouettes; no reference
// counterpart -- the definition is the section "robust carve" of vacancy_hip.h, restated in numpy in tests/robust_ref.py).
//
// One launch, one lane per voxel, the view loop inside the lane.  A lane keeps the K = m + 1 largest samples, the views
// they came from and the sample count in registers for the whole loop; the state is never read, and written once at the
// end: one float and one counter per voxel.  The view records are read with a wave-uniform index (scalar loads), and so
// is every view's projection model: the branch on it is taken by the whole wave.  Per (voxel, view) the arithmetic is
// view_distance<> of carve_common.h, the per-view kernel's; the default mode (bilinear, outside none, no truncation) is
// compiled in, every other mode takes the run-time path.
//
// Blame (overruled[i]): one histogram of n_views counters per workgroup in LDS, added to with LDS atomics, flushed with one
// 64-bit global atomic per non-zero entry.  Integer sums: exact, whatever the schedule.
//
// A wave covers 64 consecutive x of one (y, z) row, as carve_view_kernel does: the SDF taps of neighbouring lanes fall
// into the same few cache lines, and the two stores of a wave are whole lines.
#include <algorithm>
#include <vector>

#include "carve_common.h"

namespace vcy {
namespace {

constexpr int kRobustMaxViews = 1024;  // (the LDS histogram of the blame: 4 KB per workgroup)
constexpr int kRobustMaxTolerate = 3;

struct RobustView {
  ViewParams v;
  int ortho;
};

struct RobustLaunch {
  GridParams g;
  ModeParams m;  // (m.ortho is replaced per view)
  const RobustView* views;
  int n_views;
  int segs_per_row;
  double iso;
  unsigned long long* overruled;  // null: no blame
};

// Steps 1 and 2 of the top list for the sample d of view `index`; `held` entries are in the list.
template <int K>
__device__ __forceinline__ void top_insert(float (&t)[K], int (&id)[K], int held, float d, int index) {
  int pos;
  if (held < K) {
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j == held) t[j] = d, id[j] = index;
    pos = held;
  } else if (d > t[K - 1]) {
    t[K - 1] = d, id[K - 1] = index;
    pos = K - 1;
  } else {
    return;
  }
#pragma unroll
  for (int j = K - 1; j >= 1; --j) {
    if (pos == j && d > t[j - 1]) {
      t[j] = t[j - 1], id[j] = id[j - 1];
      t[j - 1] = d, id[j - 1] = index;
      pos = j - 1;
    }
  }
}

template <typename CountT, int K, bool RT>
__global__ __launch_bounds__(256) void carve_robust_kernel(RobustLaunch L) {
  __shared__ unsigned hist[K > 1 ? kRobustMaxViews : 1];
  const bool blame = K > 1 && L.overruled != nullptr;  // (K = 1 discards nothing)
  if (blame) {
    for (int i = threadIdx.x; i < L.n_views; i += 256) hist[i] = 0u;
    __syncthreads();
  }

  const int y = blockIdx.x / L.segs_per_row;
  const int seg = blockIdx.x - y * L.segs_per_row;
  const int x = seg * 256 + threadIdx.x;
  const int zl = blockIdx.y + blockIdx.z * 65535;
  const bool live = x < L.g.nx && zl < L.g.nz_local;

  if (live) {
    const float px = L.g.px[x], py = L.g.py[y], pz = L.g.pz[L.g.z0 + zl];
    float t[K];
    int id[K];
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = kInvalidSdf, id[j] = 0;
    int n = 0;
    for (int i = 0; i < L.n_views; ++i) {  // (i is uniform: the record is read once per wave)
      const RobustView& rv = L.views[i];
      float d;
      bool hit;
      if (RT) {
        ModeParams m = L.m;
        m.ortho = rv.ortho;
        hit = view_distance<true, 0, 0, false, false>(rv.v, m, px, py, pz, &d);
      } else if (rv.ortho) {
        hit = view_distance<false, VCY_INTERP_BILINEAR, VCY_OUTSIDE_NONE, false, true>(rv.v, L.m, px, py, pz, &d);
      } else {
        hit = view_distance<false, VCY_INTERP_BILINEAR, VCY_OUTSIDE_NONE, false, false>(rv.v, L.m, px, py, pz, &d);
      }
      if (!hit) continue;
      top_insert<K>(t, id, min(n, K), d, i);
      ++n;
    }

    // the (m + 1)-th largest, or the smallest of fewer
    const int keep = min(n, K) - 1;
    float sdf = kInvalidSdf;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j == keep) sdf = t[j];
    const int64_t idx = ((int64_t)zl * L.g.ny + y) * L.g.nx + x;
    L.g.sdf[idx] = sdf;
    ((CountT*)L.g.cnt)[idx] = (CountT)n;

    if (blame && n >= 1 && (double)sdf < L.iso) {
#pragma unroll
      for (int j = 0; j < K - 1; ++j)
        if (j < keep && (double)t[j] >= L.iso) atomicAdd(&hist[id[j]], 1u);
    }
  }

  if (blame) {
    __syncthreads();
    for (int i = threadIdx.x; i < L.n_views; i += 256) {
      const unsigned h = hist[i];
      if (h) atomicAdd(&L.overruled[i], (unsigned long long)h);
    }
  }
}

template <typename CountT, int K>
void launch_robust_mode(const RobustLaunch& L, bool is_default, dim3 grid, hipStream_t stream) {
  if (is_default) hipLaunchKernelGGL((carve_robust_kernel<CountT, K, false>), grid, dim3(256), 0, stream, L);
  else hipLaunchKernelGGL((carve_robust_kernel<CountT, K, true>), grid, dim3(256), 0, stream, L);
}

template <typename CountT>
void launch_robust_k(const RobustLaunch& L, int k, bool is_default, dim3 grid, hipStream_t stream) {
  if (k == 1) launch_robust_mode<CountT, 1>(L, is_default, grid, stream);
  else if (k == 2) launch_robust_mode<CountT, 2>(L, is_default, grid, stream);
  else if (k == 3) launch_robust_mode<CountT, 3>(L, is_default, grid, stream);
  else launch_robust_mode<CountT, 4>(L, is_default, grid, stream);
}

// What both entry points refuse before anything is touched.  Also hands a failure of earlier queued views to this caller
// (check_carve_views).
int robust_check(vcy_ctx* c, int n_views, const vcy_view* views, const void* const* images, int tolerate) {
  if (tolerate < 0 || tolerate > kRobustMaxTolerate) {
    set_error("robust carve: tolerate = %d outside 0 .. %d", tolerate, kRobustMaxTolerate);
    return VCY_ERR_INVALID_ARG;
  }
  if (n_views < 1 || n_views > kRobustMaxViews) {
    set_error("robust carve: %d views outside 1 .. %d", n_views, kRobustMaxViews);
    return VCY_ERR_INVALID_ARG;
  }
  if (!c) {
    set_error("VoxelCarver::CarveRobust voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (c->opt.update_option.voxel_update != VCY_UPDATE_MAX) {
    set_error("robust carve: an order statistic of the samples needs voxel_update = kMax");
    return VCY_ERR_INVALID_ARG;
  }
  if (!views || !images) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_views; ++i)
    if (!images[i]) {
      set_error("robust carve: null image of view %d", i);
      return VCY_ERR_INVALID_ARG;
    }
  // update_num = the number of samples, up to n_views: the counters must be able to hold it at the width the context's
  // halo packs travel in (voxel_max_update_num + 1 decides that width and is otherwise not applied here)
  if ((c->cnt_bytes_wire == 1 && n_views > 255) || (c->cnt_bytes_wire == 2 && n_views > 65535)) {
    set_error("robust carve: %d views do not fit the %d-byte update counters of voxel_max_update_num = %d", n_views,
              c->cnt_bytes_wire, c->opt.update_option.voxel_max_update_num);
    return VCY_ERR_INVALID_ARG;
  }
  return check_carve_views(c, n_views, views);
}

// The launch and the bookkeeping of the state; the arguments have passed robust_check.
int robust_run(vcy_ctx* c, int n_views, const vcy_view* views, const float* const* sdf_dev, int tolerate, double iso,
               int64_t* overruled) {
  VCY_HIP_CHECK(hipSetDevice(c->device));
  // views queued by earlier calls are applied (and their failure reported) first
  { const int rcf = flush_pending(c, true); if (rcf != VCY_OK) return rcf; }
  int segs = 0;
  dim3 grid;
  { const int rcg = voxel_lane_grid(c, &segs, &grid); if (rcg != VCY_OK) return rcg; }
  const vcy_update_option& u = c->opt.update_option;
  std::vector<ViewParams> vp;
  { const int rcv = resolve_views(c, n_views, views, sdf_dev, &vp); if (rcv != VCY_OK) return rcv; }
  std::vector<RobustView> rv((size_t)n_views);
  for (int i = 0; i < n_views; ++i) rv[(size_t)i] = RobustView{vp[(size_t)i], views[i].is_ortho ? 1 : 0};

  // [view records | overruled]
  const size_t off_blame = (sizeof(RobustView) * (size_t)n_views + 255) / 256 * 256;
  DeviceBuf<char> d_buf;
  VCY_HIP_CHECK(d_buf.alloc(off_blame + sizeof(unsigned long long) * (size_t)n_views));
  unsigned long long* d_blame = (unsigned long long*)(d_buf + off_blame);
  VCY_HIP_CHECK(hipMemcpyAsync(d_buf, rv.data(), sizeof(RobustView) * (size_t)n_views, hipMemcpyHostToDevice, c->stream));
  if (overruled) VCY_HIP_CHECK(hipMemsetAsync(d_blame, 0, sizeof(unsigned long long) * (size_t)n_views, c->stream));
  VCY_HIP_CHECK(c->ev_rb_begin.ensure());
  VCY_HIP_CHECK(c->ev_rb_end.ensure());

  // The counters as a reset followed by a carve of n_views would leave them: the width that holds n_views.  What the
  // arrays hold is about to be overwritten, so nothing is converted.
  const int width = !c->lazy_count ? c->cnt_bytes_wire : (n_views <= 255 ? 1 : (n_views <= 65535 ? 2 : 4));
  { const int rcw = set_count_width(c, width, /*keep_contents=*/false); if (rcw != VCY_OK) return rcw; }

  RobustLaunch L;
  L.g = slab_grid_params(c);  // (max_update_num is not read: see the definition)
  L.m = ModeParams{u.voxel_update, u.sdf_interp, u.update_outside, u.use_truncation ? 1 : 0, 0, 0};
  L.views = (const RobustView*)(char*)d_buf;
  L.n_views = n_views;
  L.segs_per_row = segs;
  L.iso = iso;
  L.overruled = overruled ? d_blame : nullptr;
  const bool is_default = u.sdf_interp == VCY_INTERP_BILINEAR && u.update_outside == VCY_OUTSIDE_NONE && !u.use_truncation;

  // From here on the state is the call's, and starts over: the launch stores every voxel, fresh or not, and leaves
  // update_num = 0 only where no view gave a sample -- sdf = lowest() there.
  c->st.written(StateWrite::robust(n_views));
  c->st.stored();

  VCY_HIP_CHECK(hipEventRecord(c->ev_rb_begin, c->stream));
  if (c->cnt_bytes == 1) launch_robust_k<uint8_t>(L, tolerate + 1, is_default, grid, c->stream);
  else if (c->cnt_bytes == 2) launch_robust_k<uint16_t>(L, tolerate + 1, is_default, grid, c->stream);
  else launch_robust_k<uint32_t>(L, tolerate + 1, is_default, grid, c->stream);
  VCY_HIP_CHECK(hipGetLastError());
  VCY_HIP_CHECK(hipEventRecord(c->ev_rb_end, c->stream));
  std::vector<unsigned long long> h_blame;
  if (overruled) {
    h_blame.resize((size_t)n_views);
    VCY_HIP_CHECK(hipMemcpyAsync(h_blame.data(), d_blame, sizeof(unsigned long long) * (size_t)n_views, hipMemcpyDeviceToHost,
                                 c->stream));
  }
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));  // (the view records go with this call)
  VCY_HIP_CHECK(hipEventElapsedTime(&c->last_robust_device_ms, c->ev_rb_begin, c->ev_rb_end));
  if (overruled)
    for (int i = 0; i < n_views; ++i) overruled[i] = (int64_t)h_blame[(size_t)i];
  return VCY_OK;
}

}  // namespace
}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_carve_robust_device(vcy_ctx* c, int n_views, const vcy_view* views, const float* const* sdf_device, int tolerate,
                            double iso_level, int64_t* overruled) {
  const int rc = robust_check(c, n_views, views, (const void* const*)sdf_device, tolerate);
  if (rc != VCY_OK) return rc;
  return robust_run(c, n_views, views, sdf_device, tolerate, iso_level, overruled);
}

int vcy_carve_robust_silhouettes(vcy_ctx* c, int n_views, const vcy_view* views, const uint8_t* const* masks_host,
                                 int tolerate, double iso_level, int64_t* overruled) {
  int rc = robust_check(c, n_views, views, (const void* const*)masks_host, tolerate);
  if (rc != VCY_OK) return rc;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  // every SDF image of the call on the device at once (the order statistic needs all views in one launch), built by the
  // batch builder of the streamed paths
  DeviceBuf<char> d_images;
  std::vector<float*> images;
  rc = alloc_view_images("robust carve", "SDF", n_views, views, &d_images, &images);
  if (rc != VCY_OK) return rc;
  rc = vcy_make_sdf_batch_device(c, n_views, views, masks_host, images.data());
  if (rc != VCY_OK) return rc;
  return robust_run(c, n_views, views, images.data(), tolerate, iso_level, overruled);
}

int vcy_last_robust_ms(const vcy_ctx* c, float* device_ms) {
  if (!c || !device_ms) return VCY_ERR_INVALID_ARG;
  *device_ms = c->last_robust_device_ms;
  return VCY_OK;
}

}  // extern "C"
