// K1 (fused), host side: what a fused carve launch needs before carve_fused_kernel (carve_fused_kernel.h) runs -- the view
// records, the window maxima, the footprint pre-pass, the live list -- the launch itself (launch_carve_fused: the stages
// that enqueue what carve_fused_plan.h has decided), and the slab planner.  The pre-pass kernels live here, next to the
// only code that launches them.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "carve_fused_device.h"

namespace vcy {
namespace {

constexpr int kWmaxPlanes = 2;           // window sizes 4 and 8

// ---- window maxima (FusedView::wmax) --------------------------------------------------------
// Each thread produces four consecutive pixels of a row; blockIdx.y = view.  Rows are read as float4
// when the image allows it (width % 4 == 0, 16-byte aligned base), element-wise otherwise.  Pixels
// beyond the image border count as -inf, i.e. windows are clipped to the image.

// a[0..7] = row[x0 .. x0 + 7] (x0 % 4 == 0, x0 < w); row == nullptr: a row below the image
__device__ __forceinline__ void wmax_load8(const float* __restrict__ row, int x0, int w, bool vec, float a[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = -INFINITY;
  if (row == nullptr) return;
  if (vec) {
    const float4 lo = *(const float4*)(row + x0);
    a[0] = lo.x, a[1] = lo.y, a[2] = lo.z, a[3] = lo.w;
    if (x0 + 4 < w) {
      const float4 hi = *(const float4*)(row + x0 + 4);
      a[4] = hi.x, a[5] = hi.y, a[6] = hi.z, a[7] = hi.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (x0 + j < w) a[j] = row[x0 + j];
  }
}

__device__ __forceinline__ void wmax_store4(float* __restrict__ row, int x0, int w, bool vec, const float o[4]) {
  if (vec) {
    *(float4*)(row + x0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < w) row[x0 + j] = o[j];
  }
}

// Plane 0: maxima of 4 x 4 windows of the image, non-finite pixels counted as +inf (a footprint
// holding one gives no bound: 0 * inf = NaN samples).  NEG: of the negated image, into plane 2.
template <bool NEG>
__global__ __launch_bounds__(256) void wmax_k4_kernel(const FusedView* __restrict__ views) {
  const FusedView& fv = views[blockIdx.y];
  const int w = fv.v.width, h = fv.v.height, wq = (fv.wrect[2] - fv.wrect[0]) >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (fv.wmax == nullptr || wq <= 0 || t >= wq * (fv.wrect[3] - fv.wrect[1])) return;
  const int yr = t / wq, y = fv.wrect[1] + yr, x0 = fv.wrect[0] + ((t - yr * wq) << 2);
  const float* img = fv.v.sdf;
  const bool vec = (w & 3) == 0 && (((uintptr_t)img | (uintptr_t)fv.wmax) & 15) == 0;
  float o[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float a[8];
    wmax_load8(y + r < h ? img + (size_t)(y + r) * w : nullptr, x0, w, vec, a);
#pragma unroll
    for (int j = 0; j < 8; ++j)  // NaN, +inf, -inf -> +inf; the -inf padding beyond the border stays
      if (x0 + j < w && y + r < h) a[j] = (fabsf(a[j]) <= 3.402823466e+38f) ? (NEG ? -a[j] : a[j]) : INFINITY;
    float p[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) p[j] = fmaxf(a[j], a[j + 1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], fmaxf(p[j], p[j + 2]));
  }
  wmax_store4(const_cast<float*>(fv.wmax) + (NEG ? 2 * (size_t)fv.wmax_plane : (size_t)0) + (size_t)y * w, x0, w, vec, o);
}

// Plane 1: maxima of 8 x 8 windows = the four 4 x 4 windows at offsets 0 / 4 of plane 0.
template <bool NEG>
__global__ __launch_bounds__(256) void wmax_k8_kernel(const FusedView* __restrict__ views) {
  const FusedView& fv = views[blockIdx.y];
  const int w = fv.v.width, h = fv.v.height, wq = (fv.wrect[2] - fv.wrect[0]) >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (fv.wmax == nullptr || wq <= 0 || t >= wq * (fv.wrect[3] - fv.wrect[1])) return;
  const int yr = t / wq, y = fv.wrect[1] + yr, x0 = fv.wrect[0] + ((t - yr * wq) << 2);
  const float* in = fv.wmax + (NEG ? 2 * (size_t)fv.wmax_plane : (size_t)0);  // (planes are multiples of 4 floats or vec is off)
  const bool vec = (w & 3) == 0 && ((uintptr_t)in & 15) == 0;
  float a[8], b[8], o[4];
  wmax_load8(in + (size_t)y * w, x0, w, vec, a);
  wmax_load8(y + 4 < h ? in + (size_t)(y + 4) * w : nullptr, x0, w, vec, b);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = fmaxf(fmaxf(a[j], a[j + 4]), fmaxf(b[j], b[j + 4]));
  wmax_store4(const_cast<float*>(in) + (size_t)fv.wmax_plane + (size_t)y * w, x0, w, vec, o);
}

// Pre-pass of the raw-tile carve kernels: blockIdx.y = view, thread = wave brick (linear, x fastest: the carve
// kernel's wave (bx, wave) of brick row (by, bz) is brick (bz * nby + by) * nbw + 4 bx + wave).
// VALU-bound (round 5: 441 vector instructions per pair, 0.41 of the 0.6 ms it takes at 1024^3 x 32 at two cycles each;
// profiles/r05/prepass.txt) -- hence the fast divisions of the brick number (div_nbw, div_nby: by nbw and nby, for launches of
// fewer than 2^32 bricks), the depth-range test on two values instead of eight, 24-bit multiplies and a scalar base
// for the window lookups in footprint_of.
template <bool SAMEF, bool GEN>
__global__ __launch_bounds__(256) void footprint_records_kernel(GridParams g, const FusedView* __restrict__ views,
                                                                int nbw, int nby, int64_t nbricks, ModeParams mode,
                                                                int want_bound, int want_lower,
                                                                FootprintRecord* __restrict__ records,
                                                                FastDivU32 div_nbw, FastDivU32 div_nby, int small32) {
  const int64_t brick = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (brick >= nbricks) return;
  const int vi = blockIdx.y;
  int bxw, by, bz;
  if (small32) {  // (uniform)
    const uint32_t b32 = (uint32_t)brick;
    const uint32_t rowb = fast_div_u32(b32, div_nbw);
    bxw = (int)(b32 - rowb * (uint32_t)nbw);
    const uint32_t zz = fast_div_u32(rowb, div_nby);
    by = (int)(rowb - zz * (uint32_t)nby);
    bz = (int)zz;
  } else {
    bxw = (int)(brick % nbw);
    const int64_t rowb = brick / nbw;
    by = (int)(rowb % nby);
    bz = (int)(rowb / nby);
  }
  const int x_lo = min(bxw * WX, g.nx - 1), x_hi = min(bxw * WX + WX - 1, g.nx - 1);
  const int y_hi = min(by * BY + BY - 1, g.ny - 1), z_hi = min(bz * BZ + BZ - 1, g.nz_local - 1);
  // (the view is uniform: its record arrives through scalar loads)
  const FusedView& fv = views[vi];
  gfloat_ptr ax = (gfloat_ptr)g.px, ay = (gfloat_ptr)g.py, az = (gfloat_ptr)g.pz;  // (uniform bases, 32-bit offsets)
  const TileInfo ti = footprint_of<SAMEF, kTileRaw, GEN>(
      fv, load_u32_index(ax, (unsigned)x_lo), load_u32_index(ax, (unsigned)x_hi), load_u32_index(ay, (unsigned)(by * BY)),
      load_u32_index(ay, (unsigned)y_hi), load_u32_index(az, (unsigned)(g.z0 + bz * BZ)),
      load_u32_index(az, (unsigned)(g.z0 + z_hi)), mode.ortho != 0, mode.outside == VCY_OUTSIDE_MAX, want_bound != 0,
      want_lower != 0);
  records[(int64_t)vi * nbricks + brick] = pack_footprint(ti, fv.v);
}

// Which workgroups of a carve launch have anything to do: a (wave brick, view) pair is dropped before the state is
// read when every sample is below the truncation limit or (kMax) not above the brick minimum the previous launch
// left (the early return of carve_fused_kernel, same test on the same records).  For a launch of few views over a
// carved grid -- the reference's `Carve(view); ExtractIsoSurface();` loop makes every view a launch of its own --
// most workgroups would only start, load 8 bytes and leave; 2 M such waves cost more than the bricks that do
// change.  This pass lists the workgroups with a live pair, list[0] = their number, list[1 ...] = their linear
// ids (any order); the carve kernel is launched over the full range and workgroups beyond list[0] leave at once.
// Entries WITH RECORDS (launches of one view, `entry_words` = kLiveEntryWords): list[0] = count, list[1] unused, then per
// listed workgroup {id, bit j = the brick of wave j is live, the kWgWaves footprint records} -- what a wave of the listed
// launch otherwise fetches AFTER it has learnt its workgroup id from the list: its record (a second round trip in a wave
// that lasts a handful) and the brick minimum for a test whose outcome is known here.
constexpr int kLiveThreads = 1024;  // (kLiveEntryWords: carve_fused.h)
__global__ __launch_bounds__(kLiveThreads) void live_workgroups_kernel(const FootprintRecord* __restrict__ recs, int64_t nbricks,
                                                                       int nviews, const float* __restrict__ bmin, int trunc,
                                                                       int nbx, int nby, int nbw, int nwg, int* __restrict__ list,
                                                                       int unit_bricks, int entry_words) {
  // (one atomic per block of 1024 workgroups: one per WAVE -- 8192 of them on one counter at 1024^3 -- took 78 us of a
  // 0.8 ms single-view launch, the serialised atomics, not the 25 MB it reads)
  __shared__ int wave_count[kLiveThreads / 64];
  __shared__ int block_base;
  const int wg = blockIdx.x * kLiveThreads + threadIdx.x;
  bool live = false;
  unsigned live_bricks = 0u;        // bit j: brick j of the unit has a live view
  FootprintRecord rec0[kWgWaves];   // (entries with records: view 0 of the workgroup's bricks)
  for (int j = 0; j < kWgWaves; ++j) rec0[j].w0 = 0u, rec0[j].w1 = 0u;
  if (wg < nwg) {
    const int bx = wg % nbx, r = wg / nbx;
    const int by = r % nby, bz = r / nby;
    constexpr int kUnitMax = kWgWaves > VCY_ROW_BRICKS ? kWgWaves : VCY_ROW_BRICKS;
#pragma unroll
    for (int j = 0; j < kUnitMax; ++j) {  // (kWgWaves bricks of a workgroup, or the segment of a wave: kRowBricks)
      if (j >= unit_bricks) break;
      const int bxw = bx * unit_bricks + j;
      if (bxw >= nbw) break;
      const int64_t brick = ((int64_t)bz * nby + by) * nbw + bxw;
      const float smin = bmin ? bmin[brick] : 0.0f;
      for (int v = 0; v < nviews; ++v) {
        const FootprintRecord rec = recs[(int64_t)v * nbricks + brick];
        const float ub = __uint_as_float(rec.w0 & ~63u);
        const bool drop = (trunc && ub < -1.0f) || (bmin != nullptr && ub <= smin);
        live = live || !drop;
        if (!drop) live_bricks |= 1u << j;
        if (v == 0 && j < kWgWaves) rec0[j] = rec;
      }
    }
  }
  const unsigned long long m = __ballot(live);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_count[wave] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < kLiveThreads / 64; ++w) {
      const int c = wave_count[w];
      wave_count[w] = total;  // exclusive offsets of the waves
      total += c;
    }
    block_base = total ? atomicAdd(&list[0], total) : 0;
  }
  __syncthreads();
  if (live) {
    const int slot = block_base + wave_count[wave] + __popcll(m & ((1ull << lane) - 1ull));
    if (entry_words == 0) {
      list[1 + slot] = wg;
    } else {  // (8-byte aligned: the list is, and entry_words is even)
      int* e = list + 2 + (int64_t)slot * kLiveEntryWords;
      e[0] = wg, e[1] = (int)live_bricks;
      for (int j = 0; j < kWgWaves; ++j) e[2 + 2 * j] = (int)rec0[j].w0, e[3 + 2 * j] = (int)rec0[j].w1;
    }
  }
}

// Exhaustive check of the short division sequences for ONE numerator: every significand of the
// denominator (blockIdx.x * 256 + threadIdx.x) in every binade 2^-60 .. 2^60 (blockIdx.y) the fast path
// admits (in_fast_div_range), against the IEEE quotient.  bad[0]: DIV 2 differs somewhere, bad[1]: DIV 1.
__global__ __launch_bounds__(256) void div_verify_kernel(float n, unsigned* __restrict__ bad) {
  const unsigned sig = blockIdx.x * 256u + threadIdx.x;
  const unsigned expo = 127u - 60u + blockIdx.y;
  const float d = __uint_as_float((expo << 23) | sig);
  const float ref = n / d;  // -fhip-fp32-correctly-rounded-divide-sqrt
  const bool b2 = div_view1(2, n, d) != ref, b1 = div_view1(1, n, d) != ref;
  if (__any(b2) && (threadIdx.x & 63) == 0) atomicOr(&bad[0], 1u);
  if (__any(b1) && (threadIdx.x & 63) == 0) atomicOr(&bad[1], 1u);
}

__global__ void fill_lowest_kernel(float* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = kInvalidSdf;
}

std::mutex g_div_mutex;
std::map<std::pair<int, uint32_t>, int> g_div_cache;  // (device, numerator bits) -> level

// 2, 1 or 0: the shortest sequence of div_view2 that equals IEEE division by every admissible depth for
// this numerator on this device.  ~1 G cases, about a millisecond, once per distinct focal length.
int div_level(vcy_ctx* c, float n) {
  uint32_t bits;
  std::memcpy(&bits, &n, 4);
  const std::pair<int, uint32_t> key(c->device, bits);
  std::lock_guard<std::mutex> lock(g_div_mutex);
  auto it = g_div_cache.find(key);
  if (it != g_div_cache.end()) return it->second;
  int level = 0;
  DeviceBuf<unsigned> d_bad;
  unsigned h_bad[2] = {1u, 1u};
  if (d_bad.alloc(2 * sizeof(unsigned)) == hipSuccess) {
    hipError_t e = hipMemsetAsync(d_bad, 0, 2 * sizeof(unsigned), c->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(div_verify_kernel, dim3((1u << 23) / 256u, 121u), dim3(256), 0, c->stream, n, d_bad);
      e = hipMemcpyAsync(h_bad, d_bad, sizeof(h_bad), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) level = h_bad[0] == 0 ? 2 : (h_bad[1] == 0 ? 1 : 0);
    else (void)hipGetLastError();
  } else {
    (void)hipGetLastError();
  }
  g_div_cache[key] = level;
  return level;
}

bool sane(float f) { return f >= 0x1p-40f && f <= 0x1p40f; }

}  // namespace

// The c0 records of a launch (FusedView layout note: c0_all[view][x brick][kC0Stride]) from the views' first rotation
// column and the x axis table, on the device: blockIdx.y = view, thread = (x brick, k).  One fp32 multiply per entry --
// the same IEEE product the host formed until round 5, when a launch with NEW views still waited for the previous
// launch, uploaded 0.5 MB of these from pageable memory and waited again (prepare_views).
namespace {
__global__ __launch_bounds__(256) void c0_records_kernel(const FusedView* __restrict__ views, const float* __restrict__ px,
                                                         int nx, int nbw, float* __restrict__ c2) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int b = t >> 3, k = t & 7;
  if (b >= nbw) return;
  const ViewParams& v = views[blockIdx.y].v;  // (uniform: scalar loads)
  const float p = px[min(b * WX + k, nx - 1)];
  float* rec = c2 + ((size_t)blockIdx.y * nbw + b) * kC0Stride;
  rec[2 * k + 0] = v.r[0][0] * p;
  rec[2 * k + 1] = v.r[1][0] * p;
  rec[16 + k] = v.r[2][0] * p;
  rec[24 + k] = 0.0f;  // (unused quarter of the 128-byte record)
}
}  // namespace

// True when the fused kernel can take these views (otherwise the per-view kernel does).
bool fused_eligible(const vcy_ctx* c, int n_views, const vcy_view* views) {
  const vcy_update_option& u = c->opt.update_option;
  if (count_width_for(c, c->st.views_carved + n_views) > 2) return false;  // (32-bit counters: the per-view kernel)
  if (u.voxel_update == VCY_UPDATE_WEIGHTED_AVERAGE && !sane(u.voxel_update_weight)) return false;
  // (the view step addresses the view and c0 records of a LAUNCH with 32-bit byte offsets, and a launch holds at most
  // kMaxFusedViews views: with them it cannot happen below 2^18 bricks along x, but the kernel relies on it)
  if (!carve_offsets_fit_32(std::min(n_views, kMaxFusedViews), (c->nx + WX - 1) / WX)) return false;
  for (int i = 0; i < n_views; ++i) {
    const vcy_view& v = views[i];
    if (v.is_ortho != views[0].is_ortho) return false;  // one projection model per launch
    if (!v.is_ortho && (!sane(v.fx) || !sane(v.fy))) return false;
    if (v.width > 8192 || v.height > 8192) return false;
  }
  return true;
}

// ---- what a context keeps between launches (carve_fused_state.h) ------------------------------------------------------
bool FusedViewCache::matches(const FusedViewKey& k, const void* vp_now, size_t vp_bytes) const {
  return valid && vp.size() == vp_bytes && std::memcmp(vp.data(), vp_now, vp_bytes) == 0 && key == k;
}
void FusedViewCache::remember(const FusedViewKey& k, const void* vp_now, size_t vp_bytes, bool samef_now, int max_quads_now) {
  vp.assign((const char*)vp_now, (const char*)vp_now + vp_bytes);
  key = k, samef = samef_now, max_quads = max_quads_now;
  valid = true;
}

int FusedViewStage::next(size_t bytes, void** out) {
  if (h[1].bytes() < bytes) {  // (the second is allocated last, after both events: where it is large enough, everything is there)
    for (int q = 0; q < 2; ++q) {
      if (ev[q]) (void)hipEventSynchronize(ev[q]);
      (void)h[q].reset();
    }
    const size_t room = bytes + bytes / 2 + 4096;
    for (int q = 0; q < 2; ++q) {
      VCY_HIP_CHECK(ev[q].ensure(hipEventDisableTiming));
      VCY_HIP_CHECK(h[q].alloc(room));
    }
  }
  idx ^= 1;
  VCY_HIP_CHECK(hipEventSynchronize(ev[idx]));  // (the copy of two launches ago: long made)
  *out = h[idx];
  return VCY_OK;
}
int FusedViewStage::copied(hipStream_t stream) {
  VCY_HIP_CHECK(hipEventRecord(ev[idx], stream));
  return VCY_OK;
}

// What a fused launch derives from its views, resident on the device (the context's staging buffer):
struct PreparedViews {
  float* d_c2;          // c0 records, [view][x brick][kC0Stride]
  FusedView* d_views;   // view blocks with their window-plane addresses and the rectangle the planes are built in
  bool samef;           // fx == fy in every view
  int max_quads;        // threads per view of the window-maximum kernels (0: no planes)
};

namespace {

// The view blocks of a launch, built in the staging buffer `fv`: the views' parameters and, with planes, their addresses
// and the rectangle of slices [zlo, zhi) in every view.
void fill_view_blocks(const vcy_ctx* c, int n_views, const ViewParams* vp, bool ortho, bool need_bound, bool need_lower,
                      int zlo, int zhi, FusedView* fv, bool* samef_out, int* max_quads_out) {
  std::memset((void*)fv, 0, sizeof(FusedView) * (size_t)n_views);
  bool samef = true;
  for (int vi = 0; vi < n_views; ++vi) {
    fv[vi].v = vp[vi];
    samef = samef && (vp[vi].fx == vp[vi].fy);
  }
  int max_quads = 0;  // threads of the window-maximum kernels, per view
  if (need_bound && c->fused.d_wmax) {
    const int planes = need_lower ? 2 * kWmaxPlanes : kWmaxPlanes;
    const double X[2] = {c->h_px_min, c->h_px_max}, Y[2] = {c->h_py_min, c->h_py_max};
    const double Z[2] = {c->h_pz[zlo], c->h_pz[zhi - 1]};
    size_t off = 0;
    for (int vi = 0; vi < n_views; ++vi) {
      const int npx = vp[vi].width * vp[vi].height;
      fv[vi].wmax = c->fused.d_wmax + off;
      fv[vi].wmax_plane = npx;
      fv[vi].has_lower = need_lower ? 1 : 0;
      off += ((size_t)planes * npx + 3) & ~(size_t)3;  // every view 16-byte aligned
      const ImageRect r = slab_image_rect(vp[vi], ortho, X, Y, Z, vp[vi].width, vp[vi].height);
      for (int i = 0; i < 4; ++i) fv[vi].wrect[i] = r.wrect[i];
      max_quads = std::max(max_quads, r.quads);
    }
  }
  *samef_out = samef, *max_quads_out = max_quads;
}

}  // namespace

// `need_bound`: window-maximum planes for the view-dropping bounds (kMax or truncation, see the kernel; without the memory
// for them the kernel scans the footprints instead, results are the same either way).  `need_lower`: two more planes, of
// the negated image (FusedView::has_lower).  [zlo, zhi): the slices whose image-space bounding box the planes must
// cover -- the context's slab for a carve, the whole grid for the slab planner.
int prepare_views(vcy_ctx* c, int n_views, const ViewParams* vp, bool ortho, bool need_bound, bool need_lower, int zlo,
                  int zhi, PreparedViews* out) {
  FusedState& f = c->fused;
  // per-view records of c0 = R[i][0] * px[x] for every wave brick along x (layout: kC0Stride above);
  // columns beyond nx repeat the last one
  const int nxp = (c->nx + WX - 1) / WX * WX, nbw = nxp / WX;
  const size_t c2_bytes = (size_t)n_views * nbw * kC0Stride * sizeof(float);
  const size_t fv_bytes = sizeof(FusedView) * (size_t)n_views;
  const size_t vp_bytes = sizeof(ViewParams) * (size_t)n_views;
  if (need_bound) {
    const int planes = need_lower ? 2 * kWmaxPlanes : kWmaxPlanes;
    size_t total = 0;
    for (int vi = 0; vi < n_views; ++vi) total += ((size_t)planes * vp[vi].width * vp[vi].height + 3) & ~(size_t)3;
    if (f.d_wmax.bytes() < total * sizeof(float)) {
      VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
      if (f.d_wmax.alloc(total * sizeof(float)) != hipSuccess) (void)hipGetLastError();  // (best effort: the kernel scans the footprints)
    }
  }
  // staging buffer owned by the context, grown on demand
  {
    const size_t had = f.d_scratch.bytes();
    const hipError_t eg = f.d_scratch.grow(c2_bytes + fv_bytes, c->stream);
    if (eg != hipSuccess || f.d_scratch.bytes() != had) f.cache.valid = false;  // (the buffer moved)
    VCY_HIP_CHECK(eg);
  }
  float* d_c2 = (float*)f.d_scratch;
  FusedView* d_views = (FusedView*)((char*)f.d_scratch + c2_bytes);
  const FusedViewKey key{f.d_wmax, (void*)d_c2, need_bound, need_lower, ortho, zlo, zhi};
  if (!f.cache.matches(key, vp, vp_bytes)) {
    // The view blocks go through page-locked memory (FusedViewStage) and the c0 records are made by a kernel behind that
    // copy: a launch with new views queues behind the previous one like any other work on the stream (round 5; until then
    // this path waited for the stream twice and uploaded the c0 records, 0.5 MB at 1024^3 x 32, from a host vector).
    static_assert(kC0Stride == 32 && WX == 8, "c0_records_kernel's record layout");
    void* stage = nullptr;
    { const int rcs = f.stage.next(fv_bytes, &stage); if (rcs != VCY_OK) return rcs; }
    bool samef = true;
    int max_quads = 0;
    fill_view_blocks(c, n_views, vp, ortho, need_bound, need_lower, zlo, zhi, (FusedView*)stage, &samef, &max_quads);
    // (the scratch may still be read by the previous launch: the copy and the kernel are queued behind it on the stream)
    VCY_HIP_CHECK(hipMemcpyAsync(d_views, stage, fv_bytes, hipMemcpyHostToDevice, c->stream));
    { const int rcs = f.stage.copied(c->stream); if (rcs != VCY_OK) return rcs; }
    hipLaunchKernelGGL(c0_records_kernel, dim3((unsigned)((nbw * WX + 255) / 256), (unsigned)n_views), dim3(256), 0, c->stream,
                       d_views, c->d_px, c->nx, nbw, d_c2);
    VCY_HIP_CHECK(hipGetLastError());
    f.cache.remember(key, vp, vp_bytes, samef, max_quads);
  }
  out->d_c2 = d_c2;
  out->d_views = d_views;
  out->samef = f.cache.samef;
  out->max_quads = f.cache.max_quads;
  return VCY_OK;
}

void build_window_planes(vcy_ctx* c, const PreparedViews& pv, int n_views, bool need_lower) {
  if (pv.max_quads <= 0) return;
  const dim3 wgrid((unsigned)((pv.max_quads + 255) / 256), (unsigned)n_views);
  hipLaunchKernelGGL(wmax_k4_kernel<false>, wgrid, dim3(256), 0, c->stream, pv.d_views);
  hipLaunchKernelGGL(wmax_k8_kernel<false>, wgrid, dim3(256), 0, c->stream, pv.d_views);
  if (need_lower) {
    hipLaunchKernelGGL(wmax_k4_kernel<true>, wgrid, dim3(256), 0, c->stream, pv.d_views);
    hipLaunchKernelGGL(wmax_k8_kernel<true>, wgrid, dim3(256), 0, c->stream, pv.d_views);
  }
}

// ---- launch_carve_fused and its stages ----------------------------------------------------------------------------------
// Which instance runs over which grid with which flags is decided by carve_fused_plan.h; the stages below enqueue.
namespace {

// ("carvetimer" 1: every chunk of every fused launch leaves three events in the context's log -- before what runs
// ahead of the carve kernel (window maxima, pre-pass, live list), before the carve kernel, after it -- read WITHOUT
// having synchronised in between by vcy_carve_log; vcy_last_carve_ms sums the last launch's chunks)
// (a launch that fails between opening a record and its last event leaves no half-recorded triplet behind:
// vcy_carve_log would fail on it, or report the times of whatever used those events before)
struct CarveLogScope {
  vcy_ctx* c;
  int n0, last0;
  int stamp = -1;
  bool done = false;
  explicit CarveLogScope(vcy_ctx* ctx) : c(ctx), n0(ctx->carve_log_n), last0(ctx->carve_log_last) {}
  ~CarveLogScope() { if (!done) c->carve_log_n = n0, c->carve_log_last = last0; }
  int open(bool first_chunk) {  // the chunk's record, and its first event
    if (!c->time_carve) return VCY_OK;
    stamp = carve_log_open(c, first_chunk);
    return mark(0);
  }
  int mark(int i) {
    if (stamp >= 0) VCY_HIP_CHECK(hipEventRecord(c->carve_log[stamp].ev[i], c->stream));
    return VCY_OK;
  }
};

FusedPlanInput plan_input(const vcy_ctx* c, const GridParams& g, int n_views, const ViewParams* vp, bool ortho,
                          int64_t views_before) {
  const vcy_update_option& u = c->opt.update_option;
  FusedPlanInput in;
  in.update = u.voxel_update, in.trunc = u.use_truncation, in.interp = u.sdf_interp;
  in.max_update_num = (int64_t)u.voxel_max_update_num, in.weight = g.weight;
  in.nx = c->nx, in.ny = c->ny, in.nz_local = c->nz_local();
  in.fresh = c->st.fresh, in.cnt_implied = c->st.cnt_implied, in.brick_min_valid = c->st.brick_min_valid;
  in.have_brick_min = c->d_brick_min != nullptr;
  in.views_before = views_before, in.n_views = n_views, in.ortho = ortho;
  const float x[2] = {c->h_px_min, c->h_px_max}, y[2] = {c->h_py_min, c->h_py_max};
  const float z[2] = {c->h_pz[c->z0], c->h_pz[c->z1 - 1]};
  in.worst = worst_pixels_per_voxel(vp, n_views, ortho, c->opt.resolution, x, y, z);
  in.knobs = c->fused.knobs;
  return in;
}

// shortest division sequence that is exact for every focal length of this batch (checked on the device)
int launch_div_level(vcy_ctx* c, int n_views, const ViewParams* vp, bool ortho) {
  if (ortho || !c->fused.knobs.use_short_div) return 0;
  int level = 2;
  for (int vi = 0; vi < n_views && level > 0; ++vi) {
    level = std::min(level, div_level(c, vp[vi].fx));
    if (vp[vi].fy != vp[vi].fx && level > 0) level = std::min(level, div_level(c, vp[vi].fy));
  }
  return level;
}

// The buffers a launch needs beside the views': brick minima, footprint records, pair counters.
int ensure_launch_buffers(vcy_ctx* c, const FusedLaunchPlan& plan, int n_views) {
  // min(sdf) per wave brick (vcy_ctx::d_brick_min): 4 bytes per 512 voxels, allocated on first use; without it
  // nothing is dropped before the state is read and marching cubes reads every brick
  const int64_t nb = (int64_t)plan.nbw * plan.nby * plan.nbz;
  if (!c->d_brick_min) {
    if (c->d_brick_min.alloc(sizeof(float) * (size_t)nb) != hipSuccess) (void)hipGetLastError();
  }
  // (st.brick_min_valid is only ever true with the array allocated and cnt_implied: StateFlags)
  // Not every wave of the launches below rewrites its entry: a wave whose every view lies below the truncation limit
  // returns before it has read anything, a workgroup left off the live list never starts.  That is harmless while the
  // entry was valid on entry (it still is).  When it was not -- the per-view kernel or a vcy_upload has written to the
  // state since, or the array has just been allocated over a slab that is not fresh -- every entry starts from
  // lowest(): "a voxel of this brick may be untouched", which never drops a view and never lets marching cubes skip
  // the brick.  (A fresh slab needs nothing: there every wave runs and stores its minimum.)
  if (c->d_brick_min && !c->st.fresh && !c->st.brick_min_valid && c->st.cnt_implied) {
    hipLaunchKernelGGL(fill_lowest_kernel, dim3((unsigned)std::min<int64_t>((nb + 255) / 256, 4096)), dim3(256), 0,
                       c->stream, c->d_brick_min, nb);
    VCY_HIP_CHECK(hipGetLastError());
  }
  if (plan.records) VCY_HIP_CHECK(c->fused.d_records.grow((size_t)plan.record_bytes, c->stream));
  if (c->fused.knobs.count_pairs) {  // "paircount" 1: one counter per brick layer of the slab, cleared by every launch
    const size_t bytes = sizeof(unsigned long long) * (size_t)plan.nbz;
    VCY_HIP_CHECK(c->fused.d_pair_count.grow(bytes, c->stream));
    VCY_HIP_CHECK(hipMemsetAsync(c->fused.d_pair_count, 0, bytes, c->stream));
    c->fused.pair_count_views = n_views;
  }
  return VCY_OK;
}

// One chunk of a launch: brick layers [l0, l0 + layers) of the slab, and what of the launch's buffers is theirs.
struct ChunkOperands {
  GridParams g;
  int64_t nbricks;
  FootprintRecord* recs;
  float* bmin;
  unsigned long long* pcnt;
};
ChunkOperands chunk_operands(const vcy_ctx* c, const GridParams& g, const FusedLaunchPlan& plan, int l0, int layers) {
  const int64_t layer_bricks = (int64_t)plan.nbw * plan.nby;
  ChunkOperands o;
  o.g = g;
  o.g.sdf = g.sdf + (int64_t)l0 * BZ * c->slice;
  o.g.cnt = (char*)g.cnt + (int64_t)l0 * BZ * c->slice * c->cnt_bytes;
  o.g.z0 = g.z0 + l0 * BZ;
  o.g.nz_local = std::min(layers * BZ, c->nz_local() - l0 * BZ);
  o.nbricks = layer_bricks * layers;
  o.recs = plan.in_kernel_prologue ? nullptr : (FootprintRecord*)c->fused.d_records;
  o.bmin = c->d_brick_min ? c->d_brick_min + (int64_t)l0 * layer_bricks : nullptr;
  o.pcnt = c->fused.knobs.count_pairs && c->fused.d_pair_count ? c->fused.d_pair_count + l0 : nullptr;  // ("paircount" 1)
  return o;
}

// The footprint records of the chunk's (wave brick, view) pairs.
int run_prepass(vcy_ctx* c, const FusedLaunchPlan& plan, const ChunkOperands& o, const PreparedViews& pv, int n_views,
                const ModeParams& m) {
  const dim3 pgrid((unsigned)((o.nbricks + 255) / 256), (unsigned)n_views);
  const FastDivU32 div_nbw = make_fast_div_u32((uint32_t)plan.nbw), div_nby = make_fast_div_u32((uint32_t)plan.nby);
#define VCY_PREPASS(SF, GN)                                                                                          \
  hipLaunchKernelGGL((footprint_records_kernel<SF, GN>), pgrid, dim3(256), 0, c->stream, o.g, pv.d_views, plan.nbw, \
                     plan.nby, o.nbricks, m, plan.need_bound ? 1 : 0, plan.want_lower ? 1 : 0, o.recs, div_nbw,     \
                     div_nby, o.nbricks < 0xffffffffLL ? 1 : 0)
  if (pv.samef) { if (plan.gen) VCY_PREPASS(true, true); else VCY_PREPASS(true, false); }
  else { if (plan.gen) VCY_PREPASS(false, true); else VCY_PREPASS(false, false); }
#undef VCY_PREPASS
  VCY_HIP_CHECK(hipGetLastError());
  return VCY_OK;
}

// What the geometry of the launch's footprint records depends on, as bytes (FusedRecordCache, carve_fused_state.h).
std::vector<char> record_key(const vcy_ctx* c, const FusedLaunchPlan& plan, const PreparedViews& pv, int n_views,
                             const ViewParams* vp, const ModeParams& m) {
  struct Head {
    int n_views, samef, gen, ortho, outside, z0, z1, nbw, nby, nbz;
    const void* at;
    size_t bytes;
  } h;
  std::memset((void*)&h, 0, sizeof(h));  // (padding is compared too)
  h.n_views = n_views, h.samef = pv.samef ? 1 : 0, h.gen = plan.gen ? 1 : 0, h.ortho = m.ortho, h.outside = m.outside;
  h.z0 = c->z0, h.z1 = c->z1, h.nbw = plan.nbw, h.nby = plan.nby, h.nbz = plan.nbz;
  h.at = (const void*)c->fused.d_records, h.bytes = c->fused.d_records.bytes();
  std::vector<char> key(sizeof(Head) + sizeof(ViewParams) * (size_t)n_views);
  std::memcpy(key.data(), &h, sizeof(Head));
  for (int vi = 0; vi < n_views; ++vi) {
    // (the bytes as FusedViewCache compares them, with what only the bound depends on blanked: the image, max_sdf)
    char* dst = key.data() + sizeof(Head) + sizeof(ViewParams) * (size_t)vi;
    std::memcpy(dst, &vp[vi], sizeof(ViewParams));
    std::memset(dst + offsetof(ViewParams, sdf), 0, sizeof(vp[vi].sdf));
    std::memset(dst + offsetof(ViewParams, max_sdf), 0, sizeof(vp[vi].max_sdf));
  }
  return key;
}

// The one place that writes the record buffer: it forgets which launch the buffer described, runs the pre-pass, and
// remembers this launch's key when a later launch may reuse the records (`key` non-null: fused_records_cacheable).
int write_records(vcy_ctx* c, const FusedLaunchPlan& plan, const ChunkOperands& o, const PreparedViews& pv, int n_views,
                  const ModeParams& m, std::vector<char>* key) {
  c->fused.rec_cache.forget();
  { const int rc = run_prepass(c, plan, o, pv, n_views, m); if (rc != VCY_OK) return rc; }
  if (key != nullptr) c->fused.rec_cache.remember(std::move(*key));
  return VCY_OK;
}

// Lists the chunk's live workgroups (live_workgroups_kernel) and copies their number into the hint; *live: that number
// when the host has waited for it ("livesync"), else kLiveNotWaited.
int list_live_workgroups(vcy_ctx* c, const FusedLaunchPlan& plan, const FusedChunkPlan& chunk, const ChunkOperands& o,
                         int n_views, int trunc, int* live) {
  FusedState& f = c->fused;
  const int nwg = chunk.units;
  // (the hint below: a race with its copy is benign, it only decides whether the NEXT launch lists its workgroups; with
  // several chunks it reflects the last one)
  VCY_HIP_CHECK(f.d_wg_list.grow(chunk.list_bytes, c->stream));
  VCY_HIP_CHECK(hipMemsetAsync(f.d_wg_list, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(live_workgroups_kernel, dim3((unsigned)((nwg + kLiveThreads - 1) / kLiveThreads)), dim3(kLiveThreads), 0,
                     c->stream, o.recs, o.nbricks, n_views, chunk.have_min ? o.bmin : nullptr, trunc, chunk.units_x, plan.nby,
                     plan.nbw, nwg, f.d_wg_list, chunk.unit_bricks, chunk.list_entry_words);
  VCY_HIP_CHECK(hipGetLastError());
  if (!f.h_live_hint && f.h_live_hint.alloc(2 * sizeof(int)) != hipSuccess) (void)hipGetLastError();
  if (f.h_live_hint) {
    f.h_live_hint[1] = nwg;
    (void)hipMemcpyAsync(&f.h_live_hint[0], f.d_wg_list, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    // (the wait, and what it buys: finish_fused_chunk)
    if (f.knobs.live_sync && hipStreamSynchronize(c->stream) == hipSuccess) *live = f.h_live_hint[0];
    else (void)hipGetLastError();
  }
  return VCY_OK;
}

// Fills the CarveLaunch of a chunk from the two plans and hands it to the unit that holds the instances.
int launch_chunk(vcy_ctx* c, const FusedLaunchPlan& plan, const FusedChunkPlan& chunk, const FusedChunkLaunch& fin,
                 const ChunkOperands& o, const PreparedViews& pv, int n_views, const ModeParams& m, CarveLogScope* log) {
  CarveLaunch launch;
  launch.update = plan.update;
  launch.trunc = m.trunc != 0, launch.samef = pv.samef, launch.checkmax = plan.checkmax, launch.big = plan.big;
  launch.gen = plan.gen, launch.div_level = m.div_level;
  launch.flavour = plan.flavour;
  launch.g = o.g, launch.views = pv.d_views, launch.c0_all = pv.d_c2, launch.n_views = n_views, launch.mode = m;
  launch.nbx = chunk.units_x, launch.nby = plan.nby, launch.cull = c->fused.knobs.use_cull ? 1 : 0;
  launch.state_flags = fin.state_flags;
  launch.records = o.recs, launch.nbricks = o.nbricks, launch.brick_min = o.bmin;
  const int* list = c->fused.d_wg_list;
  launch.wg_list = chunk.listed ? list : nullptr, launch.pair_count = o.pcnt;
  launch.grid_x = fin.grid_x, launch.stream = c->stream, launch.row_units = chunk.units;
  { const int rcl = log->mark(1); if (rcl != VCY_OK) return rcl; }
  if (fin.grid_x == 0) {
    // (no workgroup is live: nothing to launch)
  } else if (c->cnt_bytes == 1)
    launch_fused_counts8(launch);
  else
    launch_fused_counts16(launch);
  VCY_HIP_CHECK(hipGetLastError());
  return log->mark(2);
}

}  // namespace

// Carves views[0..n_views) (n_views <= 32, max_sdf already resolved) in one launch.  The caller has declared the write
// (StateFlags::written, once for all its launches); `views_before`: views applied since the fill when this one starts.
int launch_carve_fused(vcy_ctx* c, const GridParams& g, int n_views, const ViewParams* vp, bool ortho, int64_t views_before) {
  const vcy_update_option& u = c->opt.update_option;
  FusedPlanInput in = plan_input(c, g, n_views, vp, ortho, views_before);
  const FusedLaunchPlan plan = plan_fused_launch(in);
  PreparedViews pv;
  { const int rc = prepare_views(c, n_views, vp, ortho, plan.need_bound, plan.need_lower, c->z0, c->z1, &pv); if (rc != VCY_OK) return rc; }
  CarveLogScope log(c);
  { const int rc = log.open(true); if (rc != VCY_OK) return rc; }
  build_window_planes(c, pv, n_views, plan.need_lower);  // the images may have changed since the last call: rebuild every time
  if ((int64_t)plan.nbx * plan.nby * plan.nbz > 0x7fffffffLL) {
    set_error("slab too large for one launch");
    return VCY_ERR_TOO_MANY_VOXELS;
  }
  ModeParams m{u.voxel_update, u.sdf_interp, u.update_outside, u.use_truncation ? 1 : 0, ortho ? 1 : 0, 0};
  m.div_level = launch_div_level(c, n_views, vp, ortho);
  c->fused.last_div_level = m.div_level;
  { const int rc = ensure_launch_buffers(c, plan, n_views); if (rc != VCY_OK) return rc; }
  in.have_brick_min = c->d_brick_min != nullptr;  // (allocated just now, perhaps)
  for (int l0 = 0; l0 < plan.nbz; l0 += plan.chunk_layers) {
    const int layers = std::min(plan.chunk_layers, plan.nbz - l0);
    const ChunkOperands o = chunk_operands(c, g, plan, l0, layers);
    if (l0 > 0) { const int rc = log.open(false); if (rc != VCY_OK) return rc; }
    const FusedChunkPlan chunk = plan_fused_chunk(plan, in, layers, c->fused.h_live_hint, ++c->fused.live_list_age);
    // The footprint records: the last launch's, when they describe this launch's cameras and slab ("recordcache": the
    // kernel's prologue then looks the bounds up, kStateStaleBounds), else from the pre-pass.
    bool reuse = false;
    if (plan.records) {
      const bool have_planes = pv.max_quads > 0;
      const bool cacheable = fused_records_cacheable(plan, in, chunk, have_planes);
      std::vector<char> key;
      if (cacheable) key = record_key(c, plan, pv, n_views, vp, m);
      reuse = fused_reuses_records(plan, in, chunk, have_planes, cacheable && c->fused.rec_cache.matches(key));
      if (reuse) {
        ++c->fused.rec_cache.hits;
      } else {
        const int rc = write_records(c, plan, o, pv, n_views, m, cacheable ? &key : nullptr);
        if (rc != VCY_OK) return rc;
      }
    }
    int live = kLiveNotWaited;
    if (chunk.listed) { const int rc = list_live_workgroups(c, plan, chunk, o, n_views, m.trunc, &live); if (rc != VCY_OK) return rc; }
    FusedChunkLaunch fin = finish_fused_chunk(plan, in, chunk, live);
    if (reuse) fin.state_flags |= kStateStaleBounds;
    { const int rc = launch_chunk(c, plan, chunk, fin, o, pv, n_views, m, &log); if (rc != VCY_OK) return rc; }
  }
  log.done = true;
  c->st.stored();  // the launches store every voxel of a fresh slab
  // (every wave that ran to its end wrote its entry; the others' entries were valid on entry or hold lowest(), see above)
  c->st.minima_rebuilt(c->d_brick_min != nullptr);
  return VCY_OK;
}

int fused_max_views() { return kMaxFusedViews; }

// ---- slab planner ---------------------------------------------------------------------------------------------
// What a brick layer of the grid will cost a fused carve of these views, BEFORE any slab exists: with view dropping the
// layers through the object cost 1.6x the outer ones, so z-slabs of equal thickness leave the GPUs of a node unequally
// loaded (the slowest rank of eight took 1.24x the mean).  The carve kernel's time is, to a good approximation, a fixed
// cost per wave brick plus a cost per (brick, view) pair it processes.  Which pairs it processes is decided by bounds:
// a view is dropped for a brick when every sample lies below the truncation limit, or (kMax, every voxel touched) not
// above the brick's current minimum.  The first is static.  The second depends on the state -- but min(sdf) of a brick
// after the views processed so far is at least the largest LOWER bound of their samples, so the same window planes
// that give the upper bounds (built here for the negated images as well) let one thread play the kernel's decisions
// for a brick: "processed" is counted where ub > the running maximum of the lower bounds.  That over-counts only views
// whose samples lie within one footprint's variation of the running maximum.  One thread per SAMPLED brick (every
// `stride`-th in x and y, every layer), the views in sequence; the counts are summed per layer.
template <bool SAMEF, bool GEN>
__global__ __launch_bounds__(256) void plan_cost_kernel(GridParams g, const FusedView* __restrict__ views, int nviews,
                                                        int nbw, int nby, int sxn, int syn, int stride, int64_t nsample,
                                                        ModeParams mode, unsigned long long* __restrict__ layer_pairs) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = t < nsample;
  const int64_t tt = valid ? t : nsample - 1;  // (idle lanes repeat the last sample: footprint_of uses wave votes)
  const int sx = (int)(tt % sxn);
  const int64_t r = tt / sxn;
  const int sy = (int)(r % syn), bz = (int)(r / syn);
  const int bxw = min(sx * stride + stride / 2, nbw - 1), by = min(sy * stride + stride / 2, nby - 1);
  const int x_lo = min(bxw * WX, g.nx - 1), x_hi = min(bxw * WX + WX - 1, g.nx - 1);
  const int y_hi = min(by * BY + BY - 1, g.ny - 1), z_hi = min(bz * BZ + BZ - 1, g.nz_local - 1);
  const float xl = g.px[x_lo], xh = g.px[x_hi], yl = g.py[by * BY], yh = g.py[y_hi];
  const float zl = g.pz[g.z0 + bz * BZ], zh = g.pz[g.z0 + z_hi];
  const bool update_max = mode.update == VCY_UPDATE_MAX;
  float smin = -INFINITY;   // lower bound of min(sdf) of the brick once every voxel is touched
  bool touched = false;
  int count = 0;
  for (int vi = 0; vi < nviews; ++vi) {
    float lb = -INFINITY;
    const TileInfo ti = footprint_of<SAMEF, kTileRaw, GEN>(views[vi], xl, xh, yl, yh, zl, zh, mode.ortho != 0,
                                                            mode.outside == VCY_OUTSIDE_MAX, true, true, &lb);
    const bool drop = (mode.trunc != 0 && ti.ub < -1.0f) || (update_max && touched && ti.ub <= smin);
    if (!drop) {
      ++count;
      if (update_max && (ti.sure & 1)) {  // (a `sure` view touches every voxel of the brick)
        smin = touched ? fmaxf(smin, lb) : lb;
        touched = true;
      }
    }
  }
  if (!valid) count = 0;
  const int bz0 = __shfl(bz, 0, 64);
  if (__all(bz == bz0)) {  // (the usual case: one atomic per wave)
    for (int d = 32; d > 0; d >>= 1) count += __shfl_down(count, d, 64);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(&layer_pairs[bz0], (unsigned long long)count);
  } else if (count) {
    atomicAdd(&layer_pairs[bz], (unsigned long long)count);
  }
}

// pairs[l] = estimated (brick, view) pairs a fused carve of these views processes in brick layer l of the WHOLE grid,
// scaled from the sampled bricks to the layer's bricks; bricks_per_layer as the carve kernel counts them.
int plan_layer_pairs(vcy_ctx* c, int n_views, const ViewParams* vp, bool ortho, int stride, std::vector<double>* pairs,
                     int64_t* bricks_per_layer) {
  const vcy_update_option& u = c->opt.update_option;
  const int nxp = (c->nx + WX - 1) / WX * WX, nbw = nxp / WX, nby = (c->ny + BY - 1) / BY, nbz = (c->nz + BZ - 1) / BZ;
  *bricks_per_layer = (int64_t)nbw * nby;
  pairs->assign((size_t)nbz, (double)n_views * (double)nbw * nby);  // nothing dropped: every pair
  const bool drops = c->fused.knobs.use_cull && (u.voxel_update == VCY_UPDATE_MAX || u.use_truncation);
  if (!drops) return VCY_OK;
  if (stride < 1) stride = 1;
  PreparedViews pv;
  {
    const int rcp = prepare_views(c, n_views, vp, ortho, true, true, 0, c->nz, &pv);
    if (rcp != VCY_OK) return rcp;
  }
  if (pv.max_quads <= 0) return VCY_OK;  // no memory for the planes: no estimate, equal layers
  build_window_planes(c, pv, n_views, true);
  GridParams g;
  std::memset(&g, 0, sizeof(g));
  g.px = c->d_px, g.py = c->d_py, g.pz = c->d_pz;
  g.nx = c->nx, g.ny = c->ny, g.z0 = 0, g.nz_local = c->nz;
  ModeParams m{u.voxel_update, u.sdf_interp, u.update_outside, u.use_truncation ? 1 : 0, ortho ? 1 : 0, 0};
  const int sxn = (nbw + stride - 1) / stride, syn = (nby + stride - 1) / stride;
  const int64_t nsample = (int64_t)sxn * syn * nbz;
  DeviceBuf<unsigned long long> d_out;
  VCY_HIP_CHECK(d_out.alloc(sizeof(unsigned long long) * (size_t)nbz));
  std::vector<unsigned long long> h((size_t)nbz, 0ull);
  hipError_t e = hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * (size_t)nbz, c->stream);
  if (e == hipSuccess) {
    const bool gen = m.ortho != 0 || m.interp == VCY_INTERP_NN;
    const dim3 grid((unsigned)((nsample + 255) / 256));
#define VCY_PLAN(SF, GN)                                                                                           \
  hipLaunchKernelGGL((plan_cost_kernel<SF, GN>), grid, dim3(256), 0, c->stream, g, pv.d_views, n_views, nbw, nby, \
                     sxn, syn, stride, nsample, m, d_out)
    if (pv.samef) { if (gen) VCY_PLAN(true, true); else VCY_PLAN(true, false); }
    else { if (gen) VCY_PLAN(false, true); else VCY_PLAN(false, false); }
#undef VCY_PLAN
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d_out, sizeof(unsigned long long) * (size_t)nbz, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    set_error("slab planner: %s", hipGetErrorString(e));
    return VCY_ERR_HIP;
  }
  const double scale = (double)nbw * nby / ((double)sxn * syn);
  for (int l = 0; l < nbz; ++l) (*pairs)[(size_t)l] = (double)h[(size_t)l] * scale;
  return VCY_OK;
}

namespace {
__global__ void selftest_rcp_count_kernel(int* n_bad) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x + 1;  // 1 .. 65536
  const float x = (float)m;
  if (rcp_count(x) != 1.0f / x) atomicAdd(n_bad, 1);  // IEEE division (-fhip-fp32-correctly-rounded-divide-sqrt)
}
}  // namespace

// Device-side identities the fast paths of the fused kernel rest on; VCY_OK when all hold.
int selftest_fused(hipStream_t stream) {
  DeviceBuf<int> d_bad;
  int h_bad = -1;
  VCY_HIP_CHECK(d_bad.alloc(sizeof(int)));
  hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(int), stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(selftest_rcp_count_kernel, dim3(256), dim3(256), 0, stream, d_bad);
    e = hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) {
    set_error("self test failed to run: %s", hipGetErrorString(e));
    return VCY_ERR_HIP;
  }
  if (h_bad != 0) {
    set_error("self test: rcp_count differs from IEEE division for %d of 65536 counts", h_bad);
    return VCY_ERR_INTERNAL;
  }
  return VCY_OK;
}

}  // namespace vcy
