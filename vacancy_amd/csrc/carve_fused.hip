// K1 (fused), host side: what a fused carve launch needs before carve_fused_kernel (carve_fused_kernel.h) runs -- the view
// records, the window maxima, the footprint pre-pass, the live list -- the launch itself (launch_carve_fused), and the slab
// planner.  The pre-pass kernels live here, next to the only code that launches them.
#include <algorithm>
#include <cmath>
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
constexpr int kLiveListMaxViews = 8;      // launches of up to this many views over a carved grid list their live workgroups first
constexpr int64_t kRecordBytesMax = (int64_t)2 << 30;  // footprint records of one carve launch (see launch_carve_fused)

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

// What a fused launch derives from its views, resident on the device (the context's staging buffer):
struct PreparedViews {
  float* d_c2;          // c0 records, [view][x brick][kC0Stride]
  FusedView* d_views;   // view blocks with their window-plane addresses and the rectangle the planes are built in
  bool samef;           // fx == fy in every view
  int max_quads;        // threads per view of the window-maximum kernels (0: no planes)
};

// `need_bound`: window-maximum planes for the view-dropping bounds (kMax or truncation, see the kernel; without the memory
// for them the kernel scans the footprints instead, results are the same either way).  `need_lower`: two more planes, of
// the negated image (FusedView::has_lower).  [zlo, zhi): the slices whose image-space bounding box the planes must
// cover -- the context's slab for a carve, the whole grid for the slab planner.
int prepare_views(vcy_ctx* c, int n_views, const ViewParams* vp, bool need_bound, bool need_lower, int zlo, int zhi,
                  PreparedViews* out) {
  // per-view records of c0 = R[i][0] * px[x] for every wave brick along x (layout: kC0Stride above);
  // columns beyond nx repeat the last one
  const int nxp = (c->nx + WX - 1) / WX * WX, nbw = nxp / WX;
  const size_t c2_floats = (size_t)n_views * nbw * kC0Stride;
  const size_t c2_bytes = c2_floats * sizeof(float);
  const size_t fv_bytes = sizeof(FusedView) * (size_t)n_views;
  const size_t vp_bytes = sizeof(ViewParams) * (size_t)n_views;
  const int planes = need_lower ? 2 * kWmaxPlanes : kWmaxPlanes;
  if (need_bound) {
    size_t total = 0;
    for (int vi = 0; vi < n_views; ++vi) total += ((size_t)planes * vp[vi].width * vp[vi].height + 3) & ~(size_t)3;
    if (c->d_wmax.bytes() < total * sizeof(float)) {
      VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
      if (c->d_wmax.alloc(total * sizeof(float)) != hipSuccess) (void)hipGetLastError();  // (best effort: the kernel scans the footprints)
    }
  }
  // staging buffer owned by the context, grown on demand
  {
    const size_t had = c->d_fused_scratch.bytes();
    const hipError_t eg = c->d_fused_scratch.grow(c2_bytes + fv_bytes, c->stream);
    if (eg != hipSuccess || c->d_fused_scratch.bytes() != had) c->fused_cache_valid = false;  // (the buffer moved)
    VCY_HIP_CHECK(eg);
  }
  float* d_c2 = (float*)c->d_fused_scratch;
  FusedView* d_views = (FusedView*)((char*)c->d_fused_scratch + c2_bytes);
  // Everything derived from the views -- the c0 records (n_views * nx products), the image-space bounding box of the
  // slab in every view, the device copies -- depends on nothing but the views' parameters (image pointers included),
  // the planes' address and two mode flags: a launch with the SAME views as the last one (the reference's loop carves a
  // sequence of grids with one camera rig; the benchmark repeats its step) takes all of it as it is.  Comparing 4 KB
  // instead of rebuilding and comparing 0.5 MB took 0.1 ms of host time out of every launch, which is what a z-slab
  // of an 8-GPU run pays 10 % of its step for.
  const bool cached = c->fused_cache_valid && c->fused_cache_vp.size() == vp_bytes &&
                      std::memcmp(c->fused_cache_vp.data(), vp, vp_bytes) == 0 && c->fused_cache_wmax == c->d_wmax &&
                      c->fused_cache_bound == need_bound && c->fused_cache_lower == need_lower &&
                      c->fused_cache_ortho == c->fused_ortho && c->fused_cache_at == (void*)d_c2 &&
                      c->fused_cache_z[0] == zlo && c->fused_cache_z[1] == zhi;
  if (!cached) {
    // The view blocks are built in page-locked host memory -- two buffers taken in turn, each with an event that says
    // when the copy out of it has been made -- and the c0 records by a kernel behind that copy: a launch with new
    // views queues behind the previous one like any other work on the stream (round 5; until then this path waited
    // for the stream twice and uploaded the c0 records, 0.5 MB at 1024^3 x 32, from a host vector).
    static_assert(kC0Stride == 32 && WX == 8, "c0_records_kernel's record layout");
    if (c->h_fused_stage[1].bytes() < fv_bytes) {  // (the second is allocated last, after both events: where it is large enough, everything is there)
      for (int q = 0; q < 2; ++q) {
        if (c->ev_fused_stage[q]) (void)hipEventSynchronize(c->ev_fused_stage[q]);
        (void)c->h_fused_stage[q].reset();
      }
      const size_t room = fv_bytes + fv_bytes / 2 + 4096;
      for (int q = 0; q < 2; ++q) {
        VCY_HIP_CHECK(c->ev_fused_stage[q].ensure(hipEventDisableTiming));
        VCY_HIP_CHECK(c->h_fused_stage[q].alloc(room));
      }
    }
    c->fused_stage_idx ^= 1;
    VCY_HIP_CHECK(hipEventSynchronize(c->ev_fused_stage[c->fused_stage_idx]));  // (the copy of two launches ago: long made)
    FusedView* fv = (FusedView*)c->h_fused_stage[c->fused_stage_idx];
    std::memset((void*)fv, 0, fv_bytes);
    bool samef = true;
    for (int vi = 0; vi < n_views; ++vi) {
      fv[vi].v = vp[vi];
      samef = samef && (vp[vi].fx == vp[vi].fy);
    }
    int max_quads = 0;  // threads of the window-maximum kernels, per view
    if (need_bound && c->d_wmax) {
      size_t off = 0;
      for (int vi = 0; vi < n_views; ++vi) {
        const int npx = vp[vi].width * vp[vi].height;
        fv[vi].wmax = c->d_wmax + off;
        fv[vi].wmax_plane = npx;
        fv[vi].has_lower = need_lower ? 1 : 0;
        off += ((size_t)planes * npx + 3) & ~(size_t)3;  // every view 16-byte aligned
        // image-space bounding box of the slab (double precision, 16 px border; the footprints the
        // kernel looks up lie within a fraction of a pixel of the exact hull, their windows inside them)
        const int w = vp[vi].width, h = vp[vi].height;
        int rx0 = 0, ry0 = 0, rx1 = w, ry1 = h;
        {
          const double X[2] = {c->h_px_min, c->h_px_max}, Y[2] = {c->h_py_min, c->h_py_max};
          const double Z[2] = {c->h_pz[zlo], c->h_pz[zhi - 1]};
          double umin = 1e300, umax = -1e300, wmin = 1e300, wmax = -1e300;
          bool whole = false;
          for (int cr = 0; cr < 8; ++cr) {
            const double x = X[cr & 1], y = Y[(cr >> 1) & 1], z = Z[cr >> 2];
            double pc[3];
            for (int i = 0; i < 3; ++i)
              pc[i] = (double)vp[vi].t[i] + ((double)vp[vi].r[i][0] * x + (double)vp[vi].r[i][1] * y + (double)vp[vi].r[i][2] * z);
            double uu = pc[0], ww = pc[1];
            if (!c->fused_ortho) {
              if (!(pc[2] > 1e-30)) { whole = true; break; }
              uu = (double)vp[vi].fx / pc[2] * pc[0] + vp[vi].cx;
              ww = (double)vp[vi].fy / pc[2] * pc[1] + vp[vi].cy;
            }
            if (!(std::fabs(uu) < 1e9) || !(std::fabs(ww) < 1e9)) { whole = true; break; }
            umin = std::min(umin, uu), umax = std::max(umax, uu);
            wmin = std::min(wmin, ww), wmax = std::max(wmax, ww);
          }
          if (!whole) {
            rx0 = std::max(0, (int)std::floor(umin) - 16) & ~3;
            ry0 = std::max(0, (int)std::floor(wmin) - 16);
            rx1 = std::min((w + 3) & ~3, ((int)std::floor(umax) + 16 + 4) & ~3);
            ry1 = std::min(h, (int)std::floor(wmax) + 16 + 1);
            if (rx1 < rx0) rx1 = rx0;
            if (ry1 < ry0) ry1 = ry0;
          } else {
            rx1 = (w + 3) & ~3;
          }
        }
        fv[vi].wrect[0] = rx0, fv[vi].wrect[1] = ry0, fv[vi].wrect[2] = rx1, fv[vi].wrect[3] = ry1;
        max_quads = std::max(max_quads, ((rx1 - rx0) / 4) * (ry1 - ry0));
      }
    }
    // (the scratch may still be read by the previous launch: the copy and the kernel are queued behind it on the stream)
    VCY_HIP_CHECK(hipMemcpyAsync(d_views, fv, fv_bytes, hipMemcpyHostToDevice, c->stream));
    VCY_HIP_CHECK(hipEventRecord(c->ev_fused_stage[c->fused_stage_idx], c->stream));
    hipLaunchKernelGGL(c0_records_kernel, dim3((unsigned)((nbw * WX + 255) / 256), (unsigned)n_views), dim3(256), 0, c->stream,
                       d_views, c->d_px, c->nx, nbw, d_c2);
    VCY_HIP_CHECK(hipGetLastError());
    c->fused_cache_vp.assign((const char*)vp, (const char*)vp + vp_bytes);
    c->fused_cache_wmax = c->d_wmax;
    c->fused_cache_bound = need_bound;
    c->fused_cache_lower = need_lower;
    c->fused_cache_ortho = c->fused_ortho;
    c->fused_cache_at = (void*)d_c2;
    c->fused_cache_z[0] = zlo, c->fused_cache_z[1] = zhi;
    c->fused_cache_samef = samef;
    c->fused_cache_max_quads = max_quads;
    c->fused_cache_valid = true;
  }
  out->d_c2 = d_c2;
  out->d_views = d_views;
  out->samef = c->fused_cache_samef;
  out->max_quads = c->fused_cache_max_quads;
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

// Carves views[0..n_views) (n_views <= 32, max_sdf already resolved) in one launch.  The caller has declared the write
// (StateFlags::written, once for all its launches); `views_before`: views applied since the fill when this one starts.
int launch_carve_fused(vcy_ctx* c, const GridParams& g, int n_views, const ViewParams* vp, int64_t views_before) {
  const vcy_update_option& u = c->opt.update_option;
  const int nzl = c->nz_local();
  const int nxp = (c->nx + WX - 1) / WX * WX, nbw = nxp / WX;
  const bool need_bound = c->use_cull && (u.voxel_update == VCY_UPDATE_MAX || u.use_truncation);
  // (two more planes, of the negated image, for the truncating unit-weight average: FusedView::has_lower)
  const bool need_lower = need_bound && u.use_truncation && u.voxel_update == VCY_UPDATE_WEIGHTED_AVERAGE;
  PreparedViews pv;
  {
    const int rcp = prepare_views(c, n_views, vp, need_bound, need_lower, c->z0, c->z1, &pv);
    if (rcp != VCY_OK) return rcp;
  }
  float* d_c2 = pv.d_c2;
  FusedView* d_views = pv.d_views;
  const bool samef = pv.samef;

  // ("carvetimer" 1: every chunk of every fused launch leaves three events in the context's log -- before what runs
  // ahead of the carve kernel (window maxima, pre-pass, live list), before the carve kernel, after it -- read WITHOUT
  // having synchronised in between by vcy_carve_log; vcy_last_carve_ms sums the last launch's chunks)
  const bool timed = c->time_carve;
  int stamp = -1;
  // (a launch that fails between opening a record and its last event leaves no half-recorded triplet behind:
  // vcy_carve_log would fail on it, or report the times of whatever used those events before)
  struct LogGuard {
    vcy_ctx* c;
    int n0, last0;
    bool done;
    ~LogGuard() { if (!done) c->carve_log_n = n0, c->carve_log_last = last0; }
  } log_guard{c, c->carve_log_n, c->carve_log_last, false};
  if (timed) {
    stamp = carve_log_open(c, true);
    if (stamp >= 0) VCY_HIP_CHECK(hipEventRecord(c->carve_log[stamp].ev[0], c->stream));
  }
  build_window_planes(c, pv, n_views, need_lower);  // the images may have changed since the last call: rebuild every time
  const int nbx = (c->nx + BX - 1) / BX, nby = (c->ny + BY - 1) / BY, nbz = (nzl + BZ - 1) / BZ;
  if ((int64_t)nbx * nby * nbz > 0x7fffffffLL) {
    set_error("slab too large for one launch");
    return VCY_ERR_TOO_MANY_VOXELS;
  }
  ModeParams m{u.voxel_update, u.sdf_interp, u.update_outside, u.use_truncation ? 1 : 0, c->fused_ortho ? 1 : 0, 0};
  // shortest division sequence that is exact for every focal length of this batch (checked on the device)
  if (!c->fused_ortho && c->use_short_div) {
    int level = 2;
    for (int vi = 0; vi < n_views && level > 0; ++vi) {
      level = std::min(level, div_level(c, vp[vi].fx));
      if (vp[vi].fy != vp[vi].fx && level > 0) level = std::min(level, div_level(c, vp[vi].fy));
    }
    m.div_level = level;
  }
  c->last_div_level = m.div_level;
  // update_num can only exceed voxel_max_update_num after more than that many views
  const bool checkmax = views_before + n_views > (int64_t)u.voxel_max_update_num;
  // Tile kind: footprint of an 8x8x8 wave brick in pixels ~ (8*sqrt(3)*pixels_per_voxel + 3)^2.  The raw
  // 16 x 16 pixel tile covers voxels up to ~0.85 px; the 2048-pixel tile filled in place up to ~3 px; wider
  // footprints take the generic path inside the kernel either way.
  bool big = false;
  {
    const float res = c->opt.resolution;
    float worst = 0.0f;
    for (int vi = 0; vi < n_views; ++vi) {
      // pixels per voxel at the centre of the slab (bricks much closer to the camera than that
      // overflow the tile and take the generic path on their own)
      const float X = 0.5f * (c->h_px_min + c->h_px_max), Y = 0.5f * (c->h_py_min + c->h_py_max);
      const float Z = 0.5f * (c->h_pz[c->z0] + c->h_pz[c->z1 - 1]);
      const float pz = vp[vi].t[2] + (vp[vi].r[2][0] * X + (vp[vi].r[2][1] * Y + vp[vi].r[2][2] * Z));
      const float f = std::max(vp[vi].fx, vp[vi].fy);
      // orthographic: one pixel per world unit
      worst = std::max(worst, c->fused_ortho ? res : (pz > 0.0f ? f * res / pz : INFINITY));
    }
    const float side = 8.0f * 1.7320508f * worst + 3.0f;
    big = side > 15.0f;
    if (c->tile_mode == 1) big = false;
    if (c->tile_mode == 2) big = true;
  }
  // min(sdf) per wave brick (vcy_ctx::d_brick_min): 4 bytes per 512 voxels, allocated on first use; without it
  // nothing is dropped before the state is read and marching cubes reads every brick
  if (!c->d_brick_min) {
    const size_t bytes = sizeof(float) * (size_t)nbw * nby * nbz;
    if (c->d_brick_min.alloc(bytes) != hipSuccess) (void)hipGetLastError();
  }
  // (st.brick_min_valid is only ever true with the array allocated and cnt_implied: StateFlags)
  // Not every wave of the launches below rewrites its entry: a wave whose every view lies below the truncation limit
  // returns before it has read anything, a workgroup left off the live list never starts.  That is harmless while the
  // entry was valid on entry (it still is).  When it was not -- the per-view kernel or a vcy_upload has written to the
  // state since, or the array has just been allocated over a slab that is not fresh -- every entry starts from
  // lowest(): "a voxel of this brick may be untouched", which never drops a view and never lets marching cubes skip
  // the brick.  (A fresh slab needs nothing: there every wave runs and stores its minimum.)
  if (c->d_brick_min && !c->st.fresh && !c->st.brick_min_valid && c->st.cnt_implied) {
    const int64_t nb = (int64_t)nbw * nby * nbz;
    hipLaunchKernelGGL(fill_lowest_kernel, dim3((unsigned)std::min<int64_t>((nb + 255) / 256, 4096)), dim3(256), 0,
                       c->stream, c->d_brick_min, nb);
    VCY_HIP_CHECK(hipGetLastError());
  }
  // Cooperative write-back (carve_fused_kernel): pays where a launch moves the state for little arithmetic -- few views
  // over a carved grid (1024^3, one view per launch: weighted average 4.39 -> 3.41 ms, kMax 0.89 -> 0.84), and the first
  // single-view launch on a fresh grid, which stores every voxel once (2.48 -> 1.95 ms: 6.4 GB at 3.3 instead of
  // 2.6 TB/s).  "coopstore": -1 that rule, 0 never, 1 always when the layout allows it: rows of whole bricks, four
  // waves per workgroup, raw tiles.
  // (kMax: only single-view launches -- with 4 or 8 views per launch the waves of a workgroup process different numbers
  // of views and the barrier costs 3 - 4 %, profiles/r04/coop_store_batches.txt; weighted average: up to 8 views, 0 ... +2 %;
  // a fresh grid: single-view launches in either mode -- the fused 32-view launch gained nothing from whole-segment
  // stores in round 3)
  // The few-view flavour (kRowBricks: a wave walks the bricks of a row segment): launches of up to kRowMaxViews views with
  // raw tiles and records from the pre-pass, over rows of whole bricks, no update limit in reach.  "rowkernel" -1 that
  // rule, 0 never (the NB = 1 kernel with its cooperative write-back), n > 0: launches of up to min(n, 8) views.
  const int row_views = c->row_kernel < 0 ? kRowMaxViews : std::min(c->row_kernel, kRowMaxViews);
  const bool rows = !big && !checkmax && (c->nx & (WX - 1)) == 0 && n_views <= row_views && c->prologue_mode != 1;
  const int nseg = (nbw + kRowBricks - 1) / kRowBricks;  // segments per brick row
  // a launch of ONE view through the kernel instance that knows it ("oneview" 0: the general instance)
  const bool one_view = c->one_view && n_views == 1 && !rows && !big && !checkmax && c->prologue_mode != 1;
  const bool coop_ok = (kWgWaves == 4 || kWgWaves == 8) && (c->nx & (WX - 1)) == 0 && !big && !rows;
  const int coop_views = c->st.fresh ? 1 : (u.voxel_update == VCY_UPDATE_MAX ? 1 : kLiveListMaxViews);
  const bool coop = coop_ok && (c->coop_store > 0 || (c->coop_store < 0 && n_views <= coop_views));
  // "ntstore": streaming stores whenever the cooperative write-back runs (0: never) -- whole 128-byte segments that this
  // launch does not read again: 0.5 - 1.5 % on single-view launches (profiles/r06/nontemporal.txt)
  const bool nt = coop && c->nt_store != 0;
  // (kStateEager and kStateListRecords are decided per chunk below: they depend on whether the launch is a listed one)
  const int state_flags_base = (c->st.fresh ? kStateFresh : 0) | (c->st.cnt_implied ? kStateCountImplied : 0) |
                               (c->st.brick_min_valid && !c->st.fresh ? kStateBrickMinValid : 0) |
                               (coop ? kStateCoopStore : 0) | (nt ? kStateStreamStore : 0);
  // Raw tiles: the footprint records of every (wave brick, view) pair come from a pre-pass (footprint_records_kernel),
  // 8 bytes per pair.  The slab is carved in chunks of whole brick layers so that the records of a chunk stay
  // below kRecordBytesMax (1024^3 x 32 views: 0.5 GiB, one chunk; 2048^3 x 64: nine).
  const int64_t layer_bricks = (int64_t)nbw * nby;
  int chunk_layers = nbz;
  // Footprints from the pre-pass (records) or from the carve kernel's own prologue?  The pre-pass: its threads are all
  // busy where the prologue would use nviews lanes of 64, it runs at full occupancy, and the records are what the live
  // list and the early return read.  Round 5 tried the prologue for the one launch whose records are large -- 2048^3 x 64
  // views: 8.6 GB of them, written and read back in chunks, 9.1 of the step's 81.8 ms; every lane of the prologue has a
  // view there and the step becomes ONE launch -- and measured 92.8 ms: the footprints cost 20 ms in the kernel (two
  // dependent round trips in front of every wave, at the carve kernel's occupancy) against 9 in the pre-pass
  // (profiles/r05/bench_2048x64_config4_*.json).  So: "prologue" 0 or 2 records (chunks of at most kRecordBytesMax: four
  // at that shape), 1 in the kernel.
  const int64_t rec_cap = c->record_bytes_max > 0 ? c->record_bytes_max : kRecordBytesMax;  // ("recordbytes": tests force several chunks)
  const bool in_kernel_prologue = !big && c->prologue_mode == 1;
  if (!big && !in_kernel_prologue) {
    const int64_t per_layer = layer_bricks * n_views * (int64_t)sizeof(FootprintRecord);
    const int64_t cap = rec_cap;
    chunk_layers = (int)std::max<int64_t>(1, std::min<int64_t>(nbz, cap / std::max<int64_t>(per_layer, 1)));
    const size_t need = (size_t)(per_layer * chunk_layers);
    VCY_HIP_CHECK(c->d_records.grow(need, c->stream));
  }
  if (c->count_pairs) {  // "paircount" 1: one counter per brick layer of the slab, cleared by every launch
    VCY_HIP_CHECK(c->d_pair_count.grow(sizeof(unsigned long long) * (size_t)nbz, c->stream));
    VCY_HIP_CHECK(hipMemsetAsync(c->d_pair_count, 0, sizeof(unsigned long long) * (size_t)nbz, c->stream));
    c->pair_count_views = n_views;
  }
  const bool gen = m.ortho != 0 || m.interp == VCY_INTERP_NN;
  const bool want_lower = need_bound && u.use_truncation && u.voxel_update != VCY_UPDATE_MAX;
  for (int l0 = 0; l0 < nbz; l0 += chunk_layers) {
    const int layers = std::min(chunk_layers, nbz - l0);
    GridParams gc = g;  // this chunk: brick layers [l0, l0 + layers)
    gc.sdf = g.sdf + (int64_t)l0 * BZ * c->slice;
    gc.cnt = (char*)g.cnt + (int64_t)l0 * BZ * c->slice * c->cnt_bytes;
    gc.z0 = g.z0 + l0 * BZ;
    gc.nz_local = std::min(layers * BZ, nzl - l0 * BZ);
    const int64_t nbricks = layer_bricks * layers;
    FootprintRecord* recs = in_kernel_prologue ? nullptr : (FootprintRecord*)c->d_records;
    float* bmin = c->d_brick_min ? c->d_brick_min + (int64_t)l0 * layer_bricks : nullptr;
    unsigned long long* pcnt = c->count_pairs && c->d_pair_count ? c->d_pair_count + l0 : nullptr;  // ("paircount" 1)
    if (timed && l0 > 0) {
      stamp = carve_log_open(c, false);
      if (stamp >= 0) VCY_HIP_CHECK(hipEventRecord(c->carve_log[stamp].ev[0], c->stream));
    }
    if (!big && !in_kernel_prologue) {
      const dim3 pgrid((unsigned)((nbricks + 255) / 256), (unsigned)n_views);
      const FastDivU32 div_nbw = make_fast_div_u32((uint32_t)nbw), div_nby = make_fast_div_u32((uint32_t)nby);
#define VCY_PREPASS(SF, GN)                                                                                       \
  hipLaunchKernelGGL((footprint_records_kernel<SF, GN>), pgrid, dim3(256), 0, c->stream, gc, d_views, nbw, nby,   \
                     nbricks, m, need_bound ? 1 : 0, want_lower ? 1 : 0, recs, div_nbw, div_nby,                  \
                     nbricks < 0xffffffffLL ? 1 : 0)
      if (samef) { if (gen) VCY_PREPASS(true, true); else VCY_PREPASS(true, false); }
      else { if (gen) VCY_PREPASS(false, true); else VCY_PREPASS(false, false); }
#undef VCY_PREPASS
      VCY_HIP_CHECK(hipGetLastError());
    }
    // units of the launch: workgroup blocks of kWgWaves bricks, or the segments of the few-view flavour (one per wave)
    const int unit_bricks = rows ? kRowBricks : kWgWaves;
    const int units_x = rows ? nseg : nbx;
    const dim3 grid((unsigned)((int64_t)units_x * nby * layers));
    auto groups_of = [&](unsigned units) {  // workgroups that hold `units` listed units
      return rows ? dim3((units + kRowWaves - 1) / kRowWaves) : dim3(units);
    };
    // (unlisted launch of the few-view flavour: unit (g mod 8) + 8 (kRowWaves (g / 8) + wave) of workgroup g)
    dim3 launch_grid = rows ? dim3(8u * ((grid.x + 8u * kRowWaves - 1) / (8u * kRowWaves))) : grid;
    // few views over a carved grid: only the workgroups with a live (brick, view) pair (live_workgroups_kernel)
    const int* wgl = nullptr;
    int list_entry_words = 0;
    const bool have_min = u.voxel_update == VCY_UPDATE_MAX && (state_flags_base & kStateBrickMinValid) != 0 && bmin != nullptr;
    // (not when the list of the previous such launch held most workgroups anyway -- a weighted-average carve touches
    // nearly every brick with every view, and the list pass is then 4 % on top; the count arrives by an asynchronous
    // copy into page-locked memory and is only a hint: reading an older value is harmless)
    const bool list_pays = c->h_live_hint == nullptr || c->h_live_hint[1] <= 0 ||
                           (double)c->h_live_hint[0] < 0.6 * (double)c->h_live_hint[1];
    ++c->live_list_age;
    if (!big && recs != nullptr && c->use_live_list && need_bound && !c->st.fresh && n_views <= kLiveListMaxViews && (m.trunc != 0 || have_min) &&
        (list_pays || c->live_list_age % 16 == 0)) {  // (every 16th launch looks again)
      const int nwg = (int)grid.x;
      // (a launch of ONE view: entries {id, live waves, the four records} -- "listrecords" 0: ids only)
      list_entry_words = one_view && c->list_records != 0 ? kLiveEntryWords : 0;
      const size_t need = list_entry_words ? sizeof(int) * (2 + (size_t)nwg * kLiveEntryWords) : sizeof(int) * ((size_t)nwg + 1);  // (the hint below: a race with its copy is benign, it only
      // decides whether the NEXT launch lists its workgroups; with several chunks it reflects the last one)
      VCY_HIP_CHECK(c->d_wg_list.grow(need, c->stream));
      VCY_HIP_CHECK(hipMemsetAsync(c->d_wg_list, 0, sizeof(int), c->stream));
      hipLaunchKernelGGL(live_workgroups_kernel, dim3((unsigned)((nwg + kLiveThreads - 1) / kLiveThreads)), dim3(kLiveThreads), 0, c->stream, recs, nbricks,
                         n_views, have_min ? bmin : nullptr, m.trunc, units_x, nby, nbw, nwg, c->d_wg_list, unit_bricks,
                         list_entry_words);
      launch_grid = groups_of((unsigned)nwg);  // (every unit started unless the count below arrives)
      VCY_HIP_CHECK(hipGetLastError());
      wgl = c->d_wg_list;
      if (!c->h_live_hint && c->h_live_hint.alloc(2 * sizeof(int)) != hipSuccess) (void)hipGetLastError();
      if (c->h_live_hint) {
        c->h_live_hint[1] = nwg;
        (void)hipMemcpyAsync(&c->h_live_hint[0], c->d_wg_list, sizeof(int), hipMemcpyDeviceToHost, c->stream);
        // The carve kernel is launched over the listed workgroups only: the host waits for the count (the list pass is
        // 60 us of device time behind it) instead of starting every workgroup of the slab to have all but the listed
        // ones read list[0] and leave -- 512 K workgroups that do nothing else are 0.115 ms at 1024^3
        // (profiles/tools/per_view_floor.py), a sixth of a single-view launch.  ("livesync" 0: the full grid, no wait.)
        if (c->live_sync && hipStreamSynchronize(c->stream) == hipSuccess) {
          const int live = c->h_live_hint[0];
          if (live >= 0 && live <= nwg) launch_grid = groups_of((unsigned)live);
        } else {
          (void)hipGetLastError();
        }
      }
    }
    // "eagerstate": the workgroups of a one-view launch over a carved grid request their bricks' state next to the
    // footprint records when nearly all of them will need it: a listed launch (only live workgroups are started), or one
    // that skipped its list because the last one held most workgroups (-1 that rule, 0 never, 1 every one-view launch).
    // 1024^3, one view per launch: weighted average 2.51 -> 2.46 ms, kMax 0.521 -> 0.487 (profiles/r06/eager_state.txt).
    const bool nearly_all_live = wgl != nullptr ? launch_grid.x < grid.x || !list_pays : !list_pays;
    const bool eager_state = !c->st.fresh && one_view &&
                             (c->eager_state > 0 || (c->eager_state < 0 && nearly_all_live));
    CarveLaunch launch;
    launch.update = u.voxel_update == VCY_UPDATE_MAX ? VCY_UPDATE_MAX
                    : gc.weight == 1.0f             ? kUpdateWaUnitWeight
                                                    : VCY_UPDATE_WEIGHTED_AVERAGE;
    launch.trunc = m.trunc != 0, launch.samef = samef, launch.checkmax = checkmax, launch.big = big;
    launch.gen = gen, launch.div_level = m.div_level;
    launch.flavour = rows ? CarveFlavour::kRows : (one_view ? CarveFlavour::kOneView : CarveFlavour::kGeneral);
    launch.g = gc, launch.views = d_views, launch.c0_all = d_c2, launch.n_views = n_views, launch.mode = m;
    launch.nbx = units_x, launch.nby = nby, launch.cull = c->use_cull ? 1 : 0;
    launch.state_flags = state_flags_base | (eager_state ? kStateEager : 0) |
                         (wgl != nullptr && list_entry_words ? kStateListRecords : 0);
    launch.records = recs, launch.nbricks = nbricks, launch.brick_min = bmin, launch.wg_list = wgl, launch.pair_count = pcnt;
    launch.grid_x = launch_grid.x, launch.stream = c->stream, launch.row_units = (int)grid.x;
    if (stamp >= 0) VCY_HIP_CHECK(hipEventRecord(c->carve_log[stamp].ev[1], c->stream));
    if (launch_grid.x == 0) {
      // (no workgroup is live: nothing to launch)
    } else if (c->cnt_bytes == 1)
      launch_fused_counts8(launch);
    else
      launch_fused_counts16(launch);
    VCY_HIP_CHECK(hipGetLastError());
    if (stamp >= 0) VCY_HIP_CHECK(hipEventRecord(c->carve_log[stamp].ev[2], c->stream));
  }
  log_guard.done = true;
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
int plan_layer_pairs(vcy_ctx* c, int n_views, const ViewParams* vp, int stride, std::vector<double>* pairs,
                     int64_t* bricks_per_layer) {
  const vcy_update_option& u = c->opt.update_option;
  const int nxp = (c->nx + WX - 1) / WX * WX, nbw = nxp / WX, nby = (c->ny + BY - 1) / BY, nbz = (c->nz + BZ - 1) / BZ;
  *bricks_per_layer = (int64_t)nbw * nby;
  pairs->assign((size_t)nbz, (double)n_views * (double)nbw * nby);  // nothing dropped: every pair
  const bool drops = c->use_cull && (u.voxel_update == VCY_UPDATE_MAX || u.use_truncation);
  if (!drops) return VCY_OK;
  if (stride < 1) stride = 1;
  PreparedViews pv;
  {
    const int rcp = prepare_views(c, n_views, vp, true, true, 0, c->nz, &pv);
    if (rcp != VCY_OK) return rcp;
  }
  if (pv.max_quads <= 0) return VCY_OK;  // no memory for the planes: no estimate, equal layers
  build_window_planes(c, pv, n_views, true);
  GridParams g;
  std::memset(&g, 0, sizeof(g));
  g.px = c->d_px, g.py = c->d_py, g.pz = c->d_pz;
  g.nx = c->nx, g.ny = c->ny, g.z0 = 0, g.nz_local = c->nz;
  ModeParams m{u.voxel_update, u.sdf_interp, u.update_outside, u.use_truncation ? 1 : 0, c->fused_ortho ? 1 : 0, 0};
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
