// 6-connected components of the solid voxels, on the device, and the filter that carves small components away
// (vcy_label_components / vcy_keep_components; no reference counterpart -- the definitions are in vacancy_hip.h).
//
//   solid     update_num >= 1 && (double)sdf < iso_level          (marching cubes' own comparison, marching_cubes.cc:121-128)
//   label     the smallest global voxel id of the component       (unique whatever the order of the atomics)
//
// The chain, all on the context's stream:
//   1. cc_bits      one bit per voxel, 64-voxel words along x -- the streaming read of the state mc_bits does
//   2. cc_init      parent[v] = start of v's run of solid voxels inside its word (the run's first voxel points at the
//                   voxel before it when the run continues from the previous word); -1 for a voxel that is not solid.
//                   Runs along x are therefore joined without a single atomic.
//   3. cc_merge     one thread per word: for the row below in y and the one below in z, every maximal stretch of x where
//                   both rows are solid is ONE union (at its first voxel): find the two roots, atomicMin the larger
//                   root's parent to the smaller, continue with what the atomic returned when somebody else was faster.
//                   Parents only ever decrease and a tree's root is its smallest id, so one pass reaches the unique
//                   fixed point: no "changed" flag, no iteration, no host round trip.
//   4. cc_flatten   label[v] = root(v); roots append themselves to a list (a root is always the start of a run)
//   5. cc_stats     one thread per word walks the runs of its word: size and bounding box per root by integer atomics
//                   into the slot a binary search of the SORTED root list gives; a wave whose lanes all hold the same
//                   root (the common case: one large body) reduces first and issues one set of atomics.
//   6. cc_filter    one wave per 8 x 8 x 8 brick, the fused carve's layout (lane = (y & 7) | (z & 7) << 3, 8 voxels along x
//                   per lane): voxels of removed components get sdf = fill_sdf; a brick that changed has its minimum
//                   reduced again from what was read and written.
// The host reads the number of roots once (page-locked), sorts the root list (real scenes: tens of roots) and, for the
// filter, marks the slots to be removed.  Label storage: 4 bytes per voxel + 1 bit, so up to 2^31 - 1 voxels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "vcy_internal.h"

namespace vcy {
namespace cc {

typedef unsigned long long u64;

struct Stats {       // per root, in the order of the sorted root list
  u64 n;
  int mn[3], mx[3];
};
static_assert(sizeof(Stats) == 32, "layout shared with the host");

constexpr int kBitsWordsPerWave = 8;

__device__ __forceinline__ int load_parent(const int* p, int64_t i) {
  return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// IMPLIED: update_num == 0 implies sdf == lowest() (vcy_ctx::cnt_implied), so the counters need not be read
template <typename CountT, bool IMPLIED>
__global__ __launch_bounds__(256) void cc_bits_kernel(const float* __restrict__ sdf, const CountT* __restrict__ cnt, int nx,
                                                      int Wr, int64_t nwords, double iso, u64* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kBitsWordsPerWave;
  if (first >= nwords) return;
  float s[kBitsWordsPerWave];
  int n[kBitsWordsPerWave];
  int64_t row = first / Wr;
  int w = (int)(first - row * Wr);
#pragma unroll
  for (int k = 0; k < kBitsWordsPerWave; ++k) {
    const int x = w * 64 + lane;
    const bool live = first + k < nwords && x < nx;
    s[k] = kInvalidSdf;
    n[k] = 0;
    if (live) {
      s[k] = __builtin_nontemporal_load(sdf + row * nx + x);
      n[k] = IMPLIED ? 1 : (int)cnt[row * nx + x];
    }
    if (++w == Wr) w = 0, ++row;
  }
  u64 mine = 0;
#pragma unroll
  for (int k = 0; k < kBitsWordsPerWave; ++k) {
    // (a NaN compares false; a lane outside the row holds lowest() with count 0)
    const bool solid = (double)s[k] < iso && (IMPLIED ? s[k] != kInvalidSdf : n[k] >= 1);
    const u64 m = __ballot(solid);
    mine = lane == k ? m : mine;
  }
  if (lane < kBitsWordsPerWave && first + lane < nwords) bits[first + lane] = mine;
}

__global__ __launch_bounds__(256) void cc_init_kernel(const u64* __restrict__ bits, int nx, int Wr, int64_t nwords,
                                                      int* __restrict__ parent) {
  const int lane = threadIdx.x & 63;
  const int64_t wi0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (int64_t wi = wi0; wi < nwords; wi += (int64_t)gridDim.x * 4) {
    const int64_t row = wi / Wr;
    const int w = (int)(wi - row * Wr);
    const int x = w * 64 + lane;
    if (x >= nx) continue;
    const u64 m = bits[wi];
    const int64_t v = row * nx + x;
    int p = -1;
    if ((m >> lane) & 1ull) {
      const u64 gaps = ~m & ((1ull << lane) - 1ull);  // voxels below this one in the word that are not solid
      const int start = gaps ? 64 - __builtin_clzll(gaps) : 0;
      p = (int)(v - lane + start);
      if (start == 0 && lane == 0 && w > 0 && (bits[wi - 1] >> 63)) p = (int)(v - 1);  // the run goes on to the left
    }
    parent[v] = p;
  }
}

__device__ __forceinline__ int find_root(const int* p, int i) {
  int q;
  while ((q = load_parent(p, i)) != i) i = q;
  return i;
}

__device__ __forceinline__ void unite(int* p, int a, int b) {
  for (;;) {
    a = find_root(p, a);
    b = find_root(p, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    // b was a root when it was found: hang it below a -- unless somebody has hung it elsewhere since; then what it
    // points at now and a still have to meet
    const int old = atomicMin(p + b, a);
    if (old == b) return;
    b = old;
  }
}

__global__ __launch_bounds__(256) void cc_merge_kernel(const u64* __restrict__ bits, int nx, int ny, int Wr, int64_t nwords,
                                                       int* __restrict__ parent) {
  const int64_t wi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (wi >= nwords) return;
  const u64 m = bits[wi];
  if (m == 0ull) return;
  const int64_t row = wi / Wr;
  const int w = (int)(wi - row * Wr);
  const int y = (int)(row % ny);
  const int64_t v0 = row * nx + (int64_t)w * 64;
  const u64 m_left = w > 0 ? bits[wi - 1] : 0ull;
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    if (dir == 0 ? y == 0 : row < ny) continue;
    const int64_t dw = dir == 0 ? (int64_t)Wr : (int64_t)Wr * ny;
    const int64_t dv = dir == 0 ? (int64_t)nx : (int64_t)nx * ny;
    const u64 both = m & bits[wi - dw];
    if (both == 0ull) continue;
    const u64 carry = w > 0 ? (m_left & bits[wi - dw - 1]) >> 63 : 0ull;
    u64 starts = both & ~((both << 1) | carry);  // first voxel of every stretch where both rows are solid
    while (starts) {
      const int b = __builtin_ctzll(starts);
      starts &= starts - 1ull;
      unite(parent, (int)(v0 + b), (int)(v0 + b - dv));
    }
  }
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ parent, int64_t n, int* __restrict__ roots,
                                                         int cap, unsigned int* __restrict__ n_roots) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    const int p = load_parent(parent, v);
    if (p < 0) continue;
    const int r = p == (int)v ? p : find_root(parent, p);
    // (a concurrent reader that passes through v finds either ancestor)
    if (r != p) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r == (int)v) {
      const unsigned int k = atomicAdd(n_roots, 1u);
      if (k < (unsigned int)cap) roots[k] = r;
    }
  }
}

// the list again, for a list that did not fit the first time
__global__ __launch_bounds__(256) void cc_collect_kernel(const int* __restrict__ label, int64_t n, int* __restrict__ roots,
                                                         int cap, unsigned int* __restrict__ n_roots) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    if (label[v] == (int)v) {
      const unsigned int k = atomicAdd(n_roots, 1u);
      if (k < (unsigned int)cap) roots[k] = (int)v;
    }
  }
}

__device__ __forceinline__ int slot_of(const int* __restrict__ roots, int n_roots, int r) {
  int lo = 0, hi = n_roots - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (roots[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void add_stats(Stats* __restrict__ st, int slot, u64 n, int x0, int x1, int y0, int y1, int z0,
                                          int z1) {
  Stats* s = st + slot;
  atomicAdd(&s->n, n);
  atomicMin(&s->mn[0], x0);
  atomicMax(&s->mx[0], x1);
  atomicMin(&s->mn[1], y0);
  atomicMax(&s->mx[1], y1);
  atomicMin(&s->mn[2], z0);
  atomicMax(&s->mx[2], z1);
}

__global__ __launch_bounds__(256) void cc_stats_kernel(const u64* __restrict__ bits, const int* __restrict__ label, int nx,
                                                       int ny, int Wr, int64_t nwords, const int* __restrict__ roots,
                                                       int n_roots, Stats* __restrict__ st) {
  const int64_t wi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  u64 m = wi < nwords ? bits[wi] : 0ull;
  int64_t row = 0;
  int w = 0;
  if (m) {
    row = wi / Wr;
    w = (int)(wi - row * Wr);
  }
  const int y = (int)(row % ny), z = (int)(row / ny);
  const int64_t v0 = row * nx + (int64_t)w * 64;
  // runs of this word; consecutive runs of one root are summed before they go out
  int cur = -1, cnt = 0, x0 = 0, x1 = 0;
  while (m) {
    const int s = __builtin_ctzll(m);
    const u64 t = ~(m >> s);
    const int len = t ? __builtin_ctzll(t) : 64;  // (t == 0: s == 0 and the whole word is one run)
    m = len + s >= 64 ? 0ull : m & ~((1ull << (s + len)) - 1ull);
    const int r = label[v0 + s];
    if (r != cur && cnt) {
      add_stats(st, slot_of(roots, n_roots, cur), (u64)cnt, x0, x1, y, y, z, z);
      cnt = 0;
    }
    if (cnt == 0) x0 = w * 64 + s;
    cur = r;
    cnt += len;
    x1 = w * 64 + s + len - 1;
  }
  const u64 have = __ballot(cnt != 0);
  if (have == 0ull) return;
  const int first = __builtin_ctzll(have);
  const int r0 = __shfl(cur, first, 64);
  if (__ballot(cnt != 0 && cur != r0) != 0ull) {
    if (cnt) add_stats(st, slot_of(roots, n_roots, cur), (u64)cnt, x0, x1, y, y, z, z);
    return;
  }
  // one root in the whole wave
  const int big = 0x7fffffff;
  int c = cnt, ax0 = cnt ? x0 : big, ax1 = cnt ? x1 : -1, ay0 = cnt ? y : big, ay1 = cnt ? y : -1, az0 = cnt ? z : big,
      az1 = cnt ? z : -1;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    c += __shfl_xor(c, d, 64);
    ax0 = min(ax0, __shfl_xor(ax0, d, 64));
    ax1 = max(ax1, __shfl_xor(ax1, d, 64));
    ay0 = min(ay0, __shfl_xor(ay0, d, 64));
    ay1 = max(ay1, __shfl_xor(ay1, d, 64));
    az0 = min(az0, __shfl_xor(az0, d, 64));
    az1 = max(az1, __shfl_xor(az1, d, 64));
  }
  if ((int)(threadIdx.x & 63) == first) add_stats(st, slot_of(roots, n_roots, r0), (u64)c, ax0, ax1, ay0, ay1, az0, az1);
}

// One wave per brick.  `removed[slot]` != 0: the component of the slot-th root (sorted) goes.  keep0: a root known to
// stay (the largest kept component, or -1), tested before the search.
__global__ __launch_bounds__(256) void cc_filter_kernel(float* __restrict__ sdf, const int* __restrict__ label, int nx, int ny,
                                                        int nz, int nbw, int nby, int64_t nbricks,
                                                        const int* __restrict__ roots, int n_roots,
                                                        const uint8_t* __restrict__ removed, int keep0, float fill,
                                                        float* __restrict__ brick_min) {
  const int lane = threadIdx.x & 63;
  const int64_t brick = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (brick >= nbricks) return;  // (uniform per wave)
  const int bx = (int)(brick % nbw);
  const int64_t q = brick / nbw;
  const int by = (int)(q % nby), bz = (int)(q / nby);
  const int y = by * 8 + (lane & 7), z = bz * 8 + (lane >> 3);
  const bool row_ok = y < ny && z < nz;
  const int64_t v0 = ((int64_t)z * ny + y) * nx + bx * 8;
  const int nxl = min(8, nx - bx * 8);  // voxels of the brick along x (uniform)
  uint32_t gone = 0;
  if (row_ok) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < nxl) {
        const int r = label[v0 + k];
        if (r >= 0 && r != keep0 && removed[slot_of(roots, n_roots, r)]) gone |= 1u << k;
      }
    }
  }
  if (__ballot(gone != 0u) == 0ull) return;  // nothing of this brick goes: not a byte of it is touched
  float mn = INFINITY;
  if (row_ok) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < nxl) {
        float s;
        if ((gone >> k) & 1u) {
          s = fill;
          sdf[v0 + k] = fill;
        } else {
          s = sdf[v0 + k];
        }
        mn = fminf(mn, s);
      }
    }
  }
  if (brick_min != nullptr) {  // (null: the minima did not describe the state before, and do not now)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mn = fminf(mn, __shfl_xor(mn, d, 64));
    if (lane == 0) brick_min[brick] = mn;
  }
}

}  // namespace cc

using cc::Stats;

namespace {

int grow(void** p, size_t* have, size_t want) {
  if (*have >= want) return VCY_OK;
  if (*p) VCY_HIP_CHECK(hipFree(*p));
  *p = nullptr;
  *have = 0;
  VCY_HIP_CHECK(hipMalloc(p, want));
  *have = want;
  return VCY_OK;
}

bool whole_grid(const vcy_ctx* c) { return c->z0 == 0 && c->z1 == c->nz && c->halo_lo == 0; }

}  // namespace

// Steps 1 - 5.  `comps` in the order of the header (n_voxels descending, label ascending); `slot_of_comp[i]` = where
// component i's root stands in the sorted root list the device holds (cc_roots).  The begin event is recorded here, the
// end event by the caller.
static int label_components(vcy_ctx* c, double iso, std::vector<vcy_component>* comps, std::vector<int>* slot_of_comp) {
  comps->clear();
  if (slot_of_comp) slot_of_comp->clear();
  c->last_components_device_ms = 0.0f;
  c->cc_timed = false;
  { const int rcf = flush_pending(c); if (rcf != VCY_OK) return rcf; }
  c->cc_labels_valid = true;
  c->cc_n_roots = 0;
  if (c->fresh) {  // nothing carved since the fill: no voxel is solid, and the lazy fill stays lazy
    c->cc_labels_empty = true;
    return VCY_OK;
  }
  c->cc_labels_valid = false;
  const int64_t n = c->slab_voxels();
  if (n > 0x7fffffffLL) {
    set_error("component labels are 32 bits wide: %lld voxels are too many", (long long)n);
    return VCY_ERR_TOO_MANY_VOXELS;
  }
  const int nx = c->nx, ny = c->ny, Wr = (nx + 63) / 64;
  const int64_t nwords = (int64_t)Wr * ny * c->nz;
  { const int rc = grow(&c->d_cc_labels, &c->cc_labels_bytes, sizeof(int) * (size_t)n); if (rc != VCY_OK) return rc; }
  { const int rc = grow(&c->d_cc_bits, &c->cc_bits_bytes, sizeof(cc::u64) * (size_t)nwords + 64); if (rc != VCY_OK) return rc; }
  if (c->cc_roots_cap == 0) {
    const int rc = grow(&c->d_cc_roots, &c->cc_roots_bytes, (size_t)(1 << 16) * (sizeof(int) + sizeof(Stats) + 1));
    if (rc != VCY_OK) return rc;
    c->cc_roots_cap = 1 << 16;
  }
  if (!c->h_cc_report) VCY_HIP_CHECK(hipHostMalloc(&c->h_cc_report, 64, hipHostMallocDefault));
  if (!c->ev_cc_begin) VCY_HIP_CHECK(hipEventCreate(&c->ev_cc_begin));
  if (!c->ev_cc_end) VCY_HIP_CHECK(hipEventCreate(&c->ev_cc_end));
  int* label = (int*)c->d_cc_labels;
  cc::u64* bits = (cc::u64*)c->d_cc_bits;
  unsigned int* d_nroots = (unsigned int*)(bits + nwords);  // (the 64 bytes behind the words)
  const float* sdf = c->owned_slab_sdf();
  const void* cnt = c->owned_slab_cnt();

  VCY_HIP_CHECK(hipEventRecord(c->ev_cc_begin, c->stream));
  c->cc_timed = true;
  VCY_HIP_CHECK(hipMemsetAsync(d_nroots, 0, 64, c->stream));
  {
    const dim3 grid((unsigned)((nwords + 4 * cc::kBitsWordsPerWave - 1) / (4 * cc::kBitsWordsPerWave)));
#define VCY_CC_BITS(T, IMPL) \
  hipLaunchKernelGGL((cc::cc_bits_kernel<T, IMPL>), grid, dim3(256), 0, c->stream, sdf, (const T*)cnt, nx, Wr, nwords, iso, bits)
    if (c->cnt_implied) VCY_CC_BITS(uint8_t, true);
    else if (c->cnt_bytes == 1) VCY_CC_BITS(uint8_t, false);
    else if (c->cnt_bytes == 2) VCY_CC_BITS(uint16_t, false);
    else VCY_CC_BITS(uint32_t, false);
#undef VCY_CC_BITS
    VCY_HIP_CHECK(hipGetLastError());
  }
  const unsigned word_blocks = (unsigned)((nwords + 255) / 256);
  hipLaunchKernelGGL(cc::cc_init_kernel, dim3((unsigned)std::min<int64_t>((nwords + 3) / 4, 1 << 20)), dim3(256), 0, c->stream,
                     bits, nx, Wr, nwords, label);
  VCY_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(cc::cc_merge_kernel, dim3(word_blocks), dim3(256), 0, c->stream, bits, nx, ny, Wr, nwords, label);
  VCY_HIP_CHECK(hipGetLastError());
  const unsigned voxel_blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 1 << 20);
  hipLaunchKernelGGL(cc::cc_flatten_kernel, dim3(voxel_blocks), dim3(256), 0, c->stream, label, n, (int*)c->d_cc_roots,
                     c->cc_roots_cap, d_nroots);
  VCY_HIP_CHECK(hipGetLastError());
  unsigned int* h_report = (unsigned int*)c->h_cc_report;
  VCY_HIP_CHECK(hipMemcpyAsync(h_report, d_nroots, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  const int64_t n_roots = (int64_t)h_report[0];
  c->cc_labels_valid = true;
  c->cc_labels_empty = false;
  if (n_roots == 0) return VCY_OK;
  if (n_roots > c->cc_roots_cap) {  // (thousands of specks: the list did not fit; once more into a larger one)
    const int rc = grow(&c->d_cc_roots, &c->cc_roots_bytes, (size_t)n_roots * (sizeof(int) + sizeof(Stats) + 1));
    if (rc != VCY_OK) {
      c->cc_roots_cap = 0;
      return rc;
    }
    c->cc_roots_cap = (int)n_roots;
    VCY_HIP_CHECK(hipMemsetAsync(d_nroots, 0, 64, c->stream));
    hipLaunchKernelGGL(cc::cc_collect_kernel, dim3(voxel_blocks), dim3(256), 0, c->stream, label, n, (int*)c->d_cc_roots,
                       c->cc_roots_cap, d_nroots);
    VCY_HIP_CHECK(hipGetLastError());
  }
  // [stats of cap roots | cap roots | cap removal flags]
  Stats* d_stats = (Stats*)c->d_cc_roots;
  std::vector<int> roots((size_t)n_roots);
  VCY_HIP_CHECK(hipMemcpyAsync(roots.data(), c->d_cc_roots, sizeof(int) * (size_t)n_roots, hipMemcpyDeviceToHost, c->stream));
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  std::sort(roots.begin(), roots.end());
  int* d_roots = (int*)(d_stats + c->cc_roots_cap);
  std::vector<Stats> stats((size_t)n_roots);
  for (auto& s : stats) {
    s.n = 0;
    s.mn[0] = s.mn[1] = s.mn[2] = 0x7fffffff;
    s.mx[0] = s.mx[1] = s.mx[2] = -1;
  }
  VCY_HIP_CHECK(hipMemcpyAsync(d_stats, stats.data(), sizeof(Stats) * (size_t)n_roots, hipMemcpyHostToDevice, c->stream));
  VCY_HIP_CHECK(hipMemcpyAsync(d_roots, roots.data(), sizeof(int) * (size_t)n_roots, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(cc::cc_stats_kernel, dim3(word_blocks), dim3(256), 0, c->stream, bits, label, nx, ny, Wr, nwords, d_roots,
                     (int)n_roots, d_stats);
  VCY_HIP_CHECK(hipGetLastError());
  VCY_HIP_CHECK(hipMemcpyAsync(stats.data(), d_stats, sizeof(Stats) * (size_t)n_roots, hipMemcpyDeviceToHost, c->stream));
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->cc_n_roots = (int)n_roots;

  std::vector<int> order((size_t)n_roots);
  for (int i = 0; i < (int)n_roots; ++i) order[(size_t)i] = i;
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    if (stats[(size_t)a].n != stats[(size_t)b].n) return stats[(size_t)a].n > stats[(size_t)b].n;
    return roots[(size_t)a] < roots[(size_t)b];
  });
  comps->resize((size_t)n_roots);
  for (size_t i = 0; i < order.size(); ++i) {
    const size_t s = (size_t)order[i];
    vcy_component& o = (*comps)[i];
    o.label = roots[s];
    o.n_voxels = (int64_t)stats[s].n;
    for (int k = 0; k < 3; ++k) o.bb_min[k] = stats[s].mn[k], o.bb_max[k] = stats[s].mx[k];
  }
  if (slot_of_comp) *slot_of_comp = order;
  return VCY_OK;
}

static int finish_timer(vcy_ctx* c) {
  if (!c->cc_timed) return VCY_OK;
  VCY_HIP_CHECK(hipEventRecord(c->ev_cc_end, c->stream));
  VCY_HIP_CHECK(hipEventSynchronize(c->ev_cc_end));
  VCY_HIP_CHECK(hipEventElapsedTime(&c->last_components_device_ms, c->ev_cc_begin, c->ev_cc_end));
  return VCY_OK;
}

static int check_owner(const vcy_ctx* c, const char* who) {
  if (whole_grid(c)) return VCY_OK;
  // a component may continue in the neighbouring slab: the seam merge is not built yet
  set_error("%s: the context owns z [%d, %d) of %d slices; components need the whole grid in one context", who, c->z0, c->z1,
            c->nz);
  return VCY_ERR_UNSUPPORTED;
}

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_label_components(vcy_ctx* c, double iso_level, vcy_component** out, int64_t* n_out) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!out || !n_out) {
    set_error("vcy_label_components: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  *out = nullptr;
  *n_out = 0;
  { const int rc = check_owner(c, "vcy_label_components"); if (rc != VCY_OK) return rc; }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  std::vector<vcy_component> comps;
  { const int rc = label_components(c, iso_level, &comps, nullptr); if (rc != VCY_OK) return rc; }
  { const int rc = finish_timer(c); if (rc != VCY_OK) return rc; }
  if (comps.empty()) return VCY_OK;
  vcy_component* p = (vcy_component*)std::malloc(sizeof(vcy_component) * comps.size());
  if (!p) {
    set_error("vcy_label_components: out of host memory");
    return VCY_ERR_INTERNAL;
  }
  std::memcpy(p, comps.data(), sizeof(vcy_component) * comps.size());
  *out = p;
  *n_out = (int64_t)comps.size();
  return VCY_OK;
}

void vcy_components_free(vcy_component* p) { std::free(p); }

int vcy_download_labels(vcy_ctx* c, int64_t* labels) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  if (!labels || !c->cc_labels_valid) {
    set_error("vcy_download_labels: %s", labels ? "no components have been labelled on this context" : "null pointer");
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const int64_t n = c->slab_voxels();
  if (c->cc_labels_empty) {
    for (int64_t i = 0; i < n; ++i) labels[i] = -1;
    return VCY_OK;
  }
  std::vector<int> raw((size_t)n);
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  VCY_HIP_CHECK(hipMemcpy(raw.data(), c->d_cc_labels, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i) labels[i] = raw[(size_t)i];
  return VCY_OK;
}

int vcy_keep_components(vcy_ctx* c, double iso_level, int keep_largest, int64_t min_voxels, float fill_sdf,
                        int64_t* removed_components, int64_t* removed_voxels) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (removed_components) *removed_components = 0;
  if (removed_voxels) *removed_voxels = 0;
  { const int rc = check_owner(c, "vcy_keep_components"); if (rc != VCY_OK) return rc; }
  if (!std::isfinite(fill_sdf) || !((double)fill_sdf >= iso_level)) {
    // a removed voxel has to be "outside" for marching cubes, or the fill would be interpolated
    set_error("vcy_keep_components: fill_sdf %g must be finite and not below the iso level %g", (double)fill_sdf, iso_level);
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  std::vector<vcy_component> comps;
  std::vector<int> slot;
  { const int rc = label_components(c, iso_level, &comps, &slot); if (rc != VCY_OK) return rc; }
  const size_t nc = comps.size();
  std::vector<uint8_t> removed(nc, 0);
  int64_t rc_n = 0, rv_n = 0;
  int keep0 = -1;
  for (size_t i = 0; i < nc; ++i) {
    const bool keep = (keep_largest <= 0 || (int64_t)i < (int64_t)keep_largest) && comps[i].n_voxels >= min_voxels;
    if (keep) {
      if (keep0 < 0) keep0 = (int)comps[i].label;
      continue;
    }
    removed[(size_t)slot[i]] = 1;
    ++rc_n;
    rv_n += comps[i].n_voxels;
  }
  if (rc_n > 0) {
    Stats* d_stats = (Stats*)c->d_cc_roots;
    const int* d_roots = (const int*)(d_stats + c->cc_roots_cap);
    uint8_t* d_removed = (uint8_t*)(d_roots + c->cc_roots_cap);
    VCY_HIP_CHECK(hipMemcpyAsync(d_removed, removed.data(), nc, hipMemcpyHostToDevice, c->stream));
    const int nbw = (c->nx + 7) / 8, nby = (c->ny + 7) / 8, nbz = (c->nz + 7) / 8;
    const int64_t nbricks = (int64_t)nbw * nby * nbz;
    float* bmin = c->brick_min_valid && c->d_brick_min ? c->d_brick_min : nullptr;
    hipLaunchKernelGGL(cc::cc_filter_kernel, dim3((unsigned)((nbricks + 3) / 4)), dim3(256), 0, c->stream, c->owned_slab_sdf(),
                       (const int*)c->d_cc_labels, c->nx, c->ny, c->nz, nbw, nby, nbricks, d_roots, (int)nc, d_removed, keep0,
                       fill_sdf, bmin);
    VCY_HIP_CHECK(hipGetLastError());
    // (the copy reads `removed` until the stream has passed it: finish_timer waits)
  }
  { const int rc = finish_timer(c); if (rc != VCY_OK) return rc; }
  if (removed_components) *removed_components = rc_n;
  if (removed_voxels) *removed_voxels = rv_n;
  return VCY_OK;
}

int vcy_last_components_ms(const vcy_ctx* c, float* device_ms) {
  if (!c || !device_ms) return VCY_ERR_INVALID_ARG;
  *device_ms = c->last_components_device_ms;
  return VCY_OK;
}

}  // extern "C"
