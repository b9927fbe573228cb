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
//
// A grid cut into z-slabs (vcy_label_components_slab and what follows it in vacancy_hip.h): every slab runs steps 1 - 5
// over its own slices -- per-voxel storage stays a 32-bit slab-local index, everything reported is a 64-bit global id
// (z_begin * nx * ny + the local one) --, then
//   7. cc_seam_pairs   on the upper slab of a seam, one wave per 64-voxel word of its first plane: the labels of the lower
//                      slab's top plane (nx * ny int64, through host memory) against its own; one (lower, upper) pair per
//                      maximal stretch of x where both are solid -- inside such a stretch either side is one run, so one
//                      piece.  One wave-aggregated atomicAdd per word for the output slots.
// and the host joins the slabs' pieces (vcy_merge_components_host: union-find over the 64-bit provisional labels).  What
// crosses a seam is that plane and the pairs, never a slab's label volume.  The filter on a slab is cc_filter over the
// slab's own bricks with the removal flags the merged list gives.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "slab_rules.h"
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

// One wave per 64-voxel word of the slab's first plane, a lane per voxel.  `below[v]`: the label the slab below gave the
// voxel under v (global, -1: not solid); `label`: this slab's own (slab-local, -1: not solid).  A pair goes out at the
// first voxel of every maximal stretch of x in which both are solid; the stretch that continues from the previous word
// has gone out there (the carry, as in cc_merge_kernel).  *n_pairs counts every pair, stored or not: the host comes
// again with a larger list when it did not fit.
__global__ __launch_bounds__(256) void cc_seam_pairs_kernel(const int* __restrict__ label, const int64_t* __restrict__ below,
                                                            int nx, int Wr, int nwords, int64_t id0, int64_t* __restrict__ pairs,
                                                            unsigned int cap, unsigned int* __restrict__ n_pairs) {
  const int lane = threadIdx.x & 63;
  for (int wi = blockIdx.x * 4 + (threadIdx.x >> 6); wi < nwords; wi += gridDim.x * 4) {  // (uniform per wave)
    const int y = wi / Wr, w = wi - y * Wr;
    const int x = w * 64 + lane;
    int own = -1;
    int64_t low = -1;
    if (x < nx) {
      own = label[(int64_t)y * nx + x];
      low = below[(int64_t)y * nx + x];
    }
    const u64 both = __ballot(own >= 0 && low >= 0);
    if (both == 0ull) continue;
    bool left = false;  // the voxel before the word: lane 0 looks
    if (lane == 0 && w > 0) left = label[(int64_t)y * nx + x - 1] >= 0 && below[(int64_t)y * nx + x - 1] >= 0;
    const u64 carry = __ballot(left) & 1ull;
    const u64 starts = both & ~((both << 1) | carry);
    if (starts == 0ull) continue;
    const int first = __builtin_ctzll(starts);
    unsigned int base = 0;
    if (lane == first) base = atomicAdd(n_pairs, (unsigned int)__builtin_popcountll(starts));
    base = __shfl(base, first, 64);
    if ((starts >> lane) & 1ull) {
      const unsigned int k = base + (unsigned int)__builtin_popcountll(starts & ((1ull << lane) - 1ull));
      if (k < cap) {
        pairs[2 * (int64_t)k] = low;
        pairs[2 * (int64_t)k + 1] = id0 + own;
      }
    }
  }
}

}  // namespace cc

using cc::Stats;

namespace {

bool whole_grid(const vcy_ctx* c) { return c->z0 == 0 && c->z1 == c->nz && c->halo_lo == 0; }

}  // namespace

// Step 1 (vcy_internal.h): also the first kernel of the ray-cast of the hull.
int launch_solid_bits(vcy_ctx* c, double iso, unsigned long long* bits) {
  const int nx = c->nx, Wr = (nx + 63) / 64;
  const int64_t nwords = (int64_t)Wr * c->ny * c->nz_local();
  const float* sdf = c->owned_slab_sdf();
  const void* cnt = c->owned_slab_cnt();
  const dim3 grid((unsigned)((nwords + 4 * cc::kBitsWordsPerWave - 1) / (4 * cc::kBitsWordsPerWave)));
#define VCY_CC_BITS(T, IMPL) \
  hipLaunchKernelGGL((cc::cc_bits_kernel<T, IMPL>), grid, dim3(256), 0, c->stream, sdf, (const T*)cnt, nx, Wr, nwords, iso, bits)
  if (c->st.cnt_implied) VCY_CC_BITS(uint8_t, true);
  else if (c->cnt_bytes == 1) VCY_CC_BITS(uint8_t, false);
  else if (c->cnt_bytes == 2) VCY_CC_BITS(uint16_t, false);
  else VCY_CC_BITS(uint32_t, false);
#undef VCY_CC_BITS
  VCY_HIP_CHECK(hipGetLastError());
  return VCY_OK;
}

// Steps 1 - 5.  `comps` in the order of the header (n_voxels descending, label ascending); `slot_of_comp[i]` = where
// component i's root stands in the sorted root list the device holds (cc_roots).  The begin event is recorded here, the
// end event by the caller.
// Runs over the slices the context owns: on a z-slab the labels and the boxes are global (z_begin added), the pieces
// those of the slab alone.
static int label_components(vcy_ctx* c, double iso, std::vector<vcy_component>* comps, std::vector<int>* slot_of_comp) {
  comps->clear();
  if (slot_of_comp) slot_of_comp->clear();
  c->st.labelling_dropped();
  c->cc_roots_host.clear();
  c->cc_nvox_host.clear();
  c->cc_global_host.clear();
  c->last_components_device_ms = 0.0f;
  c->cc_timed = false;
  { const int rcf = flush_pending(c); if (rcf != VCY_OK) return rcf; }
  c->cc_labels_valid = true;
  c->cc_n_roots = 0;
  if (c->st.fresh) {  // nothing carved since the fill: no voxel is solid, and the lazy fill stays lazy
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
  const int64_t nwords = (int64_t)Wr * ny * c->nz_local();
  VCY_HIP_CHECK(c->d_cc_labels.grow(sizeof(int) * (size_t)n, c->stream, false));
  VCY_HIP_CHECK(c->d_cc_bits.grow(sizeof(cc::u64) * (size_t)nwords + 64, c->stream, false));
  if (c->cc_roots_cap == 0) {
    VCY_HIP_CHECK(c->d_cc_roots.grow((size_t)(1 << 16) * (sizeof(int) + sizeof(Stats) + 1), c->stream, false));
    c->cc_roots_cap = 1 << 16;
  }
  if (!c->h_cc_report) VCY_HIP_CHECK(c->h_cc_report.alloc(64));
  VCY_HIP_CHECK(c->ev_cc_begin.ensure());
  VCY_HIP_CHECK(c->ev_cc_end.ensure());
  int* label = (int*)c->d_cc_labels;
  cc::u64* bits = (cc::u64*)c->d_cc_bits;
  unsigned int* d_nroots = (unsigned int*)(bits + nwords);  // (the 64 bytes behind the words)

  VCY_HIP_CHECK(hipEventRecord(c->ev_cc_begin, c->stream));
  c->cc_timed = true;
  VCY_HIP_CHECK(hipMemsetAsync(d_nroots, 0, 64, c->stream));
  { const int rc = launch_solid_bits(c, iso, bits); if (rc != VCY_OK) return rc; }
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
    const hipError_t eg = c->d_cc_roots.grow((size_t)n_roots * (sizeof(int) + sizeof(Stats) + 1), c->stream, false);
    if (eg != hipSuccess) c->cc_roots_cap = 0;
    VCY_HIP_CHECK(eg);
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
  const int64_t id0 = (int64_t)c->z0 * c->slice;
  for (size_t i = 0; i < order.size(); ++i) {
    const size_t s = (size_t)order[i];
    vcy_component& o = (*comps)[i];
    o.label = id0 + roots[s];
    o.n_voxels = (int64_t)stats[s].n;
    for (int k = 0; k < 3; ++k) o.bb_min[k] = stats[s].mn[k], o.bb_max[k] = stats[s].mx[k];
    o.bb_min[2] += c->z0, o.bb_max[2] += c->z0;
  }
  if (slot_of_comp) *slot_of_comp = order;
  c->cc_nvox_host.resize((size_t)n_roots);
  for (size_t s = 0; s < (size_t)n_roots; ++s) c->cc_nvox_host[s] = (int64_t)stats[s].n;
  c->cc_roots_host.swap(roots);
  return VCY_OK;
}

static int finish_timer(vcy_ctx* c) {
  if (!c->cc_timed) return VCY_OK;
  VCY_HIP_CHECK(hipEventRecord(c->ev_cc_end, c->stream));
  VCY_HIP_CHECK(hipEventSynchronize(c->ev_cc_end));
  VCY_HIP_CHECK(hipEventElapsedTime(&c->last_components_device_ms, c->ev_cc_begin, c->ev_cc_end));
  return VCY_OK;
}

// Step 6 over the bricks of the owned slices (bricks are slab-local, as the fused carve's: z_begin need not be a multiple
// of 8).  removed[slot]: in the order of the sorted root list; keep0: a slab-local root that stays, or -1.
static int launch_filter(vcy_ctx* c, const std::vector<uint8_t>& removed, int keep0, float fill_sdf) {
  const size_t nc = removed.size();
  Stats* d_stats = (Stats*)c->d_cc_roots;
  const int* d_roots = (const int*)(d_stats + c->cc_roots_cap);
  uint8_t* d_removed = (uint8_t*)(d_roots + c->cc_roots_cap);
  VCY_HIP_CHECK(hipMemcpyAsync(d_removed, removed.data(), nc, hipMemcpyHostToDevice, c->stream));
  const int nzl = c->nz_local();
  const int nbw = (c->nx + 7) / 8, nby = (c->ny + 7) / 8, nbz = (nzl + 7) / 8;
  const int64_t nbricks = (int64_t)nbw * nby * nbz;
  float* bmin = c->st.brick_min_valid && c->d_brick_min ? c->d_brick_min : nullptr;
  // solid voxels go: the ray-cast's bit planes and a slab's labelling are stale, and so are the two slices the slab above
  // keeps of this one.  The kernel keeps the brick minima where they were valid.
  c->st.written(StateWrite::filter());
  hipLaunchKernelGGL(cc::cc_filter_kernel, dim3((unsigned)((nbricks + 3) / 4)), dim3(256), 0, c->stream, c->owned_slab_sdf(),
                     (const int*)c->d_cc_labels, c->nx, c->ny, nzl, nbw, nby, nbricks, d_roots, (int)nc, d_removed, keep0,
                     fill_sdf, bmin);
  VCY_HIP_CHECK(hipGetLastError());
  return VCY_OK;
}

static int check_owner(const vcy_ctx* c, const char* who) {
  if (whole_grid(c)) return VCY_OK;
  // a component may continue in the neighbouring slab: vcy_label_components_slab and the seam merge are the calls for it
  set_error("%s: the context owns z [%d, %d) of %d slices; components need the whole grid in one context "
            "(a z-slab: vcy_label_components_slab)", who, c->z0, c->z1, c->nz);
  return VCY_ERR_UNSUPPORTED;
}

// where a slab-local root stands in the sorted root list, or -1
static int host_slot_of(const vcy_ctx* c, int64_t root) {
  const std::vector<int>& r = c->cc_roots_host;
  if (root < 0 || root > 0x7fffffffLL) return -1;
  const auto it = std::lower_bound(r.begin(), r.end(), (int)root);
  return it != r.end() && *it == (int)root ? (int)(it - r.begin()) : -1;
}

// the seam calls need the labelling vcy_label_components_slab left, of the state as it is now
static int check_slab_labelled(const vcy_ctx* c, const char* who) {
  if (c->st.seams_current(c->pending.empty()) && c->cc_labels_valid) return VCY_OK;
  set_error("%s: vcy_label_components_slab has not labelled this context as its state is now: label again", who);
  return VCY_ERR_INVALID_ARG;
}

namespace {

struct UnionFind {  // over indices; a set's root is its smallest index
  std::vector<int64_t> p;
  explicit UnionFind(size_t n) : p(n) {
    for (size_t i = 0; i < n; ++i) p[i] = (int64_t)i;
  }
  int64_t find(int64_t i) {
    while (p[(size_t)i] != i) i = p[(size_t)i] = p[(size_t)p[(size_t)i]];
    return i;
  }
  void unite(int64_t a, int64_t b) {
    a = find(a), b = find(b);
    if (a == b) return;
    if (a < b) p[(size_t)b] = a;
    else p[(size_t)a] = b;
  }
};

}  // namespace

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
  if (!c->cc_global_host.empty()) {  // the merged labels (vcy_resolve_components_slab); neighbours mostly share a root
    int last = -1;
    int64_t last_global = -1;
    for (int64_t i = 0; i < n; ++i) {
      const int r = raw[(size_t)i];
      if (r != last) {
        last = r;
        last_global = r < 0 ? -1 : c->cc_global_host[(size_t)host_slot_of(c, r)];
      }
      labels[i] = last_global;
    }
    return VCY_OK;
  }
  const int64_t id0 = (int64_t)c->z0 * c->slice;  // (0 on a whole grid)
  for (int64_t i = 0; i < n; ++i) labels[i] = raw[(size_t)i] < 0 ? -1 : id0 + raw[(size_t)i];
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
  std::vector<uint8_t> gone(nc), removed(nc, 0);  // by rank in the list, by the filter's slot
  int64_t rc_n = 0, rv_n = 0;
  slab::select_components(comps.data(), (int64_t)nc, keep_largest, min_voxels, gone.data(), &rc_n, &rv_n);
  int keep0 = -1;
  for (size_t i = 0; i < nc; ++i) {
    if (gone[i]) removed[(size_t)slot[i]] = 1;
    else if (keep0 < 0) keep0 = (int)comps[i].label;
  }
  if (rc_n > 0) {
    const int rc = launch_filter(c, removed, keep0, fill_sdf);
    if (rc != VCY_OK) return rc;
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

/* ---- z-slabs ---------------------------------------------------------------------------------------------------- */

int vcy_label_components_slab(vcy_ctx* c, double iso_level, vcy_component** out, int64_t* n_out) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!out || !n_out) {
    set_error("vcy_label_components_slab: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  *out = nullptr;
  *n_out = 0;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  std::vector<vcy_component> comps;
  { const int rc = label_components(c, iso_level, &comps, nullptr); if (rc != VCY_OK) return rc; }
  { const int rc = finish_timer(c); if (rc != VCY_OK) return rc; }
  c->st.slab_labelled(iso_level);
  if (comps.empty()) return VCY_OK;
  vcy_component* p = (vcy_component*)std::malloc(sizeof(vcy_component) * comps.size());
  if (!p) {
    set_error("vcy_label_components_slab: out of host memory");
    return VCY_ERR_INTERNAL;
  }
  std::memcpy(p, comps.data(), sizeof(vcy_component) * comps.size());
  *out = p;
  *n_out = (int64_t)comps.size();
  return VCY_OK;
}

int vcy_component_top_plane(vcy_ctx* c, int64_t* plane_labels) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!plane_labels) {
    set_error("vcy_component_top_plane: null pointer");
    return VCY_ERR_INVALID_ARG;
  }
  { const int rc = check_slab_labelled(c, "vcy_component_top_plane"); if (rc != VCY_OK) return rc; }
  const int64_t slice = c->slice;
  if (c->cc_labels_empty || c->cc_n_roots == 0) {
    for (int64_t i = 0; i < slice; ++i) plane_labels[i] = -1;
    return VCY_OK;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  std::vector<int> raw((size_t)slice);
  const int64_t first = slice * (int64_t)(c->nz_local() - 1);
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  VCY_HIP_CHECK(hipMemcpy(raw.data(), (const int*)c->d_cc_labels + first, sizeof(int) * (size_t)slice, hipMemcpyDeviceToHost));
  const int64_t id0 = (int64_t)c->z0 * slice;
  for (int64_t i = 0; i < slice; ++i) plane_labels[i] = raw[(size_t)i] < 0 ? -1 : id0 + raw[(size_t)i];
  return VCY_OK;
}

int vcy_component_seam_pairs(vcy_ctx* c, const int64_t* below_plane_labels, int64_t** pairs_out, int64_t* n_pairs_out) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!below_plane_labels || !pairs_out || !n_pairs_out) {
    set_error("vcy_component_seam_pairs: null pointer");
    return VCY_ERR_INVALID_ARG;
  }
  *pairs_out = nullptr;
  *n_pairs_out = 0;
  if (c->z0 == 0) {
    set_error("vcy_component_seam_pairs: the context starts at slice 0: there is no seam below it");
    return VCY_ERR_INVALID_ARG;
  }
  { const int rc = check_slab_labelled(c, "vcy_component_seam_pairs"); if (rc != VCY_OK) return rc; }
  c->last_components_device_ms = 0.0f;
  c->cc_timed = false;
  if (c->cc_labels_empty || c->cc_n_roots == 0) return VCY_OK;  // nothing solid above the seam
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const int nx = c->nx, ny = c->ny, Wr = (nx + 63) / 64;
  const int nwords = Wr * ny;
  const size_t plane_bytes = sizeof(int64_t) * (size_t)c->slice;
  // a pair per stretch: a word of 64 voxels starts at most 32; the first guess is far smaller than that bound
  size_t cap = std::max<size_t>(4096, (size_t)nwords * 2);
  std::vector<int64_t> pairs;
  unsigned int* h_report = (unsigned int*)c->h_cc_report;
  for (int attempt = 0; attempt < 2; ++attempt) {
    VCY_HIP_CHECK(c->d_cc_seam.grow(plane_bytes + 64 + 2 * sizeof(int64_t) * cap, c->stream, false));
    int64_t* d_below = (int64_t*)c->d_cc_seam;
    unsigned int* d_n = (unsigned int*)((char*)c->d_cc_seam + plane_bytes);
    int64_t* d_pairs = (int64_t*)((char*)c->d_cc_seam + plane_bytes + 64);
    if (attempt == 0) {
      VCY_HIP_CHECK(hipEventRecord(c->ev_cc_begin, c->stream));
      c->cc_timed = true;
    }
    VCY_HIP_CHECK(hipMemcpyAsync(d_below, below_plane_labels, plane_bytes, hipMemcpyHostToDevice, c->stream));
    VCY_HIP_CHECK(hipMemsetAsync(d_n, 0, 64, c->stream));
    hipLaunchKernelGGL(cc::cc_seam_pairs_kernel, dim3((unsigned)std::min(2048, (nwords + 3) / 4)), dim3(256), 0, c->stream,
                       (const int*)c->d_cc_labels, d_below, nx, Wr, nwords, (int64_t)c->z0 * c->slice, d_pairs,
                       (unsigned int)cap, d_n);
    VCY_HIP_CHECK(hipGetLastError());
    VCY_HIP_CHECK(hipMemcpyAsync(h_report, d_n, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)h_report[0];
    if (n > cap) {  // (a checkerboard of a plane: the list did not fit; once more into one that does)
      cap = n;
      continue;
    }
    pairs.resize(2 * n);
    if (n) VCY_HIP_CHECK(hipMemcpy(pairs.data(), d_pairs, 2 * sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    break;
  }
  { const int rc = finish_timer(c); if (rc != VCY_OK) return rc; }
  const size_t n = pairs.size() / 2;
  if (n == 0) return VCY_OK;
  // the order the atomics gave is not part of the result: sorted, every pair once
  std::vector<std::pair<int64_t, int64_t>> uniq(n);
  for (size_t i = 0; i < n; ++i) uniq[i] = {pairs[2 * i], pairs[2 * i + 1]};
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  int64_t* p = (int64_t*)std::malloc(2 * sizeof(int64_t) * uniq.size());
  if (!p) {
    set_error("vcy_component_seam_pairs: out of host memory");
    return VCY_ERR_INTERNAL;
  }
  for (size_t i = 0; i < uniq.size(); ++i) p[2 * i] = uniq[i].first, p[2 * i + 1] = uniq[i].second;
  *pairs_out = p;
  *n_pairs_out = (int64_t)uniq.size();
  return VCY_OK;
}

void vcy_seam_pairs_free(int64_t* pairs) { std::free(pairs); }

int vcy_resolve_components_slab(vcy_ctx* c, int64_t n, const int64_t* provisional_labels, const int64_t* global_labels) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  { const int rc = check_slab_labelled(c, "vcy_resolve_components_slab"); if (rc != VCY_OK) return rc; }
  const size_t nr = c->cc_roots_host.size();
  if (n < 0 || (n > 0 && (!provisional_labels || !global_labels)) || (size_t)n != nr) {
    set_error("vcy_resolve_components_slab: the map has %lld entries, the slab reported %lld components", (long long)n,
              (long long)nr);
    return VCY_ERR_INVALID_ARG;
  }
  const int64_t id0 = (int64_t)c->z0 * c->slice;
  std::vector<int64_t> global(nr, -1);
  for (int64_t i = 0; i < n; ++i) {
    const int slot = host_slot_of(c, provisional_labels[i] - id0);
    if (slot < 0 || global[(size_t)slot] >= 0 || global_labels[i] < 0 || global_labels[i] > provisional_labels[i]) {
      set_error("vcy_resolve_components_slab: entry %lld (%lld -> %lld): %s", (long long)i, (long long)provisional_labels[i],
                (long long)global_labels[i],
                slot < 0 ? "the slab reported no component with this label"
                         : global[(size_t)slot] >= 0 ? "the label is named twice"
                                                     : "a merged label is the smallest of its set: not negative, not above the piece's own");
      return VCY_ERR_INVALID_ARG;  // (the installed map, if any, stays)
    }
    global[(size_t)slot] = global_labels[i];
  }
  c->cc_global_host.swap(global);
  return VCY_OK;
}

int vcy_keep_components_slab(vcy_ctx* c, float fill_sdf, int64_t n_remove, const int64_t* remove_provisional_labels,
                             int64_t* removed_voxels) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (removed_voxels) *removed_voxels = 0;
  { const int rc = check_slab_labelled(c, "vcy_keep_components_slab"); if (rc != VCY_OK) return rc; }
  if (!std::isfinite(fill_sdf) || !((double)fill_sdf >= c->st.cc_iso)) {
    set_error("vcy_keep_components_slab: fill_sdf %g must be finite and not below the iso level %g of the labelling",
              (double)fill_sdf, c->st.cc_iso);
    return VCY_ERR_INVALID_ARG;
  }
  if (n_remove < 0 || (n_remove > 0 && !remove_provisional_labels)) {
    set_error("vcy_keep_components_slab: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  const size_t nr = c->cc_roots_host.size();
  const int64_t id0 = (int64_t)c->z0 * c->slice;
  std::vector<uint8_t> removed(nr, 0);
  int64_t rv_n = 0;
  for (int64_t i = 0; i < n_remove; ++i) {
    const int slot = host_slot_of(c, remove_provisional_labels[i] - id0);
    if (slot < 0) {
      set_error("vcy_keep_components_slab: the slab reported no component with the label %lld",
                (long long)remove_provisional_labels[i]);
      return VCY_ERR_INVALID_ARG;
    }
    if (!removed[(size_t)slot]) rv_n += c->cc_nvox_host[(size_t)slot];
    removed[(size_t)slot] = 1;
  }
  c->last_components_device_ms = 0.0f;
  c->cc_timed = false;
  if (rv_n > 0) {
    int keep0 = -1;  // the largest piece that stays
    int64_t best = 0;
    for (size_t s = 0; s < nr; ++s)
      if (!removed[s] && c->cc_nvox_host[s] > best) best = c->cc_nvox_host[s], keep0 = c->cc_roots_host[s];
    VCY_HIP_CHECK(hipSetDevice(c->device));
    VCY_HIP_CHECK(hipEventRecord(c->ev_cc_begin, c->stream));
    c->cc_timed = true;
    { const int rc = launch_filter(c, removed, keep0, fill_sdf); if (rc != VCY_OK) return rc; }
    { const int rc = finish_timer(c); if (rc != VCY_OK) return rc; }  // (waits: `removed` is read until then)
    // (the labels stay those from before the removal (vcy_download_labels), but no second filter may lean on them: the
    // filter's own write has made the labelling stale)
  }
  // step 5 of the slab flow: the slab below has run its own filter as well, so the two slices kept from it are stale
  // whether or not anything went HERE -- as after a carve, extraction refuses until the halos are exchanged again
  c->st.halo_stale();
  if (removed_voxels) *removed_voxels = rv_n;
  return VCY_OK;
}

int vcy_merge_components_host(int n_slabs, const vcy_component* lists, const int64_t* n_lists, const int64_t* pairs,
                              const int64_t* n_pairs, vcy_component** merged_out, int64_t* n_merged_out,
                              int64_t* global_labels) {
  if (merged_out) *merged_out = nullptr;
  if (n_merged_out) *n_merged_out = 0;
  if (n_slabs < 1 || !n_lists || !merged_out || !n_merged_out || (n_slabs > 1 && !n_pairs)) {
    set_error("vcy_merge_components_host: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  std::vector<int64_t> first((size_t)n_slabs + 1, 0);  // slab s: entries [first[s], first[s + 1]) of `lists`
  for (int s = 0; s < n_slabs; ++s) {
    if (n_lists[s] < 0 || (s + 1 < n_slabs && n_pairs[s] < 0)) {
      set_error("vcy_merge_components_host: a negative count");
      return VCY_ERR_INVALID_ARG;
    }
    first[(size_t)s + 1] = first[(size_t)s] + n_lists[s];
  }
  const int64_t total = first[(size_t)n_slabs];
  if (total == 0) {
    for (int s = 0; s + 1 < n_slabs; ++s)
      if (n_pairs[s] > 0) {
        set_error("vcy_merge_components_host: seam %d has pairs, but no slab reported a component", s);
        return VCY_ERR_INVALID_ARG;
      }
    return VCY_OK;
  }
  if (!lists || !global_labels) {
    set_error("vcy_merge_components_host: null pointer");
    return VCY_ERR_INVALID_ARG;
  }
  // entries ordered by label per slab: the lookup of a pair's two ends
  std::vector<std::vector<std::pair<int64_t, int64_t>>> by_label((size_t)n_slabs);  // (label, entry)
  for (int s = 0; s < n_slabs; ++s) {
    auto& v = by_label[(size_t)s];
    v.reserve((size_t)n_lists[s]);
    for (int64_t i = first[(size_t)s]; i < first[(size_t)s + 1]; ++i) v.push_back({lists[i].label, i});
    std::sort(v.begin(), v.end());
    for (size_t i = 1; i < v.size(); ++i)
      if (v[i].first == v[i - 1].first) {
        set_error("vcy_merge_components_host: slab %d reports the label %lld twice", s, (long long)v[i].first);
        return VCY_ERR_INVALID_ARG;
      }
  }
  auto entry_of = [&](int s, int64_t label) -> int64_t {
    const auto& v = by_label[(size_t)s];
    const auto it = std::lower_bound(v.begin(), v.end(), std::make_pair(label, (int64_t)-1));
    return it != v.end() && it->first == label ? it->second : -1;
  };
  UnionFind uf((size_t)total);
  const int64_t* pr = pairs;
  for (int s = 0; s + 1 < n_slabs; ++s) {
    if (n_pairs[s] > 0 && !pairs) {
      set_error("vcy_merge_components_host: null pointer");
      return VCY_ERR_INVALID_ARG;
    }
    for (int64_t k = 0; k < n_pairs[s]; ++k, pr += 2) {
      const int64_t a = entry_of(s, pr[0]), b = entry_of(s + 1, pr[1]);
      if (a < 0 || b < 0) {
        set_error("vcy_merge_components_host: pair %lld of seam %d names the label %lld, which slab %d did not report",
                  (long long)k, s, (long long)(a < 0 ? pr[0] : pr[1]), a < 0 ? s : s + 1);
        return VCY_ERR_INVALID_ARG;
      }
      uf.unite(a, b);
    }
  }
  // per set: the smallest label, the sum, the joined box -- gathered at the set's root entry
  std::vector<vcy_component> acc((size_t)total);
  std::vector<char> seen((size_t)total, 0);
  for (int64_t i = 0; i < total; ++i) {
    const size_t r = (size_t)uf.find(i);
    if (!seen[r]) {
      seen[r] = 1;
      acc[r] = lists[i];
      continue;
    }
    vcy_component& o = acc[r];
    o.label = std::min(o.label, lists[i].label);
    o.n_voxels += lists[i].n_voxels;
    for (int k = 0; k < 3; ++k) {
      o.bb_min[k] = std::min(o.bb_min[k], lists[i].bb_min[k]);
      o.bb_max[k] = std::max(o.bb_max[k], lists[i].bb_max[k]);
    }
  }
  std::vector<vcy_component> merged;
  for (int64_t i = 0; i < total; ++i)
    if (uf.find(i) == i) merged.push_back(acc[(size_t)i]);
  for (int64_t i = 0; i < total; ++i) global_labels[i] = acc[(size_t)uf.find(i)].label;
  std::sort(merged.begin(), merged.end(), [](const vcy_component& a, const vcy_component& b) {
    if (a.n_voxels != b.n_voxels) return a.n_voxels > b.n_voxels;
    return a.label < b.label;
  });
  vcy_component* p = (vcy_component*)std::malloc(sizeof(vcy_component) * merged.size());
  if (!p) {
    set_error("vcy_merge_components_host: out of host memory");
    return VCY_ERR_INTERNAL;
  }
  std::memcpy(p, merged.data(), sizeof(vcy_component) * merged.size());
  *merged_out = p;
  *n_merged_out = (int64_t)merged.size();
  return VCY_OK;
}

int vcy_select_components_host(const vcy_component* components, int64_t n_components, int keep_largest, int64_t min_voxels,
                               uint8_t* removed, int64_t* removed_components, int64_t* removed_voxels,
                               const int64_t* piece_global_labels, int64_t n_pieces, uint8_t* piece_removed) {
  if (removed_components) *removed_components = 0;
  if (removed_voxels) *removed_voxels = 0;
  if (n_components < 0 || n_pieces < 0 || (n_components > 0 && (!components || !removed)) ||
      (n_pieces > 0 && (!piece_global_labels || !piece_removed))) {
    set_error("vcy_select_components_host: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  int64_t rc_n = 0, rv_n = 0;
  slab::select_components(components, n_components, keep_largest, min_voxels, removed, &rc_n, &rv_n);
  slab::select_pieces(components, n_components, removed, piece_global_labels, n_pieces, piece_removed);
  if (removed_components) *removed_components = rc_n;
  if (removed_voxels) *removed_voxels = rv_n;
  return VCY_OK;
}

}  // extern "C"
