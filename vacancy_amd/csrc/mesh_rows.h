// The row table of the mesh operators (mesh_smooth.hip, mesh_normals.hip, mesh_decimate.hip): n_items items grouped by an
// integer key into n_rows rows, every row in ascending item id.  Built in five steps on one stream, no host wait between
// them: rows_count (one thread per item, integer atomicAdd into deg[key] -- counts do not depend on the order of the adds),
// the exclusive scan of mc_kernels.hip over the n_rows + 1 counts (row offsets), rows_offsets, rows_fill (one thread per
// item takes a slot of its row with an atomicAdd on a cursor -- slots come out in arbitrary order), and a sort of every row
// by one thread, so that whatever follows does not depend on the order the atomics ran in: rows_sort_kernel, or a kernel of
// the operator's own that goes on to use the sorted row (sm_rows_kernel, dc_rows_kernel).
#pragma once

#include <climits>

#include "vcy_internal.h"

namespace vcy {
namespace rows {

typedef unsigned long long u64;

struct Table {
  int n_rows, n_items;
  const int* key;       // [n_items] the row of every item
  u64* deg;             // [n_rows + 1] counts, scanned in place
  int* off;             // [n_rows + 1] row offsets
  int* cursor;          // [n_rows]
  int* items;           // [n_items] rows of item ids
  int* bad;             // CHECKED builds only: one word, set to 1 where a key lies outside [0, n_rows); that item has no row
};

// CHECKED: the keys come from the caller unverified (a mesh's face indices before the verdict on them is read)
template <bool CHECKED>
static __global__ __launch_bounds__(256) void rows_count_kernel(Table t) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= t.n_items) return;
  const int k = t.key[i];
  if (CHECKED && (k < 0 || k >= t.n_rows)) {
    *t.bad = 1;
    return;
  }
  atomicAdd(&t.deg[k], 1ull);
}

static __global__ __launch_bounds__(256) void rows_offsets_kernel(Table t) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > t.n_rows) return;
  const int o = (int)t.deg[r];
  t.off[r] = o;
  if (r < t.n_rows) t.cursor[r] = o;
}

template <bool CHECKED>
static __global__ __launch_bounds__(256) void rows_fill_kernel(Table t) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= t.n_items) return;
  const int k = t.key[i];
  if (CHECKED && (k < 0 || k >= t.n_rows)) return;  // (counted nowhere: the rows hold the other items, off[n_rows] of them)
  const int slot = atomicAdd(&t.cursor[k], 1);  // (< off[key + 1]: the row has a slot per item counted)
  t.items[slot] = (int)i;
}

// Counts, row offsets, and the items in their rows in arbitrary order.  `total`: one word, `scratch`: the scan's,
// scan_scratch_words(n_rows + 1) words.  `counted`: the caller has cleared t.deg and counted into it already.
template <bool CHECKED = false>
inline int fill(hipStream_t s, const Table& t, u64* total, u64* scratch, bool counted = false) {
  const size_t n = (size_t)t.n_rows, m = (size_t)t.n_items;
  const dim3 blk(256), grid_r1((unsigned)((n + 256) / 256)), grid_i((unsigned)((m + 255) / 256));
  if (!counted) {
    VCY_HIP_CHECK(hipMemsetAsync(t.deg, 0, 8 * (n + 1), s));
    if (m > 0) hipLaunchKernelGGL(rows_count_kernel<CHECKED>, grid_i, blk, 0, s, t);
  }
  { const int rc = device_exclusive_scan_u64(t.deg, (int64_t)n + 1, total, scratch, s); if (rc != VCY_OK) return rc; }
  hipLaunchKernelGGL(rows_offsets_kernel, grid_r1, blk, 0, s, t);
  if (m > 0) hipLaunchKernelGGL(rows_fill_kernel<CHECKED>, grid_i, blk, 0, s, t);
  VCY_HIP_CHECK(hipGetLastError());
  return VCY_OK;
}

// ---- sorting one row by one thread -----------------------------------------------------------------------------------
// a row of up to K ids into registers, ascending, INT_MAX behind them: odd-even transposition sort, every index static
template <int K>
__device__ __forceinline__ void load_sorted(const int* row, int len, int (&r)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) r[k] = k < len ? row[k] : INT_MAX;
#pragma unroll
  for (int round = 0; round < K; ++round) {
#pragma unroll
    for (int i = round & 1; i + 1 < K; i += 2) {
      const int lo = min(r[i], r[i + 1]), hi = max(r[i], r[i + 1]);
      r[i] = lo;
      r[i + 1] = hi;
    }
  }
}

// in place in global memory, ascending; any length; correct, not fast
__device__ inline void heap_sift(int* a, int i, int n) {
  for (;;) {
    const int l = 2 * i + 1;
    if (l >= n) return;
    const int r = l + 1;
    const int m = (r < n && a[r] > a[l]) ? r : l;
    const int ai = a[i], am = a[m];
    if (ai >= am) return;
    a[i] = am;
    a[m] = ai;
    i = m;
  }
}
__device__ inline void heap_sort(int* a, int n) {
  for (int i = n / 2 - 1; i >= 0; --i) heap_sift(a, i, n);
  for (int end = n - 1; end > 0; --end) {
    const int t = a[0];
    a[0] = a[end];
    a[end] = t;
    heap_sift(a, 0, end);
  }
}

template <int K>
__device__ __forceinline__ void sort_in_registers(int* row, int len) {
  int r[K];
  load_sorted<K>(row, len, r);
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (k < len) row[k] = r[k];
}

// in place: in registers up to K1 ids, by a second, wider network up to K2 (0: there is none), beyond that the heap sort
template <int K1, int K2 = 0>
__device__ __forceinline__ void sort_row(int* row, int len) {
  if (len <= K1) return sort_in_registers<K1>(row, len);
  if constexpr (K2 > 0) {
    if (len <= K2) return sort_in_registers<K2>(row, len);
  }
  heap_sort(row, len);
}

// for callers that need the sorted rows and nothing else
template <int K1>
__global__ __launch_bounds__(256) void rows_sort_kernel(Table t) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= t.n_rows) return;
  const int b = t.off[r];
  sort_row<K1>(t.items + b, t.off[r + 1] - b);
}

}  // namespace rows
}  // namespace vcy
