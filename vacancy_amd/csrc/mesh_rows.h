// Sorting one row of ids by one thread: what the mesh operators (mesh_smooth.hip, mesh_decimate.hip) do after they have
// filled a row through an atomic cursor, so that whatever follows does not depend on the order the atomics ran in.
#pragma once

namespace vcy {
namespace sm {

// in place, ascending; one thread, any length
__device__ void heap_sift(int* a, int i, int n) {
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
__device__ void heap_sort(int* a, int n) {
  for (int i = n / 2 - 1; i >= 0; --i) heap_sift(a, i, n);
  for (int end = n - 1; end > 0; --end) {
    const int t = a[0];
    a[0] = a[end];
    a[end] = t;
    heap_sift(a, 0, end);
  }
}

}  // namespace sm
}  // namespace vcy
