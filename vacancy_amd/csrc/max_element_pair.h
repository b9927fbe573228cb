// The rule max_sdf is resolved by (include/vacancy_hip.h, VCY_OUTSIDE_MAX): exactly *std::max_element over the image.
// max_reduce_kernel (carve_kernels.hip) reduces (value, index) pairs with max_pair -- greater value first, then lower
// index: a total order on pairs whose value is no NaN, so the shape of the reduction tree does not matter -- and finishes
// with max_first_rule.  Host and device code; tests/fused_plan_host_check.cpp runs the kernel's two stages as host loops
// against std::max_element, also under the host sanitizers.
#pragma once

#include <cstdint>

#if defined(__HIP__)
#define VCY_MAX_PAIR_FN __host__ __device__ inline
#else
#define VCY_MAX_PAIR_FN inline
#endif

namespace vcy {

// (m, mi) becomes the better of itself and (v, vi).  False for a NaN v; m starts at -inf and so never is one.
// v == m holds for +0 against -0: the lower index decides, as std::max_element keeps the first of equal maxima.
VCY_MAX_PAIR_FN void max_pair(float& m, int64_t& mi, float v, int64_t vi) {
  if (v > m || (v == m && vi < mi)) {
    m = v;
    mi = vi;
  }
}

// std::max_element starts at the first element and moves on `*largest < *it`: nothing moves it off a NaN.
VCY_MAX_PAIR_FN float max_first_rule(float m, float first) { return first != first ? first : m; }

}  // namespace vcy
