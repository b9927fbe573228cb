// One half of the instances of carve_fused_kernel: update_num in ONE byte (what every BASELINE configuration runs: the
// counters are one byte until more than 255 views have been applied since the fill), behind launch_fused_counts8.
#include <cstring>

#include "carve_fused_kernel.h"

namespace vcy {
void launch_fused_counts8(const CarveLaunch& launch) { launch_fused<uint8_t>(launch); }
}  // namespace vcy

#ifdef VCY_PHASE_TIMING
// development build only (the benchmark's kernels are the one-byte ones): reads (and optionally clears) the phase counters
// of the fused kernel -- in THIS unit, whose copy of g_phase_ticks its kernels write
extern "C" int vcy_debug_phase_ticks(unsigned long long* out12, int reset) {
  unsigned long long h[256][16];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(vcy::g_phase_ticks), sizeof(h)) != hipSuccess) return -1;
  for (int q = 0; q < 16; ++q) {
    out12[q] = 0;
    for (int b = 0; b < 256; ++b) out12[q] += h[b][q];
  }
  if (reset) {
    std::memset(h, 0, sizeof(h));
    if (hipMemcpyToSymbol(HIP_SYMBOL(vcy::g_phase_ticks), h, sizeof(h)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
