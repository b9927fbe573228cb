// Host program of tests/test_footprint_unpack_host.py (compiled as HIP, host side only; no GPU, no device code).
// A footprint record is read in two ways (vacancy_amd/csrc/carve_fused.h): unpack_footprint makes a TileInfo of it, and the
// carve kernels that keep their records in registers take the same two words apart as integers -- footprint_ub_word,
// footprint_ub, unpack_footprint_scalar, footprint_base, footprint_bounds, and the constant pitch of a raw tile.  Both
// must yield the same bits for every record, including the ones the pre-pass never writes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "carve_fused.h"

static uint32_t bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

int main() {
  using namespace vcy;
  const uint32_t tws[] = {0, 1, 15}, ths[] = {0, 1, 15}, origins[] = {0, 1, 8190, 8191};
  // word 0's bound (bits 31..6): +-0, a negative and a positive finite value, +inf, and the largest finite float, whose
  // round-up to 26 bits carries into +inf (pack_footprint's `(b + 63) & ~63`)
  const uint32_t ubs[] = {0x00000000u, 0x80000000u, bits(-0.7312f) & ~63u, (bits(3.25e-3f) + 63u) & ~63u, 0x7f800000u,
                          (0x7f7fffffu + 63u) & ~63u};
  long cases = 0, bad = 0;
  auto check = [&](bool ok, const char* what, uint32_t w0, uint32_t w1) {
    if (!ok && bad++ < 20) std::printf("MISMATCH %s for record w0 = 0x%08x, w1 = 0x%08x\n", what, w0, w1);
  };
  for (uint32_t tw : tws)
    for (uint32_t th : ths)
      for (uint32_t tx0 : origins)
        for (uint32_t ty0 : origins)
          for (uint32_t sure = 0; sure < 4; ++sure)
            for (uint32_t edge = 0; edge < 4; ++edge)
              for (uint32_t ub : ubs) {
                FootprintRecord r;
                r.w0 = ub | th | (edge << 4);
                r.w1 = tx0 | (ty0 << 13) | (tw << 26) | (sure << 30);
                const TileInfo ti = unpack_footprint(r);
                const uint32_t word = footprint_ub_word(r.w0, r.w1);  // what a lane keeps of word 0
                const FootprintFields f = unpack_footprint_scalar(word, r.w1);
                const FootprintBounds b = footprint_bounds(f);
                ++cases;
                check(bits(footprint_ub(word)) == bits(ti.ub), "ub", r.w0, r.w1);
                check(f.tx0 == ti.tx0 && f.ty0 == ti.ty0, "tx0 / ty0", r.w0, r.w1);
                check(f.tw == ti.tw && f.th == ti.th && f.nq == ti.nq, "tw / th / nq", r.w0, r.w1);
                check(f.sure == ti.sure, "sure", r.w0, r.w1);
                check(footprint_base(f) == ti.base, "base", r.w0, r.w1);
                check(bits(b.lo_x) == bits(ti.lo_x) && bits(b.hi_x) == bits(ti.hi_x), "lo_x / hi_x", r.w0, r.w1);
                check(bits(b.lo_y) == bits(ti.lo_y) && bits(b.hi_y) == bits(ti.hi_y), "lo_y / hi_y", r.w0, r.w1);
                // The pitch: the kernel uses the constant kTileRaw.  It is TileInfo::pitchf of every record with a tile;
                // a record without one (pitchf 0) has no quads to fetch, is not `sure`, and no (u, w) passes its bounds,
                // so nothing is ever addressed with its pitch.
                if (tw) check(bits((float)kTileRaw) == bits(ti.pitchf), "pitchf", r.w0, r.w1);
                else check(f.nq == 0 && f.sure == 0 && !(b.lo_x <= b.hi_x) && !(b.lo_y <= b.hi_y), "no tile", r.w0, r.w1);
              }
  std::printf("%ld records, %ld mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
