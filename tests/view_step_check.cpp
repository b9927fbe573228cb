// Host program of tests/test_view_step_host.py (compiled as HIP, host side only; no GPU, no device code).
// The fused carve kernels that keep their footprint records in registers take the step between two views' runs on the
// scalar unit, with helpers of vacancy_amd/csrc/carve_fused.h that read a record's two words as integers and address the
// launch's tables with 32-bit byte offsets:
//   footprint_tile_word, footprint_has_tile, footprint_sure, footprint_tx0 / _ty0, footprint_step_base,
//   footprint_row_groups, footprint_window_unclamped; view_byte_offset, c0_view_bytes / c0_byte_offset,
//   tile_origin_bytes; and the host's guard of those offsets, carve_offsets_fit_32.
// Checked here against unpack_footprint (the TileInfo the other kernels use), field by field, over every edge value of
// every field and over random records; the clamp test against its two-sided form; the offsets against 64-bit arithmetic.
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

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

int main() {
  using namespace vcy;
  long cases = 0, bad = 0;
  auto check = [&](bool ok, const char* what, uint64_t a, uint64_t b) {
    if (!ok && bad++ < 20) std::printf("MISMATCH %s for 0x%llx, 0x%llx\n", what, (unsigned long long)a, (unsigned long long)b);
  };

  // ---- a record's fields ---------------------------------------------------------------------------------------
  auto check_record = [&](uint32_t w0, uint32_t w1) {
    FootprintRecord r;
    r.w0 = w0, r.w1 = w1;
    const TileInfo ti = unpack_footprint(r);
    const uint32_t ub_word = footprint_ub_word(w0, w1), tile_word = footprint_tile_word(w0, w1);
    const uint32_t tw = (w1 >> 26) & 15u, th = w0 & 15u;
    ++cases;
    // "has a tile" is "has quads to fetch"
    check(footprint_has_tile(tile_word) == (ti.nq != 0), "has_tile", w0, w1);
    if (ti.nq != 0) {
      check(tile_word == w1, "tile word", w0, w1);
      check(footprint_sure(tile_word) == ti.sure, "sure", w0, w1);
      check(footprint_tx0(tile_word) == ti.tx0 && footprint_ty0(tile_word) == ti.ty0, "tx0 / ty0", w0, w1);
      check(footprint_step_base(tile_word) == ti.base, "base", w0, w1);
      // the row groups: those raw_prefetch_rows requests, `4 r <= th` for r = 0 .. 3
      int groups = 0;
      for (int q = 0; q < 4; ++q) groups += (4 * q <= ti.th) ? 1 : 0;
      check(footprint_row_groups(ub_word) == groups, "row groups", w0, w1);
      check(footprint_row_groups(ub_word) == (unpack_footprint_scalar(ub_word, w1).th >> 2) + 1, "row groups (scalar)", w0, w1);
    } else if (tw == 0) {
      // no tile: every field reads what unpack_footprint gives a record without one
      check(tile_word == 0u, "tile word (no tile)", w0, w1);
      check(footprint_sure(tile_word) == ti.sure && ti.sure == 0, "sure (no tile)", w0, w1);
      check(footprint_step_base(tile_word) == ti.base && ti.base == 0, "base (no tile)", w0, w1);
      check(footprint_row_groups(ub_word) == 1, "row groups (no tile)", w0, w1);  // (never used: nothing is requested)
    } else {
      // tw != 0, th == 0: never packed (pack_footprint writes word 1 = 0 without quads); nothing to fetch, so "no tile"
      check(th == 0 && tile_word == 0u && !footprint_has_tile(tile_word) && footprint_sure(tile_word) == 0, "no quads",
            w0, w1);
    }
  };
  const uint32_t tws[] = {0, 1, 2, 14, 15}, ths[] = {0, 1, 3, 4, 7, 8, 11, 12, 15}, origins[] = {0, 1, 4095, 4096, 8190, 8191};
  const uint32_t ubs[] = {0x00000000u, 0x80000000u, bits(-0.7312f) & ~63u, (bits(3.25e-3f) + 63u) & ~63u, 0x7f800000u,
                          (0x7f7fffffu + 63u) & ~63u};
  for (uint32_t tw : tws)
    for (uint32_t th : ths)
      for (uint32_t tx0 : origins)
        for (uint32_t ty0 : origins)
          for (uint32_t sure = 0; sure < 4; ++sure)
            for (uint32_t edge = 0; edge < 4; ++edge)
              for (uint32_t ub : ubs)
                check_record(ub | th | (edge << 4), tx0 | (ty0 << 13) | (tw << 26) | (sure << 30));
  for (int i = 0; i < 400000; ++i) check_record(rnd(), rnd());  // (any two words, packed or not)
  // what pack_footprint writes for "no tile", and what a lane without a view holds
  check_record(0x7f800000u, 0u);
  const long record_cases = cases;

  // ---- the clamp test: one comparison for tx0 + 15 <= roi_max_xi && ty0 + 15 <= roi_max_yi --------------------------
  const int coords[] = {0, 1, 14, 15, 16, 17, 100, 4095, 8175, 8176, 8177, 8190, 8191};
  for (int tx0 : coords)
    for (int ty0 : coords)
      for (int rx : coords)
        for (int ry : coords) {
          ++cases;
          check(footprint_window_unclamped(tx0, ty0, rx, ry) == (tx0 + 15 <= rx && ty0 + 15 <= ry), "unclamped",
                ((uint64_t)tx0 << 16) | (uint64_t)ty0, ((uint64_t)rx << 16) | (uint64_t)ry);
        }
  for (int i = 0; i < 400000; ++i) {
    const int tx0 = (int)(rnd() & 8191u), ty0 = (int)(rnd() & 8191u);
    // (bounds near the origin + 15 as often as anywhere)
    const int rx = (rnd() & 1u) ? (int)(rnd() & 8191u) : tx0 + 15 + (int)(rnd() % 5u) - 2;
    const int ry = (rnd() & 1u) ? (int)(rnd() & 8191u) : ty0 + 15 + (int)(rnd() % 5u) - 2;
    ++cases;
    check(footprint_window_unclamped(tx0, ty0, rx, ry) == (tx0 + 15 <= rx && ty0 + 15 <= ry), "unclamped (random)",
          ((uint64_t)tx0 << 16) | (uint64_t)ty0, ((uint64_t)rx << 16) | (uint64_t)ry);
  }

  // ---- 32-bit byte offsets against 64-bit arithmetic -----------------------------------------------------------------
  for (int v = 0; v < kMaxFusedViews; ++v) {
    ++cases;
    check((uint64_t)view_byte_offset(v) == (uint64_t)v * sizeof(FusedView), "view offset", (uint64_t)v, 0);
  }
  const int widths[] = {1, 2, 16, 160, 1280, 8191, 8192};
  for (int w : widths)
    for (int tx0 : coords)
      for (int ty0 : coords) {
        ++cases;
        check((uint64_t)tile_origin_bytes((uint32_t)w, tx0, ty0) == ((uint64_t)w * (uint64_t)ty0 + (uint64_t)tx0) * 4ull,
              "tile origin", (uint64_t)w, ((uint64_t)tx0 << 16) | (uint64_t)ty0);
      }
  const uint64_t kRecBytes = (uint64_t)kC0Stride * sizeof(float);
  const int64_t guard_views[] = {1, 2, 31, 32, 63, 64}, guard_nbw[] = {1, 5, 128, 256, (1 << 18) - 1, 1 << 18, (1 << 18) + 1,
                                                                     (1 << 24) - 1, 1 << 24, (1ll << 31) - 1};
  for (int64_t nv : guard_views)
    for (int64_t nbw : guard_nbw) {
      ++cases;
      const bool fits = (uint64_t)nv * sizeof(FusedView) < (1ull << 31) && (uint64_t)nv * (uint64_t)nbw * kRecBytes < (1ull << 31);
      check(carve_offsets_fit_32(nv, nbw) == fits, "guard", (uint64_t)nv, (uint64_t)nbw);
      if (carve_offsets_fit_32(nv, nbw)) {  // then every offset of the launch is the 64-bit one, the last record's too
        const int views[] = {0, (int)nv / 2, (int)nv - 1};
        const int bricks[] = {0, (int)nbw / 2, (int)nbw - 1};
        const uint32_t per_view = c0_view_bytes((int)nbw);
        check((uint64_t)per_view == (uint64_t)nbw * kRecBytes, "c0 bytes per view", (uint64_t)nv, (uint64_t)nbw);
        for (int v : views)
          for (int b : bricks) {
            ++cases;
            const uint64_t want = ((uint64_t)v * (uint64_t)nbw + (uint64_t)b) * kRecBytes;
            check((uint64_t)c0_byte_offset(v, per_view, b) == want && want + kRecBytes <= (1ull << 31), "c0 offset",
                  (uint64_t)v, (uint64_t)b);
          }
      }
    }
  // the guard's own edges: negative counts, counts whose product leaves 64 bits
  ++cases;
  check(!carve_offsets_fit_32(-1, 4) && !carve_offsets_fit_32(4, -1) && !carve_offsets_fit_32(1ll << 40, 1ll << 40) &&
            !carve_offsets_fit_32(INT64_MAX, INT64_MAX) && carve_offsets_fit_32(0, 0) && carve_offsets_fit_32(64, 128),
        "guard edges", 0, 0);

  std::printf("%ld records, %ld cases, %ld mismatches\n", record_cases, cases, bad);
  return bad ? 1 : 0;
}
