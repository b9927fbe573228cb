// What the units of the fused carve step agree on: the geometry of a launch (tiles, workgroups, the few-view flavour)
// with its tuning defaults, the records that cross from the host and the pre-pass to carve_fused_kernel, the bits of
// `state_flags`, and the description of one launch (CarveLaunch).
//   carve_fused.h          this file
//   carve_fused_plan.h     the decisions of a launch as pure host code (plan_fused_launch), and the constants they share with the kernels
//   carve_fused_state.h    what a context keeps between launches (vcy_ctx::fused)
//   carve_fused_device.h   device helpers shared by the carve kernel and the pre-pass (sampling, tiles, footprints)
//   carve_fused_kernel.h   carve_fused_kernel and the dispatch that picks its instance
//   carve_fused_u8.hip     the instances with update_num in one byte, behind launch_fused_counts8
//   carve_fused_u16.hip    the instances with update_num in two bytes, behind launch_fused_counts16
//   carve_fused.hip        the host side (launch_carve_fused, the slab planner) and the pre-pass kernels
#pragma once
#include <algorithm>
#include <cstdint>

#include "carve_common.h"
#include "carve_fused_plan.h"

namespace vcy {

// (kWgWaves, BX / BY / BZ, WX, the few-view flavour's kRowMaxViews / kRowBricks / kRowWaves, kLiveEntryWords, the kState*
// bits, CarveFlavour and kUpdateWaUnitWeight: carve_fused_plan.h, which the host's launch plan shares)
constexpr int kMaxFusedViews = 64;         // one prologue lane per view
// Raw-pixel tile (the default: footprints up to 15 x 15 taps): 16 x 16 pixels of the image, pitch 16, 1 KB.
// The pixels go from global memory straight into LDS (global_load_lds_dword: lane L of the r-th load
// writes dword 64 r + L, i.e. pixel (L & 15, 4 r + (L >> 4))), two tiles per wave so that the next live
// view's footprint arrives while the current one is sampled -- no staging registers, no LDS stores, one
// address per PIXEL instead of four per quad.  A sample reads its four taps as two ds_read2_b32
// (offsets 0, 1 and 16, 17); columns / rows beyond the ROI repeat the edge pixel, which is the
// reference's clamp of x + 1 and y + 1 (voxel_carver.cc:51-66).
constexpr int kTileRaw = 16;
constexpr int kRawBuffers = 2;
template <int TQ>
constexpr int tile_f4_per_wave() { return TQ == kTileRaw ? kRawBuffers * 64 : TQ; }  // LDS of one wave, in float4
// The big tile: 8 KB per wave = 2048 raw pixels, pitch = width of the footprint, filled in place by LDS-direct
// loads (tile_fill; footprints up to ~44 x 44 pixels, voxels up to ~3 px); the second tap row is one address
// add away.
constexpr int kTileBig = 512;            // (in float4 units)
constexpr int kBigPixels = 4 * kTileBig;

// Cooperative write-back (kStateCoopStore, plan_fused_launch): the four waves of a workgroup hand their bricks' state
// to each other through LDS and every store instruction then writes whole 128-byte (sdf) / 64-byte (update_num) row
// segments instead of 64 scattered 16-byte pieces -- see the write-back of carve_fused_kernel.  Row pitches padded by
// 16 bytes so that the 16-byte LDS accesses of both directions spread over the banks.
constexpr int kCoopSdfPitch = 8 * VCY_WG_WAVES + 4;          // floats per row of the workgroup's 64 rows
template <typename CountT>
constexpr int coop_cnt_pitch() { return 8 * VCY_WG_WAVES + 16 / (int)sizeof(CountT); }  // counters per row
template <typename CountT>
constexpr size_t coop_lds_bytes() {
  return 64 * (size_t)kCoopSdfPitch * sizeof(float) + 64 * (size_t)coop_cnt_pitch<CountT>() * sizeof(CountT) +
         2 * VCY_WG_WAVES * sizeof(unsigned long long);  // (changed-lane masks, then "this wave takes part in the stores")
}

// ---- the few-view flavour (template parameter NB > 1 of carve_fused_kernel) -------------------------------------------
// The reference's own call pattern (examples.cc:117-149) carves ONE view per call, with an extraction in between: every
// view is a launch of its own, and such a launch spends more of a wave's life on the wave than on its 512 voxels -- block
// decode, axis loads, record unpack, tile request, barrier and write-back, 378 scalar + 290 vector instructions per brick
// next to the 290 of the voxels (profiles/r05/single_view_attribution.txt), on a CU with ONE scalar unit.  For launches of
// up to kRowMaxViews views a WAVE therefore walks NB consecutive bricks of one (y, z) row -- a "segment"; with NB = 4 the
// 32 x 8 x 8 block a workgroup of the NB = 1 kernel owns:
//   - block decode, axis loads, the records of all NB x nviews pairs (lane 8 j + v), the early-out test: once;
//   - the state of every live brick of the segment is requested up front with LDS-direct loads (global_load_lds: no
//     registers, no waits) into a staging area of the wave, and read from there when the brick's turn comes;
//   - ONE loop over the live (brick, view) pairs, in pair order: the tile of the next pair -- whether the next view of
//     this brick or the first live view of the next brick -- is in flight while this one is carved, exactly as the
//     NB = 1 kernel does between the views of its one brick;
//   - results go back to the staging area and leave it as whole row segments: 8 lanes store the 128 contiguous bytes
//     of sdf the segment has in one voxel row, 4 lanes its counters -- what the cooperative write-back gets from four
//     waves and a barrier, without the barrier.
// Waves never talk to each other; a workgroup is just kRowWaves of them.
// MEASURED (round 6, 1024^3 @1280x720, one view per launch; profiles/r06/row_kernel.txt): bit-identical to the NB = 1
// kernel, and SLOWER -- weighted average 3.17 ms per view against 2.63, first view 2.15 against 1.85, kMax 0.74 against
// 0.61.  The counters say why: a segment of four bricks costs 2062 vector + 1071 scalar instructions where four NB = 1
// waves cost 2400 + 1376 -- the decode, axis loads and barrier that are amortised were a seventh of the overhead, the
// rest is per brick and per pair whoever walks them -- while the staging area (14 KB per wave) leaves 2.7 waves per SIMD
// where the NB = 1 kernel has 5.7, and the run loops need the other waves to cover their LDS and scalar-load latencies.
// Two bricks per wave and four waves per workgroup (8 KB, 5 waves per SIMD) come closest (2.91 / 1.91 / 0.67 ms) and
// amortise next to nothing (592 + 324 per brick); workgroups of one or two waves are slower again (dispatch rate).
// So the flavour is OFF by default ("rowkernel" 0), kept and tested as the second implementation of few-view launches.
template <typename CountT, int NB>
constexpr size_t row_lds_bytes_per_wave() {  // two raw tiles, NB x 8 TileInfo, the state of NB bricks, NB changed-lane masks
  return (size_t)kRawBuffers * 1024 + (size_t)NB * kRowMaxViews * 56 /* sizeof(TileInfo) */ +
         (size_t)NB * 64 * WX * (sizeof(float) + sizeof(CountT)) + (size_t)NB * sizeof(unsigned long long);
}

// tuning knobs of the select-free view loop (development builds override them, profiles/tools/build_variant.sh)
#ifndef VCY_FAST_GROUP
#define VCY_FAST_GROUP 4   // voxels whose LDS reads are in flight together
#endif
// Waves per SIMD the kernels are compiled for (register budget 512 / waves).  The kernels whose work is done by
// the select-free loop (raw tiles, no update_num limit in reach) need 57-59 VGPRs there; what
// wants more is the checked loop with its call of the generic sampler, which those kernels rarely enter.  They
// are compiled for 7 waves (72 VGPRs: a handful of spills, placed in the rare blocks by the branch weights at
// the loop selection; 8 waves spill in the tile staging as well and lose 15 %).  The others keep 5.
#ifndef VCY_WAVES
#define VCY_WAVES 7
#endif
#ifndef VCY_WAVES_CHECKED
#define VCY_WAVES_CHECKED 5
#endif
// The unit-weight weighted average keeps update_num as floats next to sdf and carries the brick-wide weights: at 7 waves
// its PROLOGUE spills 24 bytes per lane, which every wave executes -- 3 GB of scratch written back per single-view
// launch at 1024^3 (the L2 turns over every 8 us there), a third of what the launch has to write at all
// (profiles/r04/per_view_tsdf_pmc.txt).
#ifndef VCY_WAVES_WA
#define VCY_WAVES_WA 6
#endif
// The one-view instances (NB == 0) have no view loop to keep registers for: the unit-weight average fits 7 waves (first
// view on a fresh grid 1.61 -> 1.47 ms, later views 2.53 -> 2.50; 5 waves: 1.81 / 2.65 -- profiles/r06/one_view_waves.txt)
#ifndef VCY_WAVES_WA_ONE
#define VCY_WAVES_WA_ONE 7
#endif
// ... and kMax 8, which its one tile buffer makes room for in LDS (first view 1.38 -> 1.32 ms, later views 0.537 -> 0.520;
// the unit-weight average at 8: 2.50 -> 2.82, spills)
#ifndef VCY_WAVES_ONE
#define VCY_WAVES_ONE 8
#endif

struct FusedView {
  ViewParams v;
  // Window maxima of the SDF image (built per launch by wmax_k4 / wmax_k8, carve_fused.hip), or null:
  //   wmax[p * plane + y * width + x] = max of g over [x, x + k) x [y, y + k) clipped to the image,
  //   k = 4 (p = 0) or 8 (p = 1), g = the SDF value, or +inf where it is NaN / infinite.
  // The maximum over any pw x ph rectangle with min(pw, ph) >= k is then the maximum of
  // ceil(pw/k) * ceil(ph/k) entries (windows placed inside the rectangle, overlapping at the far
  // edges): the prologue bounds a footprint with a handful of loads instead of scanning it.
  const float* wmax;
  int wmax_plane;
  // Planes 2 and 3, when has_lower != 0: the same window maxima of -g, i.e. window MINIMA of the image
  // negated.  Only built for the truncating weighted average, where a tile whose every tap is provably
  // >= -1 needs no `dist < -1` test per sample (TileInfo::sure bit 1).
  int has_lower;
  // The planes are only filled inside wrect = {x0, y0, x1, y1} (x0, x1 multiples of 4), the image-space
  // bounding box of this context's slab plus a border wider than anything a footprint lookup reaches;
  // a z-slab of a sharded grid often sees a narrow band of the image.
  int wrect[4];
};
// c0_all[view][x brick][32]: the products c0 = R[i][0] * px[x] (one fp32 multiply per entry, done on the
// host) of the 8 voxels of one wave brick along x, laid out for wide scalar loads:
//   [2 k + 0] = R[0][0] px[x_k], [2 k + 1] = R[1][0] px[x_k]  (the (x, y) pair a packed add takes as one operand)
//   [16 + k]  = R[2][0] px[x_k]                               (two neighbours = one packed operand)
// 24 of 32 floats used (128-byte records); columns beyond nx repeat the last one.
constexpr int kC0Stride = 32;

struct TileInfo {
  float lo_x, hi_x, lo_y, hi_y;  // closed range of (u,v) whose taps are in the tile
  float pitchf;
  int base;                      // -(ty0*tw + tx0)
  int tx0, ty0, tw, nq;          // nq = tw*th quads; 0: no tile for this view
  int th;
  float inv_tw;                  // 1 / tw: q / tw == (int)((q + 0.5f) * inv_tw) for q < 2^12
  float ub;                      // upper bound of any sample taken from this tile (+inf: unknown)
  int sure;                      // bit 0: every voxel of the brick provably samples inside this tile;
                                 // bit 1: and every sample is provably >= -1 (no truncation skip possible)
};
static_assert(sizeof(TileInfo) == 56, "row_lds_bytes_per_wave");

// ---- footprint records (raw-tile kernels) ------------------------------------------------------
// What footprint_of finds for a (wave brick, view) pair does not depend on the voxel state, and inside the carve
// kernel it is the worst kind of work: one lane per view (half the wave idle at 32 views, 63 of 64 lanes for a
// single view), two dependent memory round trips before the wave can do anything else, and registers the run loops
// then have to live with.  The raw-tile kernels therefore take it from a pre-pass at full occupancy
// (footprint_records_kernel: one thread per pair, lane = brick along x, the view wave-uniform, so the view
// constants are scalar operands and the window lookups of neighbouring lanes fall into the same cache lines) that
// leaves 8 bytes per pair in memory, [view][brick]; the carve kernel's prologue is one 8-byte load per lane.
//   word 0: bits 31..6 upper bound of the samples (a float rounded UP to 26 bits: still a bound),
//           bits 3..0 th, bit 4 / 5: the tile ends at the ROI's last column / row (TileInfo::hi_x / hi_y)
//   word 1: bits 12..0 tx0, 25..13 ty0, 29..26 tw (0: no tile), 31..30 TileInfo::sure
// (raw tiles: tw, th <= 15; images up to 8192 x 8192: fused_eligible)
// Everything but the bound is geometry: it depends on the camera, the grid and the slab, not on the image.  A launch that
// finds the records of its own cameras in the buffer ("recordcache", carve_fused_plan.h) takes the geometry as it is; the
// bound in them is then an earlier image's, and the kernel's prologue replaces it (kStateStaleBounds).
struct FootprintRecord {
  uint32_t w0, w1;
};
static_assert(sizeof(FootprintRecord) == kFootprintRecordBytes, "plan_fused_launch's chunk size");

// Bits 31..6 of word 0: the bound rounded UP to 26 bits.  (Shared by the pre-pass and by the carve kernel's prologue
// where it bounds the footprints of kept records itself -- kStateStaleBounds: the same truncation by construction.)
__device__ __forceinline__ uint32_t pack_footprint_ub(float ub) {
  uint32_t b = __float_as_uint(ub);
  if (!(fabsf(ub) <= 3.402823466e+38f)) b = 0x7f800000u;          // +inf / NaN: no bound
  else if (b & 0x80000000u) b &= ~63u;                            // negative: towards zero is up
  else b = (b + 63u) & ~63u;                                      // (may carry into +inf: no bound)
  return b;
}

__device__ __forceinline__ FootprintRecord pack_footprint(const TileInfo& ti, const ViewParams& v) {
  const uint32_t b = pack_footprint_ub(ti.ub);
  FootprintRecord r;
  const int tx1 = ti.tx0 + ti.tw - 1, ty1 = ti.ty0 + ti.th - 1;
  r.w0 = b | (uint32_t)ti.th | (ti.nq && tx1 == v.roi_max_xi ? 16u : 0u) | (ti.nq && ty1 == v.roi_max_yi ? 32u : 0u);
  r.w1 = ti.nq ? ((uint32_t)ti.tx0 | ((uint32_t)ti.ty0 << 13) | ((uint32_t)ti.tw << 26) | ((uint32_t)ti.sure << 30)) : 0u;
  return r;
}

// (bit casts that the host can make too: the unpack functions below are checked against each other on the CPU)
__host__ __device__ __forceinline__ float bits_as_float(uint32_t b) { return __builtin_bit_cast(float, b); }
__host__ __device__ __forceinline__ uint32_t float_as_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

__host__ __device__ __forceinline__ TileInfo unpack_footprint(const FootprintRecord r) {
  TileInfo ti;
  const int tw = (int)((r.w1 >> 26) & 15u), th = (int)(r.w0 & 15u);
  const int tx0 = (int)(r.w1 & 8191u), ty0 = (int)((r.w1 >> 13) & 8191u);
  ti.ub = bits_as_float(r.w0 & ~63u);
  ti.sure = (int)(r.w1 >> 30);
  ti.tx0 = tx0, ti.ty0 = ty0, ti.tw = tw, ti.th = (tw ? th : 0), ti.nq = tw * th;
  ti.pitchf = tw ? 16.0f : 0.0f;
  ti.inv_tw = tw ? 0.0625f : 1.0f;
  ti.base = tw ? -(ty0 * 16 + tx0) : 0;
  if (tw) {
    const int tx1 = tx0 + tw - 1, ty1 = ty0 + th - 1;
    ti.lo_x = (float)tx0, ti.lo_y = (float)ty0;
    // taps exist for floor(u) in [tx0, tx1]; at the ROI edge u == roi_max (== tx1) is still inside
    ti.hi_x = (r.w0 & 16u) ? (float)tx1 : bits_as_float(float_as_bits((float)(tx1 + 1)) - 1u);
    ti.hi_y = (r.w0 & 32u) ? (float)ty1 : bits_as_float(float_as_bits((float)(ty1 + 1)) - 1u);
  } else {
    ti.lo_x = ti.lo_y = INFINITY;  // nothing passes the tile test
    ti.hi_x = ti.hi_y = -INFINITY;
    ti.ub = INFINITY;
    ti.sure = 0;
  }
  return ti;
}

// The same record for a wave that keeps it packed (carve_fused_kernel with raw tiles, records from the pre-pass and a
// brick per wave: lane v holds the two words of view v).  Unpacked into a TileInfo by every lane and parked in LDS, each
// field a processed view needs came back through a ds_read and a v_readfirstlane; here the words of the view in hand are
// fetched with two v_readlane and taken apart as integers, which for uniform words is work of the scalar unit.
//   footprint_ub_word   what the lane keeps of word 0: the word itself, or +inf where the record has no tile
//   footprint_ub        the bound in it (TileInfo::ub)
//   unpack_footprint_scalar   the integer fields of (that word, word 1)
//   footprint_base / footprint_bounds   TileInfo::base and lo / hi, formed where they are needed
// Each equals the field of unpack_footprint bit for bit, for every record (tests/test_footprint_unpack_host.py).  The
// pitch of a raw tile is kTileRaw, which is TileInfo::pitchf of every record that has a tile.
struct FootprintFields {
  int tx0, ty0, tw, th, nq;  // (th: 0 without a tile)
  int sure;                  // TileInfo::sure
  int edge;                  // bit 0 / 1: the tile ends at the ROI's last column / row
};
struct FootprintBounds {
  float lo_x, hi_x, lo_y, hi_y;
};
__host__ __device__ __forceinline__ uint32_t footprint_ub_word(uint32_t w0, uint32_t w1) {
  return ((w1 >> 26) & 15u) ? w0 : 0x7f800000u;
}
__host__ __device__ __forceinline__ float footprint_ub(uint32_t ub_word) { return bits_as_float(ub_word & ~63u); }
__host__ __device__ __forceinline__ FootprintFields unpack_footprint_scalar(uint32_t ub_word, uint32_t w1) {
  FootprintFields f;
  const int th = (int)(ub_word & 15u);
  f.tw = (int)((w1 >> 26) & 15u);
  f.tx0 = (int)(w1 & 8191u), f.ty0 = (int)((w1 >> 13) & 8191u);
  f.th = f.tw ? th : 0, f.nq = f.tw * th;
  f.sure = f.tw ? (int)(w1 >> 30) : 0;
  f.edge = (int)((ub_word >> 4) & 3u);
  return f;
}
__host__ __device__ __forceinline__ int footprint_base(const FootprintFields& f) { return f.tw ? -(f.ty0 * 16 + f.tx0) : 0; }
__host__ __device__ __forceinline__ FootprintBounds footprint_bounds(const FootprintFields& f) {
  FootprintBounds b;
  if (f.tw) {
    const int tx1 = f.tx0 + f.tw - 1, ty1 = f.ty0 + f.th - 1;
    b.lo_x = (float)f.tx0, b.lo_y = (float)f.ty0;
    b.hi_x = (f.edge & 1) ? (float)tx1 : bits_as_float(float_as_bits((float)(tx1 + 1)) - 1u);
    b.hi_y = (f.edge & 2) ? (float)ty1 : bits_as_float(float_as_bits((float)(ty1 + 1)) - 1u);
  } else {
    b.lo_x = b.lo_y = INFINITY;  // nothing passes the tile test
    b.hi_x = b.hi_y = -INFINITY;
  }
  return b;
}

// ---- the step between two views' runs (carve_fused_kernel, the instances of carve_keeps_records) -------------------
// Between two runs the wave works on ONE view's record at a time, on the scalar unit, of which a CU has one for its four
// SIMDs: what the step asks of a record is therefore phrased as integer operations on the two words, one or two
// instructions each, and every uniform test as ONE integer comparison (a `||` of two uniform bools is carried as two
// 64-bit lane masks and costs five instructions).  The words are the lane's: footprint_ub_word and footprint_tile_word,
// which a lane forms ONCE for its view -- one vector instruction there does it for all views of the launch.
//   footprint_tile_word    word 1, or 0 where the record has nothing to fetch (tw == 0 or th == 0): "no tile" is `== 0`,
//                          and every field of a record without a tile reads 0 -- not `sure`, origin 0, base 0
//   footprint_has_tile / footprint_sure / footprint_tx0 / footprint_ty0 / footprint_step_base   of a tile word
//   footprint_row_groups   of the lane's word 0: the groups of four tile rows that hold a tap row, (th >> 2) + 1
//   footprint_window_unclamped   the whole 16 x 16 window lies inside the ROI: nothing to clamp (one comparison)
// Each equals the field of unpack_footprint for every record that has a tile and for every record without one
// (tests/test_view_step_host.py); a word 1 with tw != 0 and th == 0, which pack_footprint never writes and whose quad count
// is 0, reads "no tile" like tw == 0.
__host__ __device__ __forceinline__ uint32_t footprint_tile_word(uint32_t w0, uint32_t w1) {
  return (((w1 >> 26) & 15u) != 0u && (w0 & 15u) != 0u) ? w1 : 0u;
}
__host__ __device__ __forceinline__ bool footprint_has_tile(uint32_t tile_word) { return tile_word != 0u; }
__host__ __device__ __forceinline__ int footprint_sure(uint32_t tile_word) { return (int)(tile_word >> 30); }
__host__ __device__ __forceinline__ int footprint_tx0(uint32_t tile_word) { return (int)(tile_word & 8191u); }
__host__ __device__ __forceinline__ int footprint_ty0(uint32_t tile_word) { return (int)((tile_word >> 13) & 8191u); }
__host__ __device__ __forceinline__ int footprint_step_base(uint32_t tile_word) {  // TileInfo::base of a raw tile
  return -(footprint_ty0(tile_word) * 16 + footprint_tx0(tile_word));
}
__host__ __device__ __forceinline__ int footprint_row_groups(uint32_t ub_word) { return (int)((ub_word >> 2) & 3u) + 1; }
__host__ __device__ __forceinline__ bool footprint_window_unclamped(int tx0, int ty0, int roi_max_xi, int roi_max_yi) {
  // tx0 + 15 <= roi_max_xi && ty0 + 15 <= roi_max_yi (|operands| < 2^14: no overflow)
  const int rx = roi_max_xi - tx0, ry = roi_max_yi - ty0;
  return (rx < ry ? rx : ry) >= 15;
}
// The step addresses the launch's tables with 32-bit BYTE offsets from their three bases: the view records, the c0
// records, a view's image.  An image is at most 8192 x 8192 floats (fused_eligible), 2^28 bytes; the other two are bounded
// by carve_offsets_fit_32, which fused_eligible asks.
__host__ __device__ __forceinline__ uint32_t view_byte_offset(int view) { return (uint32_t)view * (uint32_t)sizeof(FusedView); }
__host__ __device__ __forceinline__ uint32_t c0_view_bytes(int nbw) { return (uint32_t)nbw * (uint32_t)(kC0Stride * sizeof(float)); }
__host__ __device__ __forceinline__ uint32_t c0_byte_offset(int view, uint32_t view_bytes, int brick_x) {
  return (uint32_t)view * view_bytes + (uint32_t)brick_x * (uint32_t)(kC0Stride * sizeof(float));
}
__host__ __device__ __forceinline__ uint32_t tile_origin_bytes(uint32_t width, int tx0, int ty0) {
  return (width * (uint32_t)ty0 + (uint32_t)tx0) * (uint32_t)sizeof(float);
}
// Do the view records and the c0 records of a launch of `n_views` views over `nbw` wave bricks along x end below 2^31
// bytes?  (With at most 64 views per launch the view records always do; the c0 records do up to 2^18 bricks, x
// resolutions beyond two million voxels.  A launch that does not is not a fused launch: fused_eligible.)
__host__ __device__ __forceinline__ bool carve_offsets_fit_32(int64_t n_views, int64_t nbw) {
  if (n_views < 0 || nbw < 0) return false;
  const uint64_t lim = 1ull << 31;
  if ((uint64_t)n_views >= lim || (uint64_t)nbw >= lim) return false;  // (the products below stay inside 64 bits)
  return (uint64_t)n_views * sizeof(FusedView) < lim &&
         (uint64_t)n_views * (uint64_t)nbw < lim / (uint64_t)(kC0Stride * sizeof(float));
}

// Exact n / d for 32-bit unsigned n (Granlund-Montgomery, as in mc_kernels.hip): three integer instructions where the
// compiler's division by a run-time value takes about twenty.
struct FastDivU32 {
  uint32_t d, m, s1, s2;
};
__device__ __forceinline__ uint32_t fast_div_u32(uint32_t n, const FastDivU32& f) {
  const uint32_t t = __umulhi(n, f.m);
  return (t + ((n - t) >> f.s1)) >> f.s2;
}
inline FastDivU32 make_fast_div_u32(uint32_t d) {
  FastDivU32 f;
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;  // ceil(log2 d)
  f.d = d;
  f.m = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
  f.s1 = l < 1 ? l : 1;
  f.s2 = l < 1 ? 0 : l - 1;
  return f;
}

// Launch constants of carve_fused_kernel's block decode (which workgroup block of bricks a launch index is), computed on
// the host: a single-view launch runs 2 M waves that live a few microseconds, each CU has ONE scalar unit, and the five
// integer divisions by run-time values at the head of every wave -- 25 scalar instructions and a v_rcp_iflag round trip
// each -- were a fifth of the scalar work that bounds such a launch (profiles/r05/first_view_floor.txt).
struct BlockDecode {
  int total;                           // units (workgroup blocks; segments of the few-view flavour) of the launch
  int layer, q, rem, dealt;            // workgroups per brick layer, layer / 8, layer % 8, 8 q (layers of the launch)
  FastDivU32 dq, drem, dnbx, dnby;     // divisions by q, rem (1 when rem == 0: never used then), nbx, nby
};
inline BlockDecode make_block_decode(unsigned grid_x, int nbx, int nby) {
  BlockDecode d;
  d.total = (int)grid_x;
  d.layer = nbx * nby;
  d.q = d.layer >> 3;
  d.rem = d.layer & 7;
  d.dealt = 8 * d.q * (int)(grid_x / (unsigned)std::max(d.layer, 1));
  d.dq = make_fast_div_u32((uint32_t)std::max(d.q, 1));
  d.drem = make_fast_div_u32((uint32_t)std::max(d.rem, 1));
  d.dnbx = make_fast_div_u32((uint32_t)std::max(nbx, 1));
  d.dnby = make_fast_div_u32((uint32_t)std::max(nby, 1));
  return d;
}

// One launch of carve_fused_kernel, filled per chunk by launch_carve_fused and handed to the unit that holds the
// instances for the counter width (launch_fused_counts8 / 16), whose dispatch turns the selection into template arguments.
struct CarveLaunch {
  // which instance
  int update;            // VCY_UPDATE_MAX, VCY_UPDATE_WEIGHTED_AVERAGE, or kUpdateWaUnitWeight when the weight is 1.0f
  bool trunc, samef;     // use_truncation; fx == fy in every view
  bool checkmax;         // voxel_max_update_num is in reach
  bool big;              // tile kind: kTileBig instead of kTileRaw
  bool gen;              // nearest-neighbour sampling and / or an orthographic camera
  int div_level;         // the division sequence (div_view), without meaning when `gen`
  CarveFlavour flavour;
  // the kernel's arguments, in its order (the BlockDecode is made from the launch shape)
  GridParams g;
  const FusedView* views;
  const float* c0_all;
  int n_views;
  ModeParams mode;
  int nbx, nby;          // units per brick row (workgroup blocks; segments for kRows), brick rows
  int cull;
  int state_flags;
  const FootprintRecord* records;
  int64_t nbricks;
  float* brick_min;
  const int* wg_list;
  unsigned long long* pair_count;
  // launch shape
  unsigned grid_x;       // workgroups
  hipStream_t stream;
  int row_units;         // kRows: segments of the launch (what the block decode deals to the XCDs)
};

// carve_fused_u8.hip / carve_fused_u16.hip: each unit instantiates carve_fused_kernel for one width of update_num (288
// instances each: 3 update modes x trunc x samef x 24) behind its one exported function, so that the halves build in
// parallel.  carve_fused.hip instantiates no carve kernel.
void launch_fused_counts8(const CarveLaunch& launch);
void launch_fused_counts16(const CarveLaunch& launch);

}  // namespace vcy
