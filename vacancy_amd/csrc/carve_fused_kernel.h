// K1 (fused): carve up to 64 views per launch with the voxel state held in registers.
//
// Replaces the loop `for each view: Carve(camera, roi, sdf)` (reference voxel_carver.cc:516-528
// around :415-496).  Voxels are independent and every voxel sees its views in sequence order,
// so fusing views changes nothing but where the state lives.  A workgroup is four independent
// waves; each WAVE owns an 8x8x8 brick (lane = (y & 7) | (z << 3), 8 voxels along x per lane),
// loads sdf/update_num ONCE (not at all for a fresh grid), applies all views and writes back only
// what changed.  The four wave bricks of a workgroup are adjacent in x, so together they read
// 128-byte row segments.
//
// Per view the wave keeps the image footprint of its brick in a wave-private LDS tile: 16 x 16 raw pixels
// (kTileRaw: global memory -> LDS directly, double buffered, a sample = two ds_read2_b32), or for footprints
// beyond 15 x 15 pixels a raw tile of up to 2048 pixels with the footprint's own pitch, filled in place (kTileBig).
// Either way the reference's ROI clamps of x + 1 and y + 1 (voxel_carver.cc:51-66) are applied when the
// tile is filled, never per sample.  No workgroup barrier anywhere.  A voxel whose projection falls
// outside the staged tile (brick near the camera plane, footprint larger than the tile, outside the ROI)
// takes the generic global-memory path of carve_common.h, so SAMPLING never depends on the footprint
// estimate.  DROPPING a view for a brick does (see the kernel): it is only done when the
// footprint rectangle is provably a superset of every sample, with an explicit error margin.
//
// The arithmetic of a sample is the reference's, operation for operation (carve_common.h);
// the two divides fx/z, fy/z (camera.cc:133-136) use the same Newton sequence the compiler
// emits for IEEE division minus the exponent pre-scaling, which is a no-op for operands in
// [2^-60, 2^60]; anything outside that range takes the generic path.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "carve_fused_device.h"

namespace vcy {
namespace {

// GEN: nearest-neighbour sampling and/or an orthographic camera, selected at run time from `mode`
// (compiled out of the default bilinear + pinhole kernels, where the extra branches cost 16 %).
// NB: bricks per wave -- 1: a workgroup of kWgWaves waves, a brick each (fused launches of many views); kRowBricks: the
// few-view flavour described at kRowBricks in carve_fused.h (raw tiles, records from the pre-pass, rows of whole bricks).
template <int UPDATE, bool CHECKMAX, int TQ, bool GEN, int NB>
constexpr int carve_waves_per_simd() {
  // (the few-view flavour is bounded by its LDS: 3 - 5 waves per SIMD, registers to spare)
  if (NB > 1) return NB > 2 ? 4 : 5;
  if (GEN || CHECKMAX || TQ != kTileRaw || UPDATE == VCY_UPDATE_WEIGHTED_AVERAGE) return VCY_WAVES_CHECKED;
  if (UPDATE == kUpdateWaUnitWeight) return NB == 0 ? VCY_WAVES_WA_ONE : VCY_WAVES_WA;
  return NB == 0 ? VCY_WAVES_ONE : VCY_WAVES;
}
// The instances that keep a wave's footprint records packed in registers instead of a TileInfo per view in LDS
// (unpack_footprint_scalar, carve_fused.h): kMax with raw tiles and a brick per wave.  The weighted-average instances sit
// at their register limit -- with the second record word the unit-weight truncating one spills 80 bytes per lane where it
// spilled 64 (profiles/record_regs) -- and keep the TileInfo; so do the big tile (its pitch and bounds are not in a
// record) and the few-view flavour (a lane per PAIR, LDS to spare).
template <int UPDATE, int TQ, int NB>
constexpr bool carve_keeps_records() {
  return UPDATE == VCY_UPDATE_MAX && TQ == kTileRaw && NB == 1;
}
template <typename CountT, int UPDATE, bool TRUNC, bool SAMEF, bool CHECKMAX, int TQ, bool GEN, int DIV, int NB = 1>
__global__ __launch_bounds__(64 * (NB > 1 ? kRowWaves : kWgWaves))
__attribute__((amdgpu_waves_per_eu(NB > 1 ? 1 : carve_waves_per_simd<UPDATE, CHECKMAX, TQ, GEN, NB>(),
                                   carve_waves_per_simd<UPDATE, CHECKMAX, TQ, GEN, NB>()))) void carve_fused_kernel(GridParams g,
                                                          const FusedView* __restrict__ views,
                                                          const float* __restrict__ c0_all,
                                                          int nviews_arg, ModeParams mode, int nbx,
                                                          int nby, BlockDecode bd, int cull_enabled, int state_flags,
                                                          const FootprintRecord* __restrict__ records,
                                                          int64_t nbricks, float* __restrict__ brick_min,
                                                          const int* __restrict__ wg_list,
                                                          unsigned long long* __restrict__ pair_count) {
  // brick_min[wave brick] (or null): min(sdf) over the brick as the carve kernels left it -- lowest() while a
  // voxel of it is untouched.  Written by every fused launch; READ (kStateBrickMinValid: every write to the state
  // since the slab was fresh went through a fused launch) to drop views before the state is loaded: a wave
  // whose every view is dropped returns without reading or writing anything, which is what makes the
  // reference's `Carve(); Extract(); Carve(); ...` pattern of single-view launches cheap.  Marching cubes skips
  // bricks that lie entirely outside the iso-surface with it (mc_bits).
  // state_flags: the kState* bits of carve_fused.h.
  // NB == 0: a launch of ONE view with the NB = 1 structure (a brick per wave, cooperative write-back).  The reference's
  // own loop (examples.cc:117-149) makes every view such a launch; with the view count a compile-time 1 the footprint
  // record is a scalar load unpacked into registers (no TileInfo in LDS, no read-backs), and the view loop, its
  // next-view search, the second tile buffer's bookkeeping and the re-bounding after the view fold away.
  constexpr bool kOne = NB == 0;
  constexpr bool kOneRegs = kOne;
  const int nviews = kOne ? 1 : nviews_arg;
  const int fresh = state_flags & kStateFresh;
  const bool implied = (state_flags & kStateCountImplied) != 0;
  const bool coop = NB <= 1 && (kWgWaves == 4 || kWgWaves == 8) && (state_flags & kStateCoopStore) != 0;
  const bool nt_store = (state_flags & kStateStreamStore) != 0;  // cooperative write-back with streaming stores
  constexpr bool kRows = NB > 1;  // the few-view flavour: this WAVE walks NB bricks of a row (kRowBricks)
  static_assert(!kRows || (TQ == kTileRaw && !CHECKMAX), "the few-view flavour: raw tiles, no update limit in reach");
  // dynamic LDS: [4 waves][TQ] quads, then [4 waves][nviews] TileInfo (sized by the launch; none where the records stay
  // in registers: NB == 0, kRecRegs), then the staging of the cooperative write-back
  extern __shared__ float4 fused_lds[];
  constexpr bool kRaw = TQ == kTileRaw;                  // raw-pixel tiles, loaded straight into LDS
  // kMax with raw tiles and a brick per wave: the footprint records stay PACKED, two registers per lane (lane v: view v),
  // and no TileInfo goes to LDS -- see unpack_footprint_scalar and carve_keeps_records.
  constexpr bool kRecRegs = carve_keeps_records<UPDATE, TQ, NB>();
  // (NB == 0: ONE tile buffer -- there is no next view to fetch ahead -- and no TileInfo: 18.4 KB per workgroup with the
  // cooperative write-back's staging instead of 22.5, i.e. eight workgroups per CU where seven fit)
  constexpr int kTileF4 = NB == 0 ? 64 : tile_f4_per_wave<TQ>();
  // A view can be dropped for a whole wave brick when no voxel of the brick can change:
  //   - use_truncation and every sample is provably < -1 (voxel_carver.cc:478), or
  //   - kMax, every voxel already touched, and every sample is provably <= min(sdf) of the
  //     brick (UpdateVoxelMax only writes when dist > sdf, voxel_carver.cc:82).
  // "Provably": with every tap <= M and weights >= 0, monotonicity of IEEE rounding gives
  //   dist = fl(fl(fl(w00 s00 + w10 s10) + w01 s01) + w11 s11) <= the same expression with all taps = M,
  // and the four weights sum to 1 within 2^-23 (each is a product of u-floor(u), 1-(u-floor(u)) ...),
  // so dist <= M + 2^-22 |M| for either sign of M.  ub = M + 2^-20 |M| is that bound with slack.
  // Footprints holding a NaN or an infinity give no bound (0 * inf = NaN samples).
  // (Round 6 also bounded a `sure` view by the EXACT maximum of its staged tile -- one 16-byte LDS read per lane and a wave
  // reduction once the tile has landed -- against the window maxima's over-estimate: on the benchmark scenes it never
  // dropped a single pair more and cost 8 % (profiles/r06/exact_tile.txt).  The pairs that are processed without changing
  // anything are not lost to the windows sticking out of the footprint: a distance field varies by 1 - 2 % across a
  // footprint, and so does the brick's state; what is compared is the MAXIMUM of the one with the MINIMUM of the other.)
  constexpr bool kNeedBound = TRUNC || UPDATE == VCY_UPDATE_MAX;

  VCY_SETPRIO(3);
  const int tid = threadIdx.x;
  // (the wave index is uniform, which the compiler cannot see: keeps the LDS bases of the wave in SGPRs)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  VCY_PT_DECL;
  // NB > 1: every wave has its own region [tiles | TileInfo of the NB x 8 pairs | state of NB bricks | NB masks]
  constexpr size_t kRowWaveBytes = kRows ? row_lds_bytes_per_wave<CountT, NB>() : 0;
  static_assert(kRowWaveBytes % 16 == 0, "wave regions are 16-byte aligned");
  float4* tile = kRows ? (float4*)((char*)fused_lds + wave * kRowWaveBytes) : fused_lds + wave * kTileF4;
  TileInfo* tinfo = kRows ? (TileInfo*)((char*)tile + kRawBuffers * 1024)
                          : (TileInfo*)(fused_lds + kWgWaves * kTileF4) + wave * nviews;
  float* stage_s = (float*)((char*)tinfo + NB * kRowMaxViews * sizeof(TileInfo));   // [NB][64 rows][WX]
  CountT* stage_n = (CountT*)(stage_s + NB * 64 * WX);                                 // [NB][64 rows][WX]
  typedef unsigned long long __attribute__((address_space(3))) lds_u64_row;
  lds_u64_row* stage_mask = (lds_u64_row*)(unsigned long long*)(stage_n + NB * 64 * WX);  // [NB] changed lanes
  // (sizeof(TileInfo) * kWgWaves is a multiple of 16: the staging area is 16-byte aligned)
  static_assert((sizeof(TileInfo) * kWgWaves) % 16 == 0, "alignment of the cooperative write-back's staging");
  typedef CountT CountVec8 __attribute__((ext_vector_type(WX)));
  typedef CountVec8 __attribute__((address_space(3))) lds_countvec;
  typedef unsigned long long __attribute__((address_space(3))) lds_u64;
  float* coop_s = (NB == 0 || kRecRegs) ? (float*)(fused_lds + kWgWaves * kTileF4)
                                        : (float*)((TileInfo*)(fused_lds + kWgWaves * kTileF4) + kWgWaves * nviews);
  CountT* coop_n = (CountT*)(coop_s + 64 * kCoopSdfPitch);
  lds_u64* coop_mask = (lds_u64*)(unsigned long long*)(coop_n + 64 * coop_cnt_pitch<CountT>());
  // A wave that leaves early tells the others that none of its rows is to be stored and that it will not be there to
  // store rows of theirs (s_barrier only waits for the waves of the workgroup that have not ended; the LDS writes have
  // completed before the wave ends).
  auto coop_leave = [&]() {
    if (coop) {
      if (lane == 0) coop_mask[wave] = 0ull, coop_mask[kWgWaves + wave] = 0ull;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    }
  };
  TileInfo ti_one;  // NB == 0: the one view's tile, in registers
  auto tile_of = [&](int p) -> const TileInfo& {
    if constexpr (kOneRegs) return ti_one;
    else return tinfo[p];
  };
  // kRecRegs: this lane's record -- word 0 (footprint_ub_word: the bound, th, the edge bits) and word 1
  // (footprint_tile_word: 0 where there is nothing to fetch); a lane without a view holds "no tile, no bound"
  uint32_t rec_w0 = 0x7f800000u, rec_w1 = 0u;
  auto rec_of = [&](int p) -> FootprintFields {  // the fields of view p's record, as scalars
    return unpack_footprint_scalar((uint32_t)__builtin_amdgcn_readlane((int)rec_w0, p),
                                   (uint32_t)__builtin_amdgcn_readlane((int)rec_w1, p));
  };
  // kRecRegs, kStateStaleBounds: the launch reuses an earlier launch's records -- same cameras, same slab -- and only the
  // bound in word 0 is stale (it came from that launch's images).  Lane v then bounds the footprint of view v itself: the
  // lookups footprint_of makes for the pre-pass (footprint_window_requests), in the prologue, where the sixteen state
  // registers are not live yet and nothing of it stays.  On a fresh slab without truncation no bound is compared before
  // the first run, so the first view is known -- view 0 -- and its tile is requested IN FRONT of the lookups: the two
  // share a round trip, and the wait for the lookups is the wait for the tile that begin_view() would make next anyway.
  // On any other slab the bounds are compared at once (the early-return test): the lookups are a round trip of their own.
  const bool stale_bounds = kRecRegs && (state_flags & kStateStaleBounds) != 0;
  int vi_stale = -1;  // the view whose tile that prologue has requested (what vi_pre, below, starts from)
  int cur = 0;  // raw tiles: which of the wave's buffers holds the view being carved
  auto raw_buf = [&](int b) -> float* { return (float*)tile + 256 * b; };
  // requests the raw tile of view / pair p into `buf`
  auto prefetch_tile = [&](int p, float* buf) {
    const ViewParams& v = views[kRows ? (p & 7) : p].v;
    if constexpr (kRecRegs) raw_prefetch(v, rec_of(p), lane, buf);
    else raw_prefetch(v, tile_of(p), lane, buf);
  };
  // TileInfo::sure of view / pair p, uniform
  auto sure_of = [&](int p) -> int {
    if constexpr (kRecRegs) return rec_of(p).sure;
    else return __builtin_amdgcn_readfirstlane(tile_of(p).sure);
  };
  // kRecRegs: the scalar state of the step between two runs (carve_fused.h, "the step between two views' runs").
  //   ahead        the live views BEHIND the one in hand, as a mask: the next view is its lowest bit, taking a view
  //                clears that bit, and a re-bound is an AND with the ballot of the lanes whose bound still stands
  //   cur_*        the view in hand: its tile word and the byte offset of its view record
  //   nxt_*        the same of the next view, whose tile is in flight (and its word 0, for the request); nxt_w1 == 0
  //                when there is none.  Taken apart ONCE, when the view is chosen, and handed over when it becomes the
  //                view in hand.
  //   moved_mask   the lanes whose voxels the last select-free run changed (what carve_view_fast returns as a bool)
  //   rebound_mask all ones when a run that moved the brick is followed by a re-bound (kMax with "cull" on), else zero:
  //                `moved_mask & rebound_mask` is ONE scalar instruction that sets the condition code, where the `&&` of
  //                the two uniform bools was five.  Formed from the launch's 0 / 1 by arithmetic -- from
  //                `cull_enabled != 0` the compiler sees a bool in it again.  (Another non-zero value would leave bits out
  //                of the mask and so skip a re-bound, which only ever drops views that change nothing; never add one.)
  // (c0_per_view and the mask are set in these instances only: the others compile as before)
  unsigned long long ahead = 0ull, moved_mask = 0ull;
  uint32_t cur_w1 = 0u, cur_voff = 0u, nxt_w0 = 0u, nxt_w1 = 0u, nxt_voff = 0u;
  uint32_t c0_per_view = 0u, rebound_half = 0u;
  if constexpr (kRecRegs) c0_per_view = c0_view_bytes(((g.nx + WX - 1) & ~(WX - 1)) / WX);
  if constexpr (kRecRegs && kNeedBound) rebound_half = 0u - (uint32_t)cull_enabled;
  const unsigned long long rebound_mask = ((unsigned long long)rebound_half << 32) | rebound_half;
  const int ly = lane & (BY - 1), lz = lane >> 3;
  // XCD-aware order: the dispatcher deals consecutive workgroups round-robin to the 8 XCDs, so
  // workgroup b runs on XCD b % 8.  Give every XCD one contiguous eighth of the brick list: bricks
  // that follow each other on an XCD are neighbours in x and share SDF footprint pixels and
  // z-table entries in that XCD's private L2.
  // NB > 1: the unit of the launch is a SEGMENT (NB bricks of a row) and every wave takes one -- the waves of a
  // workgroup consecutive units of the same XCD's share (b mod 8 = blockIdx mod 8, the XCD the workgroup runs on)
  int b = kRows ? ((int)(blockIdx.x & 7u) + 8 * (kRowWaves * (int)(blockIdx.x >> 3) + wave)) : (int)blockIdx.x;
  const int* list_entry = nullptr;  // NB == 0, listed launch whose entries hold {id, live waves, records}: this workgroup's
  int list_live = 0;
  FootprintRecord list_rec;
  list_rec.w0 = 0u, list_rec.w1 = 0u;
  if (wg_list != nullptr) {  // only the workgroups live_workgroups_kernel listed (wg_list[0] of them)
    if (kRows) b = (int)blockIdx.x * kRowWaves + wave;
    if (b >= wg_list[0]) return;
    if (kOne && (state_flags & kStateListRecords) != 0) {  // entries with records (live_workgroups_kernel)
      // (VECTOR loads that all lanes share, made uniform afterwards: 40 bytes per workgroup streamed through the scalar
      // cache evict the view record and the axis tables that every wave re-reads -- measured, like the records before)
      list_entry = wg_list + 2 + (int64_t)b * kLiveEntryWords;
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      typedef const u32x2 __attribute__((address_space(1))) * gent_ptr;
      const u32x2 head = ((gent_ptr)list_entry)[0], mine = ((gent_ptr)list_entry)[1 + wave];
      b = __builtin_amdgcn_readfirstlane((int)head.x);
      list_live = __builtin_amdgcn_readfirstlane((int)head.y);
      list_rec.w0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)mine.x);
      list_rec.w1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)mine.y);
    } else {
      b = wg_list[1 + b];
    }
  } else {
    if (kRows && b >= bd.total) return;
    // Every XCD takes an eighth of EVERY brick layer -- q = layer / 8 consecutive workgroups, i.e. whole rows in (y, x)
    // order -- and a different eighth in every layer (chunk (xcd + layer) mod 8), so that each XCD sees every z and,
    // over 8 layers, every y range: balanced for a slab of few layers too (a rank's slab of an 8-GPU run has 16, and
    // dealing whole layers gives XCD 7 the two most expensive ones of an outer slab).  The workgroups a layer has
    // beyond a multiple of eight go round-robin as they come.
    // (layer, q, rem, dealt and the divisions by q and rem: launch constants from the host, BlockDecode)
    const int layer = bd.layer, q = bd.q, rem = bd.rem, dealt = bd.dealt;
    if (b < dealt) {
      const int xcd = b & 7, j = b >> 3;
      const int l = (int)fast_div_u32((uint32_t)j, bd.dq), within = j - l * q;
      b = l * layer + ((xcd + l) & 7) * q + within;
    } else {
      const int r = b - dealt, l = (int)fast_div_u32((uint32_t)r, bd.drem);
      b = l * layer + 8 * q + (r - l * rem);
    }
  }
  const int brow = (int)fast_div_u32((uint32_t)b, bd.dnbx);  // (b >= 0: a launch covers fewer than 2^31 workgroups)
  const int bx = b - brow * nbx;
  const int bz = (int)fast_div_u32((uint32_t)brow, bd.dnby);
  const int by = brow - bz * nby;
  // (the wave index is uniform, which the compiler cannot see: readfirstlane keeps the x tables in scalar loads)
  // (NB > 1: the origin of the segment's first brick; moves on with the brick being carved)
  int x_first = kRows ? bx * (NB * WX) : __builtin_amdgcn_readfirstlane(bx * BX + wave * WX);  // wave brick origin
#if defined(VCY_DEV_EXIT_AT) && VCY_DEV_EXIT_AT == 1
  if (x_first >= 0) {
    coop_leave();
    return;
  }
#endif
  if (x_first >= g.nx) {                    // (a wave may leave alone: see coop_leave)
    coop_leave();
    return;
  }
  if constexpr (kOne) {
    // (the early return below, decided by the list pass on the same record and the same brick minimum)
    if (list_entry != nullptr && ((list_live >> wave) & 1) == 0) {
      coop_leave();
      return;
    }
  }
  const int zl0 = bz * BZ;
  const int y_raw = by * BY + ly, zl_raw = zl0 + lz;
  const int y = min(y_raw, g.ny - 1), zl = min(zl_raw, g.nz_local - 1);  // clones for out-of-grid lanes
  const float py = g.py[y], pz = g.pz[g.z0 + zl];
  // Lane (y, z) walks the WX voxels of its x run: in pc = t + (c0 + (c1 + c2)) (reference association) the
  // inner sum c1 + c2 = R[:,1] y + R[:,2] z is the same for the whole run and computed once per view.
  const int nxp = (g.nx + WX - 1) & ~(WX - 1);
  const bool want_bound = kNeedBound && cull_enabled;

  // This wave brick's index in the launch (fewer than 2^31: launch_carve_fused).  Computed HERE, in uniform control
  // flow: a uniform value first computed inside a divergent branch (`if (lane < nviews)` below) reaches later uses
  // through a phi that the compiler must treat as divergent -- it then lives in a VGPR, and so did the address of the
  // c0 records that shares `nxp / WX` with it: the scalar loads of the run loops had become vector loads (-15 %).
  int brick_lin = (bz * nby + by) * (nxp / WX) + (x_first / WX);
  const int x_seg = x_first, brick_seg = brick_lin;  // (NB > 1: the segment's first brick)
  // "Eager" launches (kStateEager; launch_carve_fused sets it for few-view launches whose workgroups are nearly all
  // live -- listed ones, or a weighted-average view that changes nearly every brick): the brick's state is requested HERE,
  // next to the footprint record, instead of behind the early-return test that needs the record first -- one memory round
  // trip less in the life of a wave that consists of little else.  (A wave that then returns early has read 2.5 KB for
  // nothing; y and zl are clamped and x_first < nx, so the addresses are inside the slab.)
  // Only in the instance compiled for ONE view: in the general one the ten registers, live across the prologue, put
  // lane spills into the run loops of the 32-view launch that never takes this path.
  typedef CountT CountVecE __attribute__((ext_vector_type(WX)));
  f4 eager_a = f4{0.f, 0.f, 0.f, 0.f}, eager_b = eager_a;
  CountVecE eager_c = CountVecE{};
  const bool eager = kOne && (state_flags & kStateEager) != 0 && (state_flags & kStateFresh) == 0 && (g.nx & (WX - 1)) == 0;
  if constexpr (kOne) {
    if (eager) {
      const int64_t row_e = ((int64_t)zl * g.ny + y) * g.nx + x_first;
      eager_a = *(const f4*)(g.sdf + row_e);
      eager_b = *(const f4*)(g.sdf + row_e + 4);
      eager_c = *(const CountVecE*)((const CountT*)g.cnt + row_e);
    }
  }
  // ---- prologue: lane vi bounds the footprint of the wave brick in view vi (brick_footprints) -------
  float ub_lane;
#ifdef VCY_PHASE_TIMING
  {
    asm volatile("" ::"v"(py), "v"(pz));  // the axis tables have arrived
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();
    pt_acc[12] += t_ - pt_last;
  }
#endif
  // NB > 1: lane 8 j + v holds the pair (brick j of the segment, view v)
  const int pair_j = lane >> 3, pair_v = lane & 7;
  const bool pair_valid = kRows && pair_j < NB && pair_v < nviews && x_seg + pair_j * WX < g.nx;
  if constexpr (kRows) {
    ub_lane = INFINITY;
    if (pair_valid) {
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      typedef const u32x2 __attribute__((address_space(1))) * grec_ptr;
      const u32x2 raw = ((grec_ptr)records)[(int64_t)pair_v * nbricks + (brick_seg + pair_j)];
      FootprintRecord rec;
      rec.w0 = raw.x, rec.w1 = raw.y;
      const TileInfo ti = unpack_footprint(rec);
      store_tile_info((lds_u32*)tinfo, lane, ti);
      ub_lane = ti.ub;
    }
  } else if constexpr (kOneRegs) {
    // one view: the record of (view 0, this brick) is wave-uniform.  Fetched with a VECTOR load all lanes share and made
    // uniform afterwards: the records are streamed once, and as scalar loads they evicted the view record and the x
    // tables -- which every wave re-reads -- from the scalar cache (2.72 -> 3.38 ms per weighted-average view).
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef const u32x2 __attribute__((address_space(1))) * grec_ptr;
    FootprintRecord rec;
    if (list_entry != nullptr) {  // (arrived with the workgroup id)
      rec = list_rec;
    } else {
      const u32x2 raw = ((grec_ptr)records)[brick_lin];
      rec.w0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)raw.x), rec.w1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)raw.y);
    }
    ti_one = unpack_footprint(rec);
    ub_lane = ti_one.ub;
  } else if (kRecRegs && stale_bounds) {
    // The records of an earlier launch with these cameras ("recordcache"): the lane keeps the geometry as it is and looks
    // the bound up -- what footprint_of does for the pre-pass, through the same helpers, so the words it ends up with are
    // the words the pre-pass would have written for this launch's images.
    if constexpr (kRecRegs) {
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      typedef const u32x2 __attribute__((address_space(1))) * grec_ptr;
      ub_lane = INFINITY;
      const bool has_view = lane < nviews;
      const int lv = has_view ? lane : 0;  // (lanes without a view read view 0's record and keep "no tile, no bound")
      // the record and the lane's view, requested together: one batch of loads behind one wait
      // (32-bit byte offsets from the uniform bases: the records of a launch in one chunk are at most kRecordBytesMax)
      typedef const char __attribute__((address_space(1))) * gchar_ptr;
      static_assert(kRecordBytesMax <= ((int64_t)1 << 31), "the records' byte offset is formed in 32 bits");
      u32x2 raw = *(grec_ptr)((gchar_ptr)records + (((uint32_t)lv * (uint32_t)nbricks + (uint32_t)brick_lin) << 3));
      BoundView bv = load_bound_view(views, lv);
      asm volatile("" : "+v"(raw.x), "+v"(raw.y), "+v"(bv.wmax), "+v"(bv.wmax_plane), "+v"(bv.width), "+v"(bv.roi_max_xi),
                   "+v"(bv.roi_max_yi), "+v"(bv.max_sdf));
      if (has_view) rec_w0 = footprint_ub_word(raw.x, raw.y), rec_w1 = footprint_tile_word(raw.x, raw.y);
      if (fresh && !TRUNC) {  // (uniform) nothing compares a bound before the first run: the first view is view 0
        vi_stale = 0;
        prefetch_tile(0, raw_buf(0));
      }
      const int tw = (int)((raw.y >> 26) & 15u), th = (int)(raw.x & 15u);
      if (has_view && tw != 0) {  // (a record without a tile has no bound: footprint_ub_word)
        const int tx0 = (int)(raw.y & 8191u), ty0 = (int)((raw.y >> 13) & 8191u);
        const FootprintWindows fw = footprint_windows(tx0, ty0, tx0 + tw - 1, ty0 + th - 1, bv.roi_max_xi, bv.roi_max_yi);
        float t[9];
        footprint_window_requests<false>(bv.wmax, bv.width, fw.L == 3 ? bv.wmax_plane : 0u, tx0, ty0, fw, t);
        const float ub = footprint_upper_bound(footprint_window_max(t), 0, mode.outside == VCY_OUTSIDE_MAX,
                                               ((raw.y >> 30) & 1u) != 0u, bv.max_sdf);
        rec_w0 = pack_footprint_ub(ub) | (raw.x & 63u);
      }
    }  // (if constexpr: nothing of this is instantiated in the other instances)
  } else if (kRaw && records != nullptr) {
    // raw tiles: the footprints come from the pre-pass (footprint_records_kernel), 8 bytes per view (kRecRegs: and stay
    // as they are in the lane that loaded them)
    ub_lane = INFINITY;
    if (lane < nviews) {
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      typedef const u32x2 __attribute__((address_space(1))) * grec_ptr;
      const u32x2 raw = ((grec_ptr)records)[(int64_t)lane * nbricks + brick_lin];
      if constexpr (kRecRegs) {
        rec_w0 = footprint_ub_word(raw.x, raw.y), rec_w1 = footprint_tile_word(raw.x, raw.y);
      } else {
        FootprintRecord rec;
        rec.w0 = raw.x, rec.w1 = raw.y;
        const TileInfo ti = unpack_footprint(rec);
        store_tile_info((lds_u32*)tinfo, lane, ti);
        ub_lane = ti.ub;
      }
    }
  } else if constexpr (kRecRegs) {
    // "prologue" 1: the record the pre-pass would have left for this lane's view, made here (brick_footprint_records)
    const int x_lo = min(x_first, g.nx - 1), x_hi = min(x_first + WX - 1, g.nx - 1);
    const int y_hi = min(by * BY + BY - 1, g.ny - 1);
    const int z_hi = min(zl0 + BZ - 1, g.nz_local - 1);
    const FootprintRecord rec = brick_footprint_records<SAMEF, GEN>(
        views, nviews, lane, g.px[x_lo], g.px[x_hi], g.py[by * BY], g.py[y_hi], g.pz[g.z0 + zl0], g.pz[g.z0 + z_hi],
        mode.ortho != 0, mode.outside == VCY_OUTSIDE_MAX, want_bound, want_bound && TRUNC && UPDATE != VCY_UPDATE_MAX);
    rec_w0 = footprint_ub_word(rec.w0, rec.w1), rec_w1 = footprint_tile_word(rec.w0, rec.w1);
    ub_lane = INFINITY;
  } else {
    // the big tile -- and raw tiles of a launch whose records would not fit (`records` null: 2048^3 x 64 views would
    // write and read back 8.6 GB of them in nine chunks; with 64 views every lane of this prologue has a view)
    const int x_lo = min(x_first, g.nx - 1), x_hi = min(x_first + WX - 1, g.nx - 1);
    const int y_hi = min(by * BY + BY - 1, g.ny - 1);
    const int z_hi = min(zl0 + BZ - 1, g.nz_local - 1);
    ub_lane = brick_footprints<SAMEF, TQ, GEN>(views, nviews, lane, g.px[x_lo], g.px[x_hi], g.py[by * BY], g.py[y_hi],
                                               g.pz[g.z0 + zl0], g.pz[g.z0 + z_hi], mode.ortho != 0,
                                               mode.outside == VCY_OUTSIDE_MAX, want_bound,
                                               want_bound && TRUNC && UPDATE != VCY_UPDATE_MAX, (lds_u32*)tinfo);
  }
  // this lane's bound (TileInfo::ub of its view)
  auto lane_ub = [&]() -> float {
    if constexpr (kRecRegs) return footprint_ub(rec_w0);
    else return ub_lane;
  };
  wave_lds_fence();
#if defined(VCY_DEV_EXIT_AT) && VCY_DEV_EXIT_AT == 2  // development build: where a wave's scalar instructions go (profiles/tools/salu_attribution.sh)
  {
    coop_leave();
    return;
  }
#endif
  const unsigned long long view_mask = kRows ? __ballot(pair_valid) : ((nviews >= 64) ? ~0ull : ((1ull << nviews) - 1ull));
  unsigned long long live = view_mask;  // pairs / views that may still change something (NB > 1: set here, from the kept minima)
  // (a launch covers fewer than 2^31 wave bricks: launch_carve_fused)
  // Views that cannot change this brick whatever its voxels hold now: every sample below the truncation limit, or
  // (kMax) not above the brick's minimum as the previous launch left it.  All of them: nothing to read or write.
  if (want_bound && !fresh && !(kOne && list_entry != nullptr)) {
    const bool have_min = UPDATE == VCY_UPDATE_MAX && (state_flags & kStateBrickMinValid) != 0 && brick_min != nullptr;
    if (TRUNC || have_min) {
      bool drop0 = TRUNC && lane_ub() < -1.0f;
      if (have_min) {
        float smin0;
        if constexpr (kRows) smin0 = pair_valid ? brick_min[brick_seg + pair_j] : 0.0f;  // (this lane's brick)
        else smin0 = ((cfloat_ptr)brick_min)[brick_lin];  // (uniform: a scalar load)
        drop0 = drop0 || lane_ub() <= smin0;  // (a brick with an untouched voxel holds lowest(): never true)
      }
      live = __ballot(!drop0) & view_mask;
      if (live == 0ull) {
        coop_leave();
        return;
      }
    }
  }
#ifdef VCY_PHASE_TIMING
  {
    asm volatile("" ::"v"(lane_ub()));
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();
    pt_acc[13] += t_ - pt_last;  // (includes slot 12)
  }
#endif

#if defined(VCY_DEV_EXIT_AT) && VCY_DEV_EXIT_AT == 3  // development build: where a wave's scalar instructions go (profiles/tools/salu_attribution.sh)
  {
    coop_leave();
    return;
  }
#endif
  // ---- load the wave brick's state ----------------------------------------------------------
  CountT* __restrict__ cnt = (CountT*)g.cnt;
  // update_num in registers: an int for kMax, a float for the weighted-average modes (see apply_sample)
  constexpr bool kFloatCount = UPDATE != VCY_UPDATE_MAX;
  typedef typename std::conditional<kFloatCount, float, int>::type NT;
  float s[WX];
  NT n[WX];
  // kMax on a fresh slab: the first live view of nearly every brick is `sure`, and its run (FIRST) overwrites all sixteen
  // registers -- the untouched state is only written out where something reads it: the checked paths, the write-back
  constexpr bool kLazyFresh = UPDATE == VCY_UPDATE_MAX && !TRUNC && !CHECKMAX && NB == 1;
  bool state_set = true;  // (uniform) false: fresh slab, s[] / n[] not yet formed
  auto set_fresh_state = [&]() {
    if constexpr (kLazyFresh) {
      if (!state_set) {
#pragma unroll
        for (int k = 0; k < WX; ++k) {
          s[k] = kInvalidSdf;
          n[k] = (NT)0;
        }
        state_set = true;
      }
    }
  };
  const int64_t row0 = ((int64_t)zl * g.ny + y) * g.nx;  // this lane's row; voxel k is at row0 + min(x_first + k, nx - 1)
  // The first view this brick will process is usually known BEFORE its state is: it is the first view the bounds do not
  // drop, and what the bounds are compared with -- the truncation limit, the brick minimum the previous launch left --
  // is already here.  Its tile is then requested right behind the state instead of after the state has arrived and been
  // looked at: one memory round trip less in a wave's chain, which is most of what a launch of ONE view consists of.
  // (kMax without valid minima: not known, vi_pre stays -1.  live_views() below decides as before; the request is
  // repeated there if it names another view -- it never does -- and loads complete in order, so the later one wins.)
  // (a launch that reuses its records has requested view 0's tile in its prologue on a fresh slab: vi_stale)
  int vi_pre = kRecRegs ? vi_stale : -1;
  auto prefetch_first_tile = [&]() {
    if constexpr (kRaw) {
      const bool listed_live = kOne && list_entry != nullptr;  // (the list pass has decided: the one view is live)
      const bool have_min = UPDATE == VCY_UPDATE_MAX && !fresh && (state_flags & kStateBrickMinValid) != 0 && brick_min != nullptr;
      if (!(fresh || UPDATE != VCY_UPDATE_MAX || !want_bound || have_min || listed_live)) return;
      bool drop = false;
      if (want_bound && !listed_live) {
        if (TRUNC) drop = lane_ub() < -1.0f;
        if (have_min) {
          const float smin0 = ((cfloat_ptr)brick_min)[brick_lin];
          // (lowest(): a voxel of the brick is untouched -- all_touched will be false and nothing is dropped by this rule)
          if (smin0 != kInvalidSdf) drop = drop || lane_ub() <= smin0;
        }
      }
      const unsigned long long lp = __ballot(!drop) & view_mask;
      vi_pre = lp ? (__ffsll((long long)lp) - 1) : nviews;
      if (vi_pre < nviews) prefetch_tile(vi_pre, raw_buf(0));
    }
  };
  // rows are whole bricks when nx % 8 == 0: the run is one 32-byte (sdf) and one 8/16-byte (update_num) vector
  const bool vec_io = (g.nx & (WX - 1)) == 0;
  typedef CountT CountVec __attribute__((ext_vector_type(WX)));
  if constexpr (kRows) {
    // The state of every live brick of the segment, requested NOW with LDS-direct loads into the wave's staging area
    // (row = the carving lane that owns it, 8 voxels per row): no registers, no waits -- the first tile wait below covers
    // them (loads complete in order).  An sdf request r is one z slice of a brick: lane L -> dword L & 7 of row
    // 8 r + (L >> 3), i.e. eight 32-byte row pieces; the pieces of the NB bricks of a row are requested back to back, so
    // the memory system sees the row's 128 contiguous bytes together.  Counters: 8 (u8) or 16 (u16) bytes per row.
#pragma unroll
    for (int k = 0; k < WX; ++k) {
      s[k] = kInvalidSdf;
      n[k] = (NT)0;
    }
    if (lane < NB) stage_mask[lane] = 0ull;  // (a brick that is never begun is neither read nor stored)
    if (!fresh) {
      const int yl = min(by * BY + (lane >> 3), g.ny - 1);
      const unsigned off_s = (unsigned)yl * (unsigned)g.nx + (unsigned)(lane & 7);   // (floats; + slice base + brick origin)
      constexpr int kCntPerDword = 4 / (int)sizeof(CountT);            // counters per dword: 4 (u8) or 2 (u16)
      constexpr int kCntDwordsPerRow = WX / kCntPerDword;              // 2 or 4
      constexpr int kCntRowsPerReq = 64 / kCntDwordsPerRow;            // 32 or 16 rows per request
      constexpr int kCntReqs = 64 / kCntRowsPerReq;                    // 2 or 4 requests per brick
      const int crow = lane / kCntDwordsPerRow;                        // row within a request
      typedef const CountT __attribute__((address_space(1))) * gcnt_ptr;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (((live >> (8 * j)) & 0xffull) == 0ull) continue;  // (uniform) no live view: neither read nor written
        const int xb = x_seg + j * WX;
#pragma unroll
        for (int r = 0; r < BZ; ++r) {
          const int zr = min(zl0 + r, g.nz_local - 1);
          gfloat_ptr src = (gfloat_ptr)g.sdf + ((int64_t)zr * g.ny * g.nx + xb);
          __builtin_amdgcn_global_load_lds(src + off_s, (lds_float*)(stage_s + (j * 64 + 8 * r) * WX), 4, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < kCntReqs; ++r) {
          const int row = r * kCntRowsPerReq + crow;  // = ly | lz << 3 of the lane that carves it
          const int yr = min(by * BY + (row & 7), g.ny - 1), zr = min(zl0 + (row >> 3), g.nz_local - 1);
          gcnt_ptr src = (gcnt_ptr)cnt + (((int64_t)zr * g.ny + yr) * g.nx + xb + (lane % kCntDwordsPerRow) * kCntPerDword);
          __builtin_amdgcn_global_load_lds((const uint32_t __attribute__((address_space(1)))*)src,
                                           (lds_u32*)(uint32_t*)(stage_n + (j * 64 + r * kCntRowsPerReq) * WX), 4, 0, 0);
        }
      }
    }
  } else if (fresh) {  // a fresh slab is known to be untouched everywhere: nothing to read
    if constexpr (kLazyFresh) {
      state_set = false;
    } else {
#pragma unroll
      for (int k = 0; k < WX; ++k) {
        s[k] = kInvalidSdf;
        n[k] = (NT)0;
      }
    }
  } else if (vec_io) {
    // (streaming LOADS of the state were measured too: 2.7 -> 5.3 ms per view, profiles/r06/nontemporal.txt)
    float4 a, b4;
    CountVec cv;
    if (kOne && eager) {  // (uniform) requested before the footprint record was looked at
      a = make_float4(eager_a.x, eager_a.y, eager_a.z, eager_a.w), b4 = make_float4(eager_b.x, eager_b.y, eager_b.z, eager_b.w);
      cv = eager_c;
    } else {
      a = *(const float4*)(g.sdf + row0 + x_first), b4 = *(const float4*)(g.sdf + row0 + x_first + 4);
      cv = *(const CountVec*)(cnt + row0 + x_first);
    }
    prefetch_first_tile();  // (behind the state's requests, in front of their first use)
    s[0] = a.x, s[1] = a.y, s[2] = a.z, s[3] = a.w, s[4] = b4.x, s[5] = b4.y, s[6] = b4.z, s[7] = b4.w;
#pragma unroll
    for (int k = 0; k < WX; ++k) n[k] = (NT)cv[k];
  } else {
#pragma unroll
    for (int k = 0; k < WX; ++k) {
      const int xk = min(x_first + k, g.nx - 1);
      s[k] = g.sdf[row0 + xk];
      n[k] = (NT)cnt[row0 + xk];
    }
  }

  // Every voxel of the brick touched (update_num >= 1)?  Wave-uniform; update_num never decreases, so
  // once true it stays true.  Selects the select-free update (update_max_touched) and one of the two
  // view-dropping rules.
  bool all_touched = false;
  auto refresh_all_touched = [&]() {
    if (UPDATE != VCY_UPDATE_MAX || all_touched) return;
    NT nmin = n[0];
#pragma unroll
    for (int k = 1; k < WX; ++k) nmin = min(nmin, n[k]);
    all_touched = __all(nmin >= (NT)1);
  };
  if (!fresh && !kRows) refresh_all_touched();
  // No voxel of the brick touched yet?  (Wave-uniform; true for every brick of a fresh slab.)  The first `sure`
  // view of such a brick is a plain store of the samples (carve_view_fast<FIRST>).
  bool none_touched = fresh != 0;
  auto refresh_none_touched = [&]() {
    NT nmax = n[0];
#pragma unroll
    for (int k = 1; k < WX; ++k) nmax = max(nmax, n[k]);
    none_touched = __all(nmax < (NT)1);
  };
  if (!kRows && !fresh && UPDATE == VCY_UPDATE_MAX && !all_touched) refresh_none_touched();
  // Weighted average: does every voxel of the brick carry the same update_num?  (Wave-uniform; true for a
  // fresh slab, and it stays true while every processed view updates every voxel -- the views whose tile
  // provably holds no sample below -1.)  Then the weights of the average, fn and 1 / (fn + 1), are the same
  // for the whole brick and are formed once per view instead of once per sample (carve_view_fast<UNIFORM>);
  // n[] is only brought up to date when the brick leaves this state, and at the write-back.
  bool uniform_cnt = false;
  float fnu = 0.0f;  // the common update_num (as a float, like n[])
  auto refresh_uniform_cnt = [&]() {
    if (UPDATE == VCY_UPDATE_MAX) return;
    if (fresh) {
      uniform_cnt = true;
      fnu = 0.0f;
    } else {
      const float f0 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((float)n[0])));
      bool same = true;
#pragma unroll
      for (int k = 0; k < WX; ++k) same = same && (float)n[k] == f0;
      uniform_cnt = __all(same);
      fnu = f0;
    }
  };
  if (!kRows) refresh_uniform_cnt();
  auto leave_uniform = [&]() {
    if (!uniform_cnt) return;
    uniform_cnt = false;
#pragma unroll
    for (int k = 0; k < WX; ++k) n[k] = (NT)fnu;
  };
  // views that may still change something, as a wave-uniform bit mask
  int jc = -1;  // NB > 1: the brick of the segment whose state is in registers
  // does this lane's view (pair) change nothing, as the state stands?  (`known`: the caller has established want_bound)
  auto dropped_now = [&](auto known) -> bool {
    bool drop = false;
    if (decltype(known)::value || want_bound) {
      if (TRUNC) drop = lane_ub() < -1.0f;
      if (UPDATE == VCY_UPDATE_MAX && all_touched) {
        float m = s[0];
#pragma unroll
        for (int k = 1; k < WX; ++k) m = fminf(m, s[k]);
        const float smin = wave_min(m);
        drop = drop || lane_ub() <= smin;
      }
    }
    return drop;
  };
  auto live_views = [&]() -> unsigned long long {
    const bool drop = dropped_now(std::false_type{});
    if constexpr (kRows) {  // (the bounds of the other bricks' pairs stand as they are)
      const unsigned long long cur_bits = 0xffull << (8 * jc);
      return (live & ~cur_bits) | (__ballot(!drop) & view_mask & cur_bits);
    }
    return __ballot(!drop) & view_mask;
  };
  // kRecRegs, behind a run that moved the brick: the lanes whose bound still stands (the compare's own mask -- __ballot
  // takes an int, and the mask came back through v_cndmask + v_cmp_ne)
  auto standing_bounds = [&]() -> unsigned long long {
    return __builtin_amdgcn_ballot_w64(!dropped_now(std::true_type{}));
  };
  // "no further view / pair" (kRecRegs: -1, what the lowest bit of an empty mask reads as)
  const int vi_end = kRecRegs ? -1 : (kRows ? 64 : nviews);
  // the lowest set bit of a uniform mask, -1 when it is empty: what s_ff1_i32_b64 returns (through __ffsll the empty
  // case is a compare and a select of its own)
  auto first_of = [&](unsigned long long mask) -> int {
    int r;
    asm("s_ff1_i32_b64 %0, %1" : "=s"(r) : "s"(mask));
    return r;
  };
  auto next_view = [&](unsigned long long live, int after) -> int {
    const unsigned long long rest = (after >= 63) ? 0ull : (live & ~((2ull << after) - 1ull));
    return rest ? (__ffsll((long long)rest) - 1) : vi_end;
  };

  // Lanes whose voxels changed (update_num grows with every change), accumulated over the views: what the write-back
  // stores.  (Round 3 re-read update_num from memory and compared: a dependent round trip in every wave's chain.  It
  // turned out not to be what bounds a single-view launch -- see DESIGN section 8 -- but there is no reason to keep it.)
  unsigned long long changed_lanes = 0ull;
  if (!kRows) live = live_views();
  int vi = live ? (__ffsll((long long)live) - 1) : vi_end;
  if (kRaw && (kRecRegs ? vi >= 0 : vi < vi_end) && vi != vi_pre) prefetch_tile(vi, raw_buf(0));
  if constexpr (kRecRegs) {  // the first view's scalar state (the prologue's request has taken its record apart itself)
    ahead = live & (live - 1ull);
    if (vi >= 0) cur_w1 = (uint32_t)__builtin_amdgcn_readlane((int)rec_w1, vi), cur_voff = view_byte_offset(vi);
  }
  // NB > 1: the brick whose turn it is takes its state from the staging area (the LDS-direct requests above have
  // landed once the wave has waited for its first tile) and leaves it there again when the next brick begins
  typedef CountT CountVecR __attribute__((ext_vector_type(WX)));
  typedef CountVecR __attribute__((address_space(3))) lds_countvec_r;
  auto finish_brick = [&]() {
    if constexpr (kRows) {
      leave_uniform();
      if (brick_min != nullptr && implied) {
        float m = s[0];
#pragma unroll
        for (int k = 1; k < WX; ++k) m = fminf(m, s[k]);
        const float smin = wave_min(m);
        if (lane == 0) brick_min[brick_lin] = smin;
      }
      lds_float4* rs = (lds_float4*)(float4*)(stage_s + (jc * 64 + lane) * WX);
      rs[0] = f4{s[0], s[1], s[2], s[3]};
      rs[1] = f4{s[4], s[5], s[6], s[7]};
      CountVecR cv;
#pragma unroll
      for (int k = 0; k < WX; ++k) cv[k] = (CountT)n[k];
      *(lds_countvec_r*)(CountVecR*)(stage_n + (jc * 64 + lane) * WX) = cv;
      if (lane == 0) stage_mask[jc] = fresh ? ~0ull : changed_lanes;
    }
  };
  auto begin_brick = [&](int j) {
    if constexpr (kRows) {
      jc = j;
      x_first = x_seg + j * WX;
      brick_lin = brick_seg + j;
      changed_lanes = 0ull;
      if (fresh) {
#pragma unroll
        for (int k = 0; k < WX; ++k) {
          s[k] = kInvalidSdf;
          n[k] = (NT)0;
        }
      } else {
        const lds_float4* rs = (const lds_float4*)(float4*)(stage_s + (j * 64 + lane) * WX);
        const f4 a = rs[0], b4 = rs[1];
        const CountVecR cv = *(const lds_countvec_r*)(CountVecR*)(stage_n + (j * 64 + lane) * WX);
        s[0] = a.x, s[1] = a.y, s[2] = a.z, s[3] = a.w, s[4] = b4.x, s[5] = b4.y, s[6] = b4.z, s[7] = b4.w;
#pragma unroll
        for (int k = 0; k < WX; ++k) n[k] = (NT)cv[k];
      }
      all_touched = false;
      none_touched = fresh != 0;
      if (!fresh) {
        refresh_all_touched();
        if (UPDATE == VCY_UPDATE_MAX && !all_touched) refresh_none_touched();
      }
      refresh_uniform_cnt();
    }
  };
  VCY_PT(0);
  VCY_PT_COUNT(10);

#if defined(VCY_DEV_EXIT_AT) && VCY_DEV_EXIT_AT == 4  // development build: where a wave's scalar instructions go (profiles/tools/salu_attribution.sh)
  {
    coop_leave();
    return;
  }
#endif
  // ---- views ------------------------------------------------------------------------------
  int n_processed = 0;  // (wave-uniform: an SGPR; only read with "paircount" on)
  const bool is_ortho = GEN && mode.ortho != 0, is_nn = GEN && mode.interp == VCY_INTERP_NN;
  // What a view's run works with, set by begin_view() for the view `vi`: its parameters, this brick's record of x
  // products, the next live view (whose tile is in flight), the tile's geometry, c1 + c2 of this lane.
  // (the view records are read-only for the whole launch: the constant address space keeps their fields in scalar
  // loads -- through a plain pointer that is carried from one loop to the other they became vector loads with a
  // vmcnt(0) wait in front of every run)
  typedef const ViewParams __attribute__((address_space(4))) cview;
  cview* vp = nullptr;
  cfloat_ptr c0 = nullptr;
  int vnext = vi_end;
  float pitchf = 0.0f;
  int base = 0, big_pitch = 0;
  const lds_float* rawcur = nullptr;
  float h12x = 0.0f, h12y = 0.0f, h12z = 0.0f;
  typedef const char __attribute__((address_space(4))) cbyte;
  auto view_at = [&](uint32_t voff) -> cview* { return (cview*)((cbyte*)views + voff); };  // (FusedView::v comes first)
  static_assert(offsetof(FusedView, v) == 0, "view_at");
  // kRecRegs: the next live view from `vnext` on -- its record, taken apart once, and the request of its tile
  auto request_next = [&]() {
    if (vnext < 0) {
      nxt_w1 = 0u;  // (not `sure`: the run loop ends)
      return;
    }
    nxt_w0 = (uint32_t)__builtin_amdgcn_readlane((int)rec_w0, vnext);
    nxt_w1 = (uint32_t)__builtin_amdgcn_readlane((int)rec_w1, vnext);
    nxt_voff = view_byte_offset(vnext);
    if (footprint_has_tile(nxt_w1)) raw_prefetch_step(view_at(nxt_voff), nxt_w0, nxt_w1, lane, raw_buf(cur ^ 1));
  };
  auto begin_view = [&]() {
    const int vv = kRows ? (vi & 7) : vi;  // the view of pair vi
    const ViewParams& v = views[vv].v;
    if constexpr (kRecRegs) {  // (both from 32-bit offsets: carve_offsets_fit_32)
      vp = view_at(cur_voff);
      c0 = (cfloat_ptr)((cbyte*)c0_all + c0_byte_offset(vi, c0_per_view, x_first / WX));
    } else {
      vp = (cview*)&v;
      // this view's record of the wave brick's x products: (x, y) pairs at [2 k], z at [16 + k]
      c0 = (cfloat_ptr)(c0_all + ((size_t)vv * (nxp / WX) + (x_first / WX)) * kC0Stride);
    }
    // stage this view's tile (wave-private: program order is enough)
    VCY_SETPRIO(3);
    wave_lds_fence();
    if (kRaw) {
      raw_tile_wait();  // this view's pixels have landed in raw_buf(cur)
    } else {
      tile_fill(v, tile_of(vi), lane, (float*)tile);
    }
    wave_lds_fence();
    // the next live view's tile is fetched while this one is computed
    if constexpr (kRecRegs) {
      vnext = first_of(ahead);
      request_next();
    } else {
      vnext = next_view(live, vi);
      if (kRaw && vnext < vi_end) prefetch_tile(vnext, raw_buf(cur ^ 1));
    }
    ++n_processed;
    if constexpr (kRecRegs) {  // (a raw tile's pitch is 16; a record without a tile is never sampled from)
      pitchf = (float)kTileRaw, base = footprint_step_base(cur_w1);
    } else {
      pitchf = tile_of(vi).pitchf, base = tile_of(vi).base;
    }
    big_pitch = kRaw ? 16 : (int)pitchf;  // pixels per row of the big tile
    rawcur = (const lds_float*)raw_buf(cur);
    // c1 + c2 of this lane's (y, z): the inner sum of pc = t + (c0 + (c1 + c2)) (voxel_carver.cc:453)
    h12x = vp->r[0][1] * py + vp->r[0][2] * pz, h12y = vp->r[1][1] * py + vp->r[1][2] * pz;
    h12z = vp->r[2][1] * py + vp->r[2][2] * pz;
    VCY_SETPRIO(0);
    VCY_PT(1);
  };
  // Behind a view's run: what the views that follow ask of the state, and the step to the next live view.
  // kRecRegs: the step to the next live view, behind a re-bound if the run calls for one
  auto step_rec = [&](bool rebound) {
    if (rebound) {
      ahead &= standing_bounds();  // (min(sdf) only grows: a bound that fell stays fallen)
      const int v2 = first_of(ahead);
      if (v2 != vnext) {
        vnext = v2;
        // (the dropped view's pixels may still be arriving in that buffer: loads complete in order)
        request_next();
      }
    }
    // the next view becomes the view in hand, with what was taken out of its record when its tile was requested
    vi = vnext, cur_w1 = nxt_w1, cur_voff = nxt_voff;
    ahead &= ahead - 1ull;  // (its bit is the lowest one; an empty mask stays empty)
    cur ^= 1;
    VCY_PT(5);
  };
  auto end_view = [&](bool brick_moved) {
    VCY_SETPRIO(3);
    if (brick_moved) VCY_PT_COUNT(11);
    none_touched = false;  // (a checked view may have touched only some voxels)
    if (!kOne) refresh_all_touched();  // (only the views that follow ask)

    // state moved: some of the remaining views may have become droppable (min(sdf) only grows)
    // (an unchanged brick leaves every bound comparison as it was)
    if constexpr (kRecRegs) {
      step_rec(want_bound && brick_moved);
      return;
    }
    if (!kOne && want_bound && UPDATE == VCY_UPDATE_MAX && brick_moved) {
      live = live_views();
      const int v2 = next_view(live, vi);
      if (v2 != vnext) {
        vnext = v2;
        // (the dropped view's pixels may still be arriving in that buffer: loads complete in order)
        if (kRaw && vnext < vi_end) prefetch_tile(vnext, raw_buf(cur ^ 1));
      }
    }
    vi = vnext;
    cur ^= 1;
    VCY_PT(5);
  };
  // TileInfo::sure of the view end_view() stepped to when it is another select-free run of the brick in registers
  // (bit 0 set), else 0.
  auto next_fast_bits = [&]() -> int {
    if constexpr (kRecRegs) return footprint_sure(cur_w1);  // (0 when there is no further view)
    if (kOne || vi >= vi_end) return 0;
    if (kRows && (vi >> 3) != jc) return 0;  // (the pair belongs to another brick of the segment)
    const int bits = sure_of(vi);
    return (bits & 1) != 0 ? bits : 0;
  };
  while (kRecRegs ? vi >= 0 : vi < vi_end) {
    if constexpr (kRows) {
      if ((vi >> 3) != jc) {  // (uniform) the next pair belongs to another brick of the segment
        raw_tile_wait();      // everything requested so far has landed: the state of every brick, this pair's tile
        wave_lds_fence();
        if (jc >= 0) finish_brick();
        begin_brick(vi >> 3);
        // the bounds of this brick's pairs against its state as it really is (the kept minima may be invalid or absent)
        live = live_views();
        if (((live >> vi) & 1ull) == 0ull) {
          vi = next_view(live, vi);
          // (the dropped pair's pixels may still be arriving in that buffer: loads complete in order)
          if (vi < vi_end) prefetch_tile(vi, raw_buf(cur));
          continue;
        }
      }
    }
    begin_view();
    // the four taps of the sample whose upper left pixel is tile element idx
    auto quad_at = [&](unsigned idx) -> float4 {
      if constexpr (kRaw) {
        const lds_float* p = rawcur + idx;
        return make_float4(p[0], p[1], p[16], p[17]);
      } else {
        const lds_float* p = (const lds_float*)(float*)tile + idx;
        const lds_float* p2 = p + big_pitch;
        return make_float4(p[0], p[1], p2[0], p2[1]);
      }
    };

    // Straight-line fast path for the 8 voxels of this thread (no divergent control flow, so
    // the eight LDS reads and the arithmetic interleave); voxels the tile does not cover are
    // only recorded here and handled below.  SURE: the prologue has proved that every voxel of the
    // brick samples inside this tile (TileInfo::sure), so the per-voxel tests are compiled out.
    auto carve_view = [&](auto sure_tag) {
      constexpr bool SURE = decltype(sure_tag)::value;
      cview& v = *vp;
      // the closed range of (u, w) whose taps are in the tile (kRecRegs: formed here, only the checked loop asks)
      float lo_x, hi_x, lo_y, hi_y;
      if constexpr (kRecRegs) {
        const FootprintBounds fb = footprint_bounds(rec_of(vi));
        lo_x = fb.lo_x, hi_x = fb.hi_x, lo_y = fb.lo_y, hi_y = fb.hi_y;
      } else {
        lo_x = tile_of(vi).lo_x, hi_x = tile_of(vi).hi_x;
        lo_y = tile_of(vi).lo_y, hi_y = tile_of(vi).hi_y;
      }
      bool slow[WX];
      bool any_slow = false;
      bool moved = false;  // some voxel of this lane changed
      // Every operation is the reference's, in its order, as plain fp32 instructions.
#pragma unroll
      for (int k = 0; k < WX; ++k) {
        const float pcz = v.t[2] + (c0[16 + k] + h12z);
        // pinhole: u = fx / z * x + cx (camera.cc:133-136); orthographic: u = x (camera.cc:201-205)
        float qx = 1.0f, qy = 1.0f;
        if (!is_ortho) {
          qx = div_view<DIV>(v.fx, pcz);
          qy = SAMEF ? qx : div_view<DIV>(v.fy, pcz);
        }
        const float pcx = v.t[0] + (c0[2 * k] + h12x), pcy = v.t[1] + (c0[2 * k + 1] + h12y);
        const float u = is_ortho ? pcx : qx * pcx + v.cx;
        const float w = is_ortho ? pcy : qy * pcy + v.cy;
        bool in_tile = true;
        if (!SURE) {
          // orthographic: only `pc.z < 0` is skipped (voxel_carver.cc:456)
          const bool zfast = is_ortho ? !(pcz < 0.0f) : in_fast_div_range(pcz);
          in_tile = zfast && u >= lo_x && u <= hi_x && w >= lo_y && w <= hi_y;
          slow[k] = !in_tile;
          any_slow = any_slow || !in_tile;
        }
        const float fu = floorf(u), fw = floorf(w);
        const float lu = u - fu, lv = w - fw;
        const float mu = 1.0f - lu, mv = 1.0f - lv;
        // any index is harmless when !in_tile (the sample is discarded); keep it inside the tile
        unsigned idx = (unsigned)((int)__builtin_fmaf(fw, pitchf, fu) + base);
        if (!SURE) idx = min(idx, (unsigned)(kRaw ? 256 - 18 : max(kBigPixels - big_pitch - 2, 0)));
        const float4 q = quad_at(idx);
        // ((1-lu)(1-lv)) s00 + (lu (1-lv)) s10 + ((1-lu) lv) s01 + (lu lv) s11, summed left to right (:69-73)
        float dist = ((((mu * mv) * q.x) + ((lu * mv) * q.y)) + ((mu * lv) * q.z)) + ((lu * lv) * q.w);
        if (is_nn) {
          // SdfInterpolationNn (voxel_carver.cc:16-38): round half away from zero == floor + (frac >= .5)
          // for the non-negative in-ROI coordinates; the quad already holds the ROI-clamped neighbours
          const float top = lu >= 0.5f ? q.y : q.x, bot = lu >= 0.5f ? q.w : q.z;
          dist = lv >= 0.5f ? bot : top;
        }
        bool ok = in_tile;
        if (TRUNC) ok = ok && !(dist < -1.0f);
        if (CHECKMAX) ok = ok && !(n[k] > (NT)g.max_update_num);
        moved = apply_sample<UPDATE>(ok, dist, g.weight, s[k], n[k]) || moved;
      }
      if (!SURE && any_slow) {
#pragma unroll
        for (int k = 0; k < WX; ++k) {
          if (slow[k]) {
            float dist = 0.0f;
            bool ok = sample_generic((const ViewParams*)vp, mode, g.px[min(x_first + k, g.nx - 1)], py, pz, &dist);
            if (CHECKMAX) ok = ok && !(n[k] > (NT)g.max_update_num);
            moved = apply_sample<UPDATE>(ok, dist, g.weight, s[k], n[k]) || moved;
          }
        }
      }
      const unsigned long long mv = __ballot(moved);
      changed_lanes |= mv;
      return mv != 0ull;
    };
    // ---- select-free fast path -------------------------------------------------------------
    // A `sure` tile (every sample provably inside it and inside div_view2's depth range) whose update
    // needs no per-voxel case distinction: kMax on a brick that is touched everywhere, or the unit-weight
    // average on a state with "update_num == 0 implies sdf == lowest()".  Same operations as above, in
    // the same order; what changes is what they cost on the SIMD:
    //  - the LDS byte address of the taps comes out of the float pipeline: a = fw * (bytes per tile row) +
    //    (fu * (bytes per element) + (element size * base + tile offset)), every term an integer below 2^22,
    //    evaluated in units of 2^-149 so that the bits of the result ARE the address (2 fma instead of fma,
    //    cvt, shift-add);
    //  - the two wave-uniform terms of that sum sit in VGPRs (back-to-back scalar operands halve the issue rate);
    //  - the update is a compare / select / carry chain through VCC (update_max_touched), or a plain store for
    //    a brick that has not been touched at all (FIRST).
    // (GEN kernels take them too: nearest-neighbour taps and orthographic projection are uniform branches
    // inside the run)
    constexpr bool kFastMax = UPDATE == VCY_UPDATE_MAX && !TRUNC && !CHECKMAX;
    constexpr bool kFastWa = UPDATE == kUpdateWaUnitWeight && !CHECKMAX;
    // general weights: only the brick-wide flavour (UNIFORM) of the run, where the weights are formed once per view
    constexpr bool kFastWaGeneral = UPDATE == VCY_UPDATE_WEIGHTED_AVERAGE && !CHECKMAX;
    // FIRST: no voxel of the brick has been touched yet (a fresh slab): the update is `sdf = dist, update_num = 1`
    // for every voxel (voxel_carver.cc:482-486), whatever the old value.
    // NOTRUNC: the prologue has proved that no sample of this tile is below -1 (TileInfo::sure bit 1): the
    // truncation test of the weighted average and its two selects are compiled out.
    // UNIFORM (implies NOTRUNC): every voxel has update_num == fnu before this view and is updated by it.
    auto carve_view_fast = [&](auto first_tag, auto notrunc_tag, auto uniform_tag) -> bool {
      constexpr bool FIRST = decltype(first_tag)::value;
      constexpr bool NOTRUNC = decltype(notrunc_tag)::value;
      constexpr bool UNIFORM = decltype(uniform_tag)::value;
      cview& v = *vp;
      // the brick's common weights, in VGPRs (uniform values; opaque to the compiler so that they are not
      // folded back into scalar operands): (fn * sdf + dist) * (1 / (fn + 1)), voxel_carver.cc:88-95
      float fn_v = 0.0f, inv_v = 0.0f, wgt_v = 1.0f;
      if constexpr (UNIFORM) {
        const float f1 = fnu + 1.0f;
        asm volatile("v_mov_b32_e32 %0, %1" : "=v"(fn_v) : "s"(fnu));
        if constexpr (UPDATE == kUpdateWaUnitWeight) {
          inv_v = rcp_count(fn_v + 1.0f);
        } else {  // (w * n, w and 1 / (w * (n + 1)) of voxel_carver.cc:91-93)
          asm volatile("v_mov_b32_e32 %0, %1" : "=v"(wgt_v) : "s"(g.weight));
          inv_v = div_fast(1.0f, wgt_v * (fn_v + 1.0f));
          fn_v = wgt_v * fn_v;
        }
        fnu = f1;
      }
      // uniform -> VGPR (opaque to the compiler, which would otherwise fold them back into SGPR operands)
      float pitch16, cmagic;
      constexpr int kElemB = 4;                 // bytes per tile element (a pixel)
      // The address sum is carried out in units of 2^-149, i.e. in denormals (fp32 denormals are on for this
      // library and v_fma_f32 handles them at full rate): the bit pattern of the result IS the integer, no
      // mask or conversion needed.  The constant may be negative (base < 0); the final sum never is.
      constexpr float kAddrUnit = 0x1p-149f;
      {
        const float p16 = pitchf * ((float)kElemB * kAddrUnit);  // bytes per tile row; pitch <= 512: exact
        const unsigned lds_off = kRaw ? (unsigned)(size_t)rawcur : (unsigned)(size_t)(const lds_float*)(float*)tile;
        const int ci = kElemB * base + (int)lds_off;  // |16 base| < 2^22 (TileInfo::sure)
        const float cm = ci < 0 ? -__int_as_float(-ci) : __int_as_float(ci);
        asm volatile("v_mov_b32_e32 %0, %1" : "=v"(pitch16) : "s"(p16));
        asm volatile("v_mov_b32_e32 %0, %1" : "=v"(cmagic) : "s"(cm));
      }
      // Four voxels at a time.  Phase A: image coordinates, fractions and the LDS reads (in flight
      // together); phase B: weights, sample, update.
      unsigned long long took = 0;
      constexpr int kGroup = VCY_FAST_GROUP;
#pragma unroll
      for (int k0 = 0; k0 < WX; k0 += kGroup) {
        float lu[kGroup], lv[kGroup];
        f4 q[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
          const int k = k0 + j;
          const float pcz = v.t[2] + (c0[16 + k] + h12z);
          const float qx = div_view<DIV>(v.fx, pcz);
          const float qy = SAMEF ? qx : div_view<DIV>(v.fy, pcz);
          const float pcx = v.t[0] + (c0[2 * k] + h12x), pcy = v.t[1] + (c0[2 * k + 1] + h12y);
          float u = qx * pcx + v.cx, w = qy * pcy + v.cy;
          if constexpr (GEN) {
            if (is_ortho) u = pcx, w = pcy;  // (uniform) camera.cc:201-205
          }
          const float fu = floorf(u), fw = floorf(w);
          lu[j] = u - fu;
          lv[j] = w - fw;
          const float a = __builtin_fmaf(fw, pitch16, __builtin_fmaf(fu, (float)kElemB * kAddrUnit, cmagic));
          const unsigned addr = __float_as_uint(a);
          const lds_float* tp = (const lds_float*)(size_t)addr;
          if constexpr (kRaw) {
            q[j] = f4{tp[0], tp[1], tp[16], tp[17]};
          } else {
            const lds_float* tp2 = tp + big_pitch;
            q[j] = f4{tp[0], tp[1], tp2[0], tp2[1]};
          }
        }
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
          const int k = k0 + j;
          const float mu = 1.0f - lu[j], mv = 1.0f - lv[j];
          float dist =
              ((((mu * mv) * q[j].x) + ((lu[j] * mv) * q[j].y)) + ((mu * lv[j]) * q[j].z)) + ((lu[j] * lv[j]) * q[j].w);
          if constexpr (GEN) {
            if (is_nn) {  // (uniform) SdfInterpolationNn, as in the checked loop above
              const float top = lu[j] >= 0.5f ? q[j].y : q[j].x, bot = lu[j] >= 0.5f ? q[j].w : q[j].z;
              dist = lv[j] >= 0.5f ? bot : top;
            }
          }
          if constexpr (FIRST) {
            s[k] = dist;
            n[k] = (NT)1;
          } else if constexpr (kFastMax) {
            update_max_touched(dist, s[k], n[k], took);
          } else if constexpr (UNIFORM) {
            if constexpr (UPDATE == kUpdateWaUnitWeight) s[k] = (fn_v * s[k] + dist) * inv_v;
            else s[k] = (fn_v * s[k] + wgt_v * dist) * inv_v;
          } else if constexpr (kFastWa) {
            update_wa_unit<TRUNC && !NOTRUNC>(dist, s[k], n[k], took);
          }
        }
      }
      // every lane took every sample, unless the update was conditional (kMax on a touched brick, the truncating average)
      constexpr bool kConditional = !FIRST && !UNIFORM && (kFastMax || (kFastWa && TRUNC && !NOTRUNC));
      changed_lanes |= kConditional ? took : ~0ull;
      if constexpr (kRecRegs) moved_mask = (kFastMax && !FIRST) ? took : ~0ull;
      return (kFastMax && !FIRST) ? took != 0ull : true;
    };
    bool brick_moved;
    int sure_bits;
    if constexpr (kRecRegs) sure_bits = footprint_sure(cur_w1);
    else sure_bits = sure_of(vi);
    const bool sure = (sure_bits & 1) != 0, never_truncated = (sure_bits & 2) != 0;
    // (Branch weights: the checked loops below are the rare ones in the kernels that have a select-free loop;
    // the register allocator then spills there, if anywhere, and not in the loops that do the work.)
    const bool fast_first = kFastMax && sure && none_touched;
    const bool fast_next = (kFastMax && sure && all_touched) || (kFastWa && sure && implied);
    // general weights: every voxel updated by this view and all counts equal -- a first touch stores the sample
    // (voxel_carver.cc:482-486), later views average with the brick's weights
    const bool fast_general = kFastWaGeneral && sure && uniform_cnt && (!TRUNC || never_truncated);
    if (kLazyFresh && fast_first) state_set = true;  // (FIRST writes every s[k], n[k])
    else set_fresh_state();
    if (kFastWaGeneral && __builtin_expect_with_probability(fast_general, 1, 0.9)) {
      if (fnu < 1.0f) {
        brick_moved = carve_view_fast(std::true_type{}, std::false_type{}, std::false_type{});
        fnu = 1.0f;
      } else {
        brick_moved = carve_view_fast(std::false_type{}, std::true_type{}, std::true_type{});
      }
      VCY_PT(2);
      VCY_PT_COUNT(7);
    } else if (kFastMax && __builtin_expect_with_probability(fast_next || fast_first, 1, 0.99)) {
      // kMax, select-free.  The first touch of an untouched brick (FIRST, a plain store of the samples: it leaves the
      // brick touched everywhere) and the runs of every `sure` view that follows are a loop of their own: the state --
      // s[], n[] -- is carried by that loop's back edge alone and stays in the registers the update chains work on.
      // (As one of five paths that met behind the view, the run ended with 16 register moves into the set the other
      // paths leave the state in, and the loop latch moved all 16 back: 32 of 328 vector instructions per pair,
      // profiles/view_loop.)  A view that is not `sure` leaves the loop and comes back in through the checked paths below.
      // run(): one select-free run and the step to the view behind it; is that view another one of this loop?
      auto run = [&](auto first_tag) -> bool {
        brick_moved = carve_view_fast(first_tag, std::false_type{}, std::false_type{});
        VCY_PT(2);
        VCY_PT_COUNT(7);
        end_view(brick_moved);
        if (!all_touched || (next_fast_bits() & 1) == 0) return false;
        begin_view();
        return true;
      };
      if constexpr (kRecRegs) {
        // (the same loop; what says whether it goes on is the next view's `sure` bit itself, an integer tested where
        // it is needed -- as run()'s bool it was carried to the latch as a lane mask and tested there a second time)
        auto run_rec = [&](auto first_tag) -> uint32_t {
          brick_moved = carve_view_fast(first_tag, std::false_type{}, std::false_type{});
          VCY_PT(2);
          VCY_PT_COUNT(7);
          // end_view() for a run of this loop.  The brick is touched everywhere -- FIRST stores every voxel, the others
          // are only entered on such a brick; said here, the tests of it fold away instead of living on as lane masks
          // -- and "moved, and a re-bound is wanted" is one AND of two masks.
          VCY_SETPRIO(3);
          if (brick_moved) VCY_PT_COUNT(11);
          none_touched = false, all_touched = true;
          step_rec((moved_mask & rebound_mask) != 0ull);
          uint32_t go_on = cur_w1 & (1u << 30);
          if (go_on != 0u) begin_view();
          // (opaque BEHIND the join: the loop keeps one exit, at its latch, tested with one compare.  Threaded through
          // the `if`, the two exits were merged again with a lane-mask flag.)
          asm volatile("" : "+s"(go_on));
          return go_on;
        };
        uint32_t more_rec = 1u;
        if (fast_first) more_rec = run_rec(std::true_type{});
        while (more_rec != 0u) more_rec = run_rec(std::false_type{});
        continue;
      }
      bool more = true;
      if (fast_first) more = run(std::true_type{});
      while (more) more = run(std::false_type{});
      continue;
    } else if (kFastWa && __builtin_expect_with_probability(fast_next, 1, 0.9)) {
      // weighted average: no truncation test when it cannot fire, and brick-wide weights while the counts agree.
      // (One pass through the outer loop per view.  Loops of their own for the three flavours, like kMax has above, take
      // the 25 register moves per pair out of these runs too, but the allocator then spills inside them: scratch 64 ->
      // 112 bytes, 25.6 -> 33.5 ms per step in --mode tsdf -- profiles/view_loop/README.md.)
      const bool all_updated = kFastWa && (!TRUNC || never_truncated);
      if (kFastWa && all_updated && uniform_cnt) {
        brick_moved = carve_view_fast(std::false_type{}, std::true_type{}, std::true_type{});
      } else if (kFastWa && all_updated) {
        brick_moved = carve_view_fast(std::false_type{}, std::true_type{}, std::false_type{});
      } else {
        if (kFastWa) leave_uniform();
        brick_moved = carve_view_fast(std::false_type{}, std::false_type{}, std::false_type{});
      }
      VCY_PT(2);
      VCY_PT_COUNT(7);
    } else if (sure) {
      leave_uniform();
      brick_moved = carve_view(std::true_type{});
      VCY_PT(3);
      VCY_PT_COUNT(8);
    } else {
      leave_uniform();
      brick_moved = carve_view(std::false_type{});
      VCY_PT(4);
      VCY_PT_COUNT(9);
    }
    end_view(brick_moved);
  }

  // ---- write back what changed (update_num grows with every change) ----------------------------
  if constexpr (kRows) {
    if (jc >= 0) finish_brick();
    wave_lds_fence();
    if (pair_count != nullptr && lane == 0) atomicAdd(&pair_count[bz], (unsigned long long)n_processed);
    // Whole row segments: request i writes z slice i of the segment -- lane L the 16-byte chunk L & 7 of voxel row
    // 8 i + (L >> 3), so 8 lanes store the 128 contiguous bytes the segment has in that row (NB = 4) -- for the rows
    // whose carving lane changed (stage_mask of the chunk's brick; every row of a fresh slab).
    {
      const int yw = by * BY + (lane >> 3), c16 = lane & 7, jw = c16 >> 1;
      const unsigned long long mw = jw < NB ? stage_mask[jw] : 0ull;
      const bool col_ok = jw < NB && yw < g.ny && x_seg + 4 * c16 < g.nx;
#pragma unroll
      for (int i = 0; i < BZ; ++i) {
        const int row = 8 * i + (lane >> 3);
        if (zl0 + i < g.nz_local && col_ok && ((mw >> row) & 1ull) != 0ull) {
          const f4 q = *(const lds_float4*)(float4*)(stage_s + (jw * 64 + row) * WX + (c16 & 1) * 4);
          *(float4*)(g.sdf + (((int64_t)(zl0 + i) * g.ny + yw) * g.nx + x_seg + 4 * c16)) = make_float4(q.x, q.y, q.z, q.w);
        }
      }
      // counters: lane L the 8 (u8) / 16 (u16) bytes brick L & 3 has in voxel row 16 i + (L >> 2)
      const int jn = lane & 3;
      const unsigned long long mn = jn < NB ? stage_mask[jn] : 0ull;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 16 * i + (lane >> 2);
        const int yn = by * BY + (row & 7), zn = zl0 + (row >> 3);
        if (jn < NB && yn < g.ny && zn < g.nz_local && x_seg + WX * jn < g.nx && ((mn >> row) & 1ull) != 0ull) {
          const CountVecR cv = *(const lds_countvec_r*)(CountVecR*)(stage_n + (jn * 64 + row) * WX);
          *(CountVecR*)(cnt + (((int64_t)zn * g.ny + yn) * g.nx + x_seg + WX * jn)) = cv;
        }
      }
    }
    return;
  }
  leave_uniform();
  set_fresh_state();  // (no view was processed)
  // Where this lane's run lies is worked out again from the thread id (opaque to the compiler): kept from the prologue
  // it occupies three registers through every view, and the weighted-average kernels are short of exactly those --
  // their loop pre-header spilled to scratch, which every wave executes.
  int tid_w = (int)threadIdx.x;
  asm volatile("" : "+v"(tid_w));
  const int lane_w = tid_w & 63;
  const int y_w = by * BY + (lane_w & (BY - 1)), zl_w = zl0 + (lane_w >> 3);
  const bool lane_valid_w = y_w < g.ny && zl_w < g.nz_local;
  const int64_t row0_w = ((int64_t)min(zl_w, g.nz_local - 1) * g.ny + min(y_w, g.ny - 1)) * g.nx;
  // ("paircount" 1: (brick, view) pairs processed, per brick layer of the launch -- what the slab planner's
  // estimate is checked against, and what bench.py reports as the fraction of pairs the scene leaves)
#if defined(VCY_DEV_EXIT_AT) && VCY_DEV_EXIT_AT == 5  // development build: where a wave's scalar instructions go (profiles/tools/salu_attribution.sh)
  {
    coop_leave();
    return;
  }
#endif
  if (pair_count != nullptr && lane == 0) atomicAdd(&pair_count[bz], (unsigned long long)n_processed);
  if (brick_min != nullptr && implied) {  // (lanes outside the grid hold copies of voxels inside it)
    float m = s[0];
#pragma unroll
    for (int k = 1; k < WX; ++k) m = fminf(m, s[k]);
    const float smin = wave_min(m);
    if (lane == 0) brick_min[brick_lin] = smin;
  }
  if (coop) {
    // Cooperative write-back.  A wave's own stores are 64 pieces of 16 bytes in 64 different rows; the 128-byte line of
    // a row is completed by the other three waves of the workgroup at other times, and in a launch that also READS the
    // state (a view over a carved grid) the L2 writes such lines back before they are complete: 10.4 GB written for
    // 6.4 GB of state at 1024^3 in weighted-average mode, and four write requests where one would do
    // (profiles/r04/per_view_tsdf_pmc.txt).  Here every wave leaves its runs in LDS (row = lane, columns of its brick),
    // and after one barrier the waves share out the 64 rows of the workgroup's 32 x 8 x 8 block: 8 lanes = one
    // 128-byte row segment of sdf, 4 lanes = one row segment of update_num.  A row is stored when the lane that owned
    // it changed (coop_mask: a wave that left early, or a lane outside the grid, owns none).
    const bool changed = lane_valid_w && (fresh != 0 || ((changed_lanes >> lane_w) & 1ull) != 0ull);
    const unsigned long long my_mask = __ballot(changed);
    {
      lds_float4* rs = (lds_float4*)(float4*)(coop_s + lane_w * kCoopSdfPitch + wave * WX);
      rs[0] = f4{s[0], s[1], s[2], s[3]};
      rs[1] = f4{s[4], s[5], s[6], s[7]};
      CountVec8 cv;
#pragma unroll
      for (int k = 0; k < WX; ++k) cv[k] = (CountT)n[k];
      *(lds_countvec*)(CountVec8*)(coop_n + lane_w * coop_cnt_pitch<CountT>() + wave * WX) = cv;
      if (lane == 0) coop_mask[wave] = my_mask, coop_mask[kWgWaves + wave] = 1ull;
    }
    __syncthreads();
    // the row groups are dealt to the waves that are still here (a wave whose every view was dropped has left)
    int n_here = 0, my_rank = 0;
#pragma unroll
    for (int w = 0; w < kWgWaves; ++w) {
      const int here = __builtin_amdgcn_readfirstlane((int)coop_mask[kWgWaves + w]);
      n_here += here;
      my_rank += (w < wave) ? here : 0;
    }
    const int xb = bx * BX;
    // sdf: a row of the block is 2 kWgWaves chunks of 16 bytes, an instruction covers 64 / (2 kWgWaves) rows
    constexpr int kSdfChunks = 2 * kWgWaves, kSdfRows = 64 / kSdfChunks;
    for (int gi = my_rank; gi < 64 / kSdfRows; gi += n_here) {
      const int r = gi * kSdfRows + lane / kSdfChunks, ch = lane % kSdfChunks;
      if ((coop_mask[ch >> 1] >> r) & 1ull) {
        const f4 v = *(lds_float4*)(float4*)(coop_s + r * kCoopSdfPitch + ch * 4);
        const int64_t rowg = ((int64_t)(zl0 + (r >> 3)) * g.ny + (by * BY + (r & 7))) * g.nx;
        // (whole 128-byte row segments: as streaming stores when the launch asks for it -- kStateStreamStore.  A scalar
        // base with 32-bit offsets instead of these 64-bit row addresses was measured in round 6: 23 vector instructions
        // fewer per wave, 18 scalar ones more, +1 % in time -- profiles/r06/one_view.txt)
        if (nt_store) __builtin_nontemporal_store(v, (f4*)(g.sdf + rowg + xb + ch * 4));
        else *(float4*)(g.sdf + rowg + xb + ch * 4) = make_float4(v.x, v.y, v.z, v.w);
      }
    }
    // update_num: kWgWaves chunks of 8 counters per row, 64 / kWgWaves rows per instruction
    constexpr int kCntRows = 64 / kWgWaves;
    for (int gi = my_rank; gi < 64 / kCntRows; gi += n_here) {
      const int r = gi * kCntRows + lane / kWgWaves, ch = lane % kWgWaves;
      if ((coop_mask[ch] >> r) & 1ull) {
        const CountVec8 cv = *(lds_countvec*)(CountVec8*)(coop_n + r * coop_cnt_pitch<CountT>() + ch * WX);
        const int64_t rowg = ((int64_t)(zl0 + (r >> 3)) * g.ny + (by * BY + (r & 7))) * g.nx;
        if (nt_store) __builtin_nontemporal_store(cv, (CountVec8*)(cnt + rowg + xb + ch * WX));
        else *(CountVec8*)(cnt + rowg + xb + ch * WX) = cv;
      }
    }
  } else if (lane_valid_w) {
    if (vec_io) {
      bool changed = fresh != 0;  // (a fresh slab has never been written: every voxel is stored)
#ifdef VCY_FLOOR_NO_STORES  // development build (issue floor): results stay live, nothing is stored
      {  // (every value stays live: a dead s[k] would take its whole update chain with it)
        float ssum = 0.0f, nsum = 0.0f;
#pragma unroll
        for (int k = 0; k < WX; ++k) ssum += s[k], nsum += (float)n[k];
        changed = ssum == 1.2345e-30f && nsum == 777.25f;
      }
#else
      changed = changed || ((changed_lanes >> lane_w) & 1ull) != 0ull;
#endif
      if (changed) {
        *(float4*)(g.sdf + row0_w + x_first) = make_float4(s[0], s[1], s[2], s[3]);
        *(float4*)(g.sdf + row0_w + x_first + 4) = make_float4(s[4], s[5], s[6], s[7]);
        CountVec cv;
#pragma unroll
        for (int k = 0; k < WX; ++k) cv[k] = (CountT)n[k];
        *(CountVec*)(cnt + row0_w + x_first) = cv;
      }
    } else {
#pragma unroll
      for (int k = 0; k < WX; ++k) {
        if (x_first + k < g.nx) {
          const int64_t idx = row0_w + x_first + k;
          if (fresh || ((changed_lanes >> lane_w) & 1ull) != 0ull) {  // (unchanged voxels of a changed lane store what they hold)
            g.sdf[idx] = s[k];
            cnt[idx] = (CountT)n[k];
          }
        }
      }
    }
  }
  VCY_PT(6);
  VCY_PT_FLUSH(lane);
}

// The launch of one instance: block size, dynamic LDS and the block decode of its flavour.
template <typename CountT, int UPDATE, bool TRUNC, bool SAMEF, bool CHECKMAX, int TQ, bool GEN, int DIV, int NB>
void launch_instance(const CarveLaunch& l) {
  constexpr bool kRows = NB > 1;
  // dynamic LDS.  kRows: every wave its own region.  Otherwise: the waves' tiles (NB == 0: ONE raw tile each), the
  // TileInfo of every (wave, view) (NB == 0 and carve_keeps_records: none, the records are in registers), the staging
  // of the cooperative write-back.
  const size_t coop = (l.state_flags & kStateCoopStore) ? coop_lds_bytes<CountT>() : 0;
  constexpr bool rec_regs = carve_keeps_records<UPDATE, TQ, NB>();
  const size_t lds = kRows    ? (size_t)kRowWaves * row_lds_bytes_per_wave<CountT, NB>()
                     : NB == 0 ? (size_t)kWgWaves * 64 * sizeof(float4) + coop
                               : (size_t)kWgWaves * tile_f4_per_wave<TQ>() * sizeof(float4) +
                                     (rec_regs ? 0 : (size_t)kWgWaves * l.n_views * sizeof(TileInfo)) + coop;
  // (kRows: `grid_x` workgroups of kRowWaves waves, a segment per wave; the decode deals the launch's segments to the XCDs)
  const BlockDecode bd = make_block_decode(kRows ? (unsigned)l.row_units : l.grid_x, l.nbx, l.nby);
  hipLaunchKernelGGL((carve_fused_kernel<CountT, UPDATE, TRUNC, SAMEF, CHECKMAX, TQ, GEN, DIV, NB>), dim3(l.grid_x),
                     dim3(64 * (kRows ? kRowWaves : kWgWaves)), lds, l.stream, l.g, l.views, l.c0_all,
                     NB == 0 ? 1 : l.n_views, l.mode, l.nbx, l.nby, bd, l.cull, l.state_flags, l.records, l.nbricks,
                     l.brick_min, l.wg_list, l.pair_count);
}

// f(std::integral_constant<int, V>) for the V among Vs that equals `value`: a run-time selection as a template argument.
// (A value that is not among them selects a kernel that was not built: an error, never a launch that does not happen.)
template <int... Vs, typename F>
void with_constant(int value, F&& f) {
  if (!((value == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...)) {
    fprintf(stderr, "carve_fused_kernel: no instance for selection %d\n", value);
    abort();
  }
}

// The instance of carve_fused_kernel a launch selects.  Per update mode, trunc and samef: the general flavour with or
// without the update limit, either tile kind; the one-view and the few-view flavours with raw tiles and no limit; each
// with the generic sampler (GEN, DIV 0) or one of the three division sequences -- 24 instances.
template <typename CountT>
void launch_fused(const CarveLaunch& l) {
  const int nb = l.flavour == CarveFlavour::kGeneral ? 1 : (l.flavour == CarveFlavour::kOneView ? 0 : kRowBricks);
#ifdef VCY_DEV_BENCH_KERNELS_ONLY
  // development builds (profiles/tools/build_variant.sh): only the instantiations bench.py launches,
  // a 20x shorter compile; anything else aborts
  // (the benchmark's 32 / 64 views fit one-byte counters: vcy_ctx::cnt_bytes, lazy widening)
  if (l.big || l.checkmax || l.gen || l.div_level != 2 || !l.samef || sizeof(CountT) != 1 ||
      l.update == VCY_UPDATE_WEIGHTED_AVERAGE) {
    fprintf(stderr, "VCY_DEV_BENCH_KERNELS_ONLY: kernel variant not built\n");
    abort();
  }
  if constexpr (sizeof(CountT) == 1)
    with_constant<VCY_UPDATE_MAX, kUpdateWaUnitWeight>(l.update, [&](auto update) {
      with_constant<0, 1>(l.trunc, [&](auto trunc) {
        with_constant<1, 0, kRowBricks>(nb, [&](auto nbv) {
          launch_instance<CountT, decltype(update)::value, decltype(trunc)::value != 0, true, false, kTileRaw, false, 2,
                          decltype(nbv)::value>(l);
        });
      });
    });
#else
  with_constant<VCY_UPDATE_MAX, VCY_UPDATE_WEIGHTED_AVERAGE, kUpdateWaUnitWeight>(l.update, [&](auto update) {
    with_constant<0, 1>(l.trunc, [&](auto trunc) {
      with_constant<0, 1>(l.samef, [&](auto samef) {
        with_constant<-1, 0, 1, 2>(l.gen ? -1 : l.div_level, [&](auto div) {  // (-1: GEN)
          constexpr int kU = decltype(update)::value, kDiv = decltype(div)::value < 0 ? 0 : decltype(div)::value;
          constexpr bool kT = decltype(trunc)::value != 0, kS = decltype(samef)::value != 0, kGen = decltype(div)::value < 0;
          if (nb == 1)
            with_constant<0, 1>(l.checkmax, [&](auto cm) {
              with_constant<kTileRaw, kTileBig>(l.big ? kTileBig : kTileRaw, [&](auto tq) {
                launch_instance<CountT, kU, kT, kS, decltype(cm)::value != 0, decltype(tq)::value, kGen, kDiv, 1>(l);
              });
            });
          else
            with_constant<0, kRowBricks>(nb, [&](auto nbv) {
              launch_instance<CountT, kU, kT, kS, false, kTileRaw, kGen, kDiv, decltype(nbv)::value>(l);
            });
        });
      });
    });
  });
#endif
}

}  // namespace
}  // namespace vcy
