// The decisions of a fused carve launch as pure host code: which instance of carve_fused_kernel runs, over which grid,
// with which state flags, in chunks of how many brick layers -- from the update option, the slab's shape, what the
// context knows about its state, the views' count and scale, and the knobs of vcy_set_param.  launch_carve_fused
// (carve_fused.hip) asks and enqueues; nothing here touches a stream, a buffer or the context.  Host code only, no HIP:
// tests/fused_plan_host_check.cpp states what every rule gives on both sides of its edge; the table of the rules is in
// DESIGN.md ("The fused carve's launch plan").
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "vacancy_hip.h"  // VCY_UPDATE_*, VCY_INTERP_*

namespace vcy {

// ---- the geometry of a launch (what the kernels, the pre-pass and the plan agree on; more of it: carve_fused.h) -------
// Waves per workgroup.  The waves never talk to each other, so 1 and 2 are just as correct; measured, they are
// 3 % slower in the default mode (four bricks adjacent in x start together and share rows and footprints).
#ifndef VCY_WG_WAVES
#define VCY_WG_WAVES 4   // (development builds: 8 is 7 % faster for single-view weighted-average launches, 7 % slower for the fused 32-view launch)
#endif
constexpr int kWgWaves = VCY_WG_WAVES;
constexpr int BX = 8 * kWgWaves, BY = 8, BZ = 8;  // voxels per workgroup: kWgWaves 8x8x8 wave bricks along x
constexpr int WX = 8;                    // wave brick is WX x BY x BZ, lane = (y & 7) | (z << 3), WX voxels per lane
// The few-view flavour (carve_fused.h: a wave walks kRowBricks bricks of a row segment, kRowWaves waves per workgroup)
constexpr int kRowMaxViews = 8;          // pairs are numbered 8 j + v
#ifndef VCY_ROW_BRICKS
#define VCY_ROW_BRICKS 4
#endif
#ifndef VCY_ROW_WAVES
#define VCY_ROW_WAVES 2
#endif
constexpr int kRowBricks = VCY_ROW_BRICKS;
constexpr int kRowWaves = VCY_ROW_WAVES;
constexpr int kLiveListMaxViews = 8;      // launches of up to this many views over a carved grid list their live workgroups first
// Ints per entry of a live list whose entries carry records (live_workgroups_kernel): {id, live waves, kWgWaves records}.
constexpr int kLiveEntryWords = 2 + 2 * kWgWaves;
constexpr int64_t kRecordBytesMax = (int64_t)2 << 30;  // footprint records of one chunk of a carve launch
constexpr int kFootprintRecordBytes = 8;  // sizeof(FootprintRecord), carve_fused.h

// Internal update mode: kWeightedAverage with voxel_update_weight == 1.0f (the default weight).
constexpr int kUpdateWaUnitWeight = 2;

// The bits of carve_fused_kernel's `state_flags`: what launch_carve_fused knows about the slab and asks of the launch.
constexpr int kStateFresh = 1;          // the slab is fresh: known sdf = lowest(), update_num = 0, never written
constexpr int kStateCountImplied = 2;   // update_num == 0 implies sdf == lowest() (no vcy_upload since the fill)
constexpr int kStateBrickMinValid = 4;  // the brick minima are valid: every write to the state since the slab was fresh
                                        // went through a fused launch
constexpr int kStateCoopStore = 8;      // cooperative write-back: whole row segments, through LDS (kCoopSdfPitch, carve_fused.h)
constexpr int kStateStreamStore = 16;   // ... with streaming stores ("ntstore")
constexpr int kStateEager = 32;         // one-view launch: the state is requested next to the footprint record ("eagerstate")
constexpr int kStateListRecords = 64;   // one-view launch: the entries of wg_list carry the bricks' records (kLiveEntryWords)
constexpr int kStateStaleBounds = 128;  // the records are an earlier launch's ("recordcache"): their geometry holds, the bounds
                                        // in them do not -- the kernel's prologue looks them up (fused_reuses_records)

// Which structure of carve_fused_kernel a launch takes (its template parameter NB: 1, 0, kRowBricks).
enum class CarveFlavour {
  kGeneral,  // a brick per wave, any number of views
  kOneView,  // the same for a launch of ONE view, the view count a compile-time constant
  kRows,     // the few-view flavour: a wave walks a segment of kRowBricks bricks (carve_fused.h)
};

// ---- the knobs (vcy_set_param / vcy_get_param, by the names in quotes; defaults as they stand) -------------------------
struct FusedKnobs {
  int tile_mode = 0;             // "tile": 0 auto, 1 the 16 x 16 pixel tile, 2 the 2048-pixel tile filled in place
  int row_kernel = 0;            // "rowkernel": launches of up to this many views take the few-view flavour; -1 = up to 8, 0 = never (the default: measured slower, carve_fused.h kRowBricks)
  int one_view = 1;              // "oneview": single-view launches take the kernel instance compiled for one view (carve_fused_kernel NB == 0)
  int coop_store = -1;           // "coopstore": write-back of a workgroup's bricks through LDS in whole row segments; -1 = where it pays (plan_fused_launch), 0 / 1 = never / whenever possible
  int nt_store = -1;             // "ntstore": streaming stores in the cooperative write-back (-1 / 1: whenever it runs -- 0.5 - 1.5 % on single-view launches; 0 never)
  int prologue_mode = 0;         // "prologue": 0 / 2 footprint records from the pre-pass (chunked); 1 footprints in the carve kernel's prologue (slower at every shape measured)
  int64_t record_bytes_max = 0;  // "recordbytes": footprint records per launch chunk (0: 2 GiB); tests force several chunks
  bool use_live_list = true;     // "livelist" 0: every workgroup is launched and decides for itself
  int list_records = 1;          // "listrecords": the live list of a one-view launch carries the footprint records and per-wave live bits (0: workgroup ids only)
  int eager_state = -1;          // "eagerstate": one-view launches request a brick's state next to its footprint record instead of behind the early-return test (-1: when most workgroups were live last time, 0 never, 1 always)
  bool live_sync = true;         // "livesync" 0: the carve kernel of a listed launch starts every workgroup instead of waiting for the list's length
  bool use_cull = true;          // "cull" 0: never drop provably idle views
  bool count_pairs = false;      // "paircount" 1: the fused kernel counts the (brick, view) pairs it processes
  bool use_short_div = true;     // "shortdiv" 0: always the full division sequence
  bool record_cache = true;      // "recordcache" 0: every launch makes its footprint records anew (fused_reuses_records)
};

// What the decisions read.  (fx == fy in every view is no decision: it selects a template argument and comes from
// prepare_views, which itself asks need_bound / need_lower of the plan.)
struct FusedPlanInput {
  int update = VCY_UPDATE_MAX;            // vcy_update_option::voxel_update
  bool trunc = false;                     // ... use_truncation
  int interp = VCY_INTERP_BILINEAR;       // ... sdf_interp
  int64_t max_update_num = 255;           // ... voxel_max_update_num
  float weight = 1.0f;                    // ... voxel_update_weight
  int nx = 0, ny = 0, nz_local = 0;       // the slab
  bool fresh = false, cnt_implied = true, brick_min_valid = false;  // StateFlags
  bool have_brick_min = false;            // the brick-minimum array exists (known once ensure_launch_buffers has run: read per chunk only)
  int64_t views_before = 0;               // views applied since the fill when this launch starts
  int n_views = 0;
  bool ortho = false;                     // one projection model per launch (fused_eligible)
  float worst = 0.0f;                     // worst_pixels_per_voxel over the views
  FusedKnobs knobs;
};

// Pixels per voxel of one view at (X, Y, Z), the centre of the slab (bricks much closer to the camera than that overflow
// the tile and take the generic path on their own); orthographic: one pixel per world unit.  View: ViewParams.
template <class View>
inline float pixels_per_voxel(const View& v, bool ortho, float res, float X, float Y, float Z) {
  const float pz = v.t[2] + (v.r[2][0] * X + (v.r[2][1] * Y + v.r[2][2] * Z));
  const float f = std::max(v.fx, v.fy);
  return ortho ? res : (pz > 0.0f ? f * res / pz : INFINITY);
}
// x / y / z: the extreme voxel centres of the slab
template <class View>
inline float worst_pixels_per_voxel(const View* vp, int n_views, bool ortho, float res, const float x[2], const float y[2],
                                    const float z[2]) {
  float worst = 0.0f;
  for (int vi = 0; vi < n_views; ++vi) {
    const float X = 0.5f * (x[0] + x[1]), Y = 0.5f * (y[0] + y[1]);
    const float Z = 0.5f * (z[0] + z[1]);
    worst = std::max(worst, pixels_per_voxel(vp[vi], ortho, res, X, Y, Z));
  }
  return worst;
}

// Everything that is fixed per launch.
struct FusedLaunchPlan {
  bool need_bound;          // window-maximum planes for the view-dropping bounds
  bool need_lower;          // two more planes, of the negated image, for the truncating weighted average (FusedView::has_lower)
  bool want_lower;          // the pre-pass looks the lower bounds up
  bool checkmax;            // voxel_max_update_num is in reach
  bool big;                 // tile kind: kTileBig instead of kTileRaw
  bool gen;                 // nearest-neighbour sampling and / or an orthographic camera
  bool rows, one_view;      // -> flavour
  bool coop, nt;            // cooperative write-back; ... with streaming stores
  bool in_kernel_prologue;  // footprints in the carve kernel's prologue
  bool records;             // footprints from the pre-pass: !big && !in_kernel_prologue
  int update;               // VCY_UPDATE_MAX, VCY_UPDATE_WEIGHTED_AVERAGE, or kUpdateWaUnitWeight
  CarveFlavour flavour;
  int state_flags_base;     // the kState* bits that do not depend on the chunk (all but kStateEager, kStateListRecords)
  int nbw, nbx, nby, nbz;   // wave bricks along x; workgroup blocks along x; brick rows; brick layers
  int nseg;                 // segments per brick row (the few-view flavour)
  int chunk_layers;         // brick layers per chunk
  int64_t record_bytes;     // footprint records of one chunk (0 without records)
};

inline FusedLaunchPlan plan_fused_launch(const FusedPlanInput& in) {
  const FusedKnobs& k = in.knobs;
  FusedLaunchPlan p;
  const int nxp = (in.nx + WX - 1) / WX * WX;
  p.nbw = nxp / WX;
  p.nbx = (in.nx + BX - 1) / BX, p.nby = (in.ny + BY - 1) / BY, p.nbz = (in.nz_local + BZ - 1) / BZ;
  p.nseg = (p.nbw + kRowBricks - 1) / kRowBricks;
  p.need_bound = k.use_cull && (in.update == VCY_UPDATE_MAX || in.trunc);
  // (two more planes, of the negated image, for the truncating unit-weight average: FusedView::has_lower)
  p.need_lower = p.need_bound && in.trunc && in.update == VCY_UPDATE_WEIGHTED_AVERAGE;
  p.want_lower = p.need_bound && in.trunc && in.update != VCY_UPDATE_MAX;
  // update_num can only exceed voxel_max_update_num after more than that many views
  p.checkmax = in.views_before + in.n_views > in.max_update_num;
  // Tile kind: footprint of an 8x8x8 wave brick in pixels ~ (8*sqrt(3)*pixels_per_voxel + 3)^2.  The raw
  // 16 x 16 pixel tile covers voxels up to ~0.85 px; the 2048-pixel tile filled in place up to ~3 px; wider
  // footprints take the generic path inside the kernel either way.
  const float side = 8.0f * 1.7320508f * in.worst + 3.0f;
  p.big = side > 15.0f;
  if (k.tile_mode == 1) p.big = false;
  if (k.tile_mode == 2) p.big = true;
  p.gen = in.ortho || in.interp == VCY_INTERP_NN;
  // Cooperative write-back (carve_fused_kernel): pays where a launch moves the state for little arithmetic -- few views
  // over a carved grid (1024^3, one view per launch: weighted average 4.39 -> 3.41 ms, kMax 0.89 -> 0.84), and the first
  // single-view launch on a fresh grid, which stores every voxel once (2.48 -> 1.95 ms: 6.4 GB at 3.3 instead of
  // 2.6 TB/s).  "coopstore": -1 that rule, 0 never, 1 always when the layout allows it: rows of whole bricks, four
  // waves per workgroup, raw tiles.
  // (kMax: only single-view launches -- with 4 or 8 views per launch the waves of a workgroup process different numbers
  // of views and the barrier costs 3 - 4 %, profiles/r04/coop_store_batches.txt; weighted average: up to 8 views, 0 ... +2 %;
  // a fresh grid: single-view launches in either mode -- the fused 32-view launch gained nothing from whole-segment
  // stores in round 3)
  // The few-view flavour (kRowBricks: a wave walks the bricks of a row segment): launches of up to kRowMaxViews views with
  // raw tiles and records from the pre-pass, over rows of whole bricks, no update limit in reach.  "rowkernel" -1 that
  // rule, 0 never (the NB = 1 kernel with its cooperative write-back), n > 0: launches of up to min(n, 8) views.
  const int row_views = k.row_kernel < 0 ? kRowMaxViews : std::min(k.row_kernel, kRowMaxViews);
  p.rows = !p.big && !p.checkmax && (in.nx & (WX - 1)) == 0 && in.n_views <= row_views && k.prologue_mode != 1;
  // a launch of ONE view through the kernel instance that knows it ("oneview" 0: the general instance)
  p.one_view = k.one_view && in.n_views == 1 && !p.rows && !p.big && !p.checkmax && k.prologue_mode != 1;
  const bool coop_ok = (kWgWaves == 4 || kWgWaves == 8) && (in.nx & (WX - 1)) == 0 && !p.big && !p.rows;
  const int coop_views = in.fresh ? 1 : (in.update == VCY_UPDATE_MAX ? 1 : kLiveListMaxViews);
  p.coop = coop_ok && (k.coop_store > 0 || (k.coop_store < 0 && in.n_views <= coop_views));
  // "ntstore": streaming stores whenever the cooperative write-back runs (0: never) -- whole 128-byte segments that this
  // launch does not read again: 0.5 - 1.5 % on single-view launches (profiles/r06/nontemporal.txt)
  p.nt = p.coop && k.nt_store != 0;
  p.update = in.update == VCY_UPDATE_MAX ? VCY_UPDATE_MAX
             : in.weight == 1.0f         ? kUpdateWaUnitWeight
                                         : VCY_UPDATE_WEIGHTED_AVERAGE;
  p.flavour = p.rows ? CarveFlavour::kRows : (p.one_view ? CarveFlavour::kOneView : CarveFlavour::kGeneral);
  // (kStateEager and kStateListRecords are decided per chunk: they depend on whether the launch is a listed one)
  p.state_flags_base = (in.fresh ? kStateFresh : 0) | (in.cnt_implied ? kStateCountImplied : 0) |
                       (in.brick_min_valid && !in.fresh ? kStateBrickMinValid : 0) |
                       (p.coop ? kStateCoopStore : 0) | (p.nt ? kStateStreamStore : 0);
  // Raw tiles: the footprint records of every (wave brick, view) pair come from a pre-pass (footprint_records_kernel),
  // 8 bytes per pair.  The slab is carved in chunks of whole brick layers so that the records of a chunk stay
  // below kRecordBytesMax (1024^3 x 32 views: 0.5 GiB, one chunk; 2048^3 x 64: nine).
  // Footprints from the pre-pass (records) or from the carve kernel's own prologue?  The pre-pass: its threads are all
  // busy where the prologue would use nviews lanes of 64, it runs at full occupancy, and the records are what the live
  // list and the early return read.  Round 5 tried the prologue for the one launch whose records are large -- 2048^3 x 64
  // views: 8.6 GB of them, written and read back in chunks, 9.1 of the step's 81.8 ms; every lane of the prologue has a
  // view there and the step becomes ONE launch -- and measured 92.8 ms: the footprints cost 20 ms in the kernel (two
  // dependent round trips in front of every wave, at the carve kernel's occupancy) against 9 in the pre-pass
  // (profiles/r05/bench_2048x64_config4_*.json).  So: "prologue" 0 or 2 records (chunks of at most kRecordBytesMax: four
  // at that shape), 1 in the kernel.
  const int64_t rec_cap = k.record_bytes_max > 0 ? k.record_bytes_max : kRecordBytesMax;
  p.in_kernel_prologue = !p.big && k.prologue_mode == 1;
  p.records = !p.big && !p.in_kernel_prologue;
  p.chunk_layers = p.nbz;
  p.record_bytes = 0;
  if (p.records) {
    const int64_t per_layer = (int64_t)p.nbw * p.nby * in.n_views * (int64_t)kFootprintRecordBytes;
    p.chunk_layers = (int)std::max<int64_t>(1, std::min<int64_t>(p.nbz, rec_cap / std::max<int64_t>(per_layer, 1)));
    p.record_bytes = per_layer * p.chunk_layers;
  }
  return p;
}

// What is fixed for a chunk of `layers` brick layers before its list pass.
struct FusedChunkPlan {
  int unit_bricks;       // bricks per unit: kWgWaves of a workgroup block, kRowBricks of a segment
  int units_x;           // units per brick row
  int units;             // units of the chunk (the block decode's total; `nwg` of the list pass)
  unsigned full_grid;    // workgroups of the unlisted launch
  unsigned listed_grid;  // workgroups that hold every unit of a listed launch (used unless the count arrives)
  bool list_pays;        // the list of the previous such launch did not hold most workgroups
  bool listed;           // the live list is built
  bool have_min;         // ... with the brick minima in its test
  int list_entry_words;  // kLiveEntryWords: the entries carry the records; 0: ids only
  size_t list_bytes;     // of the list
};

// workgroups that hold `units` listed units
inline unsigned fused_groups_of(const FusedLaunchPlan& p, unsigned units) {
  return p.rows ? (units + kRowWaves - 1) / kRowWaves : units;
}

// `hint`: null, or {live workgroups, workgroups} of the last listed launch; `age`: listed-or-not chunks so far, this
// one included.
inline FusedChunkPlan plan_fused_chunk(const FusedLaunchPlan& p, const FusedPlanInput& in, int layers, const int* hint,
                                       int64_t age) {
  const FusedKnobs& k = in.knobs;
  FusedChunkPlan c;
  // units of the launch: workgroup blocks of kWgWaves bricks, or the segments of the few-view flavour (one per wave)
  c.unit_bricks = p.rows ? kRowBricks : kWgWaves;
  c.units_x = p.rows ? p.nseg : p.nbx;
  c.units = (int)(unsigned)((int64_t)c.units_x * p.nby * layers);
  const unsigned grid = (unsigned)c.units;
  // (unlisted launch of the few-view flavour: unit (g mod 8) + 8 (kRowWaves (g / 8) + wave) of workgroup g)
  c.full_grid = p.rows ? 8u * ((grid + 8u * kRowWaves - 1) / (8u * kRowWaves)) : grid;
  c.listed_grid = fused_groups_of(p, grid);  // (every unit started unless the count arrives)
  // few views over a carved grid: only the workgroups with a live (brick, view) pair (live_workgroups_kernel)
  c.have_min = in.update == VCY_UPDATE_MAX && (p.state_flags_base & kStateBrickMinValid) != 0 && in.have_brick_min;
  // (not when the list of the previous such launch held most workgroups anyway -- a weighted-average carve touches
  // nearly every brick with every view, and the list pass is then 4 % on top; the count arrives by an asynchronous
  // copy into page-locked memory and is only a hint: reading an older value is harmless)
  c.list_pays = hint == nullptr || hint[1] <= 0 || (double)hint[0] < 0.6 * (double)hint[1];
  c.listed = p.records && k.use_live_list && p.need_bound && !in.fresh && in.n_views <= kLiveListMaxViews &&
             (in.trunc || c.have_min) && (c.list_pays || age % 16 == 0);  // (every 16th launch looks again)
  // (a launch of ONE view: entries {id, live waves, the four records} -- "listrecords" 0: ids only)
  c.list_entry_words = c.listed && p.one_view && k.list_records != 0 ? kLiveEntryWords : 0;
  c.list_bytes = !c.listed ? 0
                 : c.list_entry_words ? sizeof(int) * (2 + (size_t)c.units * kLiveEntryWords)
                                      : sizeof(int) * ((size_t)c.units + 1);
  return c;
}

// What the launch of a chunk takes once the list's length is known -- or is not waited for.
struct FusedChunkLaunch {
  unsigned grid_x;    // workgroups (0: no workgroup is live, nothing to launch)
  bool eager_state;
  int state_flags;
};
constexpr int kLiveNotWaited = -1;  // `live`: no list, "livesync" 0, or the wait failed

inline FusedChunkLaunch finish_fused_chunk(const FusedLaunchPlan& p, const FusedPlanInput& in, const FusedChunkPlan& c,
                                           int live) {
  FusedChunkLaunch f;
  f.grid_x = c.listed ? c.listed_grid : c.full_grid;
  // The carve kernel is launched over the listed workgroups only: the host waits for the count (the list pass is
  // 60 us of device time behind it) instead of starting every workgroup of the slab to have all but the listed
  // ones read list[0] and leave -- 512 K workgroups that do nothing else are 0.115 ms at 1024^3
  // (profiles/tools/per_view_floor.py), a sixth of a single-view launch.  ("livesync" 0: the full grid, no wait.)
  if (c.listed && live >= 0 && live <= c.units) f.grid_x = fused_groups_of(p, (unsigned)live);
  // "eagerstate": the workgroups of a one-view launch over a carved grid request their bricks' state next to the
  // footprint records when nearly all of them will need it: a listed launch (only live workgroups are started), or one
  // that skipped its list because the last one held most workgroups (-1 that rule, 0 never, 1 every one-view launch).
  // 1024^3, one view per launch: weighted average 2.51 -> 2.46 ms, kMax 0.521 -> 0.487 (profiles/r06/eager_state.txt).
  const bool nearly_all_live = c.listed ? f.grid_x < (unsigned)c.units || !c.list_pays : !c.list_pays;
  f.eager_state = !in.fresh && p.one_view && (in.knobs.eager_state > 0 || (in.knobs.eager_state < 0 && nearly_all_live));
  f.state_flags = p.state_flags_base | (f.eager_state ? kStateEager : 0) |
                  (c.listed && c.list_entry_words ? kStateListRecords : 0);
  return f;
}

// ---- footprint records kept across launches ("recordcache") ------------------------------------------------------------
// A footprint record is geometry -- the tile's origin and size, the edge bits, `sure` -- and one bound.  The geometry
// depends on the cameras, the grid and the slab; only the bound depends on the images.  The cameras of a capture rig are
// calibrated once, so a context that carves the same rig again finds the geometry of its last launch still in its record
// buffer, and the carve kernel's prologue can look the bounds up itself (kStateStaleBounds): nothing is left of the
// pre-pass.  That holds for the launches whose kernel instance has such a prologue and whose records are what the last
// launch left; every other launch runs the pre-pass as it always did.
//
// fused_records_cacheable: the launch is of the kind that may reuse records -- and, when it does not (the key of the
// buffer's contents differs), of the kind whose records a later launch may reuse.  `have_planes`: the window planes of
// this launch exist.  `c`: the plan of the launch's first chunk (one-chunk launches only, so: of the launch).
inline bool fused_records_cacheable(const FusedLaunchPlan& p, const FusedPlanInput& in, const FusedChunkPlan& c,
                                    bool have_planes) {
  // the instance keeps its records in registers (carve_keeps_records, carve_fused_kernel.h): kMax, raw tiles, a brick per wave
  const bool keeps_records = p.update == VCY_UPDATE_MAX && !p.big && p.flavour == CarveFlavour::kGeneral;
  return in.knobs.record_cache && keeps_records && p.need_bound && !p.want_lower &&
         p.records /* not the kernel's own prologue, "prologue" 1 */ && p.chunk_layers >= p.nbz && have_planes &&
         !c.listed /* the list pass reads the bounds from the records */;
}
// `key_matches`: the record buffer holds what a launch with this one's cameras, slab and buffer left (FusedRecordKey).
inline bool fused_reuses_records(const FusedLaunchPlan& p, const FusedPlanInput& in, const FusedChunkPlan& c,
                                 bool have_planes, bool key_matches) {
  return fused_records_cacheable(p, in, c, have_planes) && key_matches;
}

// ---- the rectangle the window planes of a view are built in -----------------------------------------------------------
// Image-space bounding box of the slab [x] x [y] x [z] (extreme voxel centres; double precision, 16 px border; the
// footprints the kernel looks up lie within a fraction of a pixel of the exact hull, their windows inside them).
// wrect = {x0, y0, x1, y1}, x0 and x1 multiples of 4; quads = threads of the window-maximum kernels for it.  A corner
// behind the camera or beyond 1e9 pixels: the whole image.  View: ViewParams.
struct ImageRect {
  int wrect[4];
  int quads;
};
template <class View>
inline ImageRect slab_image_rect(const View& v, bool ortho, const double X[2], const double Y[2], const double Z[2], int w,
                                 int h) {
  int rx0 = 0, ry0 = 0, rx1 = w, ry1 = h;
  double umin = 1e300, umax = -1e300, wmin = 1e300, wmax = -1e300;
  bool whole = false;
  for (int cr = 0; cr < 8; ++cr) {
    const double x = X[cr & 1], y = Y[(cr >> 1) & 1], z = Z[cr >> 2];
    double pc[3];
    for (int i = 0; i < 3; ++i)
      pc[i] = (double)v.t[i] + ((double)v.r[i][0] * x + (double)v.r[i][1] * y + (double)v.r[i][2] * z);
    double uu = pc[0], ww = pc[1];
    if (!ortho) {
      if (!(pc[2] > 1e-30)) { whole = true; break; }
      uu = (double)v.fx / pc[2] * pc[0] + v.cx;
      ww = (double)v.fy / pc[2] * pc[1] + v.cy;
    }
    if (!(std::fabs(uu) < 1e9) || !(std::fabs(ww) < 1e9)) { whole = true; break; }
    umin = std::min(umin, uu), umax = std::max(umax, uu);
    wmin = std::min(wmin, ww), wmax = std::max(wmax, ww);
  }
  if (!whole) {
    rx0 = std::max(0, (int)std::floor(umin) - 16) & ~3;
    ry0 = std::max(0, (int)std::floor(wmin) - 16);
    rx1 = std::min((w + 3) & ~3, ((int)std::floor(umax) + 16 + 4) & ~3);
    ry1 = std::min(h, (int)std::floor(wmax) + 16 + 1);
    if (rx1 < rx0) rx1 = rx0;
    if (ry1 < ry0) ry1 = ry0;
  } else {
    rx1 = (w + 3) & ~3;
  }
  return ImageRect{{rx0, ry0, rx1, ry1}, ((rx1 - rx0) / 4) * (ry1 - ry0)};
}

}  // namespace vcy
