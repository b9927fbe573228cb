// The decisions of a fused carve launch (vacancy_amd/csrc/carve_fused_plan.h), as a program of its own, also under
// AddressSanitizer and UBSan (make fused_plan_host_check; driven by tests/test_fused_plan_host.py).
//
// Every flavour of the fused carve gives the same voxel state, so a driver that picks another flavour passes every
// state test and only gets slower.  Here every rule of the table of DESIGN.md ("The fused carve's launch plan") is
// asked on both sides of its edge, and what must come out is written down as literals, per named case.
// Behind them the one value a launch resolves from its images on the host's account, max_sdf: the two stages of
// max_reduce_kernel as host loops over the kernel's own pair order (max_element_pair.h), against std::max_element.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "carve_fused_plan.h"
#include "max_element_pair.h"

using namespace vcy;

namespace {

int failures = 0, checks = 0;
const char* g_case = "";
#define EXPECT(what, want)                                                                                  \
  do {                                                                                                      \
    ++checks;                                                                                               \
    const long long got_ = (long long)(what), want_ = (long long)(want);                                    \
    if (got_ != want_) {                                                                                    \
      std::printf("FAILED %s:%d [%s]: %s = %lld, expected %lld\n", __FILE__, __LINE__, g_case, #what, got_, want_); \
      if (++failures > 40) std::exit(1);                                                                    \
    }                                                                                                       \
  } while (0)

// 64^3, kMax, bilinear, already carved through fused launches (the brick minima valid), one view well inside the raw tile
FusedPlanInput carved_max(int n_views) {
  FusedPlanInput in;
  in.update = VCY_UPDATE_MAX, in.trunc = false, in.interp = VCY_INTERP_BILINEAR;
  in.max_update_num = 255, in.weight = 1.0f;
  in.nx = in.ny = in.nz_local = 64;
  in.fresh = false, in.cnt_implied = true, in.brick_min_valid = true, in.have_brick_min = true;
  in.views_before = 40, in.n_views = n_views, in.ortho = false;
  in.worst = 0.5f;  // side 9.9 pixels
  return in;
}
FusedPlanInput fresh_max(int n_views) {
  FusedPlanInput in = carved_max(n_views);
  in.fresh = true, in.brick_min_valid = false, in.views_before = 0;
  return in;
}
FusedPlanInput carved_average(int n_views, bool trunc) {
  FusedPlanInput in = carved_max(n_views);
  in.update = VCY_UPDATE_WEIGHTED_AVERAGE, in.trunc = trunc;
  return in;
}
constexpr int kGeneral = (int)CarveFlavour::kGeneral, kOneView = (int)CarveFlavour::kOneView, kRows = (int)CarveFlavour::kRows;

void check_bounds_and_modes() {
  g_case = "kMax";
  FusedLaunchPlan p = plan_fused_launch(carved_max(4));
  EXPECT(p.need_bound, 1); EXPECT(p.need_lower, 0); EXPECT(p.want_lower, 0); EXPECT(p.update, 0); EXPECT(p.gen, 0);
  g_case = "kMax, truncation";
  FusedPlanInput in = carved_max(4);
  in.trunc = true;
  p = plan_fused_launch(in);
  EXPECT(p.need_bound, 1); EXPECT(p.need_lower, 0); EXPECT(p.want_lower, 0);
  g_case = "average";
  p = plan_fused_launch(carved_average(4, false));
  EXPECT(p.need_bound, 0); EXPECT(p.need_lower, 0); EXPECT(p.want_lower, 0); EXPECT(p.update, 2);
  g_case = "average, truncation";
  p = plan_fused_launch(carved_average(4, true));
  EXPECT(p.need_bound, 1); EXPECT(p.need_lower, 1); EXPECT(p.want_lower, 1); EXPECT(p.update, 2);
  g_case = "average, truncation, weight 0.5";
  in = carved_average(4, true);
  in.weight = 0.5f;
  EXPECT(plan_fused_launch(in).update, 1);
  g_case = "average, truncation, cull 0";
  in = carved_average(4, true);
  in.knobs.use_cull = false;
  p = plan_fused_launch(in);
  EXPECT(p.need_bound, 0); EXPECT(p.need_lower, 0); EXPECT(p.want_lower, 0);
  g_case = "orthographic";
  in = carved_max(4);
  in.ortho = true;
  EXPECT(plan_fused_launch(in).gen, 1);
  g_case = "nearest neighbour";
  in = carved_max(4);
  in.interp = VCY_INTERP_NN;
  EXPECT(plan_fused_launch(in).gen, 1);
}

void check_update_limit() {
  g_case = "254 + 1 views of 255";
  FusedPlanInput in = carved_max(1);
  in.views_before = 254;
  FusedLaunchPlan p = plan_fused_launch(in);
  EXPECT(p.checkmax, 0); EXPECT((int)p.flavour, kOneView);
  g_case = "255 + 1 views of 255";
  in.views_before = 255;
  p = plan_fused_launch(in);
  EXPECT(p.checkmax, 1); EXPECT(p.one_view, 0); EXPECT((int)p.flavour, kGeneral); EXPECT(p.coop, 1);
  g_case = "255 + 1 views of 255, rowkernel -1";
  in.knobs.row_kernel = -1;
  EXPECT(plan_fused_launch(in).rows, 0);
  g_case = "223 + 32 / 224 + 32 views of 255";
  in = carved_max(32);
  in.views_before = 223;
  EXPECT(plan_fused_launch(in).checkmax, 0);
  in.views_before = 224;
  EXPECT(plan_fused_launch(in).checkmax, 1);
}

void check_tile_kind() {
  // side = 8 sqrt(3) worst + 3: 14.9996 at 0.866 pixels per voxel, 15.0010 at 0.8661
  for (int tile = 0; tile <= 2; ++tile) {
    FusedPlanInput in = carved_max(1);
    in.knobs.tile_mode = tile;
    in.worst = 0.866f;
    g_case = "side just below 15";
    EXPECT(plan_fused_launch(in).big, tile == 2 ? 1 : 0);
    in.worst = 0.8661f;
    g_case = "side just above 15";
    EXPECT(plan_fused_launch(in).big, tile == 1 ? 0 : 1);
  }
  g_case = "big tile";
  FusedPlanInput in = carved_max(1);
  in.worst = 2.0f;
  in.knobs.row_kernel = -1, in.knobs.coop_store = 1;
  FusedLaunchPlan p = plan_fused_launch(in);
  EXPECT(p.big, 1); EXPECT(p.rows, 0); EXPECT(p.one_view, 0); EXPECT(p.coop, 0); EXPECT(p.nt, 0);
  EXPECT(p.records, 0); EXPECT(p.in_kernel_prologue, 0); EXPECT(p.chunk_layers, 8); EXPECT(p.record_bytes, 0);
  EXPECT(plan_fused_chunk(p, in, 8, nullptr, 1).listed, 0);
  g_case = "a view behind the slab's centre";
  in = carved_max(1);
  in.worst = INFINITY;
  EXPECT(plan_fused_launch(in).big, 1);
}

void check_rows() {
  struct { int knob, n_views, rows; } cases[] = {
      {-1, 8, 1}, {-1, 9, 0}, {3, 3, 1}, {3, 4, 0}, {20, 8, 1}, {20, 9, 0}, {0, 1, 0}, {1, 1, 1}, {1, 2, 0}};
  for (const auto& cs : cases) {
    g_case = "rowkernel";
    FusedPlanInput in = carved_max(cs.n_views);
    in.knobs.row_kernel = cs.knob;
    const FusedLaunchPlan p = plan_fused_launch(in);
    EXPECT(p.rows, cs.rows);
    EXPECT((int)p.flavour, cs.rows ? kRows : (cs.n_views == 1 ? kOneView : kGeneral));
    if (cs.rows) { EXPECT(p.one_view, 0); EXPECT(p.coop, 0); }
  }
  g_case = "rowkernel -1, nx 60";
  FusedPlanInput in = carved_max(1);
  in.knobs.row_kernel = -1;
  in.nx = 60;
  FusedLaunchPlan p = plan_fused_launch(in);
  EXPECT(p.rows, 0); EXPECT((int)p.flavour, kOneView); EXPECT(p.coop, 0); EXPECT(p.nt, 0);
  EXPECT(p.nbw, 8); EXPECT(p.nbx, 2);
  g_case = "nx 64";
  in = carved_max(1);
  p = plan_fused_launch(in);
  EXPECT(p.coop, 1); EXPECT(p.nbw, 8); EXPECT(p.nbx, 2); EXPECT(p.nby, 8); EXPECT(p.nbz, 8); EXPECT(p.nseg, 2);
  g_case = "nx 60, coopstore 1";
  in.nx = 60, in.knobs.coop_store = 1;
  EXPECT(plan_fused_launch(in).coop, 0);
  for (int prologue = 0; prologue <= 2; ++prologue) {
    g_case = "prologue, rowkernel -1";
    in = carved_max(1);
    in.knobs.prologue_mode = prologue, in.knobs.row_kernel = -1;
    p = plan_fused_launch(in);
    EXPECT(p.rows, prologue == 1 ? 0 : 1); EXPECT(p.in_kernel_prologue, prologue == 1 ? 1 : 0);
    EXPECT(p.records, prologue == 1 ? 0 : 1);
    g_case = "prologue";
    in.knobs.row_kernel = 0;
    p = plan_fused_launch(in);
    EXPECT(p.one_view, prologue == 1 ? 0 : 1); EXPECT((int)p.flavour, prologue == 1 ? kGeneral : kOneView);
    EXPECT(p.coop, 1);
    EXPECT(p.chunk_layers, 8); EXPECT(p.record_bytes, prologue == 1 ? 0 : 4096);
    EXPECT(plan_fused_chunk(p, in, 8, nullptr, 1).listed, prologue == 1 ? 0 : 1);
  }
  g_case = "oneview 0";
  in = carved_max(1);
  in.knobs.one_view = 0;
  EXPECT((int)plan_fused_launch(in).flavour, kGeneral);
}

void check_coop() {
  struct { const char* name; FusedPlanInput in; int coop; } cases[] = {
      {"fresh, 1 view", fresh_max(1), 1},           {"fresh, 2 views", fresh_max(2), 0},
      {"carved kMax, 1 view", carved_max(1), 1},    {"carved kMax, 2 views", carved_max(2), 0},
      {"carved average, 8 views", carved_average(8, false), 1}, {"carved average, 9 views", carved_average(9, false), 0},
  };
  for (auto& cs : cases) {
    g_case = cs.name;
    FusedLaunchPlan p = plan_fused_launch(cs.in);
    EXPECT(p.coop, cs.coop); EXPECT(p.nt, cs.coop);
    cs.in.knobs.nt_store = 0;
    EXPECT(plan_fused_launch(cs.in).nt, 0);
    cs.in.knobs.nt_store = 1;
    EXPECT(plan_fused_launch(cs.in).nt, cs.coop);
    cs.in.knobs.coop_store = 0;
    EXPECT(plan_fused_launch(cs.in).coop, 0);
    cs.in.knobs.coop_store = 1;
    EXPECT(plan_fused_launch(cs.in).coop, 1);
  }
  g_case = "fresh average, 2 views";
  FusedPlanInput in = carved_average(2, false);
  in.fresh = true, in.brick_min_valid = false;
  EXPECT(plan_fused_launch(in).coop, 0);
  g_case = "coopstore 1, 32 views";
  in = carved_max(32);
  in.knobs.coop_store = 1;
  FusedLaunchPlan p = plan_fused_launch(in);
  EXPECT(p.coop, 1); EXPECT(p.state_flags_base, 2 | 4 | 8 | 16);
}

void check_state_flags_base() {
  g_case = "carved kMax, 1 view";
  EXPECT(plan_fused_launch(carved_max(1)).state_flags_base, 2 | 4 | 8 | 16);
  g_case = "carved kMax, 8 views";
  EXPECT(plan_fused_launch(carved_max(8)).state_flags_base, 2 | 4);
  g_case = "fresh, 1 view";
  EXPECT(plan_fused_launch(fresh_max(1)).state_flags_base, 1 | 2 | 8 | 16);
  g_case = "fresh with minima called valid";
  FusedPlanInput in = fresh_max(8);
  in.brick_min_valid = true;
  EXPECT(plan_fused_launch(in).state_flags_base, 1 | 2);
  g_case = "after an upload";
  in = carved_max(8);
  in.cnt_implied = false, in.brick_min_valid = false;
  EXPECT(plan_fused_launch(in).state_flags_base, 0);
  g_case = "ntstore 0";
  in = carved_max(1);
  in.knobs.nt_store = 0;
  EXPECT(plan_fused_launch(in).state_flags_base, 2 | 4 | 8);
}

void check_chunk_layers() {
  // 64^3 x 32 views: 8 x 8 wave bricks per layer, 8 bytes per (brick, view): 16384 bytes per layer, 8 layers
  struct { const char* name; int64_t recordbytes; int layers; int64_t bytes; } cases[] = {
      {"default cap", 0, 8, 131072},       {"exactly one layer", 16384, 1, 16384}, {"less than one layer", 16383, 1, 16384},
      {"one byte", 1, 1, 16384},           {"all layers", 131072, 8, 131072},      {"three layers and a bit", 3 * 16384 + 5, 3, 49152},
      {"one short of two", 32767, 1, 16384},
  };
  for (const auto& cs : cases) {
    g_case = cs.name;
    FusedPlanInput in = carved_max(32);
    in.knobs.record_bytes_max = cs.recordbytes;
    const FusedLaunchPlan p = plan_fused_launch(in);
    EXPECT(p.records, 1); EXPECT(p.chunk_layers, cs.layers); EXPECT(p.record_bytes, cs.bytes);
  }
  g_case = "2048^3 x 64 views, default cap";  // 256 x 256 bricks x 64 views x 8 bytes = 32 MiB per layer: 64 of 256 layers
  FusedPlanInput in = carved_max(64);
  in.nx = in.ny = in.nz_local = 2048;
  FusedLaunchPlan p = plan_fused_launch(in);
  EXPECT(p.chunk_layers, 64); EXPECT(p.record_bytes, (int64_t)2 << 30);
  g_case = "60 x 60 x 60";  // 8 x 8 x 8 bricks all the same
  in = carved_max(1);
  in.nx = in.ny = in.nz_local = 60;
  p = plan_fused_launch(in);
  EXPECT(p.nbw, 8); EXPECT(p.nby, 8); EXPECT(p.nbz, 8); EXPECT(p.chunk_layers, 8); EXPECT(p.record_bytes, 4096);
}

void check_live_list() {
  g_case = "carved kMax, 8 views";
  FusedPlanInput in = carved_max(8);
  FusedLaunchPlan p = plan_fused_launch(in);
  FusedChunkPlan c = plan_fused_chunk(p, in, 8, nullptr, 1);
  EXPECT(c.listed, 1); EXPECT(c.have_min, 1); EXPECT(c.list_entry_words, 0); EXPECT(c.units, 128); EXPECT(c.units_x, 2);
  EXPECT(c.unit_bricks, 4); EXPECT(c.full_grid, 128); EXPECT(c.listed_grid, 128); EXPECT(c.list_bytes, 516);
  g_case = "carved kMax, 9 views";
  in = carved_max(9);
  EXPECT(plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1).listed, 0);
  g_case = "carved kMax, 1 view";
  in = carved_max(1);
  p = plan_fused_launch(in);
  c = plan_fused_chunk(p, in, 8, nullptr, 1);
  EXPECT(c.listed, 1); EXPECT(c.list_entry_words, 10); EXPECT(c.list_bytes, 5128);
  g_case = "carved kMax, 1 view, 3 layers";
  c = plan_fused_chunk(p, in, 3, nullptr, 1);
  EXPECT(c.units, 48); EXPECT(c.full_grid, 48); EXPECT(c.list_bytes, 1928);
  g_case = "listrecords 0";
  in.knobs.list_records = 0;
  c = plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1);
  EXPECT(c.listed, 1); EXPECT(c.list_entry_words, 0); EXPECT(c.list_bytes, 516);
  g_case = "oneview 0";
  in = carved_max(1);
  in.knobs.one_view = 0;
  EXPECT(plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1).list_entry_words, 0);
  g_case = "livelist 0";
  in = carved_max(1);
  in.knobs.use_live_list = false;
  EXPECT(plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1).listed, 0);
  g_case = "cull 0";
  in = carved_max(1);
  in.knobs.use_cull = false;
  EXPECT(plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1).listed, 0);
  g_case = "fresh";
  in = fresh_max(1);
  EXPECT(plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1).listed, 0);
  g_case = "kMax, minima not valid";
  in = carved_max(1);
  in.brick_min_valid = false;
  c = plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1);
  EXPECT(c.listed, 0); EXPECT(c.have_min, 0);
  g_case = "kMax, minima not valid, truncation";
  in.trunc = true;
  c = plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1);
  EXPECT(c.listed, 1); EXPECT(c.have_min, 0);
  g_case = "kMax, no array";
  in = carved_max(1);
  in.have_brick_min = false;
  c = plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1);
  EXPECT(c.listed, 0); EXPECT(c.have_min, 0);
  g_case = "average";
  in = carved_average(1, false);
  EXPECT(plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1).listed, 0);
  g_case = "average, truncation";
  in = carved_average(8, true);
  c = plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1);
  EXPECT(c.listed, 1); EXPECT(c.have_min, 0);
  in = carved_average(9, true);
  EXPECT(plan_fused_chunk(plan_fused_launch(in), in, 8, nullptr, 1).listed, 0);

  // the hint of the last listed launch, {live, workgroups}: the list pays below 0.6
  in = carved_max(1);
  p = plan_fused_launch(in);
  struct { const char* name; int live, total; int64_t age; int pays, listed; } hints[] = {
      {"hint 59 of 100", 59, 100, 1, 1, 1},          {"hint 60 of 100", 60, 100, 1, 0, 0},
      {"hint 60 of 100, age 15", 60, 100, 15, 0, 0}, {"hint 60 of 100, age 16", 60, 100, 16, 0, 1},
      {"hint 60 of 100, age 17", 60, 100, 17, 0, 0}, {"hint 60 of 100, age 32", 60, 100, 32, 0, 1},
      {"hint 59 of 100, age 17", 59, 100, 17, 1, 1}, {"hint 100 of 100", 100, 100, 3, 0, 0},
      {"hint after a reset", 0, 0, 3, 1, 1},         {"hint 0 of 100", 0, 100, 3, 1, 1},
  };
  for (const auto& h : hints) {
    g_case = h.name;
    const int hint[2] = {h.live, h.total};
    c = plan_fused_chunk(p, in, 8, hint, h.age);
    EXPECT(c.list_pays, h.pays); EXPECT(c.listed, h.listed);
  }
  g_case = "no hint, age 15";
  c = plan_fused_chunk(p, in, 8, nullptr, 15);
  EXPECT(c.list_pays, 1); EXPECT(c.listed, 1);
}

void check_rows_grids() {
  g_case = "rows, 64^3";  // 2 segments of 4 bricks per row, 8 rows, 8 layers; 2 waves per workgroup
  FusedPlanInput in = carved_max(1);
  in.knobs.row_kernel = -1;
  FusedLaunchPlan p = plan_fused_launch(in);
  FusedChunkPlan c = plan_fused_chunk(p, in, 8, nullptr, 1);
  EXPECT(c.unit_bricks, 4); EXPECT(c.units_x, 2); EXPECT(c.units, 128); EXPECT(c.full_grid, 64); EXPECT(c.listed_grid, 64);
  EXPECT(c.listed, 1); EXPECT(c.list_entry_words, 0);
  EXPECT(finish_fused_chunk(p, in, c, 5).grid_x, 3);
  EXPECT(finish_fused_chunk(p, in, c, 128).grid_x, 64);
  EXPECT(finish_fused_chunk(p, in, c, 129).grid_x, 64);
  EXPECT(finish_fused_chunk(p, in, c, 0).grid_x, 0);
  EXPECT(finish_fused_chunk(p, in, c, kLiveNotWaited).grid_x, 64);
  EXPECT(finish_fused_chunk(p, in, c, 5).state_flags, 2 | 4);
  g_case = "rows, 72 x 64, one layer";  // 9 bricks: 3 segments per row, 24 units: 16 workgroups deal them by eights, 12 hold them
  in.nx = 72;
  p = plan_fused_launch(in);
  EXPECT(p.nseg, 3);
  c = plan_fused_chunk(p, in, 1, nullptr, 1);
  EXPECT(c.units, 24); EXPECT(c.full_grid, 16); EXPECT(c.listed_grid, 12);
  in.knobs.use_live_list = false;
  c = plan_fused_chunk(p, in, 1, nullptr, 1);
  EXPECT(finish_fused_chunk(p, in, c, kLiveNotWaited).grid_x, 16);
}

void check_finish() {
  FusedPlanInput in = carved_max(1);
  FusedLaunchPlan p = plan_fused_launch(in);
  FusedChunkPlan c = plan_fused_chunk(p, in, 8, nullptr, 1);  // listed, 128 workgroups, the list pays
  struct { const char* name; int live; unsigned grid; int eager; int flags; } cases[] = {
      {"live 0", 0, 0, 1, 2 | 4 | 8 | 16 | 32 | 64},
      {"live 37", 37, 37, 1, 2 | 4 | 8 | 16 | 32 | 64},
      {"live 127", 127, 127, 1, 2 | 4 | 8 | 16 | 32 | 64},
      {"live 128 of 128", 128, 128, 0, 2 | 4 | 8 | 16 | 64},
      {"live 129 of 128", 129, 128, 0, 2 | 4 | 8 | 16 | 64},
      {"not waited for", kLiveNotWaited, 128, 0, 2 | 4 | 8 | 16 | 64},
  };
  for (const auto& cs : cases) {
    g_case = cs.name;
    const FusedChunkLaunch f = finish_fused_chunk(p, in, c, cs.live);
    EXPECT(f.grid_x, cs.grid); EXPECT(f.eager_state, cs.eager); EXPECT(f.state_flags, cs.flags);
  }
  const int most[2] = {100, 128};
  g_case = "not listed: the last list held most workgroups";
  c = plan_fused_chunk(p, in, 8, most, 3);
  FusedChunkLaunch f = finish_fused_chunk(p, in, c, kLiveNotWaited);
  EXPECT(c.listed, 0); EXPECT(f.grid_x, 128); EXPECT(f.eager_state, 1); EXPECT(f.state_flags, 2 | 4 | 8 | 16 | 32);
  g_case = "listed again at age 16, every workgroup live";
  c = plan_fused_chunk(p, in, 8, most, 16);
  f = finish_fused_chunk(p, in, c, 128);
  EXPECT(c.listed, 1); EXPECT(f.grid_x, 128); EXPECT(f.eager_state, 1); EXPECT(f.state_flags, 2 | 4 | 8 | 16 | 32 | 64);
  g_case = "livelist 0";
  in.knobs.use_live_list = false;
  c = plan_fused_chunk(p, in, 8, nullptr, 1);
  f = finish_fused_chunk(p, in, c, kLiveNotWaited);
  EXPECT(f.grid_x, 128); EXPECT(f.eager_state, 0); EXPECT(f.state_flags, 2 | 4 | 8 | 16);
  g_case = "livelist 0, eagerstate 1";
  in.knobs.eager_state = 1;
  EXPECT(finish_fused_chunk(p, in, c, kLiveNotWaited).eager_state, 1);
  g_case = "eagerstate 0";
  in = carved_max(1);
  in.knobs.eager_state = 0;
  c = plan_fused_chunk(p, in, 8, nullptr, 1);
  EXPECT(finish_fused_chunk(p, in, c, 37).eager_state, 0);
  g_case = "fresh, eagerstate 1";
  in = fresh_max(1);
  in.knobs.eager_state = 1;
  p = plan_fused_launch(in);
  c = plan_fused_chunk(p, in, 8, nullptr, 1);
  f = finish_fused_chunk(p, in, c, kLiveNotWaited);
  EXPECT(f.eager_state, 0); EXPECT(f.state_flags, 1 | 2 | 8 | 16); EXPECT(f.grid_x, 128);
  g_case = "two views, eagerstate 1";
  in = carved_max(2);
  in.knobs.eager_state = 1;
  p = plan_fused_launch(in);
  c = plan_fused_chunk(p, in, 8, nullptr, 1);
  f = finish_fused_chunk(p, in, c, 37);
  EXPECT(f.eager_state, 0); EXPECT(f.grid_x, 37); EXPECT(f.state_flags, 2 | 4);
}

// What the defaults give, as the driver's comments promise: one view the instance compiled for it with the cooperative
// write-back and streaming stores; 8 and 32 views the general instance without; never the few-view flavour.
void check_defaults() {
  for (int fresh = 0; fresh <= 1; ++fresh) {
    const int views[3] = {1, 8, 32};
    for (int n : views) {
      g_case = fresh ? "defaults, fresh kMax" : "defaults, carved kMax";
      const FusedPlanInput in = fresh ? fresh_max(n) : carved_max(n);
      const FusedLaunchPlan p = plan_fused_launch(in);
      EXPECT((int)p.flavour, n == 1 ? kOneView : kGeneral);
      EXPECT(p.coop, n == 1 ? 1 : 0); EXPECT(p.nt, n == 1 ? 1 : 0);
      EXPECT(p.rows, 0); EXPECT(p.big, 0); EXPECT(p.checkmax, 0); EXPECT(p.records, 1); EXPECT(p.in_kernel_prologue, 0);
      EXPECT(p.chunk_layers, 8); EXPECT(p.record_bytes, 4096 * n);
      EXPECT(plan_fused_chunk(p, in, 8, nullptr, 1).listed, !fresh && n <= 8 ? 1 : 0);
    }
  }
  g_case = "default knobs";
  const FusedKnobs k;
  EXPECT(k.tile_mode, 0); EXPECT(k.row_kernel, 0); EXPECT(k.one_view, 1); EXPECT(k.coop_store, -1); EXPECT(k.nt_store, -1);
  EXPECT(k.prologue_mode, 0); EXPECT(k.record_bytes_max, 0); EXPECT(k.use_live_list, 1); EXPECT(k.list_records, 1);
  EXPECT(k.eager_state, -1); EXPECT(k.live_sync, 1); EXPECT(k.use_cull, 1); EXPECT(k.count_pairs, 0); EXPECT(k.use_short_div, 1);
}

struct View {  // the members of ViewParams the geometry reads
  float r[3][3], t[3], fx, fy, cx, cy;
};
View looking_down_z(float fx, float fy, float cx, float cy) { return View{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, {0, 0, 0}, fx, fy, cx, cy}; }

void check_pixels_per_voxel() {
  const View views[2] = {looking_down_z(4.0f, 8.0f, 0, 0), looking_down_z(16.0f, 2.0f, 0, 0)};
  const float x[2] = {-1.0f, 1.0f}, y[2] = {-1.0f, 1.0f}, z[2] = {2.0f, 6.0f}, behind[2] = {-3.0f, 1.0f};
  g_case = "pixels per voxel";  // max(fx, fy) * resolution / depth of the centre: 8 / 4 / 4, 16 / 4 / 4
  EXPECT(worst_pixels_per_voxel(views, 1, false, 0.25f, x, y, z) == 0.5f, 1);
  EXPECT(worst_pixels_per_voxel(views, 2, false, 0.25f, x, y, z) == 1.0f, 1);
  EXPECT(worst_pixels_per_voxel(views, 2, true, 0.25f, x, y, z) == 0.25f, 1);
  EXPECT(worst_pixels_per_voxel(views, 2, false, 0.25f, x, y, behind) == INFINITY, 1);
  EXPECT(worst_pixels_per_voxel(views, 0, false, 0.25f, x, y, z) == 0.0f, 1);
}

void check_rect() {
  const View v = looking_down_z(100.0f, 100.0f, 320.0f, 240.0f);
  const double Y[2] = {-0.5, 0.5};
  {
    g_case = "rect: slab in front";  // u in [270, 370], v in [215, 265] (the near face), 16 px border
    const double X[2] = {-1.0, 1.0}, Z[2] = {2.0, 4.0};
    const ImageRect r = slab_image_rect(v, false, X, Y, Z, 640, 480);
    EXPECT(r.wrect[0], 252); EXPECT(r.wrect[1], 199); EXPECT(r.wrect[2], 388); EXPECT(r.wrect[3], 282); EXPECT(r.quads, 2822);
  }
  {
    g_case = "rect: a corner behind the camera";
    const double X[2] = {-1.0, 1.0}, Z[2] = {-1.0, 4.0};
    const ImageRect r = slab_image_rect(v, false, X, Y, Z, 637, 480);
    EXPECT(r.wrect[0], 0); EXPECT(r.wrect[1], 0); EXPECT(r.wrect[2], 640); EXPECT(r.wrect[3], 480); EXPECT(r.quads, 76800);
  }
  {
    g_case = "rect: orthographic";  // u = x, v = y, whatever z is
    const double X[2] = {10.5, 100.25}, Yo[2] = {20.75, 50.5}, Z[2] = {-1.0, 4.0};
    const ImageRect r = slab_image_rect(v, true, X, Yo, Z, 640, 480);
    EXPECT(r.wrect[0], 0); EXPECT(r.wrect[1], 4); EXPECT(r.wrect[2], 120); EXPECT(r.wrect[3], 67); EXPECT(r.quads, 1890);
  }
  {
    g_case = "rect: left of the image";  // u in [-680, -80]: empty, not negative
    const double X[2] = {-20.0, -16.0}, Z[2] = {2.0, 4.0};
    const ImageRect r = slab_image_rect(v, false, X, Y, Z, 640, 480);
    EXPECT(r.wrect[0], 0); EXPECT(r.wrect[1], 199); EXPECT(r.wrect[2], 0); EXPECT(r.wrect[3], 282); EXPECT(r.quads, 0);
  }
  {
    g_case = "rect: larger than the image";
    const double X[2] = {-10.0, 10.0}, Yb[2] = {-10.0, 10.0}, Z[2] = {2.0, 4.0};
    const ImageRect r = slab_image_rect(v, false, X, Yb, Z, 638, 480);
    EXPECT(r.wrect[0], 0); EXPECT(r.wrect[1], 0); EXPECT(r.wrect[2], 640); EXPECT(r.wrect[3], 480);
  }
}

// ---- max_sdf: the two stages of max_reduce_kernel (carve_kernels.hip) as host loops, against std::max_element ----------
// 64 blocks of 256 lanes take the pixels in strides, every block reduces its lanes by a halving tree, one block does
// the same with the 64 partial pairs and applies the first-pixel rule -- with max_pair and max_first_rule, the functions
// the kernel is made of (max_element_pair.h).
void reduce_block(const float* p, const int64_t* pidx, int64_t n, int block, int blocks, float* out, int64_t* out_idx) {
  float sm[256];
  int64_t si[256];
  for (int t = 0; t < 256; ++t) {
    float m = -INFINITY;
    int64_t mi = INT64_MAX;
    for (int64_t i = (int64_t)block * 256 + t; i < n; i += (int64_t)blocks * 256) max_pair(m, mi, p[i], pidx ? pidx[i] : i);
    sm[t] = m, si[t] = mi;
  }
  for (int s = 128; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) max_pair(sm[t], si[t], sm[t + s], si[t + s]);
  *out = sm[0], *out_idx = si[0];
}
float max_sdf_by_pairs(const std::vector<float>& img) {
  float part[64], m;
  int64_t part_idx[64], mi;
  for (int b = 0; b < 64; ++b) reduce_block(img.data(), nullptr, (int64_t)img.size(), b, 64, &part[b], &part_idx[b]);
  reduce_block(part, part_idx, 64, 0, 1, &m, &mi);
  return max_first_rule(m, img[0]);
}
uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
void expect_max_element(const char* name, const std::vector<float>& img) {
  g_case = name;
  const float want = *std::max_element(img.begin(), img.end()), got = max_sdf_by_pairs(img);
  EXPECT(got != got, want != want);                              // a NaN exactly where std::max_element gives one
  if (want == want) EXPECT(bits_of(got), bits_of(want));         // else the same bits: the sign of a zero included
}
void check_max_element() {
  uint32_t seed = 12345u;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
  const float nan = std::nanf(""), inf = INFINITY;
  for (size_t n : {(size_t)1, (size_t)2, (size_t)255, (size_t)256, (size_t)257, (size_t)16387, (size_t)48 * 40, (size_t)1280 * 720}) {
    std::vector<float> a(n);
    for (float& v : a) v = rnd();
    expect_max_element("max_element: noise", a);
    std::vector<float> b = a;
    b[n / 2] = b[n - 1] = 3.0f, b[n / 3] = nan;
    expect_max_element("max_element: tied maxima, a NaN that is not first", b);
    b[0] = nan;
    expect_max_element("max_element: the first pixel a NaN", b);
    std::vector<float> z(n);
    for (size_t i = 0; i < n; ++i) z[i] = (i % 7 == 3) ? (i % 2 ? 0.0f : -0.0f) : -1.0f - (float)(i % 5);
    expect_max_element("max_element: zero maximum, a zero of either sign first", z);
    for (float& v : z) v = -v == 0.0f ? -v : v;                  // every zero's sign flipped
    expect_max_element("max_element: zero maximum, the other sign first", z);
    z[0] = -0.0f;
    expect_max_element("max_element: -0 at the first pixel", z);
    expect_max_element("max_element: -inf everywhere", std::vector<float>(n, -inf));
    expect_max_element("max_element: NaN everywhere", std::vector<float>(n, nan));
    b.assign(n, -inf), b[n - 1] = inf, b[n / 2] = nan;
    expect_max_element("max_element: +inf the last pixel", b);
    b.assign(n, nan), b[0] = -2.0f;
    expect_max_element("max_element: only the first pixel is no NaN", b);
    b.assign(n, 3.4028234664e38f), b[n / 2] = -3.4028234664e38f;
    expect_max_element("max_element: FLT_MAX and lowest()", b);
    b.assign(n, -1e-45f), b[n - 1] = 1e-45f;
    expect_max_element("max_element: denormals", b);
  }
}

}  // namespace

int main() {
  static_assert(kWgWaves == 4 && kRowBricks == 4 && kRowWaves == 2 && kRowMaxViews == 8 && kLiveListMaxViews == 8 &&
                    kLiveEntryWords == 10 && WX == 8 && BX == 32 && BY == 8 && BZ == 8,
                "the literals below are those of the default build");
  check_bounds_and_modes();
  check_update_limit();
  check_tile_kind();
  check_rows();
  check_coop();
  check_state_flags_base();
  check_chunk_layers();
  check_live_list();
  check_rows_grids();
  check_finish();
  check_defaults();
  check_pixels_per_voxel();
  check_rect();
  check_max_element();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
