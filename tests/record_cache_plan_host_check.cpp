// "This launch reuses the footprint records of the last one" (vacancy_amd/csrc/carve_fused_plan.h: fused_reuses_records,
// fused_records_cacheable), as a program of its own, also under AddressSanitizer and UBSan (driven by
// tests/test_record_cache_plan_host.py).
//
// A launch that reuses records it should have made gives wrong drops; one that never reuses passes every state test and
// only gets slower.  Here every condition of the rule is asked on both sides, one named case each, against literals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "carve_fused_plan.h"

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

// 64^3, kMax, bilinear, 32 views 0.5 pixels per voxel (raw tiles), every knob at its default
FusedPlanInput fresh_max(int n_views) {
  FusedPlanInput in;
  in.update = VCY_UPDATE_MAX, in.trunc = false, in.interp = VCY_INTERP_BILINEAR;
  in.max_update_num = 255, in.weight = 1.0f;
  in.nx = in.ny = in.nz_local = 64;
  in.fresh = true, in.cnt_implied = true, in.brick_min_valid = false, in.have_brick_min = true;
  in.views_before = 0, in.n_views = n_views, in.ortho = false;
  in.worst = 0.5f;
  return in;
}
FusedPlanInput carved_max(int n_views) {
  FusedPlanInput in = fresh_max(n_views);
  in.fresh = false, in.brick_min_valid = true, in.views_before = 40;
  return in;
}

struct Answer {
  int cacheable, reuse_on_match, reuse_on_mismatch, stale_flag_is_new_bit;
};
Answer ask(const FusedPlanInput& in, bool have_planes = true) {
  const FusedLaunchPlan p = plan_fused_launch(in);
  const FusedChunkPlan c = plan_fused_chunk(p, in, p.chunk_layers, nullptr, 1);
  const FusedChunkLaunch f = finish_fused_chunk(p, in, c, kLiveNotWaited);
  Answer a;
  a.cacheable = fused_records_cacheable(p, in, c, have_planes) ? 1 : 0;
  a.reuse_on_match = fused_reuses_records(p, in, c, have_planes, true) ? 1 : 0;
  a.reuse_on_mismatch = fused_reuses_records(p, in, c, have_planes, false) ? 1 : 0;
  a.stale_flag_is_new_bit = (f.state_flags & kStateStaleBounds) == 0 ? 1 : 0;  // (the plan never sets it: the driver does)
  return a;
}
#define EXPECT_ANSWER(in_, planes_, cacheable_)                                       \
  do {                                                                                \
    const Answer a_ = ask(in_, planes_);                                              \
    EXPECT(a_.cacheable, cacheable_);                                                 \
    EXPECT(a_.reuse_on_match, cacheable_);  /* a launch of the kind reuses on a hit */ \
    EXPECT(a_.reuse_on_mismatch, 0);        /* ... and nothing reuses on a miss */    \
    EXPECT(a_.stale_flag_is_new_bit, 1);                                              \
  } while (0)

void check_rule() {
  FusedPlanInput in;
  g_case = "the headline: fresh kMax, 32 views";
  EXPECT_ANSWER(fresh_max(32), true, 1);
  g_case = "carved kMax, 32 views";
  EXPECT_ANSWER(carved_max(32), true, 1);
  g_case = "kMax with truncation";
  in = fresh_max(32), in.trunc = true;
  EXPECT_ANSWER(in, true, 1);

  g_case = "the knob: recordcache 0";
  in = fresh_max(32), in.knobs.record_cache = false;
  EXPECT_ANSWER(in, true, 0);
  g_case = "the knob: recordcache 1 (the default)";
  in = fresh_max(32);
  EXPECT(in.knobs.record_cache, 1);
  EXPECT_ANSWER(in, true, 1);

  g_case = "the key: matches / differs";
  {
    const FusedLaunchPlan p = plan_fused_launch(in);
    const FusedChunkPlan c = plan_fused_chunk(p, in, p.chunk_layers, nullptr, 1);
    EXPECT(fused_reuses_records(p, in, c, true, true), 1);
    EXPECT(fused_reuses_records(p, in, c, true, false), 0);
  }

  g_case = "flavour: one view takes the one-view instance";
  EXPECT((int)plan_fused_launch(fresh_max(1)).flavour, (int)CarveFlavour::kOneView);
  EXPECT_ANSWER(fresh_max(1), true, 0);
  g_case = "flavour: one view, oneview 0 -> general";
  in = fresh_max(1), in.knobs.one_view = 0;
  EXPECT((int)plan_fused_launch(in).flavour, (int)CarveFlavour::kGeneral);
  EXPECT_ANSWER(in, true, 1);
  g_case = "flavour: rowkernel -1, 8 views -> rows";
  in = fresh_max(8), in.knobs.row_kernel = -1;
  EXPECT((int)plan_fused_launch(in).flavour, (int)CarveFlavour::kRows);
  EXPECT_ANSWER(in, true, 0);
  g_case = "flavour: rowkernel -1, 9 views -> general";
  in = fresh_max(9), in.knobs.row_kernel = -1;
  EXPECT_ANSWER(in, true, 1);

  g_case = "keeps its records: weighted average does not";
  in = fresh_max(32), in.update = VCY_UPDATE_WEIGHTED_AVERAGE;
  EXPECT_ANSWER(in, true, 0);
  g_case = "keeps its records: weighted average with truncation (bounds and lower bounds) does not";
  in.trunc = true;
  EXPECT(plan_fused_launch(in).need_bound, 1); EXPECT(plan_fused_launch(in).want_lower, 1);
  EXPECT_ANSWER(in, true, 0);
  g_case = "keeps its records: the big tile does not (tile 2)";
  in = fresh_max(32), in.knobs.tile_mode = 2;
  EXPECT_ANSWER(in, true, 0);
  g_case = "keeps its records: the big tile does not (0.8661 pixels per voxel)";
  in = fresh_max(32), in.worst = 0.8661f;
  EXPECT_ANSWER(in, true, 0);
  g_case = "keeps its records: raw tiles just below (0.866 pixels per voxel)";
  in.worst = 0.866f;
  EXPECT_ANSWER(in, true, 1);
  g_case = "keeps its records: with the update limit in reach too";
  in = carved_max(32), in.views_before = 224;
  EXPECT(plan_fused_launch(in).checkmax, 1);
  EXPECT_ANSWER(in, true, 1);

  g_case = "need_bound: cull 0";
  in = fresh_max(32), in.knobs.use_cull = false;
  EXPECT(plan_fused_launch(in).need_bound, 0);
  EXPECT_ANSWER(in, true, 0);

  g_case = "prologue 1: no records";
  in = fresh_max(32), in.knobs.prologue_mode = 1;
  EXPECT_ANSWER(in, true, 0);
  g_case = "prologue 2: records";
  in.knobs.prologue_mode = 2;
  EXPECT_ANSWER(in, true, 1);

  // 64^3 x 32 views: 16384 bytes of records per brick layer, 8 layers
  g_case = "one chunk: recordbytes exactly the launch";
  in = fresh_max(32), in.knobs.record_bytes_max = 131072;
  EXPECT(plan_fused_launch(in).chunk_layers, 8);
  EXPECT_ANSWER(in, true, 1);
  g_case = "chunked: one byte less";
  in.knobs.record_bytes_max = 131071;
  EXPECT(plan_fused_launch(in).chunk_layers, 7);
  EXPECT_ANSWER(in, true, 0);

  g_case = "window planes: none (out of memory for them)";
  EXPECT_ANSWER(fresh_max(32), false, 0);
  g_case = "window planes: there";
  EXPECT_ANSWER(fresh_max(32), true, 1);

  g_case = "listed: 8 views over a carved grid";
  in = carved_max(8), in.knobs.one_view = 0;
  {
    const FusedLaunchPlan p = plan_fused_launch(in);
    EXPECT(plan_fused_chunk(p, in, p.chunk_layers, nullptr, 1).listed, 1);
  }
  EXPECT_ANSWER(in, true, 0);
  g_case = "not listed: 9 views over a carved grid";
  EXPECT_ANSWER(carved_max(9), true, 1);
  g_case = "not listed: 8 views over a fresh grid";
  EXPECT_ANSWER(fresh_max(8), true, 1);
  g_case = "not listed: 8 views, livelist 0";
  in = carved_max(8), in.knobs.use_live_list = false;
  EXPECT_ANSWER(in, true, 1);
  g_case = "not listed: the last list held most workgroups";
  in = carved_max(8);
  {
    const int hint[2] = {100, 128};
    const FusedLaunchPlan p = plan_fused_launch(in);
    const FusedChunkPlan c = plan_fused_chunk(p, in, p.chunk_layers, hint, 3);
    EXPECT(c.listed, 0);
    EXPECT(fused_reuses_records(p, in, c, true, true), 1);
    const FusedChunkPlan c16 = plan_fused_chunk(p, in, p.chunk_layers, hint, 16);  // (every 16th launch looks again)
    EXPECT(c16.listed, 1);
    EXPECT(fused_reuses_records(p, in, c16, true, true), 0);
  }

  g_case = "the flags";
  EXPECT(kStateStaleBounds, 128);
  EXPECT(kStateStaleBounds & (kStateFresh | kStateCountImplied | kStateBrickMinValid | kStateCoopStore | kStateStreamStore |
                              kStateEager | kStateListRecords), 0);
}

}  // namespace

int main() {
  check_rule();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
