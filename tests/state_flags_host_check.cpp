// What a context keeps beside its voxel state (vacancy_amd/csrc/state_flags.h), as a program of its own under
// AddressSanitizer and UBSan (make state_flags_host_check; driven by tests/test_state_model_cpu.py).
//
// From every combination of the flags that a context can reach -- and a few it cannot -- every writer's declaration is
// applied, and what comes out is compared with the table of DESIGN.md ("Writers declare, caches compare"), written out
// here as data: a row says for each flag whether the writer leaves it ('='), clears it ('0') or sets it ('1').
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "state_flags.h"

using vcy::StateFlags;
using vcy::StateWrite;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAILED %s:%d: ", __FILE__, __LINE__);  \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      if (++failures > 20) std::exit(1);                  \
    }                                                     \
  } while (0)

constexpr int64_t kViews = 7;   // views of the call, or the largest count an upload brings
enum ViewsRule { kAdd, kSet, kSetMax, kZero };

struct Row {
  const char* writer;
  char fresh, halo, implied, minima;  // '=' stays, '0' cleared, '1' set
  ViewsRule views;
  bool is_fill;
  StateWrite decl;  // (unused by the fill)
};

// The transition table.  `fresh` is a fact about memory: only the fill sets it, and no declaration clears it (stored()).
const Row kTable[] = {
    //                          fresh halo impl minima  views
    {"fill / reset / create",    '1', '0', '1', '0', kZero, true, {}},
    {"upload",                   '=', '0', '0', '0', kSetMax, false, StateWrite::upload(0)},  // (decl made per state below)
    {"silhouettes, fused",       '=', '0', '=', '=', kAdd, false, StateWrite::silhouettes(kViews, true, false)},
    {"silhouettes, per view",    '=', '0', '=', '0', kAdd, false, StateWrite::silhouettes(kViews, false, false)},
    {"queue flush, fused",       '=', '=', '=', '=', kAdd, false, StateWrite::silhouettes(kViews, true, true)},
    {"queue flush, per view",    '=', '=', '=', '0', kAdd, false, StateWrite::silhouettes(kViews, false, true)},
    {"robust",                   '=', '0', '1', '0', kSet, false, StateWrite::robust(kViews)},
    {"depth",                    '=', '0', '=', '0', kAdd, false, StateWrite::depth(kViews)},
    {"component filter",         '=', '0', '=', '=', kAdd /* of nothing */, false, StateWrite::filter()},
};

bool expect(char rule, bool before) { return rule == '=' ? before : rule == '1'; }

// the labelling of a state: none, of the state as it is, of an earlier state
enum Labelling { kNone, kCurrent, kStale };

StateFlags make(bool fresh, bool halo, bool implied, bool minima, int64_t views, Labelling lab) {
  StateFlags s;
  s.fresh = fresh, s.halo_valid = halo, s.cnt_implied = implied, s.brick_min_valid = minima, s.views_carved = views;
  s.epoch = 41;
  if (lab == kStale) s.slab_labelled(0.25);
  if (lab == kStale) ++s.epoch;
  if (lab == kCurrent) s.slab_labelled(0.25);
  return s;
}

void apply(const Row& r, StateFlags* s) {
  if (r.is_fill) {
    s->filled();
  } else if (r.views == kSetMax) {
    s->written(StateWrite::upload(s->views_carved > kViews ? s->views_carved : kViews));  // as vcy_upload declares it
  } else {
    s->written(r.decl);
  }
}

void check_table() {
  const int64_t views_before[] = {0, 3, 300};
  int states = 0;
  for (int bits = 0; bits < 16; ++bits)
    for (int64_t v0 : views_before)
      for (int lab = kNone; lab <= kStale; ++lab) {
        const bool fresh = bits & 1, halo = bits & 2, implied = bits & 4, minima = bits & 8;
        if (minima && !implied) continue;  // the one combination no sequence of calls reaches (check_closure)
        ++states;
        for (const Row& r : kTable) {
          StateFlags s = make(fresh, halo, implied, minima, v0, (Labelling)lab);
          const StateFlags b = s;
          CHECK(s.seams_current(true) == (lab == kCurrent), "%s: the labelling before", r.writer);
          apply(r, &s);
          CHECK(s.fresh == expect(r.fresh, b.fresh), "%s: fresh %d from %d", r.writer, s.fresh, b.fresh);
          CHECK(s.halo_valid == expect(r.halo, b.halo_valid), "%s: halo_valid %d from %d", r.writer, s.halo_valid, b.halo_valid);
          CHECK(s.cnt_implied == expect(r.implied, b.cnt_implied), "%s: cnt_implied %d from %d", r.writer, s.cnt_implied, b.cnt_implied);
          CHECK(s.brick_min_valid == expect(r.minima, b.brick_min_valid), "%s: brick_min_valid %d from %d (implied %d)", r.writer,
                s.brick_min_valid, b.brick_min_valid, b.cnt_implied);
          const int64_t want = r.views == kZero  ? 0
                               : r.views == kSet ? kViews
                               : r.views == kSetMax ? (v0 > kViews ? v0 : kViews)
                               : v0 + (r.decl.views_added);
          CHECK(s.views_carved == want, "%s: views_carved %lld, expected %lld", r.writer, (long long)s.views_carved, (long long)want);
          CHECK(s.epoch == b.epoch + 1, "%s: the epoch moved by %lld", r.writer, (long long)(s.epoch - b.epoch));
          // every writer makes the slab labelling stale, with or without queued views
          CHECK(!s.seams_current(true) && !s.seams_current(false), "%s: the seam calls may still follow", r.writer);
          CHECK(s.cc_iso == b.cc_iso, "%s: the labelling's iso level moved", r.writer);
        }
      }
  CHECK(states == 12 * 3 * 3, "%d states", states);
  // the filter adds no view, the others kViews
  CHECK(StateWrite::filter().views_added == 0 && StateWrite::depth(kViews).views_added == kViews, "views added");
}

// Not a writer's: what else moves the flags, and the exceptions of the table.
void check_the_rest() {
  for (int lab = kNone; lab <= kStale; ++lab)
    for (int halo = 0; halo < 2; ++halo) {
      // a filter call that removes nothing launches nothing and declares nothing: only the halo goes (the neighbour ran its own)
      StateFlags s = make(false, halo, true, true, 3, (Labelling)lab);
      const StateFlags b = s;
      s.halo_stale();
      CHECK(!s.halo_valid && s.epoch == b.epoch && s.brick_min_valid && s.cnt_implied && s.views_carved == 3, "halo_stale");
      CHECK(s.seams_current(true) == (lab == kCurrent), "a filter that removed nothing keeps the labelling");
      CHECK(!s.seams_current(false), "queued views: the seam calls must wait for them");
    }
  {
    // the queue: queueing makes the halo stale; a halo installed afterwards survives the flush and nothing else
    StateFlags s = make(false, true, true, true, 2, kNone);
    s.halo_stale();
    s.written(StateWrite::silhouettes(2, true, true));
    CHECK(!s.halo_valid, "a flush must not make a stale halo valid");
    s.halo_stale();
    s.halo_installed();
    s.written(StateWrite::silhouettes(2, true, true));
    CHECK(s.halo_valid && s.views_carved == 6, "the flush keeps a halo installed since the views were queued");
    for (const Row& r : kTable) {
      StateFlags t = s;
      apply(r, &t);
      CHECK(t.halo_valid == (r.halo == '='), "%s: an installed halo %s", r.writer, t.halo_valid ? "stayed" : "went");
    }
  }
  {
    // labelling: current until the next write; dropped by another labelling; the iso level is kept
    StateFlags s = make(false, false, true, false, 1, kNone);
    CHECK(!s.seams_current(true), "never labelled");
    s.slab_labelled(-0.5);
    CHECK(s.seams_current(true) && !s.seams_current(false) && s.cc_iso == -0.5, "labelled");
    s.halo_installed();
    s.stored();
    CHECK(s.seams_current(true), "installing a halo or materialising is no write");
    s.labelling_dropped();
    CHECK(!s.seams_current(true), "dropped");
    s.slab_labelled(0.0);
    s.filled();
    CHECK(!s.seams_current(true), "the fill makes the labelling stale");
    s.slab_labelled(0.0);  // (a fresh slab may be labelled: nothing is solid)
    CHECK(s.seams_current(true) && s.fresh, "labelled while fresh");
  }
  {
    // fresh and the minima: stored() and minima_rebuilt() are the fused launch's on success
    StateFlags s;
    CHECK(!s.fresh && !s.halo_valid && s.cnt_implied && !s.brick_min_valid && s.views_carved == 0 && s.cc_epoch != s.epoch, "defaults");
    s.filled();
    s.written(StateWrite::silhouettes(2, true, false));
    CHECK(s.fresh && !s.brick_min_valid, "a declaration neither stores nor rebuilds");
    s.stored();
    s.minima_rebuilt(false);
    CHECK(!s.fresh && !s.brick_min_valid, "no array, no minima");
    s.minima_rebuilt(true);
    CHECK(s.brick_min_valid, "minima after a fused launch");
    s.written(StateWrite::upload(9));
    s.minima_rebuilt(true);
    CHECK(!s.brick_min_valid && !s.cnt_implied, "no minima while the counters imply nothing");
    s.written(StateWrite::robust(4));
    s.minima_rebuilt(true);
    CHECK(s.brick_min_valid && s.cnt_implied && s.views_carved == 4, "the robust carve starts the state over");
    // no writer of today keeps the minima and brings counters of its own; one that did would still lose the minima
    s.written(StateWrite{StateWrite::kMinimaKept, StateWrite::kCountsArbitrary, 0, -1, StateWrite::kHaloStale});
    CHECK(!s.brick_min_valid && !s.cnt_implied && s.views_carved == 4, "minima kept by a writer of arbitrary counters");
  }
}

// brick_min_valid without cnt_implied is never reached: from the defaults, every function in every order, to a fixed point
void check_closure() {
  bool seen[32] = {false};
  auto key = [](const StateFlags& s) { return (s.fresh ? 1 : 0) | (s.halo_valid ? 2 : 0) | (s.cnt_implied ? 4 : 0) | (s.brick_min_valid ? 8 : 0); };
  StateFlags todo[32];
  int n_todo = 0;
  todo[n_todo++] = StateFlags();
  seen[key(todo[0])] = true;
  while (n_todo > 0) {
    const StateFlags s = todo[--n_todo];
    for (int op = 0; op < 16; ++op) {
      StateFlags t = s;
      if (op < 9) apply(kTable[op], &t);
      else if (op == 9) t.stored();
      else if (op == 10) t.minima_rebuilt(true);
      else if (op == 11) t.minima_rebuilt(false);
      else if (op == 12) t.halo_installed();
      else if (op == 13) t.halo_stale();
      else if (op == 14) t.slab_labelled(0.0);
      else t.labelling_dropped();
      CHECK(!(t.brick_min_valid && !t.cnt_implied), "brick minima valid without cnt_implied after operation %d", op);
      if (!seen[key(t)]) seen[key(t)] = true, todo[n_todo++] = t;
    }
  }
  int n_seen = 0;
  for (int k = 0; k < 16; ++k) n_seen += seen[k] ? 1 : 0;
  CHECK(n_seen == 12, "%d combinations of the four flags are reachable, expected the 12 of the table check", n_seen);
}

}  // namespace

int main() {
  static_assert(sizeof(kTable) / sizeof(kTable[0]) == 9, "nine rows");
  check_table();
  check_the_rest();
  check_closure();
  if (failures) {
    std::printf("state_flags_host_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("state_flags_host_check: ok\n");
  return 0;
}
