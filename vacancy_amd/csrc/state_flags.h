// What a context knows about its voxel state beside the state itself, and the one place where that knowledge changes.
// The rule: whoever changes a voxel of the owned slab says so ONCE per API call, with written(), before its first launch or
// copy that does; the fill says filled().  A cache of something derived from the state remembers the epoch it describes
// (the ray-cast's bit planes: vcy_ctx::rn_epoch; the slab labelling: cc_epoch).  Everything else only reads the fields.
// Host code only, no HIP: tests/state_flags_host_check.cpp checks every transition against the table of DESIGN.md
// ("Writers declare, caches compare").
#pragma once

#include <cstdint>

namespace vcy {

// The facts about one writer that decide what survives it.
struct StateWrite {
  enum Minima { kMinimaLost, kMinimaKept } minima;  // kept: by the writer's own kernel, where they were valid
  // "update_num == 0 implies sdf == lowest()": untouched, true again (the state starts over), or unknown
  enum Counts { kCountsLeft, kCountsImplied, kCountsArbitrary } counts;
  int64_t views_added;                        // to views_carved ...
  int64_t views_set;                          // ... or, when >= 0, its new value
  enum Halo { kHaloStale, kHaloStays } halo;  // stays: the flush of queued views alone

  // The writers.  `queued` (flush_pending): the views made the halo stale when they were queued, and a halo installed since
  // then came from a neighbour that has applied the same views.
  static StateWrite silhouettes(int64_t n_views, bool fused, bool queued) {  // (the fused kernel keeps the brick minima)
    return {fused ? kMinimaKept : kMinimaLost, kCountsLeft, n_views, -1, queued ? kHaloStays : kHaloStale};
  }
  static StateWrite depth(int64_t n_views) { return {kMinimaLost, kCountsLeft, n_views, -1, kHaloStale}; }
  static StateWrite robust(int64_t n_views) { return {kMinimaLost, kCountsImplied, 0, n_views, kHaloStale}; }
  static StateWrite upload(int64_t max_count) { return {kMinimaLost, kCountsArbitrary, 0, max_count, kHaloStale}; }
  static StateWrite filter() { return {kMinimaKept, kCountsLeft, 0, -1, kHaloStale}; }
  // (its final kernel writes columns along z and does not reduce the bricks' minima again)
  static StateWrite redistance() { return {kMinimaLost, kCountsLeft, 0, -1, kHaloStale}; }
};

struct StateFlags {
  // Lazy initialisation, a fact about memory rather than a cache: after filled() the slab is KNOWN to be sdf = lowest(),
  // update_num = 0 without having been written.  The fused carve starts from that knowledge (no state read, no fill pass)
  // and the robust carve overwrites it; everything else calls materialize() first.
  bool fresh = false;
  bool halo_valid = false;       // the halo slices below the slab are the neighbour's last two, as the state is now
  bool cnt_implied = true;       // update_num == 0 implies sdf == lowest(): no vcy_upload since the fill
  bool brick_min_valid = false;  // vcy_ctx::d_brick_min is current (only ever true with cnt_implied and the array allocated)
  int64_t views_carved = 0;      // upper bound on any voxel's update_num (each carved view adds at most one)
  int64_t epoch = 0;             // bumped by every write and by the fill
  int64_t cc_epoch = -1;         // the epoch vcy_label_components_slab labelled (-1: no slab labelling) ...
  double cc_iso = 0.0;           // ... at this iso level

  void filled() {
    written({StateWrite::kMinimaLost, StateWrite::kCountsImplied, 0, 0, StateWrite::kHaloStale});
    fresh = true;  // written lazily
  }
  void written(const StateWrite& w) {
    ++epoch;
    if (w.halo != StateWrite::kHaloStays) halo_valid = false;
    if (w.counts != StateWrite::kCountsLeft) cnt_implied = w.counts == StateWrite::kCountsImplied;
    if (w.minima != StateWrite::kMinimaKept || !cnt_implied) brick_min_valid = false;
    views_carved = w.views_set >= 0 ? w.views_set : views_carved + w.views_added;
  }
  // every voxel of the slab is in memory (materialize, a fused launch that succeeded, the robust launch)
  void stored() { fresh = false; }
  // launch_carve_fused alone, after a launch that succeeded: every wave that ran wrote its brick's entry
  void minima_rebuilt(bool have_array) { brick_min_valid = have_array && cnt_implied; }

  void halo_installed() { halo_valid = true; }
  // the state BELOW this slab moves without a write here: a view was queued (the neighbour queues it too), or the slab
  // flow's filter step ran (the neighbour runs its own)
  void halo_stale() { halo_valid = false; }

  void slab_labelled(double iso) { cc_epoch = epoch, cc_iso = iso; }
  void labelling_dropped() { cc_epoch = -1; }  // another labelling replaces the slab's (label_components starts)
  // the seam calls may lean on the slab labelling: it describes the state as it is, and no queued view is about to change it
  bool seams_current(bool pending_empty) const { return cc_epoch == epoch && pending_empty; }
};

}  // namespace vcy
