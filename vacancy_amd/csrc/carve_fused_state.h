// What the fused carve keeps in a context between its launches, with one owner: the knobs, the buffers it grows on
// demand, the cache of what the last launch derived from its views, and the hint of the last live list.
// vcy_ctx::fused; the code that uses it: carve_fused.hip.  (Included by vcy_internal.h, ahead of the context and of
// carve_common.h, so it cannot live in carve_fused.h next to the launch's other types.)
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "carve_fused_plan.h"  // FusedKnobs
#include "vcy_resources.h"

namespace vcy {

// Everything derived from the views of a launch -- the c0 records (n_views * nx products), the image-space bounding box
// of the slab in every view, the device copies -- depends on nothing but the views' parameters (image pointers included)
// and this key: a launch with the SAME views as the last one (the reference's loop carves a sequence of grids with one
// camera rig; the benchmark repeats its step) takes all of it as it is.  Comparing 4 KB instead of rebuilding and
// comparing 0.5 MB took 0.1 ms of host time out of every launch, which is what a z-slab of an 8-GPU run pays 10 % of
// its step for.
struct FusedViewKey {
  const float* wmax;         // the planes' address
  const void* at;            // where the records were built (the staging buffer may move)
  bool bound, lower, ortho;  // need_bound, need_lower, the projection model
  int zlo, zhi;              // the slices the rectangles cover
  bool operator==(const FusedViewKey& o) const {
    return wmax == o.wmax && at == o.at && bound == o.bound && lower == o.lower && ortho == o.ortho && zlo == o.zlo &&
           zhi == o.zhi;
  }
};
struct FusedViewCache {
  bool valid = false;    // FusedState::d_scratch holds what `vp` under `key` gives
  std::vector<char> vp;  // the ViewParams of the launch that filled it
  FusedViewKey key{};
  bool samef = true;     // what that launch found: fx == fy in every view ...
  int max_quads = 0;     // ... and the threads per view of the window-maximum kernels
  bool matches(const FusedViewKey& k, const void* vp_now, size_t vp_bytes) const;
  void remember(const FusedViewKey& k, const void* vp_now, size_t vp_bytes, bool samef_now, int max_quads_now);
};

// Which launch the record buffer (FusedState::d_records) describes ("recordcache", fused_reuses_records in
// carve_fused_plan.h).  The key is everything the GEOMETRY of a footprint record depends on, as bytes (record_key in
// carve_fused.hip builds it): the view count; of every view the rotation, translation, fx, fy, cx, cy, width, height and
// the ROI -- not the image pointer, not max_sdf, not the plane addresses, which only the bound depends on; fx == fy in
// every view, the generic sampler, the projection model and the outside mode; the slab and its bricks; the buffer's
// address and size (a regrown buffer is another buffer).  Whatever writes the buffer forgets the key first and remembers
// its own afterwards, if it is of the kind a later launch may reuse (write_records, the one place).  vcy_reset does not
// touch it: the records do not depend on the voxel state.
struct FusedRecordCache {
  bool valid = false;
  std::vector<char> key;
  int hits = 0;  // launches that reused the records (vcy_get_param "recordcache_hits")
  bool matches(const std::vector<char>& k) const { return valid && key == k; }
  void remember(std::vector<char>&& k) { key = std::move(k), valid = true; }
  void forget() { valid = false; }
};

// The view blocks of a launch with new views are built in page-locked host memory -- two buffers taken in turn, each
// with an event that says when the copy out of it has been made -- so that such a launch queues behind the previous
// one like any other work on the stream.
struct FusedViewStage {
  PinnedBuf<> h[2];
  Event ev[2];  // "the copy out of buffer q has been made"
  int idx = 0;
  int next(size_t bytes, void** out);  // the other buffer, at least `bytes` large, once the copy out of it has been made
  int copied(hipStream_t stream);      // the copy out of the buffer handed out last is queued on `stream`
};

struct FusedState {
  FusedKnobs knobs;
  FusedViewCache cache;
  FusedViewStage stage;
  DeviceBuf<> d_scratch;       // c0 records + view blocks of one launch (prepare_views)
  DeviceBuf<float> d_wmax;     // window-maximum planes of the views of one launch
  DeviceBuf<> d_records;       // footprint records of one chunk, 8 bytes per (wave brick, view)
  FusedRecordCache rec_cache;  // ... and which launch they describe
  DeviceBuf<int> d_wg_list;    // live workgroups of a chunk of few views ([0] = count), live_workgroups_kernel
  PinnedBuf<int> h_live_hint;  // page-locked {live workgroups, workgroups} of the last listed chunk (a hint: plan_fused_chunk)
  int64_t live_list_age = 0;   // chunks launched so far
  DeviceBuf<unsigned long long> d_pair_count;  // "paircount" 1: (brick, view) pairs per brick layer of the slab, of the last launch (vcy_last_carve_pairs)
  int pair_count_views = 0;
  int last_div_level = 0;      // division variant of the last launch (vcy_get_param "div_level")

  void forget_live_hint() {    // the slab starts over (vcy_reset): the next few-view launch lists its workgroups
    if (h_live_hint) h_live_hint[0] = h_live_hint[1] = 0;
  }
};

}  // namespace vcy
