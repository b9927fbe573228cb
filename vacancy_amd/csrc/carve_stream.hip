// The streamed silhouette paths of the C ABI: silhouettes in host memory become SDF images on the device in chunks of
// 32 -- page-locked staging, DMA, device transform -- while the previous chunk is carved.  Three entry points share one
// layout, one producer step and one consume step: vcy_make_sdf_batch_device (images only, into caller-owned memory),
// vcy_carve_batch_silhouettes (one context) and vcy_carve_batch_silhouettes_sharded (the z-slabs of one grid, the devices
// sharing the producer).  The kernels and their launches: sdf2d.hip, carve_kernels.hip, carve_fused.hip.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "rccl_api.h"

namespace vcy {
namespace {

#ifndef VCY_STAGE_THREADS
#define VCY_STAGE_THREADS 4   // (8 and 16 measured: the producer side of 32 silhouettes at 1280 x 720 stays at 1.45 - 1.5 ms)
#endif
constexpr int kStageThreads = VCY_STAGE_THREADS;  // host threads that copy silhouettes into page-locked staging and queue their DMAs
constexpr int kChunk = 32;  // views per fused launch of the streamed paths: the next 32 silhouettes upload and transform meanwhile

// Slot sizes of the streamed paths, all from the largest image of the call and rounded to 256 bytes.
struct StreamLayout {
  size_t sz_mask;  // one silhouette (staging and device)
  size_t sz_sdf;   // one SDF image in the pool of a context: four times the silhouette's slot
  size_t stride;   // one SDF image of the sharded producer: what a rank sends per chunk is `per` of these
  size_t sz_scr;   // transform scratch of one image
  explicit StreamLayout(size_t max_px)
      : sz_mask((max_px + 255) / 256 * 256),
        sz_sdf(sz_mask * sizeof(float)),
        stride((max_px * sizeof(float) + 255) / 256 * 256),
        sz_scr((device_make_sdf_scratch_bytes(1, (int)max_px) + 255) / 256 * 256) {}
};

// How a step or a call failed: the code of the library call that failed (its message is set), or VCY_ERR_HIP with the
// runtime call that failed first, which the entry point words.  The first failure stays.
struct Failure {
  int rc = VCY_OK;
  hipError_t e = hipSuccess;
  const char* what = "";
  bool hip(hipError_t err, const char* w) {
    if (err != hipSuccess && rc == VCY_OK) rc = VCY_ERR_HIP, e = err, what = w;
    return err == hipSuccess;
  }
};

// The producer step: silhouette j of `m` is copied into slot j of the page-locked `stage` and its DMA into slot j of
// `dmask` is queued on `st`, by `n_thr` host threads (pageable memory would be copied through the runtime's own bounce
// buffer by one thread); `uploaded` (if any) is recorded behind the DMAs; then MakeSignedDistanceField
// (voxel_carver.cc:405-408) for all of them at once, into out[j].
Failure produce_images(hipStream_t st, int device, int m, const vcy_view* views, const uint8_t* const* masks_host,
                       float* const* out, char* stage, char* dmask, char* scratch, const StreamLayout& L,
                       const vcy_carver_option& o, int n_thr, hipEvent_t uploaded) {
  n_thr = std::max(1, std::min(m, n_thr));
  std::vector<const uint8_t*> mptr((size_t)m);
  std::vector<hipError_t> terr((size_t)n_thr, hipSuccess);
  auto worker = [&](int t) {
    if (t > 0) (void)hipSetDevice(device);
    for (int j = t; j < m; j += n_thr) {
      const size_t npx = (size_t)views[j].width * views[j].height;
      std::memcpy(stage + (size_t)j * L.sz_mask, masks_host[j], npx);
      mptr[(size_t)j] = (const uint8_t*)(dmask + (size_t)j * L.sz_mask);
      const hipError_t e = hipMemcpyAsync(dmask + (size_t)j * L.sz_mask, stage + (size_t)j * L.sz_mask, npx, hipMemcpyHostToDevice, st);
      if (e != hipSuccess) terr[(size_t)t] = e;
    }
  };
  std::vector<std::thread> threads;
  for (int t = 1; t < n_thr; ++t) threads.emplace_back(worker, t);
  worker(0);
  for (std::thread& th : threads) th.join();
  Failure f;
  for (int t = 0; t < n_thr; ++t) f.hip(terr[(size_t)t], "mask upload");
  if (uploaded) f.hip(hipEventRecord(uploaded, st), "hipEventRecord");
  if (f.rc == VCY_OK && m > 0)
    f.rc = device_make_sdf_batch(st, m, mptr.data(), views, o.sdf_minmax_normalize != 0, o.update_option.use_truncation != 0,
                                 o.update_option.truncation_band, scratch, L.sz_scr, out);
  return f;
}

// Four timing events per chunk of a streamed batch (vcy_last_stream_ms): around its production on the producer stream
// and around its carve on the context's stream.
hipError_t reserve_stream_events(vcy_ctx* c, int n_chunks) {
  c->stream_timed_chunks = 0;
  hipError_t e = hipSuccess;
  while (e == hipSuccess && (int)c->stream_events.size() < 4 * n_chunks) {
    Event ev;
    e = ev.ensure();
    if (e == hipSuccess) c->stream_events.push_back(std::move(ev));
  }
  return e;
}

// The consume step: chunk `ci` (m views, their images complete once `ready` has happened) is carved on the context's
// stream, stamped on both sides, and `consumed` recorded behind it.
Failure consume_chunk(vcy_ctx* c, int ci, hipEvent_t ready, hipEvent_t consumed, int m, const vcy_view* views,
                      const float* const* images) {
  Failure f;
  f.hip(hipStreamWaitEvent(c->stream, ready, 0), "hipStreamWaitEvent");
  f.hip(hipEventRecord(c->stream_events[(size_t)4 * ci + 2], c->stream), "hipEventRecord");
  if (f.rc == VCY_OK) f.rc = launch_carve(c, m, views, images);
  f.hip(hipEventRecord(c->stream_events[(size_t)4 * ci + 3], c->stream), "hipEventRecord");
  f.hip(hipEventRecord(consumed, c->stream), "hipEventRecord");
  if (f.rc == VCY_OK) c->stream_timed_chunks = ci + 1;
  return f;
}

}  // namespace
}  // namespace vcy

using namespace vcy;

extern "C" {

// MakeSignedDistanceField for n silhouettes in host memory into CALLER-owned device images (sdf_device_out[i]: w * h
// floats on the context's device): page-locked staging -> DMA -> device transform, in groups of 32.  Returns when the
// images are complete.  What a rank of a multi-GPU job calls for ITS share of the views (views r, r + G, ...) before the
// images are exchanged (vacancy_amd.dist.carve_silhouettes_sharded): every GPU building every SDF would leave the
// streamed path producer-bound at 8 GPUs.
int vcy_make_sdf_batch_device(vcy_ctx* c, int n_views, const vcy_view* views, const uint8_t* const* masks_host,
                              float* const* sdf_device_out) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  if (n_views < 0 || (n_views > 0 && (!views || !masks_host || !sdf_device_out))) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  if (n_views == 0) return VCY_OK;
  size_t max_px = 0;
  for (int i = 0; i < n_views; ++i) {
    const int rc = check_view_static(&views[i]);
    if (rc != VCY_OK) return rc;
    if (!masks_host[i] || !sdf_device_out[i]) {
      set_error("null silhouette or output image");
      return VCY_ERR_INVALID_ARG;
    }
    max_px = std::max(max_px, (size_t)views[i].width * views[i].height);
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const int group = std::min(kChunk, n_views);
  const StreamLayout L(max_px);
  // staging of the streamed entry point, grown on demand (page-locking 64 MB per call would cost more than the work):
  // masks [group] | scratch [group]
  VCY_HIP_CHECK(c->d_stream_pool.grow((size_t)group * (L.sz_mask + L.sz_scr), c->stream));
  VCY_HIP_CHECK(c->h_pinned.grow((size_t)group * L.sz_mask, c->aux_stream, c->aux_stream != nullptr));
  char* d_tmp = (char*)c->d_stream_pool;
  hipStream_t st = c->stream;  // (the context's own stream: the caller's next call on it finds the images complete)
  Failure f;
  for (int first = 0; first < n_views && f.rc == VCY_OK; first += group) {
    if (first > 0 && !f.hip(hipStreamSynchronize(st), "hipStreamSynchronize")) break;  // staging and scratch are reused
    f = produce_images(st, c->device, std::min(group, n_views - first), views + first, masks_host + first, sdf_device_out + first,
                       (char*)c->h_pinned, d_tmp, d_tmp + (size_t)group * L.sz_mask, L, c->opt, 1, nullptr);
  }
  if (f.e != hipSuccess) set_error("vcy_make_sdf_batch_device: mask upload failed");
  if (hipStreamSynchronize(st) != hipSuccess && f.rc == VCY_OK) {
    set_error("vcy_make_sdf_batch_device: %s", hipGetErrorString(hipGetLastError()));
    f.rc = VCY_ERR_HIP;
  }
  return f.rc;
}

// Streams n silhouettes through the device: masks are uploaded and turned into SDFs on a second
// stream in chunks of 32 views while the previous chunk is being fused into the grid on the
// context's stream (two sets of SDF buffers, ordered with events; BASELINE config 5).
int vcy_carve_batch_silhouettes(vcy_ctx* c, int n_views, const vcy_view* views,
                                const uint8_t* const* masks_host) {
  if (!c) {
    set_error("VoxelCarver::Carve voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (n_views <= 0 || !views || !masks_host) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  size_t max_px = 0;
  for (int i = 0; i < n_views; ++i) {
    int rc = check_carve_views(c, 1, &views[i]);
    if (rc != VCY_OK) return rc;
    if (!masks_host[i]) {
      set_error("null silhouette");
      return VCY_ERR_INVALID_ARG;
    }
    max_px = std::max(max_px, (size_t)views[i].width * views[i].height);
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const int per_set = std::min(kChunk, n_views), n_chunks = (n_views + kChunk - 1) / kChunk;
  const StreamLayout L(max_px);
  // [2 sets][per_set] SDF images + [2 sets][per_set] masks + [per_set] transform scratch; cached in
  // the context and grown on demand
  VCY_HIP_CHECK(c->d_stream_pool.grow(2 * per_set * (L.sz_sdf + L.sz_mask) + per_set * L.sz_scr + 256, c->stream));
  // page-locked staging, two sets
  VCY_HIP_CHECK(c->h_pinned.grow(2 * (size_t)per_set * L.sz_mask, c->aux_stream, c->aux_stream != nullptr));
  Failure f;  // of the call: a runtime failure is worded where the call returns
  auto done = [&]() {
    if (f.e != hipSuccess) set_error("%s failed: %s", f.what, hipGetErrorString(f.e));
    return f.rc;
  };
  if (!c->aux_stream) {
    f.hip(c->aux_stream.create(hipStreamNonBlocking), "hipStreamCreate");
    for (int k = 0; k < 2; ++k) {
      f.hip(c->ev_ready[k].ensure(hipEventDisableTiming), "hipEventCreate");
      f.hip(c->ev_consumed[k].ensure(hipEventDisableTiming), "hipEventCreate");
      f.hip(c->ev_uploaded[k].ensure(hipEventDisableTiming), "hipEventCreate");
    }
  }
  hipStream_t aux = c->aux_stream;
  const auto t_entry = std::chrono::steady_clock::now();
  if (f.rc != VCY_OK || !f.hip(reserve_stream_events(c, n_chunks), "hipEventCreate")) return done();
  char* pool = (char*)c->d_stream_pool;
  char* masks = pool + 2 * per_set * L.sz_sdf;
  char* scratch = pool + 2 * per_set * (L.sz_sdf + L.sz_mask);
  const int n_thr = std::min(kStageThreads, (int)std::thread::hardware_concurrency());
  std::vector<float*> images[2];  // of the two sets
  for (int set = 0; set < 2; ++set)
    for (int j = 0; j < per_set; ++j) images[set].push_back((float*)(pool + ((size_t)set * per_set + j) * L.sz_sdf));
  // producer for chunk ci: upload + SDF on the aux stream
  auto produce = [&](int ci) {
    const int set = ci & 1, first = ci * kChunk, m = std::min(kChunk, n_views - first);
    if (ci >= 2) {
      f.hip(hipStreamWaitEvent(aux, c->ev_consumed[set], 0), "hipStreamWaitEvent");  // device buffers free
      f.hip(hipEventSynchronize(c->ev_uploaded[set]), "hipEventSynchronize");        // staging free
    }
    f.hip(hipEventRecord(c->stream_events[(size_t)4 * ci + 0], aux), "hipEventRecord");
    if (f.rc == VCY_OK)
      f = produce_images(aux, c->device, m, views + first, masks_host + first, images[set].data(),
                         (char*)c->h_pinned + (size_t)set * per_set * L.sz_mask, masks + (size_t)set * per_set * L.sz_mask, scratch, L,
                         c->opt, n_thr, c->ev_uploaded[set]);
    f.hip(hipEventRecord(c->stream_events[(size_t)4 * ci + 1], aux), "hipEventRecord");
    f.hip(hipEventRecord(c->ev_ready[set], aux), "hipEventRecord");
  };
  produce(0);
  for (int ci = 0; ci < n_chunks && f.rc == VCY_OK; ++ci) {
    const int set = ci & 1, first = ci * kChunk, m = std::min(kChunk, n_views - first);
    if (ci + 1 < n_chunks) produce(ci + 1);  // next chunk's SDFs build while this chunk carves
    if (f.rc == VCY_OK) f = consume_chunk(c, ci, c->ev_ready[set], c->ev_consumed[set], m, views + first, images[set].data());
  }
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(aux);
  c->stream_wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
  return done();
}

int vcy_last_stream_ms(vcy_ctx* c, float* produce_ms, float* carve_ms, float* wall_ms) {
  if (!c || !produce_ms || !carve_ms || !wall_ms) return VCY_ERR_INVALID_ARG;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  *produce_ms = *carve_ms = 0.0f;
  for (int ci = 0; ci < c->stream_timed_chunks; ++ci) {
    float a = 0.0f, b = 0.0f;
    VCY_HIP_CHECK(hipEventElapsedTime(&a, c->stream_events[(size_t)4 * ci + 0], c->stream_events[(size_t)4 * ci + 1]));
    VCY_HIP_CHECK(hipEventElapsedTime(&b, c->stream_events[(size_t)4 * ci + 2], c->stream_events[(size_t)4 * ci + 3]));
    *produce_ms += a;
    *carve_ms += b;
  }
  *wall_ms = c->stream_wall_ms;
  return VCY_OK;
}

}  // extern "C"

/* ---- sharded silhouette producer ---------------------------------------------------------------------------------
 * Carve(vector<Camera>, vector<Image1b>) (reference voxel_carver.cc:516-528 around :394-413) over the z-slabs of ONE
 * grid held by this process.  Round 4 handed every slab context the whole list (vcy_carve_batch_silhouettes per slab):
 * each GPU uploaded every silhouette and built every SDF, and at 8 GPUs the producer (1.6 ms per 32 views at 1280 x 720)
 * was longer than a rank's carve (1.0 ms).  Here the devices SHARE the producer: device r of R uploads and transforms the
 * views r, r + R, ... of every chunk of 32, ONE ncclAllGather per chunk hands every device all the images (W * H * 4
 * bytes each), and every slab carves the chunk from its device's copy -- while the next chunk is produced and gathered
 * on the producer streams.  Slabs that share a device share its images (round 4 built them once per slab).
 * One host thread per producer rank, like ShardedVoxelCarver's thread per slab; results are bit-identical to the
 * per-slab form (same images, same fused launches).                                                                  */
namespace vcy {
namespace {

// What one producer rank keeps between calls.  The stream is declared first, so it goes last; the destructor's body
// waits for it, on its device, before the members go.
struct ProducerRank {
  int device = 0;
  Stream aux;
  DeviceBuf<char> pool;      // masks [2][per] | scratch [per] | send [per]
  DeviceBuf<char> recv[2];   // the gathered images of a chunk, two sets
  PinnedBuf<> pinned;
  Event ev_ready[2], ev_uploaded[2], ev_sent;
  std::vector<Event> ev_consumed[2];  // per slab of this rank

  ~ProducerRank() {
    if (!aux) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(aux);
  }
};
struct ProducerGroup {
  std::vector<int> devices;  // per rank (distinct unless the test hook splits a device)
  std::vector<ProducerRank> ranks;
  explicit ProducerGroup(const std::vector<int>& d) : devices(d), ranks(d.size()) {}
};
auto& g_producers = *new std::vector<std::unique_ptr<ProducerGroup>>;  // (never destroyed, like the communicator groups)

int get_producer(const std::vector<int>& devices, ProducerGroup** out) {
  if ((*out = find_in(g_producers, devices))) return VCY_OK;
  std::unique_ptr<ProducerGroup> g(new ProducerGroup(devices));
  for (size_t r = 0; r < devices.size(); ++r) {
    ProducerRank& pr = g->ranks[r];
    pr.device = devices[r];
    hipError_t e = hipSetDevice(pr.device);
    if (e == hipSuccess) e = pr.aux.create(hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
      e = pr.ev_ready[k].ensure(hipEventDisableTiming);
      if (e == hipSuccess) e = pr.ev_uploaded[k].ensure(hipEventDisableTiming);
    }
    if (e == hipSuccess) e = pr.ev_sent.ensure(hipEventDisableTiming);
    if (e != hipSuccess) {
      set_error("sharded producer: device %d: %s", pr.device, hipGetErrorString(e));
      return VCY_ERR_HIP;
    }
  }
  *out = g.get();
  g_producers.push_back(std::move(g));
  return VCY_OK;
}

// all threads of one call meet here (test hook path and error hand-over)
struct HostBarrier {
  std::mutex m;
  std::condition_variable cv;
  int n, waiting = 0, phase = 0;
  explicit HostBarrier(int n_) : n(n_) {}
  void wait() {
    std::unique_lock<std::mutex> lk(m);
    const int ph = phase;
    if (++waiting == n) {
      waiting = 0;
      ++phase;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return phase != ph; });
    }
  }
};

// One call of vcy_carve_batch_silhouettes_sharded: what its rank threads share.
struct ShardedCall {
  vcy_ctx* const* slabs;
  int n_slabs, n_views;
  const vcy_view* views;
  const uint8_t* const* masks_host;
  std::vector<int> rank_of;      // per slab
  int R;                         // producer ranks
  HaloGroup* comm = nullptr;     // their communicators (R > 1 on distinct devices), else the device-copy form of the gather
  ProducerGroup* pg = nullptr;
  int n_chunks, per;             // per: images a rank produces per chunk
  StreamLayout L;
  size_t send_bytes;             // what a rank contributes to the gather of a chunk
  HostBarrier barrier;

  std::atomic<int> failed{VCY_OK};  // the first failure of any rank, with its text
  std::atomic<bool> aborted{false};
  std::mutex mutex;                 // of the two
  std::string err_text;

  ShardedCall(vcy_ctx* const* slabs_, int n_slabs_, int n_views_, const vcy_view* views_, const uint8_t* const* masks_,
              std::vector<int> rank_of_, int R_, size_t max_px)
      : slabs(slabs_), n_slabs(n_slabs_), n_views(n_views_), views(views_), masks_host(masks_), rank_of(std::move(rank_of_)),
        R(R_), n_chunks((n_views_ + kChunk - 1) / kChunk), per((std::min(kChunk, n_views_) + R_ - 1) / R_), L(max_px),
        send_bytes((size_t)per * L.stride), barrier(R_) {}

  bool ok() const { return failed.load() == VCY_OK; }
  void fail(int code, const std::string& text) {
    std::lock_guard<std::mutex> lk(mutex);
    if (failed.load() == VCY_OK) {
      err_text = text;
      failed.store(code);
    }
  }
  bool hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) fail(VCY_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return e == hipSuccess;
  }
  void fail(const Failure& f) {  // a step's outcome into the call's
    if (hip_ok(f.e, f.what) && f.rc != VCY_OK) fail(f.rc, vcy_last_error());
  }
  // A collective that failed on one rank after others had enqueued it: ncclCommAbort on every communicator of the group
  // ends the stranded kernels; the group (and the producer with its streams) is dropped after the threads have joined
  // and rebuilt by the next call.
  void abort_group() {
    std::lock_guard<std::mutex> lk(mutex);
    if (aborted.load() || !comm) return;
    aborted.store(true);
    for (Comm& cm : comm->comms) cm.abort();  // (aborted communicators are gone: their holders are empty)
  }
};

// One producer rank of one call, on a host thread of its own: chunk ci + 1 is produced and gathered while the rank's
// slabs carve chunk ci.
struct RankWorker {
  ShardedCall& k;
  const int r;
  ProducerRank& pr;
  std::vector<vcy_ctx*> mine;  // the rank's slabs
  char *mask_base = nullptr, *scratch = nullptr, *send = nullptr;  // where the rank's pool is cut

  RankWorker(ShardedCall& call, int rank) : k(call), r(rank), pr(call.pg->ranks[(size_t)rank]) {
    for (int s = 0; s < k.n_slabs; ++s)
      if (k.rank_of[(size_t)s] == r) mine.push_back(k.slabs[s]);
  }

  // buffers and events of this rank, grown on demand
  void reserve() {
    const size_t pool_need = 2 * (size_t)k.per * k.L.sz_mask + (size_t)k.per * k.L.sz_scr + (k.R > 1 ? k.send_bytes : 0) + 256;
    const size_t recv_need = k.send_bytes * (size_t)k.R;
    if (k.ok()) k.hip_ok(pr.pool.grow(pool_need, pr.aux), "hipMalloc");
    if (k.ok() && std::min(pr.recv[0].bytes(), pr.recv[1].bytes()) < recv_need) {  // (either may be empty after a failed call)
      for (vcy_ctx* c : mine) (void)hipStreamSynchronize(c->stream);              // (the slabs carve from these)
      for (int s = 0; s < 2 && k.ok(); ++s) k.hip_ok(pr.recv[s].grow(recv_need, nullptr, false), "hipMalloc");
    }
    if (k.ok()) k.hip_ok(pr.pinned.grow(2 * (size_t)k.per * k.L.sz_mask, pr.aux), "hipHostMalloc");
    for (int s = 0; s < 2; ++s)
      while (k.ok() && pr.ev_consumed[s].size() < mine.size()) {
        Event ev;
        if (k.hip_ok(ev.ensure(hipEventDisableTiming), "hipEventCreate")) pr.ev_consumed[s].push_back(std::move(ev));
      }
    for (vcy_ctx* c : mine) {  // the timing record of vcy_last_stream_ms, per slab
      c->stream_timed_chunks = 0;
      if (k.ok()) k.hip_ok(reserve_stream_events(c, k.n_chunks), "hipEventCreate");
    }
    mask_base = pr.pool;
    scratch = pr.pool + 2 * (size_t)k.per * k.L.sz_mask;
    send = scratch + (size_t)k.per * k.L.sz_scr;
  }

  // The exchange of chunk set `set`: every rank's images into every rank's recv[set].
  void gather_chunk(int set) {
    if (k.comm) {  // the exchange: ONE all-gather per chunk, every device receives every rank's images
      // Whether this chunk is gathered is decided JOINTLY: a rank that skipped the collective (its producer, a HIP
      // call or its carve failed) while the others had enqueued theirs would leave them waiting for ever in their
      // closing hipStreamSynchronize, with g_rccl_mutex held.  Every rank has finished what can fail before the
      // first barrier; between the two barriers nobody writes `failed`, so every rank reads the same value.
      k.barrier.wait();
      const bool gather = k.ok();
      k.barrier.wait();
      if (gather) {
        const ncclResult_t nr = g_rccl.AllGather(send, pr.recv[set], k.send_bytes, ncclUint8, k.comm->comms[(size_t)r].get(), pr.aux);
        if (nr != ncclSuccess) {
          // (some ranks may already have enqueued theirs: only aborting the communicators gets them out)
          k.fail(VCY_ERR_HIP, std::string("ncclAllGather: ") + g_rccl.GetErrorString(nr));
          k.abort_group();
        }
      }
    } else {  // (test hook: several ranks on one device -- the same data movement as device copies)
      if (k.ok()) k.hip_ok(hipEventRecord(pr.ev_sent, pr.aux), "hipEventRecord");
      k.barrier.wait();
      for (int q = 0; q < k.R && k.ok(); ++q) {
        k.hip_ok(hipStreamWaitEvent(pr.aux, k.pg->ranks[(size_t)q].ev_sent, 0), "hipStreamWaitEvent");
        const char* src = k.pg->ranks[(size_t)q].pool + 2 * (size_t)k.per * k.L.sz_mask + (size_t)k.per * k.L.sz_scr;
        k.hip_ok(hipMemcpyAsync(pr.recv[set] + (size_t)q * k.send_bytes, src, k.send_bytes, hipMemcpyDeviceToDevice, pr.aux), "gather copy");
      }
      (void)hipStreamSynchronize(pr.aux);
      k.barrier.wait();  // nobody overwrites its send buffer before every rank has copied it
    }
  }

  // Chunk ci on the producer stream: this rank's share of it built, every rank's share gathered, `ev_ready` behind both.
  // Runs for every chunk, also after the call has failed: the other ranks wait at the barriers of the gather.
  void produce_chunk(int ci) {
    const int set = ci & 1, first = ci * kChunk, m = std::min(kChunk, k.n_views - first);
    const bool live = k.ok();
    if (live && ci >= 2) {
      for (size_t s = 0; s < mine.size(); ++s) k.hip_ok(hipStreamWaitEvent(pr.aux, pr.ev_consumed[set][s], 0), "hipStreamWaitEvent");
      k.hip_ok(hipEventSynchronize(pr.ev_uploaded[set]), "hipEventSynchronize");
    }
    if (live) {
      for (vcy_ctx* c : mine) k.hip_ok(hipEventRecord(c->stream_events[(size_t)4 * ci + 0], pr.aux), "hipEventRecord");
      std::vector<const uint8_t*> mhost;
      std::vector<float*> optr;
      std::vector<vcy_view> myviews;
      char* dst = k.R > 1 ? send : pr.recv[set];  // (a single rank builds in place in the set its slabs carve from)
      for (int j = r, i = 0; j < m; j += k.R, ++i) {  // this rank's share of the chunk: views r, r + R, ...
        mhost.push_back(k.masks_host[first + j]);
        optr.push_back((float*)(dst + (size_t)i * k.L.stride));
        myviews.push_back(k.views[first + j]);
      }
      const size_t set_off = (size_t)set * k.per * k.L.sz_mask;
      k.fail(produce_images(pr.aux, pr.device, (int)mhost.size(), myviews.data(), mhost.data(), optr.data(), (char*)pr.pinned + set_off,
                            mask_base + set_off, scratch, k.L, k.slabs[0]->opt, 1, pr.ev_uploaded[set]));
    }
    if (k.R > 1) gather_chunk(set);
    if (k.ok()) {
      for (vcy_ctx* c : mine) k.hip_ok(hipEventRecord(c->stream_events[(size_t)4 * ci + 1], pr.aux), "hipEventRecord");
      k.hip_ok(hipEventRecord(pr.ev_ready[set], pr.aux), "hipEventRecord");
    }
  }

  void run() {
    k.hip_ok(hipSetDevice(pr.device), "hipSetDevice");
    reserve();
    k.barrier.wait();  // every rank has its buffers (or the call has failed) before anything is enqueued
    produce_chunk(0);
    for (int ci = 0; ci < k.n_chunks; ++ci) {
      const int set = ci & 1, first = ci * kChunk, m = std::min(kChunk, k.n_views - first);
      if (ci + 1 < k.n_chunks) produce_chunk(ci + 1);  // the next chunk is produced and gathered while this one is carved
      if (!k.ok()) continue;                           // (keep meeting the others at the barriers of produce_chunk)
      std::vector<const float*> ptrs((size_t)m);  // the slot of view j in the gathered set: rank j % R, its image j / R
      for (int j = 0; j < m; ++j) ptrs[(size_t)j] = (const float*)(pr.recv[set] + ((size_t)(j % k.R) * k.per + (size_t)(j / k.R)) * k.L.stride);
      for (size_t s = 0; s < mine.size() && k.ok(); ++s)
        k.fail(consume_chunk(mine[s], ci, pr.ev_ready[set], pr.ev_consumed[set][s], m, k.views + first, ptrs.data()));
    }
    for (vcy_ctx* c : mine) (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(pr.aux);
  }
};

int check_sharded_arguments(vcy_ctx* const* slabs, int n_slabs, int n_views, const vcy_view* views,
                            const uint8_t* const* masks_host, size_t* max_px) {
  if (!slabs || n_slabs <= 0 || n_views <= 0 || !views || !masks_host) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  *max_px = 0;
  for (int i = 0; i < n_views; ++i) {
    if (!masks_host[i]) {
      set_error("null silhouette");
      return VCY_ERR_INVALID_ARG;
    }
    *max_px = std::max(*max_px, (size_t)views[i].width * views[i].height);
  }
  for (int s = 0; s < n_slabs; ++s) {
    if (!slabs[s]) {
      set_error("VoxelCarver::Carve voxel grid has not been initialized");
      return VCY_ERR_NOT_INITIALIZED;
    }
    const int rc = check_carve_views(slabs[s], n_views, views);
    if (rc != VCY_OK) return rc;
    const vcy_carver_option &a = slabs[0]->opt, &b = slabs[s]->opt;
    if (a.sdf_minmax_normalize != b.sdf_minmax_normalize || a.update_option.use_truncation != b.update_option.use_truncation ||
        a.update_option.truncation_band != b.update_option.truncation_band) {
      set_error("vcy_carve_batch_silhouettes_sharded: the slabs do not share one option set");
      return VCY_ERR_INVALID_ARG;
    }
  }
  return VCY_OK;
}

}  // namespace

void drop_producers() { g_producers.clear(); }

}  // namespace vcy

extern "C" int vcy_carve_batch_silhouettes_sharded(vcy_ctx* const* slabs, int n_slabs, int n_views, const vcy_view* views,
                                                   const uint8_t* const* masks_host) {
  size_t max_px = 0;
  int rc = check_sharded_arguments(slabs, n_slabs, n_views, views, masks_host, &max_px);
  if (rc != VCY_OK) return rc;
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  // producer ranks: one per distinct device, in order of first appearance.  Test hook VCY_TEST_SPLIT_PRODUCERS=1: one
  // rank per SLAB even on a shared device, the all-gather then being device copies -- the share / slot / gather
  // layout of an R-device run, exercised on one GPU.
  const char* split_env = std::getenv("VCY_TEST_SPLIT_PRODUCERS");
  const bool split = split_env && split_env[0] == '1';
  std::vector<int> devices, rank_of((size_t)n_slabs);
  for (int s = 0; s < n_slabs; ++s) {
    size_t r = 0;
    if (split) r = devices.size();
    else while (r < devices.size() && devices[r] != slabs[s]->device) ++r;
    if (r == devices.size()) devices.push_back(slabs[s]->device);
    rank_of[(size_t)s] = (int)r;
  }
  const int R = (int)devices.size();
  bool distinct = true;
  for (int a = 0; a < R; ++a)
    for (int b = a + 1; b < R; ++b) distinct = distinct && devices[(size_t)a] != devices[(size_t)b];
  ShardedCall call(slabs, n_slabs, n_views, views, masks_host, std::move(rank_of), R, max_px);
  if (R > 1 && distinct) {
    if (!load_rccl()) return VCY_ERR_UNSUPPORTED;
    rc = get_group(devices, &call.comm);
    if (rc != VCY_OK) return rc;
  }
  rc = get_producer(devices, &call.pg);
  if (rc != VCY_OK) return rc;

  const auto t_entry = std::chrono::steady_clock::now();
  std::vector<std::thread> threads;
  for (int r = 1; r < R; ++r) threads.emplace_back([&call, r] { RankWorker(call, r).run(); });
  RankWorker(call, 0).run();
  for (std::thread& t : threads) t.join();
  const float wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
  for (int s = 0; s < n_slabs; ++s) slabs[s]->stream_wall_ms = wall;
  if (call.aborted.load()) {
    drop_group(call.comm);
    drop_from(g_producers, call.pg);
  }
  (void)hipSetDevice(slabs[0]->device);
  if (!call.ok()) {
    set_error("%s", call.err_text.c_str());
    return call.failed.load();
  }
  return VCY_OK;
}
