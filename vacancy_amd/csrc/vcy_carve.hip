// The carve entry points of the C ABI: the checks of their views, the queue of views that wait for one fused launch,
// the silhouette paths (one view, a batch into caller-owned images, the streamed batch), the slab planner's wrappers
// and the two host SDF functions.  The kernels and their launches: carve_kernels.hip, carve_fused.hip, sdf2d.hip.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

#include "vcy_internal.h"

using namespace vcy;

extern "C" {

/* ---- carving entry points ------------------------------------------------ */

static int check_view_static(const vcy_view* v) {
  if (!v || v->width <= 0 || v->height <= 0) {
    set_error("invalid view");
    return VCY_ERR_INVALID_ARG;
  }
  // The reference indexes sdf.at() unchecked (assert only); a ROI outside the image is
  // undefined there and rejected here.
  if (v->roi_min[0] < 0 || v->roi_min[1] < 0 || v->roi_max[0] >= v->width ||
      v->roi_max[1] >= v->height || v->roi_min[0] > v->roi_max[0] || v->roi_min[1] > v->roi_max[1]) {
    set_error("ROI [%d,%d]-[%d,%d] outside the %dx%d SDF image", v->roi_min[0], v->roi_min[1],
              v->roi_max[0], v->roi_max[1], v->width, v->height);
    return VCY_ERR_INVALID_ARG;
  }
  return VCY_OK;
}

static int check_view(const vcy_ctx* c, const vcy_view* v) {
  if (!c) {
    set_error("VoxelCarver::Carve voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (c->deferred_rc != VCY_OK) {  // views queued by earlier calls failed to apply (see vcy_ctx::deferred_rc)
    vcy_ctx* m = const_cast<vcy_ctx*>(c);
    const int rc = m->deferred_rc;
    set_error("an earlier queued view failed: %s", m->deferred_msg.c_str());
    m->deferred_rc = VCY_OK;
    m->deferred_msg.clear();
    return rc;
  }
  return check_view_static(v);
}

}  // extern "C"
namespace vcy {
int check_carve_views(vcy_ctx* c, int n_views, const vcy_view* views) {
  for (int i = 0; i < n_views; ++i) {
    const int rc = check_view(c, &views[i]);
    if (rc != VCY_OK) return rc;
  }
  return VCY_OK;
}
}  // namespace vcy
extern "C" {

int vcy_carve_batch_device(vcy_ctx* c, int n_views, const vcy_view* views,
                           const float* const* sdf_device) {
  if (n_views <= 0 || !views || !sdf_device) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_views; ++i) {
    int rc = check_view(c, &views[i]);
    if (rc != VCY_OK) return rc;
    if (!sdf_device[i]) {
      set_error("null SDF pointer");
      return VCY_ERR_INVALID_ARG;
    }
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  return launch_carve(c, n_views, views, sdf_device);
}

// An idle image buffer of at least `bytes` (from the pool, else newly allocated).
static int acquire_sdf_buffer(vcy_ctx* c, size_t bytes, DeviceBuf<float>* out) {
  for (size_t i = 0; i < c->sdf_pool.size(); ++i) {
    if (c->sdf_pool[i].bytes() >= bytes) {
      *out = std::move(c->sdf_pool[i]);
      c->sdf_pool.erase(c->sdf_pool.begin() + (long)i);
      return VCY_OK;
    }
  }
  VCY_HIP_CHECK(out->alloc(bytes));
  return VCY_OK;
}

// Whether a view accepted by a per-view entry point may wait for a fused launch.
static bool can_defer(vcy_ctx* c, const vcy_view* view) {
  if (!c->defer || !c->use_fused || !fused_eligible(c, 1, view)) return false;
  return true;
}

#ifndef VCY_STAGE_THREADS
#define VCY_STAGE_THREADS 4   // (8 and 16 measured: the producer side of 32 silhouettes at 1280 x 720 stays at 1.45 - 1.5 ms)
#endif
constexpr int kStageThreads = VCY_STAGE_THREADS;  // host threads that copy silhouettes into page-locked staging and queue their DMAs
constexpr int kMaxPendingViews = 32;  // queued images held at most (3.7 MB each at 1280x720)

// Queues (view, private device image): flushes first if the queue is full or of the other projection
// model (one model per fused launch).
static int enqueue_view(vcy_ctx* c, const vcy_view* view, DeviceBuf<float> d_img) {
  int rc = VCY_OK;
  if (!c->pending.empty() && (c->pending.front().view.is_ortho != 0) != (view->is_ortho != 0)) rc = flush_pending(c, true);
  if (rc == VCY_OK) {
    c->pending.push_back(vcy_ctx::PendingView{*view, std::move(d_img)});
    c->halo_valid = false;
    if ((int)c->pending.size() >= kMaxPendingViews) rc = flush_pending(c, true);
  } else {
    c->sdf_pool.push_back(std::move(d_img));
  }
  return rc;
}

int vcy_carve_device(vcy_ctx* c, const vcy_view* view, const float* sdf_device) {
  int rc = check_view(c, view);
  if (rc != VCY_OK) return rc;
  if (!sdf_device) {
    set_error("null SDF pointer");
    return VCY_ERR_INVALID_ARG;
  }
  if (!can_defer(c, view)) return vcy_carve_batch_device(c, 1, view, &sdf_device);
  // the caller may change or free its image after this returns: keep a copy (stream-ordered)
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const size_t bytes = sizeof(float) * (size_t)view->width * view->height;
  DeviceBuf<float> d;
  rc = acquire_sdf_buffer(c, bytes, &d);
  if (rc != VCY_OK) return rc;
  const hipError_t e = hipMemcpyAsync(d, sdf_device, bytes, hipMemcpyDeviceToDevice, c->stream);
  if (e != hipSuccess) {
    c->sdf_pool.push_back(std::move(d));
    set_error("SDF copy failed: %s", hipGetErrorString(e));
    return VCY_ERR_HIP;
  }
  return enqueue_view(c, view, std::move(d));
}

int vcy_carve(vcy_ctx* c, const vcy_view* view, const float* sdf_host) {
  int rc = check_view(c, view);
  if (rc != VCY_OK) return rc;
  if (!sdf_host) {
    set_error("null SDF pointer");
    return VCY_ERR_INVALID_ARG;
  }
  if (!can_defer(c, view)) {
    float* d = nullptr;
    rc = vcy_sdf_upload(c, sdf_host, view->width, view->height, &d);
    if (rc != VCY_OK) return rc;
    rc = vcy_carve_batch_device(c, 1, view, (const float* const*)&d);
    int rc2 = vcy_device_free(c, d);  // synchronises the stream first
    return rc != VCY_OK ? rc : rc2;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const size_t bytes = sizeof(float) * (size_t)view->width * view->height;
  DeviceBuf<float> d;
  rc = acquire_sdf_buffer(c, bytes, &d);
  if (rc != VCY_OK) return rc;
  // the previous user of a pooled buffer may be a launch still running: order the copy after it
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(d, sdf_host, bytes, hipMemcpyHostToDevice);  // caller's buffer is free on return
  if (e != hipSuccess) {
    c->sdf_pool.push_back(std::move(d));
    set_error("hipMemcpy H2D failed: %s", hipGetErrorString(e));
    return VCY_ERR_HIP;
  }
  return enqueue_view(c, view, std::move(d));
}

int vcy_carve_silhouette(vcy_ctx* c, const vcy_view* view, const uint8_t* mask, float* sdf_out) {
  int rc = check_view(c, view);
  if (rc != VCY_OK) return rc;
  if (!mask) {
    set_error("null silhouette");
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const vcy_update_option& u = c->opt.update_option;
  const size_t npx = (size_t)view->width * view->height;
  // device staging kept in the context: [mask u8][transform scratch]; the SDF goes to a pooled image
  const size_t off_scr = (npx + 255) / 256 * 256;
  const size_t need = off_scr + device_make_sdf_scratch_bytes(view->width, view->height);
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));  // the staging may still feed the previous call's kernels
  VCY_HIP_CHECK(c->d_sil_scratch.grow(need, c->stream, false));
  char* d = (char*)c->d_sil_scratch;
  DeviceBuf<float> d_img;
  rc = acquire_sdf_buffer(c, npx * sizeof(float), &d_img);
  if (rc != VCY_OK) return rc;
  auto give_back = [&](int code) {
    (void)hipStreamSynchronize(c->stream);
    c->sdf_pool.push_back(std::move(d_img));
    return code;
  };
  if (hipMemcpy(d, mask, npx, hipMemcpyHostToDevice) != hipSuccess) {  // caller's mask is free on return
    set_error("mask upload failed");
    return give_back(VCY_ERR_HIP);
  }
  // MakeSignedDistanceField(silhouette, roi_min, roi_max, sdf, option_.sdf_minmax_normalize,
  //   use_truncation, truncation_band), reference voxel_carver.cc:405-408 -- on the device
  rc = device_make_sdf(c->stream, (const uint8_t*)d, view->width, view->height, view->roi_min, view->roi_max,
                       c->opt.sdf_minmax_normalize != 0, u.use_truncation != 0, u.truncation_band, d + off_scr, d_img);
  if (rc != VCY_OK) return give_back(rc);
  if (sdf_out) {
    hipError_t e = hipMemcpyAsync(sdf_out, d_img, npx * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      set_error("sdf download failed: %s", hipGetErrorString(e));
      return give_back(VCY_ERR_HIP);
    }
  }
  if (can_defer(c, view)) return enqueue_view(c, view, std::move(d_img));
  const float* img = d_img;
  rc = vcy_carve_batch_device(c, 1, view, &img);
  return give_back(rc);
}

int vcy_make_sdf_device(vcy_ctx* c, const uint8_t* mask_host, int w, int h, const int32_t rmin[2],
                        const int32_t rmax[2], int normalize, int truncate, float band, float** sdf_device_out) {
  if (!c || !mask_host || !sdf_device_out || w <= 0 || h <= 0 || rmin[0] < 0 || rmin[1] < 0 || rmax[0] >= w ||
      rmax[1] >= h || rmin[0] > rmax[0] || rmin[1] > rmax[1]) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const size_t npx = (size_t)w * h;
  DeviceBuf<char> tmp;
  float* sdf = nullptr;  // the caller's once returned (vcy_device_free)
  const size_t off_scr = (npx + 255) / 256 * 256;
  VCY_HIP_CHECK(hipMalloc(&sdf, npx * sizeof(float)));
  if (tmp.alloc(off_scr + device_make_sdf_scratch_bytes(w, h)) != hipSuccess) {
    (void)hipFree(sdf);
    set_error("out of device memory");
    return VCY_ERR_HIP;
  }
  int rc = VCY_OK;
  if (hipMemcpyAsync(tmp, mask_host, npx, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = VCY_ERR_HIP;
  if (rc == VCY_OK)
    rc = device_make_sdf(c->stream, (const uint8_t*)tmp, w, h, rmin, rmax, normalize != 0, truncate != 0, band,
                         tmp + off_scr, sdf);
  (void)hipStreamSynchronize(c->stream);
  if (rc != VCY_OK) {
    (void)hipFree(sdf);
    return rc;
  }
  *sdf_device_out = sdf;
  return VCY_OK;
}

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
  const vcy_update_option& u = c->opt.update_option;
  const int group = std::min(32, n_views);
  const size_t sz_mask = (max_px + 255) / 256 * 256;
  const size_t sz_scr = (device_make_sdf_scratch_bytes(1, (int)max_px) + 255) / 256 * 256;
  // staging of the streamed entry point, grown on demand (page-locking 64 MB per call would cost more than the work)
  const size_t need_dev = (size_t)group * (sz_mask + sz_scr), need_pin = (size_t)group * sz_mask;
  VCY_HIP_CHECK(c->d_stream_pool.grow(need_dev, c->stream));
  VCY_HIP_CHECK(c->h_pinned.grow(need_pin, c->aux_stream, c->aux_stream != nullptr));
  char* d_tmp = (char*)c->d_stream_pool;
  void* h_stage = c->h_pinned;
  int rc = VCY_OK;
  hipStream_t st = c->stream;
  for (int first = 0; first < n_views && rc == VCY_OK; first += group) {
    const int m = std::min(group, n_views - first);
    std::vector<const uint8_t*> mptr((size_t)m);
    std::vector<float*> optr((size_t)m);
    if (first > 0 && hipStreamSynchronize(st) != hipSuccess) rc = VCY_ERR_HIP;  // staging and scratch are reused
    for (int j = 0; j < m && rc == VCY_OK; ++j) {
      const size_t npx = (size_t)views[first + j].width * views[first + j].height;
      std::memcpy((char*)h_stage + (size_t)j * sz_mask, masks_host[first + j], npx);
      if (hipMemcpyAsync(d_tmp + (size_t)j * sz_mask, (char*)h_stage + (size_t)j * sz_mask, npx, hipMemcpyHostToDevice, st) != hipSuccess)
        rc = VCY_ERR_HIP;
      mptr[(size_t)j] = (const uint8_t*)(d_tmp + (size_t)j * sz_mask);
      optr[(size_t)j] = sdf_device_out[first + j];
    }
    if (rc == VCY_OK)
      rc = device_make_sdf_batch(st, m, mptr.data(), views + first, c->opt.sdf_minmax_normalize != 0, u.use_truncation != 0,
                                 u.truncation_band, d_tmp + (size_t)group * sz_mask, sz_scr, optr.data());
    else
      set_error("vcy_make_sdf_batch_device: mask upload failed");
  }
  if (hipStreamSynchronize(st) != hipSuccess && rc == VCY_OK) {
    set_error("vcy_make_sdf_batch_device: %s", hipGetErrorString(hipGetLastError()));
    rc = VCY_ERR_HIP;
  }
  return rc;
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
    int rc = check_view(c, &views[i]);
    if (rc != VCY_OK) return rc;
    if (!masks_host[i]) {
      set_error("null silhouette");
      return VCY_ERR_INVALID_ARG;
    }
    max_px = std::max(max_px, (size_t)views[i].width * views[i].height);
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const vcy_update_option& u = c->opt.update_option;
  const int chunk = 32;  // per fused launch here: the next 32 silhouettes upload and transform meanwhile
  const int per_set = std::min(chunk, n_views);
  const size_t px_al = (max_px + 255) / 256 * 256;
  // [2 sets][per_set] SDF images + [2 sets][per_set] masks + [per_set] transform scratch; cached in
  // the context and grown on demand
  const size_t sz_sdf = px_al * sizeof(float), sz_mask = px_al;
  const size_t sz_scr = (device_make_sdf_scratch_bytes(1, (int)max_px) + 255) / 256 * 256;
  const size_t total = 2 * per_set * (sz_sdf + sz_mask) + per_set * sz_scr + 256;
  int rc = VCY_OK;
  auto fail_hip = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && rc == VCY_OK) {
      set_error("%s failed: %s", what, hipGetErrorString(e));
      rc = VCY_ERR_HIP;
    }
    return e != hipSuccess;
  };
  VCY_HIP_CHECK(c->d_stream_pool.grow(total, c->stream));
  // page-locked staging: pageable memory would be copied through the runtime's own bounce buffer by
  // one thread; here a few host threads fill it and the DMA engine takes it from there
  const size_t pinned_total = 2 * (size_t)per_set * sz_mask;
  VCY_HIP_CHECK(c->h_pinned.grow(pinned_total, c->aux_stream, c->aux_stream != nullptr));
  if (!c->aux_stream) {
    fail_hip(c->aux_stream.create(hipStreamNonBlocking), "hipStreamCreate");
    for (int k = 0; k < 2 && rc == VCY_OK; ++k) {
      fail_hip(c->ev_ready[k].ensure(hipEventDisableTiming), "hipEventCreate");
      fail_hip(c->ev_consumed[k].ensure(hipEventDisableTiming), "hipEventCreate");
      fail_hip(c->ev_uploaded[k].ensure(hipEventDisableTiming), "hipEventCreate");
    }
    if (rc != VCY_OK) return rc;
  }
  hipStream_t aux = c->aux_stream;
  // timing of the two sides (vcy_last_stream_ms): per chunk, events around its production (staging copy, H2D, SDF
  // build; on the producer stream) and around its carve (on the context's stream)
  const auto t_entry = std::chrono::steady_clock::now();
  const int n_chunks_t = (n_views + chunk - 1) / chunk;
  while ((int)c->stream_events.size() < 4 * n_chunks_t) {
    Event ev;
    if (fail_hip(ev.ensure(), "hipEventCreate")) return rc;
    c->stream_events.push_back(std::move(ev));
  }
  c->stream_timed_chunks = 0;
  char* pool = (char*)c->d_stream_pool;
  char* scratch = pool + 2 * per_set * (sz_sdf + sz_mask);
  auto sdf_buf = [&](int set, int j) { return (float*)(pool + ((size_t)set * per_set + j) * sz_sdf); };
  auto mask_buf = [&](int set, int j) {
    return (uint8_t*)(pool + 2 * per_set * sz_sdf + ((size_t)set * per_set + j) * sz_mask);
  };
  auto stage_buf = [&](int set, int j) { return (uint8_t*)c->h_pinned + ((size_t)set * per_set + j) * sz_mask; };
  const int n_chunks = (n_views + chunk - 1) / chunk;
  // producer for chunk ci: upload + SDF on the aux stream
  auto produce = [&](int ci) {
    const int set = ci & 1, first = ci * chunk, m = std::min(chunk, n_views - first);
    if (ci >= 2) {
      fail_hip(hipStreamWaitEvent(aux, c->ev_consumed[set], 0), "hipStreamWaitEvent");  // device buffers free
      fail_hip(hipEventSynchronize(c->ev_uploaded[set]), "hipEventSynchronize");        // staging free
    }
    std::vector<const uint8_t*> mptr(m);
    std::vector<float*> optr(m);
    for (int j = 0; j < m; ++j) {
      mptr[j] = mask_buf(set, j);
      optr[j] = sdf_buf(set, j);
    }
    fail_hip(hipEventRecord(c->stream_events[(size_t)4 * ci + 0], aux), "hipEventRecord");
    // host threads: copy silhouette j into the staging buffer, then queue its DMA
    const int n_thr = std::max(1, std::min(m, std::min(kStageThreads, (int)std::thread::hardware_concurrency())));
    std::vector<hipError_t> terr((size_t)n_thr, hipSuccess);
    auto worker = [&](int t) {
      (void)hipSetDevice(c->device);
      for (int j = t; j < m; j += n_thr) {
        const vcy_view& v = views[first + j];
        const size_t npx = (size_t)v.width * v.height;
        std::memcpy(stage_buf(set, j), masks_host[first + j], npx);
        const hipError_t e = hipMemcpyAsync(mask_buf(set, j), stage_buf(set, j), npx, hipMemcpyHostToDevice, aux);
        if (e != hipSuccess) terr[(size_t)t] = e;
      }
    };
    if (rc == VCY_OK) {
      std::vector<std::thread> pool_thr;
      for (int t = 1; t < n_thr; ++t) pool_thr.emplace_back(worker, t);
      worker(0);
      for (auto& th : pool_thr) th.join();
      for (int t = 0; t < n_thr; ++t) fail_hip(terr[(size_t)t], "mask upload");
    }
    fail_hip(hipEventRecord(c->ev_uploaded[set], aux), "hipEventRecord");
    if (rc == VCY_OK) {
      // MakeSignedDistanceField(...) for the whole chunk at once, reference voxel_carver.cc:405-408
      int r2 = device_make_sdf_batch(aux, m, mptr.data(), views + first, c->opt.sdf_minmax_normalize != 0,
                                     u.use_truncation != 0, u.truncation_band, scratch, sz_scr, optr.data());
      if (r2 != VCY_OK) rc = r2;
    }
    fail_hip(hipEventRecord(c->stream_events[(size_t)4 * ci + 1], aux), "hipEventRecord");
    fail_hip(hipEventRecord(c->ev_ready[set], aux), "hipEventRecord");
  };
  if (rc == VCY_OK) produce(0);
  for (int ci = 0; ci < n_chunks && rc == VCY_OK; ++ci) {
    const int set = ci & 1, first = ci * chunk, m = std::min(chunk, n_views - first);
    if (ci + 1 < n_chunks) produce(ci + 1);  // next chunk's SDFs build while this chunk carves
    if (rc != VCY_OK) break;
    fail_hip(hipStreamWaitEvent(c->stream, c->ev_ready[set], 0), "hipStreamWaitEvent");
    std::vector<const float*> ptrs(m);
    for (int j = 0; j < m; ++j) ptrs[j] = sdf_buf(set, j);
    fail_hip(hipEventRecord(c->stream_events[(size_t)4 * ci + 2], c->stream), "hipEventRecord");
    int r2 = launch_carve(c, m, views + first, ptrs.data());
    if (r2 != VCY_OK) rc = r2;
    fail_hip(hipEventRecord(c->stream_events[(size_t)4 * ci + 3], c->stream), "hipEventRecord");
    fail_hip(hipEventRecord(c->ev_consumed[set], c->stream), "hipEventRecord");
    if (rc == VCY_OK) c->stream_timed_chunks = ci + 1;
  }
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(aux);
  c->stream_wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
  return rc;
}

int vcy_partition_layers(const double* layer_cost, int n_layers, int n_slabs, int nz, int32_t* z_bounds) {
  if (!layer_cost || !z_bounds || n_layers < 1 || n_slabs < 1 || n_slabs > n_layers || nz <= (n_layers - 1) * 8 ||
      nz > n_layers * 8) {
    set_error("vcy_partition_layers: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  if (n_slabs > 1 && n_layers > 1 && nz - (n_layers - 1) * 8 == 1 && n_slabs > n_layers - 1) {
    set_error("vcy_partition_layers: the last layer is a single slice and cannot be a slab of its own");
    return VCY_ERR_INVALID_ARG;
  }
  for (int l = 0; l < n_layers; ++l)
    if (!(layer_cost[l] >= 0.0) || !(layer_cost[l] < 1e280)) {
      set_error("vcy_partition_layers: layer costs must be finite and non-negative");
      return VCY_ERR_INVALID_ARG;
    }
  partition_layers(layer_cost, n_layers, n_slabs, nz, z_bounds);
  return VCY_OK;
}

int vcy_plan_z_slabs(vcy_ctx* c, int n_views, const vcy_view* views, const float* const* sdf_device, int n_slabs,
                     int sample_stride, float brick_cost, int32_t* z_bounds, double* layer_cost, int max_layers,
                     int* n_layers) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  if (n_views <= 0 || !views || !sdf_device || !z_bounds) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_views; ++i) {
    const int rc = check_view_static(&views[i]);
    if (rc != VCY_OK) return rc;
    if (!sdf_device[i]) {
      set_error("null SDF pointer");
      return VCY_ERR_INVALID_ARG;
    }
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  return plan_z_slabs(c, n_views, views, sdf_device, n_slabs, sample_stride, brick_cost, z_bounds, layer_cost,
                      max_layers, n_layers);
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

int vcy_distance_transform_l1(const uint8_t* mask, int w, int h, const int32_t rmin[2],
                              const int32_t rmax[2], float* out) {
  if (!mask || !out || w <= 0 || h <= 0 || rmin[0] < 0 || rmin[1] < 0 || rmax[0] >= w || rmax[1] >= h) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  host_distance_transform_l1(mask, w, h, rmin, rmax, out);
  return VCY_OK;
}

int vcy_make_sdf(const uint8_t* mask, int w, int h, const int32_t rmin[2], const int32_t rmax[2],
                 int normalize, int truncate, float band, float* out) {
  if (!mask || !out || w <= 0 || h <= 0 || rmin[0] < 0 || rmin[1] < 0 || rmax[0] >= w || rmax[1] >= h) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  host_make_sdf(mask, w, h, rmin, rmax, normalize != 0, truncate != 0, band, out);
  return VCY_OK;
}

}  // extern "C"
