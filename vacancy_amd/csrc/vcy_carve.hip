// The per-view carve entry points of the C ABI: the checks of their views, the queue of views that wait for one fused
// launch, the silhouette of one view, the slab planner's wrappers and the two host SDF functions.  The streamed batches:
// carve_stream.hip.  The kernels and their launches: carve_kernels.hip, carve_fused.hip, sdf2d.hip.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vcy_internal.h"

using namespace vcy;

namespace vcy {
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

int check_carve_views(vcy_ctx* c, int n_views, const vcy_view* views) {
  for (int i = 0; i < n_views; ++i) {
    const int rc = check_view(c, &views[i]);
    if (rc != VCY_OK) return rc;
  }
  return VCY_OK;
}
}  // namespace vcy

extern "C" {

/* ---- carving entry points ------------------------------------------------ */

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

constexpr int kMaxPendingViews = 32;  // queued images held at most (3.7 MB each at 1280x720)

// Queues (view, private device image): flushes first if the queue is full or of the other projection
// model (one model per fused launch).
static int enqueue_view(vcy_ctx* c, const vcy_view* view, DeviceBuf<float> d_img) {
  int rc = VCY_OK;
  if (!c->pending.empty() && (c->pending.front().view.is_ortho != 0) != (view->is_ortho != 0)) rc = flush_pending(c, true);
  if (rc == VCY_OK) {
    c->pending.push_back(vcy_ctx::PendingView{*view, std::move(d_img)});
    c->st.halo_stale();  // the neighbour below queues the view too: what was taken from it will not be its last two slices
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
