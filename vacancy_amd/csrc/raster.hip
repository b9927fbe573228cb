// K16: the rasteriser -- an indexed mesh into views: depth, face id, hit bits, agreement with silhouettes (vcy_raster_mesh /
// vcy_mesh_agreement; no reference counterpart -- the definition is the section "rasterising an indexed mesh" of
// vacancy_hip.h, restated in numpy in tests/raster_ref.py; the serial host function is raster_host.hip).
//
// The arithmetic of a (face, view, pixel) fragment is raster_fragment.h, shared with the host function.  The winner of a
// pixel is the smallest (depth bits, face index), so the image does not depend on the order in which fragments arrive:
//   key image   one uint64 per pixel and view, (depth bits << 32) | face, all ones = no fragment; depths are
//               non-negative floats, so their bits order as integers, and a 64-bit atomicMin keeps the winner.
//   rs_raster   one lane per face, the view loop inside the lane: the three world positions are loaded once and stay in
//               registers, the view records are read with a wave-uniform index (scalar loads), the projection is
//               recomputed per view -- no projected-vertex buffer.  A lane walks its candidate box itself while the box
//               holds at most "rasterwide" pixels; the faces with larger boxes are balloted, and for each the wave
//               broadcasts the projected corners and its 64 lanes cover the box in 8 x 8 tiles.  No list, no second
//               launch, no capacity.  A fragment reads the key with a plain load and issues the atomic only when its own
//               key is smaller: keys only fall, so a stale read costs an unneeded atomic and never a missed one.
//               n_dropped: ballot and one integer add per wave, view and class.
//   rs_resolve  one lane per pixel, a wave over 64 consecutive pixels of a row: key -> depth and face, the wave's ballot is
//               the hit word; for the agreement, ballots against the silhouette and one integer add per wave and count.
// No float atomics.  The voxel state is neither read nor written: any context will do, and nothing is declared.
#include <algorithm>
#include <cmath>
#include <vector>

#include "raster_fragment.h"
#include "raster_launch.h"
#include "vcy_internal.h"

namespace vcy {
namespace rs {

__device__ __forceinline__ void propose(u64* keys, int64_t at, u64 key) {
  if (key < keys[at]) atomicMin(keys + at, key);
}

__global__ __launch_bounds__(256) void rs_raster_kernel(Launch L) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < L.n_faces;  // (no early return: the wave draws its wide faces together)
  int id[3] = {0, 0, 0};
  float P[3][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
  if (live) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      id[k] = L.faces[3 * i + k];
      const float* at = L.vtx + 3 * (int64_t)id[k];
      P[k][0] = at[0], P[k][1] = at[1], P[k][2] = at[2];
    }
  }
  for (int k = 0; k < L.n_views; ++k) {  // (k is uniform: the records are read once per wave)
    const View& v = L.views[k];
    u64* keys = L.targets[k].keys;
    Point p[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = project(v, P[j]);
    Face f;
    const int cls = setup_face(v, id, p, f);  // (a dropped face, and a lane without one, has an empty box)
    const u64 drop0 = __ballot(live && cls == kDropUnusable), drop1 = __ballot(live && cls == kDropDegenerate);
    if (lane == 0) {
      if (drop0) atomicAdd(L.dropped + 2 * k, (u64)__builtin_popcountll(drop0));
      if (drop1) atomicAdd(L.dropped + 2 * k + 1, (u64)__builtin_popcountll(drop1));
    }
    const long long n_px = live && cls == kDrawn ? box_pixels(f) : 0;
    const bool is_wide = n_px > L.wide;
    if (n_px > 0 && !is_wide) {
      for (int y = f.y0; y <= f.y1; ++y)
        for (int x = f.x0; x <= f.x1; ++x) {
          const u64 key = fragment_key(v, f, (int)i, x, y);
          if (key != kMissKey) propose(keys, (int64_t)v.w * y + x, key);
        }
    }
    u64 todo = __ballot(is_wide);
    while (todo) {  // (uniform)
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      int bid[3];
      Point bp[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        bid[j] = __shfl(id[j], src);
        bp[j].u = __shfl(p[j].u, src);
        bp[j].w = __shfl(p[j].w, src);
        bp[j].z = __shfl(p[j].z, src);
        bp[j].usable = true;
      }
      const int face = (int)(i - lane) + src;
      Face g;
      (void)setup_face(v, bid, bp, g);  // the source lane's setup, from the same bits
      const int dx = lane & 7, dy = lane >> 3;
      for (long long ty = g.y0; ty <= g.y1; ty += 8)
        for (long long tx = g.x0; tx <= g.x1; tx += 8) {
          const long long x = tx + dx, y = ty + dy;
          if (x <= g.x1 && y <= g.y1) {
            const u64 key = fragment_key(v, g, face, (int)x, (int)y);
            if (key != kMissKey) propose(keys, (int64_t)v.w * y + x, key);
          }
        }
    }
  }
}

// grid (waves of the largest view / 4, views of the launch)
template <bool AGREE>
__global__ __launch_bounds__(256) void rs_resolve_kernel(const View* __restrict__ views, const Target* __restrict__ targets,
                                                         u64* __restrict__ counts) {
  const View& v = views[blockIdx.y];
  const Target& t = targets[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int64_t words = ((int64_t)v.w + 63) / 64;
  const int64_t word = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (uniform in the wave)
  if (word >= words * v.h) return;
  const int64_t y = word / words, x = (word - y * words) * 64 + lane;
  const bool in_img = x < v.w;
  const int64_t px = y * v.w + x;
  const u64 key = in_img ? t.keys[px] : kMissKey;
  const bool hit = key != kMissKey;
  if (in_img) {
    if (t.depth) t.depth[px] = hit ? bits_float((uint32_t)(key >> 32)) : INFINITY;
    if (t.face) t.face[px] = hit ? (int32_t)(uint32_t)key : -1;
  }
  const u64 hb = __ballot(hit);
  if (t.hits && lane == 0) t.hits[word] = hb;
  if (AGREE) {
    const bool in_roi = in_img && x >= v.rx0 && x <= v.rx1 && y >= v.ry0 && y <= v.ry1;
    const bool mask = in_roi && t.mask[px] != 0;  // (a hit lies inside the ROI: candidate pixels do)
    const u64 both = __ballot(mask && hit), only_mask = __ballot(mask && !hit), only_mesh = __ballot(!mask && hit);
    if (lane == 0) {
      u64* c = counts + 3 * (size_t)blockIdx.y;
      if (both) atomicAdd(c + 0, (u64)__builtin_popcountll(both));
      if (only_mask) atomicAdd(c + 1, (u64)__builtin_popcountll(only_mask));
      if (only_mesh) atomicAdd(c + 2, (u64)__builtin_popcountll(only_mesh));
    }
  }
}

hipError_t launch_raster(const Launch& L, hipStream_t stream) {
  if (L.n_faces <= 0) return hipSuccess;
  hipLaunchKernelGGL(rs_raster_kernel, dim3((unsigned)((L.n_faces + 255) / 256)), dim3(256), 0, stream, L);
  return hipGetLastError();
}

}  // namespace rs

namespace {

size_t hit_words(const vcy_view& v) { return (((size_t)v.width + 63) / 64) * (size_t)v.height; }

// where the images of one view lie among those of its chunk (the sizing of the pool and the chunk's records both walk the
// views through this); the key images come first, one behind the other, so that one fill covers them
struct ImageSlots { size_t depth, face, hits, mask; };
ImageSlots take_images(PoolLayout& at, const vcy_view& v, bool depth, bool face, bool hits, bool mask) {
  const size_t px = (size_t)v.width * (size_t)v.height;
  return ImageSlots{depth ? at.take(4 * px) : 0, face ? at.take(4 * px) : 0, hits ? at.take(8 * hit_words(v)) : 0,
                    mask ? at.take(px) : 0};
}

// vcy_raster_mesh (masks == null) and vcy_mesh_agreement (masks, counts) behind their argument checks
int raster_device(vcy_ctx* c, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces, int n_views,
                  const vcy_view* views, float* const* depth, int32_t* const* face, uint64_t* const* hits, int64_t* n_dropped,
                  const uint8_t* const* masks, int64_t* counts) {
  VCY_HIP_CHECK(hipSetDevice(c->device));
  c->last_raster_ms[0] = c->last_raster_ms[1] = 0.0f;
  for (Event& e : c->ev_rs) VCY_HIP_CHECK(e.ensure());
  const auto wants = [&](int i, int which) {
    return which == 0 ? depth && depth[i] : which == 1 ? face && face[i] : which == 2 ? hits && hits[i] : masks != nullptr;
  };

  // [view records | targets | drop counters | agreement counters | vertices | faces | of the largest chunk: the key images,
  //  then per view depth, face ids, hit bits, silhouette]: sized once, so that the mesh outlives the chunks
  PoolLayout at;
  const size_t at_views = at.take(sizeof(rs::View) * rs::kMaxViewsPerLaunch),
               at_targets = at.take(sizeof(rs::Target) * rs::kMaxViewsPerLaunch),
               at_dropped = at.take(sizeof(rs::u64) * 2 * rs::kMaxViewsPerLaunch),
               at_counts = at.take(sizeof(rs::u64) * 3 * rs::kMaxViewsPerLaunch),
               at_vtx = at.take(sizeof(float) * 3 * (size_t)n_vertices), at_faces = at.take(sizeof(int32_t) * 3 * (size_t)n_faces),
               at_images = at.total();
  size_t image_bytes = 0;
  for (int first = 0; first < n_views; first += rs::kMaxViewsPerLaunch) {
    PoolLayout images;
    const int last = std::min(n_views, first + rs::kMaxViewsPerLaunch);
    for (int i = first; i < last; ++i) (void)images.take(8 * (size_t)views[i].width * (size_t)views[i].height);
    for (int i = first; i < last; ++i) (void)take_images(images, views[i], wants(i, 0), wants(i, 1), wants(i, 2), wants(i, 3));
    image_bytes = std::max(image_bytes, images.total());
  }
  VCY_HIP_CHECK(c->d_rs_buf.grow(at_images + image_bytes, c->stream, false));
  char* base = (char*)c->d_rs_buf;
  if (n_vertices > 0)
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_vtx, vertices, sizeof(float) * 3 * (size_t)n_vertices, hipMemcpyHostToDevice, c->stream));
  if (n_faces > 0)
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_faces, faces, sizeof(int32_t) * 3 * (size_t)n_faces, hipMemcpyHostToDevice, c->stream));

  rs::Launch L{};
  L.n_faces = n_faces;
  L.vtx = (const float*)(base + at_vtx);
  L.faces = (const int32_t*)(base + at_faces);
  L.views = (const rs::View*)(base + at_views);
  L.targets = (const rs::Target*)(base + at_targets);
  L.wide = c->raster_wide;
  L.dropped = (rs::u64*)(base + at_dropped);
  L.counts = (rs::u64*)(base + at_counts);

  // One chunk.  Its copies read `rec`, `tgt` and the caller's silhouettes and write the caller's arrays asynchronously until
  // the wait at its end: a failure in between is returned through the loop below, which waits before anything is destroyed.
  std::vector<rs::View> rec;
  std::vector<rs::Target> tgt;
  std::vector<ImageSlots> slots;
  std::vector<rs::u64> dropped_host((size_t)2 * rs::kMaxViewsPerLaunch);
  auto chunk = [&](int first, float* raster_ms, float* resolve_ms) -> int {
    const int m = std::min(rs::kMaxViewsPerLaunch, n_views - first);
    rec.assign((size_t)m, rs::View{});
    tgt.assign((size_t)m, rs::Target{});
    slots.assign((size_t)m, ImageSlots{});
    PoolLayout images;
    char* image_base = base + at_images;
    int64_t words_max = 0;
    for (int i = 0; i < m; ++i) {
      const vcy_view& v = views[first + i];
      rs::fill_view(v, &rec[(size_t)i]);
      tgt[(size_t)i].keys = (rs::u64*)(image_base + images.take(8 * (size_t)v.width * (size_t)v.height));
      words_max = std::max(words_max, (int64_t)hit_words(v));
    }
    const size_t key_bytes = images.total();
    for (int i = 0; i < m; ++i) {
      const int at_call = first + i;
      const vcy_view& v = views[at_call];
      const ImageSlots s = take_images(images, v, wants(at_call, 0), wants(at_call, 1), wants(at_call, 2), wants(at_call, 3));
      slots[(size_t)i] = s;
      rs::Target& t = tgt[(size_t)i];
      t.depth = wants(at_call, 0) ? (float*)(image_base + s.depth) : nullptr;
      t.face = wants(at_call, 1) ? (int32_t*)(image_base + s.face) : nullptr;
      t.hits = wants(at_call, 2) ? (rs::u64*)(image_base + s.hits) : nullptr;
      t.mask = masks ? (const uint8_t*)(image_base + s.mask) : nullptr;
      if (masks)
        VCY_HIP_CHECK(hipMemcpyAsync(image_base + s.mask, masks[at_call], (size_t)v.width * (size_t)v.height,
                                     hipMemcpyHostToDevice, c->stream));
    }
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_views, rec.data(), sizeof(rs::View) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_targets, tgt.data(), sizeof(rs::Target) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    VCY_HIP_CHECK(hipMemsetAsync(base + at_dropped, 0, sizeof(rs::u64) * 5 * rs::kMaxViewsPerLaunch, c->stream));  // (both counter arrays: each a multiple of 256 bytes)

    VCY_HIP_CHECK(hipEventRecord(c->ev_rs[0], c->stream));
    VCY_HIP_CHECK(hipMemsetAsync(image_base, 0xff, key_bytes, c->stream));
    L.n_views = m;
    VCY_HIP_CHECK(rs::launch_raster(L, c->stream));
    VCY_HIP_CHECK(hipEventRecord(c->ev_rs[1], c->stream));
    const dim3 grid((unsigned)((words_max + 3) / 4), (unsigned)m);
    if (masks) hipLaunchKernelGGL((rs::rs_resolve_kernel<true>), grid, dim3(256), 0, c->stream, L.views, L.targets, L.counts);
    else hipLaunchKernelGGL((rs::rs_resolve_kernel<false>), grid, dim3(256), 0, c->stream, L.views, L.targets, L.counts);
    VCY_HIP_CHECK(hipGetLastError());
    VCY_HIP_CHECK(hipEventRecord(c->ev_rs[2], c->stream));

    for (int i = 0; i < m; ++i) {
      const int at_call = first + i;
      const vcy_view& v = views[at_call];
      const size_t px = (size_t)v.width * (size_t)v.height;
      const ImageSlots& s = slots[(size_t)i];
      if (wants(at_call, 0))
        VCY_HIP_CHECK(hipMemcpyAsync(depth[at_call], image_base + s.depth, 4 * px, hipMemcpyDeviceToHost, c->stream));
      if (wants(at_call, 1))
        VCY_HIP_CHECK(hipMemcpyAsync(face[at_call], image_base + s.face, 4 * px, hipMemcpyDeviceToHost, c->stream));
      if (wants(at_call, 2))
        VCY_HIP_CHECK(hipMemcpyAsync(hits[at_call], image_base + s.hits, 8 * hit_words(v), hipMemcpyDeviceToHost, c->stream));
    }
    if (n_dropped)
      VCY_HIP_CHECK(hipMemcpyAsync(dropped_host.data(), base + at_dropped, sizeof(rs::u64) * 2 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (masks)  // (int64 counts of pixels: the unsigned counters' bits)
      VCY_HIP_CHECK(hipMemcpyAsync(counts + 3 * (size_t)first, base + at_counts, sizeof(rs::u64) * 3 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    VCY_HIP_CHECK(hipStreamSynchronize(c->stream));  // (the host arrays above are read and written until here)
    if (n_dropped)
      for (int k = 0; k < 2 * m; ++k) n_dropped[2 * (size_t)first + (size_t)k] = (int64_t)dropped_host[(size_t)k];
    VCY_HIP_CHECK(hipEventElapsedTime(raster_ms, c->ev_rs[0], c->ev_rs[1]));
    VCY_HIP_CHECK(hipEventElapsedTime(resolve_ms, c->ev_rs[1], c->ev_rs[2]));
    return VCY_OK;
  };
  float total[2] = {0.0f, 0.0f};
  for (int first = 0; first < n_views; first += rs::kMaxViewsPerLaunch) {
    float ms[2] = {0.0f, 0.0f};
    const int rc = chunk(first, &ms[0], &ms[1]);
    if (rc != VCY_OK) {
      (void)hipStreamSynchronize(c->stream);  // (queued copies still name host memory of this call and of the caller)
      return rc;
    }
    total[0] += ms[0], total[1] += ms[1];
  }
  c->last_raster_ms[0] = total[0], c->last_raster_ms[1] = total[1];
  return VCY_OK;
}

}  // namespace

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_raster_mesh(vcy_ctx* c, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces, int n_views,
                    const vcy_view* views, float* const* depth_host, int32_t* const* face_host, uint64_t* const* hits_host,
                    int64_t* n_dropped) {
  { const int rc = raster_check_args("vcy_raster_mesh", n_vertices, n_faces, vertices, faces, n_views, views); if (rc != VCY_OK) return rc; }
  if (!c) {  // (behind the argument checks: those need no context)
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  return raster_device(c, n_vertices, n_faces, vertices, faces, n_views, views, depth_host, face_host, hits_host, n_dropped,
                       nullptr, nullptr);
}

int vcy_mesh_agreement(vcy_ctx* c, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces, int n_views,
                       const vcy_view* views, const uint8_t* const* masks_host, int64_t* counts) {
  if (!masks_host || !counts) {
    set_error("vcy_mesh_agreement: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  { const int rc = raster_check_args("vcy_mesh_agreement", n_vertices, n_faces, vertices, faces, n_views, views); if (rc != VCY_OK) return rc; }
  for (int i = 0; i < n_views; ++i)
    if (!masks_host[i]) {
      set_error("vcy_mesh_agreement: null silhouette");
      return VCY_ERR_INVALID_ARG;
    }
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  return raster_device(c, n_vertices, n_faces, vertices, faces, n_views, views, nullptr, nullptr, nullptr, nullptr, masks_host,
                       counts);
}

int vcy_last_raster_ms(const vcy_ctx* c, float* raster_ms, float* resolve_ms) {
  if (!c) return VCY_ERR_INVALID_ARG;
  if (raster_ms) *raster_ms = c->last_raster_ms[0];
  if (resolve_ms) *resolve_ms = c->last_raster_ms[1];
  return VCY_OK;
}

}  // extern "C"
