// K17: the shading pass behind the rasteriser -- per-vertex attributes interpolated at every pixel's winning face, and the
// photometric error of the rendering against the photographs (vcy_shade_mesh / vcy_mesh_photo_error; no reference
// counterpart -- the definition is the section "shading a rasterised mesh" of vacancy_hip.h, restated in numpy in
// tests/shade_ref.py; the serial host function is shade_host.hip).
//
// Deferred: the key images are filled by the unchanged rs_raster_kernel (raster.hip, through raster_launch.h), and
//   rs_shade   one lane per pixel, a wave over 64 consecutive pixels of a row, blockIdx.y the view (rs_resolve_kernel's
//              grid).  A hit lane takes the face from its key, loads the three indices and positions, re-projects them and
//              evaluates the weights with the rasteriser's own functions (raster_shade.h), gathers 3 x channels attributes
//              and writes what is asked for.  `channels` is a template parameter: the attribute loop is unrolled and a
//              pixel's values leave in one store.
//   <3, true>  the photometric flavour writes no image: it reads the photograph as uploaded (three bytes per pixel -- every
//              texel is read once, by the lane of its pixel, so a packing pass to one dword per texel, as the colour path
//              has it for its gathers, would move more bytes than it saves) and the silhouette, sums the seven integers in
//              the wave (32-bit: a workgroup's largest sum is 256 * 65025), then in the workgroup through LDS, and issues
//              one 64-bit integer atomic add per counter per workgroup that counted a pixel.  Workgroups are dispatched a
//              view at a time, so those in flight would all add to the seven words of one view: every view has kSumSlots
//              copies of its counters, each on a cache line of its own, a workgroup adds to copy blockIdx.x % kSumSlots, and
//              the host adds the copies up (integers: the same seven numbers).
// No float atomics.  The voxel state is neither read nor written: any context will do, and nothing is declared.
#include <algorithm>
#include <vector>

#include "raster_launch.h"
#include "raster_shade.h"
#include "vcy_internal.h"

namespace vcy {
namespace rs {

struct ShadeTarget {  // one per view of a launch, in device memory, beside its View and its Target
  float* value;          // any of the three outputs may be null
  uint8_t* value8;
  float* bary;
  const uint8_t* photo;  // the photometric flavour: the photograph, and the silhouette or null
  const uint8_t* mask;
};

struct ShadeLaunch {
  const float* vtx;
  const int32_t* faces;
  const float* attr;
  const View* views;
  const Target* targets;        // the keys
  const ShadeTarget* shade;
  float background[4];
  u64* sums;                    // kSumSlots x kSlotStride per view (photometric flavour)
};

constexpr int kSumSlots = 16;    // copies of a view's counters
constexpr int kSlotStride = 16;  // 64-bit words from one copy to the next: 128 bytes, kSums of them used

template <int C> struct Values { float v[C]; };
template <int C> struct Bytes { uint8_t v[C]; };

// the sum of `x` over the wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d);
  return x;
}

// grid (waves of the largest view / 4, views of the launch)
template <int C, bool ERR>
__global__ __launch_bounds__(256) void rs_shade_kernel(ShadeLaunch L) {
  const View& v = L.views[blockIdx.y];  // (uniform: the records are read once per wave)
  const ShadeTarget& t = L.shade[blockIdx.y];
  const u64* keys = L.targets[blockIdx.y].keys;
  const int lane = threadIdx.x & 63;
  const int64_t words = ((int64_t)v.w + 63) / 64;
  const int64_t word = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (uniform in the wave)
  const bool in_rows = word < words * v.h;
  if (!ERR && !in_rows) return;  // (the photometric flavour stays for the workgroup's sum)
  const int64_t y = word / words, x = (word - y * words) * 64 + lane;
  const bool in_img = in_rows && x < v.w;
  const int64_t px = y * v.w + x;
  const u64 key = in_img ? keys[px] : kMissKey;
  bool hit = key != kMissKey;
  if (ERR) hit = hit && (!t.mask || t.mask[px] != 0);

  float val[C];
  double b[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < C; ++c) val[c] = L.background[c];
  if (hit) {
    Face f;
    winner_face(v, L.vtx, L.faces, (int64_t)(uint32_t)key, f);
    weights(v, f, (int)x, (int)y, b);
    shade<C>(f, b, L.attr, val);
  }

  if constexpr (!ERR) {
    if (!in_img) return;
    if (t.value) {
      Values<C> out;
#pragma unroll
      for (int c = 0; c < C; ++c) out.v[c] = val[c];
      *(Values<C>*)(t.value + C * px) = out;
    }
    if (t.value8) {
      Bytes<C> out;
#pragma unroll
      for (int c = 0; c < C; ++c) out.v[c] = quantize(val[c]);
      *(Bytes<C>*)(t.value8 + C * px) = out;
    }
    if (t.bary) {
      Values<3> out;
#pragma unroll
      for (int k = 0; k < 3; ++k) out.v[k] = (float)b[k];
      *(Values<3>*)(t.bary + 3 * px) = out;
    }
  } else {
    static_assert(C == 3, "the photometric error is defined for three channels");
    __shared__ uint32_t part[4][kSums];
    uint32_t s[kSums] = {0, 0, 0, 0, 0, 0, 0};
    if (hit) {
      s[0] = 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int d = (int)quantize(val[c]) - (int)t.photo[3 * px + c];
        s[1 + c] = (uint32_t)(d < 0 ? -d : d);
        s[4 + c] = (uint32_t)(d * d);
      }
    }
    const bool any = __ballot(hit) != 0;  // (uniform)
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
      const uint32_t sum = any ? wave_sum(s[k]) : 0u;
      if (lane == 0) part[threadIdx.x >> 6][k] = sum;
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
      const uint32_t sum = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
      u64* slot = L.sums + ((size_t)blockIdx.y * kSumSlots + blockIdx.x % kSumSlots) * kSlotStride;
      if (sum) atomicAdd(slot + threadIdx.x, (u64)sum);  // (n == 0: every sum is 0)
    }
  }
}

}  // namespace rs

namespace {

size_t hit_words(const vcy_view& v) { return (((size_t)v.width + 63) / 64) * (size_t)v.height; }

// where the images of one view lie among those of its chunk, behind the key images
struct ShadeSlots { size_t value, value8, bary, photo, mask; };
ShadeSlots take_images(PoolLayout& at, const vcy_view& v, int channels, bool value, bool value8, bool bary, bool photo, bool mask) {
  const size_t px = (size_t)v.width * (size_t)v.height;
  return ShadeSlots{value ? at.take(4 * px * (size_t)channels) : 0, value8 ? at.take(px * (size_t)channels) : 0,
                    bary ? at.take(12 * px) : 0, photo ? at.take(3 * px) : 0, mask ? at.take(px) : 0};
}

template <bool ERR>
void launch_shade(int channels, dim3 grid, hipStream_t stream, const rs::ShadeLaunch& S) {
  if (ERR) hipLaunchKernelGGL((rs::rs_shade_kernel<3, true>), grid, dim3(256), 0, stream, S);
  else if (channels == 1) hipLaunchKernelGGL((rs::rs_shade_kernel<1, false>), grid, dim3(256), 0, stream, S);
  else if (channels == 2) hipLaunchKernelGGL((rs::rs_shade_kernel<2, false>), grid, dim3(256), 0, stream, S);
  else if (channels == 3) hipLaunchKernelGGL((rs::rs_shade_kernel<3, false>), grid, dim3(256), 0, stream, S);
  else hipLaunchKernelGGL((rs::rs_shade_kernel<4, false>), grid, dim3(256), 0, stream, S);
}

// vcy_shade_mesh (photos == null) and vcy_mesh_photo_error (photos, sums; channels 3) behind their argument checks
int shade_device(vcy_ctx* c, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                 const float* attributes, int channels, const float* background, int n_views, const vcy_view* views,
                 float* const* value, uint8_t* const* value8, float* const* bary, const uint8_t* const* photos,
                 const uint8_t* const* masks, int64_t* sums) {
  VCY_HIP_CHECK(hipSetDevice(c->device));
  c->last_shade_ms[0] = c->last_shade_ms[1] = 0.0f;
  for (Event& e : c->ev_sh) VCY_HIP_CHECK(e.ensure());
  const auto wants = [&](int i, int which) {
    return which == 0 ? value && value[i] : which == 1 ? value8 && value8[i] : which == 2 ? bary && bary[i]
           : which == 3 ? photos != nullptr : masks != nullptr;
  };

  // the rasteriser's pool (vcy_ctx::d_rs_buf), laid out for this call:
  // [view records | raster targets | shade targets | drop counters | agreement counters (unused) | the sums' copies | vertices |
  //  faces | attributes | of the largest chunk: the key images, then per view value, value8, bary, photograph, silhouette]
  PoolLayout at;
  const size_t at_views = at.take(sizeof(rs::View) * rs::kMaxViewsPerLaunch),
               at_targets = at.take(sizeof(rs::Target) * rs::kMaxViewsPerLaunch),
               at_shade = at.take(sizeof(rs::ShadeTarget) * rs::kMaxViewsPerLaunch),
               at_dropped = at.take(sizeof(rs::u64) * 2 * rs::kMaxViewsPerLaunch),
               at_counts = at.take(sizeof(rs::u64) * 3 * rs::kMaxViewsPerLaunch),
               at_sums = at.take(sizeof(rs::u64) * rs::kSumSlots * rs::kSlotStride * rs::kMaxViewsPerLaunch),
               at_vtx = at.take(sizeof(float) * 3 * (size_t)n_vertices), at_faces = at.take(sizeof(int32_t) * 3 * (size_t)n_faces),
               at_attr = at.take(sizeof(float) * (size_t)channels * (size_t)n_vertices), at_images = at.total();
  size_t image_bytes = 0;
  for (int first = 0; first < n_views; first += rs::kMaxViewsPerLaunch) {
    PoolLayout images;
    const int last = std::min(n_views, first + rs::kMaxViewsPerLaunch);
    for (int i = first; i < last; ++i) (void)images.take(8 * (size_t)views[i].width * (size_t)views[i].height);
    for (int i = first; i < last; ++i)
      (void)take_images(images, views[i], channels, wants(i, 0), wants(i, 1), wants(i, 2), wants(i, 3), wants(i, 4));
    image_bytes = std::max(image_bytes, images.total());
  }
  VCY_HIP_CHECK(c->d_rs_buf.grow(at_images + image_bytes, c->stream, false));
  char* base = (char*)c->d_rs_buf;
  if (n_vertices > 0) {
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_vtx, vertices, sizeof(float) * 3 * (size_t)n_vertices, hipMemcpyHostToDevice, c->stream));
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_attr, attributes, sizeof(float) * (size_t)channels * (size_t)n_vertices, hipMemcpyHostToDevice, c->stream));
  }
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
  rs::ShadeLaunch S{};
  S.vtx = L.vtx, S.faces = L.faces, S.views = L.views, S.targets = L.targets;
  S.attr = (const float*)(base + at_attr);
  S.shade = (const rs::ShadeTarget*)(base + at_shade);
  for (int k = 0; k < 4; ++k) S.background[k] = k < channels && background ? background[k] : 0.0f;
  S.sums = (rs::u64*)(base + at_sums);

  // One chunk.  Its copies read `rec`, `tgt`, `sht` and the caller's images and write the caller's arrays asynchronously
  // until the wait at its end: a failure in between is returned through the loop below, which waits before anything is
  // destroyed.
  std::vector<rs::View> rec;
  std::vector<rs::Target> tgt;
  std::vector<rs::ShadeTarget> sht;
  std::vector<ShadeSlots> slots;
  std::vector<rs::u64> sums_host(photos ? (size_t)rs::kSumSlots * rs::kSlotStride * rs::kMaxViewsPerLaunch : 0);
  auto chunk = [&](int first, float* raster_ms, float* shade_ms) -> int {
    const int m = std::min(rs::kMaxViewsPerLaunch, n_views - first);
    rec.assign((size_t)m, rs::View{});
    tgt.assign((size_t)m, rs::Target{});
    sht.assign((size_t)m, rs::ShadeTarget{});
    slots.assign((size_t)m, ShadeSlots{});
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
      const size_t px = (size_t)v.width * (size_t)v.height;
      const ShadeSlots s = take_images(images, v, channels, wants(at_call, 0), wants(at_call, 1), wants(at_call, 2),
                                       wants(at_call, 3), wants(at_call, 4));
      slots[(size_t)i] = s;
      rs::ShadeTarget& t = sht[(size_t)i];
      t.value = wants(at_call, 0) ? (float*)(image_base + s.value) : nullptr;
      t.value8 = wants(at_call, 1) ? (uint8_t*)(image_base + s.value8) : nullptr;
      t.bary = wants(at_call, 2) ? (float*)(image_base + s.bary) : nullptr;
      t.photo = photos ? (const uint8_t*)(image_base + s.photo) : nullptr;
      t.mask = masks ? (const uint8_t*)(image_base + s.mask) : nullptr;
      if (photos) VCY_HIP_CHECK(hipMemcpyAsync(image_base + s.photo, photos[at_call], 3 * px, hipMemcpyHostToDevice, c->stream));
      if (masks) VCY_HIP_CHECK(hipMemcpyAsync(image_base + s.mask, masks[at_call], px, hipMemcpyHostToDevice, c->stream));
    }
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_views, rec.data(), sizeof(rs::View) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_targets, tgt.data(), sizeof(rs::Target) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_shade, sht.data(), sizeof(rs::ShadeTarget) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    // (the three counter arrays lie one behind the other: each a multiple of 256 bytes)
    VCY_HIP_CHECK(hipMemsetAsync(base + at_dropped, 0, sizeof(rs::u64) * (5 + rs::kSumSlots * rs::kSlotStride) * rs::kMaxViewsPerLaunch, c->stream));

    VCY_HIP_CHECK(hipEventRecord(c->ev_sh[0], c->stream));
    VCY_HIP_CHECK(hipMemsetAsync(image_base, 0xff, key_bytes, c->stream));
    L.n_views = m;
    VCY_HIP_CHECK(rs::launch_raster(L, c->stream));
    VCY_HIP_CHECK(hipEventRecord(c->ev_sh[1], c->stream));
    const dim3 grid((unsigned)((words_max + 3) / 4), (unsigned)m);
    if (photos) launch_shade<true>(3, grid, c->stream, S);
    else launch_shade<false>(channels, grid, c->stream, S);
    VCY_HIP_CHECK(hipGetLastError());
    VCY_HIP_CHECK(hipEventRecord(c->ev_sh[2], c->stream));

    for (int i = 0; i < m; ++i) {
      const int at_call = first + i;
      const vcy_view& v = views[at_call];
      const size_t px = (size_t)v.width * (size_t)v.height;
      const ShadeSlots& s = slots[(size_t)i];
      if (wants(at_call, 0))
        VCY_HIP_CHECK(hipMemcpyAsync(value[at_call], image_base + s.value, 4 * px * (size_t)channels, hipMemcpyDeviceToHost, c->stream));
      if (wants(at_call, 1))
        VCY_HIP_CHECK(hipMemcpyAsync(value8[at_call], image_base + s.value8, px * (size_t)channels, hipMemcpyDeviceToHost, c->stream));
      if (wants(at_call, 2))
        VCY_HIP_CHECK(hipMemcpyAsync(bary[at_call], image_base + s.bary, 12 * px, hipMemcpyDeviceToHost, c->stream));
    }
    if (photos)
      VCY_HIP_CHECK(hipMemcpyAsync(sums_host.data(), base + at_sums, sizeof(rs::u64) * rs::kSumSlots * rs::kSlotStride * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    VCY_HIP_CHECK(hipStreamSynchronize(c->stream));  // (the host arrays above are read and written until here)
    if (photos)  // (the copies of every counter added up; int64 sums: the unsigned counters' bits)
      for (int i = 0; i < m; ++i)
        for (int k = 0; k < rs::kSums; ++k) {
          rs::u64 sum = 0;
          for (int slot = 0; slot < rs::kSumSlots; ++slot) sum += sums_host[((size_t)i * rs::kSumSlots + (size_t)slot) * rs::kSlotStride + (size_t)k];
          sums[(size_t)rs::kSums * (size_t)(first + i) + (size_t)k] = (int64_t)sum;
        }
    VCY_HIP_CHECK(hipEventElapsedTime(raster_ms, c->ev_sh[0], c->ev_sh[1]));
    VCY_HIP_CHECK(hipEventElapsedTime(shade_ms, c->ev_sh[1], c->ev_sh[2]));
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
  c->last_shade_ms[0] = total[0], c->last_shade_ms[1] = total[1];
  return VCY_OK;
}

int no_context() {
  set_error("voxel grid has not been initialized");
  return VCY_ERR_NOT_INITIALIZED;
}

}  // namespace

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_shade_mesh(vcy_ctx* c, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                   const float* attributes, int n_views, const vcy_view* views, const vcy_shade_option* option,
                   float* const* value_host, uint8_t* const* value8_host, float* const* bary_host) {
  { const int rc = shade_check_args("vcy_shade_mesh", n_vertices, n_faces, vertices, faces, attributes, n_views, views, option); if (rc != VCY_OK) return rc; }
  if (!c) return no_context();  // (behind the argument checks: those need no context)
  return shade_device(c, n_vertices, n_faces, vertices, faces, attributes, option->channels, option->background, n_views, views,
                      value_host, value8_host, bary_host, nullptr, nullptr, nullptr);
}

int vcy_mesh_photo_error(vcy_ctx* c, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                         const float* colors, int n_views, const vcy_view* views, const uint8_t* const* photos_host,
                         const uint8_t* const* masks_host, int64_t* sums) {
  { const int rc = photo_error_check_args("vcy_mesh_photo_error", n_vertices, n_faces, vertices, faces, colors, n_views, views, photos_host, masks_host, sums); if (rc != VCY_OK) return rc; }
  if (!c) return no_context();
  return shade_device(c, n_vertices, n_faces, vertices, faces, colors, 3, nullptr, n_views, views, nullptr, nullptr, nullptr,
                      photos_host, masks_host, sums);
}

int vcy_last_shade_ms(const vcy_ctx* c, float* raster_ms, float* shade_ms) {
  if (!c) return VCY_ERR_INVALID_ARG;
  if (raster_ms) *raster_ms = c->last_shade_ms[0];
  if (shade_ms) *shade_ms = c->last_shade_ms[1];
  return VCY_OK;
}

}  // extern "C"
