// Colours of mesh vertices from the input photographs, with occlusion (vcy_color_vertices / vcy_color_vertices_host; no
// reference counterpart -- the definition is the section "colour of vertices" of vacancy_hip.h, restated in numpy in
// tests/color_ref.py).
//
// One function, cl::add_view, holds the arithmetic of one (vertex, view) pair -- the carve's projection, ROI test and
// samplers (carve_common.h:54-105) term for term, the depth test, the weight -- and is compiled for the host and for the
// device; the library's flags (no FMA contraction, correctly rounded division and square root, denormals kept) make the two
// agree to the bit.
//
// The device path, all on the context's stream, per chunk of up to 64 views:
//   1. depth        uploaded as given, or ray-cast by render.hip and left in its device buffer (render_depth_device)
//   2. cl_pack      the photographs, uploaded as they are (3 bytes per texel), become one dword per texel (RGBX): a tap
//                   is one load instead of three
//   3. cl_color     one lane per vertex, the view loop inside the lane: sums run in ascending view index without atomics
//                   or sorting.  The view records are read with a wave-uniform index (scalar loads); the accumulators
//                   stay in registers and pass through memory only between the chunks of a call with more than 64 views.
// Per (vertex, view): about 40 flops against one depth dword and one (NN) or four (bilinear) gathered texels -- latency-
// and gather-bound; vertices of an extraction come in the raster order of their cells, so neighbouring lanes gather from
// neighbouring pixels, and the input is not reordered.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "vcy_internal.h"

namespace vcy {
namespace cl {

struct View {           // one per view of a launch, in device memory (host function: on the stack of its loop)
  float R[9], t[3];     // w2c
  float fx, fy, cx, cy;
  float rx0f, ry0f, rx1f, ry1f;  // (float)int, as the carve compares
  int rx0, ry0, rx1, ry1;
  int ortho, w;
  const uint8_t* rgb;    // host function: 3 bytes per texel
  const uint32_t* rgbx;  // device: r | g << 8 | b << 16
  const float* depth;
};

struct Acc {
  float s[3], w;     // S_c, W
  int n;             // n_used
  float w_best;
  int best_view;
  float best[3];
};

__host__ __device__ __forceinline__ void acc_init(Acc& a) {
  a.s[0] = a.s[1] = a.s[2] = a.w = 0.0f;
  a.n = 0;
  a.w_best = -1.0f;
  a.best_view = -1;
  a.best[0] = a.best[1] = a.best[2] = 0.0f;
}

template <bool PACKED>
__host__ __device__ __forceinline__ void texel(const View& v, int x, int y, float (&c)[3]) {
  const int64_t at = (int64_t)v.w * y + x;
  if (PACKED) {
    const uint32_t p = v.rgbx[at];
    c[0] = (float)(p & 0xffu), c[1] = (float)((p >> 8) & 0xffu), c[2] = (float)((p >> 16) & 0xffu);
  } else {
    const uint8_t* p = v.rgb + 3 * at;
    c[0] = (float)p[0], c[1] = (float)p[1], c[2] = (float)p[2];
  }
}

__host__ __device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// Steps 1 - 6 of the definition for view `index`.  nrm is not read in VCY_COLOR_MEAN.
template <int MODE, int INTERP, bool PACKED>
__host__ __device__ __forceinline__ void add_view(const View& v, int index, float tol, float min_cos, const float (&p)[3],
                                                  const float (&nrm)[3], Acc& a) {
  float pc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float c0 = v.R[3 * r + 0] * p[0];
    const float c1 = v.R[3 * r + 1] * p[1];
    const float c2 = v.R[3 * r + 2] * p[2];
    pc[r] = v.t[r] + (c0 + (c1 + c2));
  }
  if (pc[2] < 0.0f) return;
  float u, w;
  if (v.ortho) {
    u = pc[0];
    w = pc[1];
  } else {
    u = v.fx / pc[2] * pc[0] + v.cx;
    w = v.fy / pc[2] * pc[1] + v.cy;
  }
  const bool inside = u >= v.rx0f && w >= v.ry0f && u <= v.rx1f && w <= v.ry1f;  // (NaN: outside)
  if (!inside) return;
  // the carve's nearest pixel: where the depth is read, and the NN sample
  int xi = (int)roundf(u);
  int yi = (int)roundf(w);
  xi = imax(xi, v.rx0);
  yi = imax(yi, v.ry0);
  xi = imin(xi, v.rx1);
  yi = imin(yi, v.ry1);
  const float limit = v.depth[(int64_t)v.w * yi + xi] + tol;
  if (!(pc[2] <= limit)) return;

  float wt = 1.0f;
  if (MODE != VCY_COLOR_MEAN) {
    float cosv;
    float nc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float c0 = v.R[3 * r + 0] * nrm[0];
      const float c1 = v.R[3 * r + 1] * nrm[1];
      const float c2 = v.R[3 * r + 2] * nrm[2];
      nc[r] = c0 + (c1 + c2);
    }
    if (v.ortho) {
      cosv = nc[2];
    } else {
      const float q0 = pc[0] * pc[0], q1 = pc[1] * pc[1], q2 = pc[2] * pc[2];
      const float len = sqrtf((q0 + q1) + q2);
      const float d0 = nc[0] * pc[0], d1 = nc[1] * pc[1], d2 = nc[2] * pc[2];
      cosv = ((d0 + d1) + d2) / len;
    }
    wt = fabsf(cosv);
    if (!(wt > min_cos)) return;  // (a NaN weight never contributes)
  }

  float c[3];
  if (INTERP == VCY_INTERP_NN) {
    texel<PACKED>(v, xi, yi, c);
  } else {
    const float fu = floorf(u), fw = floorf(w);
    int x0 = (int)fu, y0 = (int)fw;
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = imax(x0, v.rx0);
    y0 = imax(y0, v.ry0);
    x1 = imin(x1, v.rx1);
    y1 = imin(y1, v.ry1);
    const float lu = u - (float)x0;
    const float lv = w - (float)y0;
    float s00[3], s10[3], s01[3], s11[3];
    texel<PACKED>(v, x0, y0, s00);
    texel<PACKED>(v, x1, y0, s10);
    texel<PACKED>(v, x0, y1, s01);
    texel<PACKED>(v, x1, y1, s11);
    const float k00 = (1.0f - lu) * (1.0f - lv), k10 = lu * (1.0f - lv), k01 = (1.0f - lu) * lv, k11 = lu * lv;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float e = k00 * s00[k];
      const float f = k10 * s10[k];
      const float g = k01 * s01[k];
      const float h = k11 * s11[k];
      c[k] = ((e + f) + g) + h;
    }
  }

#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float term = wt * c[k];
    a.s[k] += term;
  }
  a.w += wt;
  a.n += 1;
  if (wt > a.w_best) {
    a.w_best = wt;
    a.best_view = index;
    a.best[0] = c[0], a.best[1] = c[1], a.best[2] = c[2];
  }
}

template <int MODE>
__host__ __device__ __forceinline__ void result(const Acc& a, const float (&fallback)[3], float (&rgb)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) rgb[k] = a.n == 0 ? fallback[k] : (MODE == VCY_COLOR_BEST ? a.best[k] : a.s[k] / a.w);
}

struct Launch {
  int64_t n;              // vertices
  const float* vtx;       // 3 per vertex
  const float* nrm;       // 3 per vertex, null in VCY_COLOR_MEAN
  const View* views;
  int n_views, view0;     // the views of this launch are view0 .. view0 + n_views - 1 of the call
  float tol, min_cos;
  float fallback[3];
  int first, last;        // chunk of the call: the accumulators start here / the results are written here
  float* carry;           // 10 arrays of n dwords: the fields of Acc in their order (null when the call is one launch)
  float* rgb;
  int32_t* n_used;        // never null on the device
  int32_t* best_view;
};

constexpr int kCarryWords = 10;

template <int MODE, int INTERP>
__global__ __launch_bounds__(256) void cl_color_kernel(Launch L) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= L.n) return;
  const float p[3] = {L.vtx[3 * i], L.vtx[3 * i + 1], L.vtx[3 * i + 2]};
  float nrm[3] = {0.0f, 0.0f, 0.0f};
  if (MODE != VCY_COLOR_MEAN) nrm[0] = L.nrm[3 * i], nrm[1] = L.nrm[3 * i + 1], nrm[2] = L.nrm[3 * i + 2];
  Acc a;
  if (L.first) {
    acc_init(a);
  } else {
    const float* c = L.carry + i;
    a.s[0] = c[0], a.s[1] = c[L.n], a.s[2] = c[2 * L.n], a.w = c[3 * L.n];
    a.n = __float_as_int(c[4 * L.n]);
    a.w_best = c[5 * L.n];
    a.best_view = __float_as_int(c[6 * L.n]);
    a.best[0] = c[7 * L.n], a.best[1] = c[8 * L.n], a.best[2] = c[9 * L.n];
  }
  for (int k = 0; k < L.n_views; ++k)  // (k is uniform: the record is read once per wave)
    add_view<MODE, INTERP, true>(L.views[k], L.view0 + k, L.tol, L.min_cos, p, nrm, a);
  if (!L.last) {
    float* c = L.carry + i;
    c[0] = a.s[0], c[L.n] = a.s[1], c[2 * L.n] = a.s[2], c[3 * L.n] = a.w;
    c[4 * L.n] = __int_as_float(a.n);
    c[5 * L.n] = a.w_best;
    c[6 * L.n] = __int_as_float(a.best_view);
    c[7 * L.n] = a.best[0], c[8 * L.n] = a.best[1], c[9 * L.n] = a.best[2];
    return;
  }
  float rgb[3];
  result<MODE>(a, L.fallback, rgb);
  L.rgb[3 * i] = rgb[0], L.rgb[3 * i + 1] = rgb[1], L.rgb[3 * i + 2] = rgb[2];
  L.n_used[i] = a.n;
  L.best_view[i] = a.best_view;
}

struct PackJob {  // one per view of a launch
  const uint8_t* rgb;
  uint32_t* rgbx;
  int64_t n_px;
};

__global__ __launch_bounds__(256) void cl_pack_kernel(const PackJob* __restrict__ jobs) {
  const PackJob j = jobs[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (the launch is sized for the largest view)
  if (i >= j.n_px) return;
  const uint8_t* p = j.rgb + 3 * i;
  j.rgbx[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

constexpr int kMaxViewsPerLaunch = 64;  // (the ray-cast's: a chunk's depth images come from one launch of it)

void fill_view(const vcy_view& v, View* r) {
  for (int row = 0; row < 3; ++row) {
    for (int col = 0; col < 3; ++col) r->R[row * 3 + col] = v.w2c[row * 4 + col];
    r->t[row] = v.w2c[row * 4 + 3];
  }
  r->fx = v.fx, r->fy = v.fy, r->cx = v.cx, r->cy = v.cy;
  r->rx0 = v.roi_min[0], r->ry0 = v.roi_min[1], r->rx1 = v.roi_max[0], r->ry1 = v.roi_max[1];
  r->rx0f = (float)r->rx0, r->ry0f = (float)r->ry0, r->rx1f = (float)r->rx1, r->ry1f = (float)r->ry1;
  r->ortho = v.is_ortho != 0, r->w = v.width;
  r->rgb = nullptr, r->rgbx = nullptr, r->depth = nullptr;
}

}  // namespace cl

namespace {

// where the images of one view lie among those of its chunk: the photograph as given, RGBX, the depth image when the
// caller uploads one (the sizing of the pool and the chunk's copies both walk the views through this)
struct ImageSlots { size_t raw, rgbx, depth; };
ImageSlots take_images(PoolLayout& at, size_t px, bool with_depth) {
  return ImageSlots{at.take(3 * px), at.take(4 * px), with_depth ? at.take(4 * px) : 0};
}

// the checks the two entry points share; depth_required: the host function's
int check_args(const char* who, int64_t n_vertices, const float* vertices, const float* normals, int n_views,
               const vcy_view* views, const uint8_t* const* photos, const float* const* depth, bool depth_required,
               const vcy_color_option* o, const float* rgb_out) {
  if (n_vertices < 0 || n_views <= 0 || !views || !photos || !o || (depth_required && !depth) ||
      (n_vertices > 0 && (!vertices || !rgb_out))) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  if (o->mode != VCY_COLOR_MEAN && o->mode != VCY_COLOR_WEIGHTED && o->mode != VCY_COLOR_BEST) {
    set_error("%s: unknown mode %d", who, o->mode);
    return VCY_ERR_INVALID_ARG;
  }
  if (o->interp != VCY_INTERP_NN && o->interp != VCY_INTERP_BILINEAR) {
    set_error("%s: unknown interp %d", who, o->interp);
    return VCY_ERR_INVALID_ARG;
  }
  if (!(o->depth_tolerance >= 0.0f) || !std::isfinite(o->depth_tolerance) || !(o->min_cos >= 0.0f) || !std::isfinite(o->min_cos)) {
    set_error("%s: depth_tolerance and min_cos must be finite and >= 0 (%g, %g)", who, (double)o->depth_tolerance,
              (double)o->min_cos);
    return VCY_ERR_INVALID_ARG;
  }
  if (o->mode != VCY_COLOR_MEAN && !normals && n_vertices > 0) {
    set_error("%s: modes VCY_COLOR_WEIGHTED and VCY_COLOR_BEST need normals", who);
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_views; ++i) {
    const int rc = check_render_view(&views[i], i);
    if (rc != VCY_OK) return rc;
    if (!photos[i] || (depth && !depth[i])) {
      set_error("%s: view %d has no photograph or no depth image", who, i);
      return VCY_ERR_INVALID_ARG;
    }
  }
  return VCY_OK;
}

template <int MODE, int INTERP>
void color_host(int64_t n, const float* vertices, const float* normals, int n_views, const cl::View* views,
                const vcy_color_option& o, float* rgb_out, int32_t* n_used_out, int32_t* best_view_out) {
  const float fallback[3] = {o.fallback[0], o.fallback[1], o.fallback[2]};
  for (int64_t i = 0; i < n; ++i) {
    const float p[3] = {vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]};
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    if (MODE != VCY_COLOR_MEAN) nrm[0] = normals[3 * i], nrm[1] = normals[3 * i + 1], nrm[2] = normals[3 * i + 2];
    cl::Acc a;
    cl::acc_init(a);
    for (int k = 0; k < n_views; ++k) cl::add_view<MODE, INTERP, false>(views[k], k, o.depth_tolerance, o.min_cos, p, nrm, a);
    float rgb[3];
    cl::result<MODE>(a, fallback, rgb);
    rgb_out[3 * i] = rgb[0], rgb_out[3 * i + 1] = rgb[1], rgb_out[3 * i + 2] = rgb[2];
    if (n_used_out) n_used_out[i] = a.n;
    if (best_view_out) best_view_out[i] = a.best_view;
  }
}

// MODE x INTERP -> instance
#define VCY_CL_DISPATCH(mode, interp, CALL)                                                      \
  do {                                                                                           \
    if ((interp) == VCY_INTERP_NN) {                                                             \
      if ((mode) == VCY_COLOR_MEAN) { CALL(VCY_COLOR_MEAN, VCY_INTERP_NN); }                     \
      else if ((mode) == VCY_COLOR_WEIGHTED) { CALL(VCY_COLOR_WEIGHTED, VCY_INTERP_NN); }        \
      else { CALL(VCY_COLOR_BEST, VCY_INTERP_NN); }                                              \
    } else {                                                                                     \
      if ((mode) == VCY_COLOR_MEAN) { CALL(VCY_COLOR_MEAN, VCY_INTERP_BILINEAR); }               \
      else if ((mode) == VCY_COLOR_WEIGHTED) { CALL(VCY_COLOR_WEIGHTED, VCY_INTERP_BILINEAR); }  \
      else { CALL(VCY_COLOR_BEST, VCY_INTERP_BILINEAR); }                                        \
    }                                                                                            \
  } while (0)

int color_device(vcy_ctx* c, double iso, int64_t n, const float* vertices, const float* normals, int n_views,
                 const vcy_view* views, const uint8_t* const* photos, const float* const* depth, const vcy_color_option& o,
                 float* rgb_out, int32_t* n_used_out, int32_t* best_view_out) {
  VCY_HIP_CHECK(hipSetDevice(c->device));
  c->last_color_device_ms = 0.0f;
  VCY_HIP_CHECK(c->ev_cl_begin.ensure());
  VCY_HIP_CHECK(c->ev_cl_end.ensure());
  const bool with_normals = o.mode != VCY_COLOR_MEAN;
  const int n_chunks = (n_views + cl::kMaxViewsPerLaunch - 1) / cl::kMaxViewsPerLaunch;

  // [view records | pack jobs | vertices | normals | rgb | n_used | best_view | carry | per view of the largest chunk:
  //  photograph as given, RGBX, depth (when uploaded)]: sized once, so that what the first part holds outlives the chunks
  PoolLayout at;
  const size_t at_views = at.take(sizeof(cl::View) * cl::kMaxViewsPerLaunch),
               at_jobs = at.take(sizeof(cl::PackJob) * cl::kMaxViewsPerLaunch), at_vtx = at.take(sizeof(float) * 3 * (size_t)n),
               at_nrm = at.take(with_normals ? sizeof(float) * 3 * (size_t)n : 0), at_rgb = at.take(sizeof(float) * 3 * (size_t)n),
               at_used = at.take(sizeof(int32_t) * (size_t)n), at_best = at.take(sizeof(int32_t) * (size_t)n),
               at_carry = at.take(n_chunks > 1 ? sizeof(float) * cl::kCarryWords * (size_t)n : 0), at_images = at.total();
  size_t image_bytes = 0;
  for (int first = 0; first < n_views; first += cl::kMaxViewsPerLaunch) {
    PoolLayout images;
    for (int i = first; i < std::min(n_views, first + cl::kMaxViewsPerLaunch); ++i)
      (void)take_images(images, (size_t)views[i].width * (size_t)views[i].height, depth != nullptr);
    image_bytes = std::max(image_bytes, images.total());
  }
  VCY_HIP_CHECK(c->d_cl_buf.grow(at_images + image_bytes, c->stream, false));
  char* base = (char*)c->d_cl_buf;

  VCY_HIP_CHECK(hipMemcpyAsync(base + at_vtx, vertices, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  if (with_normals)
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_nrm, normals, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));

  cl::Launch L{};
  L.n = n;
  L.vtx = (const float*)(base + at_vtx);
  L.nrm = with_normals ? (const float*)(base + at_nrm) : nullptr;
  L.views = (const cl::View*)(base + at_views);
  L.tol = o.depth_tolerance, L.min_cos = o.min_cos;
  L.fallback[0] = o.fallback[0], L.fallback[1] = o.fallback[1], L.fallback[2] = o.fallback[2];
  L.carry = n_chunks > 1 ? (float*)(base + at_carry) : nullptr;
  L.rgb = (float*)(base + at_rgb);
  L.n_used = (int32_t*)(base + at_used);
  L.best_view = (int32_t*)(base + at_best);

  // One chunk.  Its copies read `rec`, `jobs` and the caller's images asynchronously until the wait at its end: a failure
  // in between is returned through the loop below, which waits before anything is destroyed.
  float render_ms = 0.0f;
  std::vector<cl::View> rec;
  std::vector<cl::PackJob> jobs;
  std::vector<const float*> depth_dev;
  auto chunk = [&](int first, float* ms_out) -> int {
    const int m = std::min(cl::kMaxViewsPerLaunch, n_views - first);
    rec.assign((size_t)m, cl::View{});
    jobs.assign((size_t)m, cl::PackJob{});
    depth_dev.assign((size_t)m, nullptr);
    if (!depth) {
      // (the ray-cast waits for its launch; its buffer is next written by the next chunk's, behind this chunk's wait)
      const int rc = render_depth_device(c, iso, m, views + first, depth_dev.data(), "vcy_color_vertices");
      if (rc != VCY_OK) return rc;
      render_ms += c->last_render_device_ms;
    }
    PoolLayout images;
    char* image_base = base + at_images;
    int64_t px_max = 0;
    for (int i = 0; i < m; ++i) {
      const vcy_view& v = views[first + i];
      const size_t px = (size_t)v.width * (size_t)v.height;
      cl::fill_view(v, &rec[(size_t)i]);
      const ImageSlots slots = take_images(images, px, depth != nullptr);
      uint8_t* raw = (uint8_t*)(image_base + slots.raw);
      uint32_t* rgbx = (uint32_t*)(image_base + slots.rgbx);
      VCY_HIP_CHECK(hipMemcpyAsync(raw, photos[first + i], 3 * px, hipMemcpyHostToDevice, c->stream));
      if (depth) {
        float* d = (float*)(image_base + slots.depth);
        VCY_HIP_CHECK(hipMemcpyAsync(d, depth[first + i], 4 * px, hipMemcpyHostToDevice, c->stream));
        depth_dev[(size_t)i] = d;
      }
      rec[(size_t)i].rgbx = rgbx;
      rec[(size_t)i].depth = depth_dev[(size_t)i];
      jobs[(size_t)i] = cl::PackJob{raw, rgbx, (int64_t)px};
      px_max = std::max(px_max, (int64_t)px);
    }
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_views, rec.data(), sizeof(cl::View) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_jobs, jobs.data(), sizeof(cl::PackJob) * (size_t)m, hipMemcpyHostToDevice, c->stream));

    VCY_HIP_CHECK(hipEventRecord(c->ev_cl_begin, c->stream));
    hipLaunchKernelGGL(cl::cl_pack_kernel, dim3((unsigned)((px_max + 255) / 256), (unsigned)m), dim3(256), 0, c->stream,
                       (const cl::PackJob*)(base + at_jobs));
    VCY_HIP_CHECK(hipGetLastError());
    L.n_views = m, L.view0 = first;
    L.first = first == 0, L.last = first + m == n_views;
    const dim3 grid((unsigned)((n + 255) / 256));
#define VCY_CL_LAUNCH(M, I) hipLaunchKernelGGL((cl::cl_color_kernel<M, I>), grid, dim3(256), 0, c->stream, L)
    VCY_CL_DISPATCH(o.mode, o.interp, VCY_CL_LAUNCH);
#undef VCY_CL_LAUNCH
    VCY_HIP_CHECK(hipGetLastError());
    VCY_HIP_CHECK(hipEventRecord(c->ev_cl_end, c->stream));
    if (L.last) {
      VCY_HIP_CHECK(hipMemcpyAsync(rgb_out, base + at_rgb, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
      if (n_used_out)
        VCY_HIP_CHECK(hipMemcpyAsync(n_used_out, base + at_used, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
      if (best_view_out)
        VCY_HIP_CHECK(hipMemcpyAsync(best_view_out, base + at_best, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    VCY_HIP_CHECK(hipStreamSynchronize(c->stream));  // (the host arrays above are read and written until here)
    VCY_HIP_CHECK(hipEventElapsedTime(ms_out, c->ev_cl_begin, c->ev_cl_end));
    return VCY_OK;
  };
  float ms_total = 0.0f;
  for (int first = 0; first < n_views; first += cl::kMaxViewsPerLaunch) {
    float ms = 0.0f;
    const int rc = chunk(first, &ms);
    if (rc != VCY_OK) {
      (void)hipStreamSynchronize(c->stream);  // (queued copies still name host memory of this call and of the caller)
      return rc;
    }
    ms_total += ms;
  }
  c->last_color_device_ms = ms_total;
  if (!depth) c->last_render_device_ms = render_ms;  // (of all chunks, not of the last)
  return VCY_OK;
}

}  // namespace

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_color_vertices_host(int64_t n_vertices, const float* vertices, const float* normals, int n_views,
                            const vcy_view* views, const uint8_t* const* photos, const float* const* depth,
                            const vcy_color_option* option, float* rgb_out, int32_t* n_used_out, int32_t* best_view_out) {
  { const int rc = check_args("vcy_color_vertices_host", n_vertices, vertices, normals, n_views, views, photos, depth, true, option, rgb_out); if (rc != VCY_OK) return rc; }
  if (n_vertices == 0) return VCY_OK;
  std::vector<cl::View> rec((size_t)n_views);
  for (int i = 0; i < n_views; ++i) {
    cl::fill_view(views[i], &rec[(size_t)i]);
    rec[(size_t)i].rgb = photos[i];
    rec[(size_t)i].depth = depth[i];
  }
#define VCY_CL_HOST(M, I) color_host<M, I>(n_vertices, vertices, normals, n_views, rec.data(), *option, rgb_out, n_used_out, best_view_out)
  VCY_CL_DISPATCH(option->mode, option->interp, VCY_CL_HOST);
#undef VCY_CL_HOST
  return VCY_OK;
}

int vcy_color_vertices(vcy_ctx* c, double iso_level, int64_t n_vertices, const float* vertices, const float* normals,
                       int n_views, const vcy_view* views, const uint8_t* const* photos_host, const float* const* depth_host,
                       const vcy_color_option* option, float* rgb_out, int32_t* n_used_out, int32_t* best_view_out) {
  { const int rc = check_args("vcy_color_vertices", n_vertices, vertices, normals, n_views, views, photos_host, depth_host, false, option, rgb_out); if (rc != VCY_OK) return rc; }
  if (!c) {  // (behind the argument checks: those need no context)
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!depth_host && !(c->z0 == 0 && c->z1 == c->nz && c->halo_lo == 0)) {
    set_error("vcy_color_vertices: the context owns z [%d, %d) of %d slices; without depth images the hull is ray-cast here, "
              "which needs the whole grid in one context (a z-slab passes the merged depth of vcy_render_merge_host)",
              c->z0, c->z1, c->nz);
    return VCY_ERR_UNSUPPORTED;
  }
  if (n_vertices == 0) return VCY_OK;
  return color_device(c, iso_level, n_vertices, vertices, normals, n_views, views, photos_host, depth_host, *option, rgb_out,
                      n_used_out, best_view_out);
}

int vcy_last_color_ms(const vcy_ctx* c, float* device_ms) {
  if (!c || !device_ms) return VCY_ERR_INVALID_ARG;
  *device_ms = c->last_color_device_ms;
  return VCY_OK;
}

}  // extern "C"
