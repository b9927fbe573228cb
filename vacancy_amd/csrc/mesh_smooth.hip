// K-smooth: Taubin smoothing of an indexed mesh and Mesh::CalcNormal of the result, on the device (vcy_smooth_mesh; the
// definition is the section "mesh smoothing" of vacancy_hip.h, the serial statement mesh_smooth_host.hip).
//
// All launches go to the context's stream with no host wait between them, in three groups:
//   build    the vertex -> incident-corner table of the mesh: mesh_rows.h's row table of the corners by faces[c] (count,
//            scan, offsets, fill), then sm_rows (one thread per vertex sorts its row ascending: the canonical row of the
//            definition whatever order the atomics ran in; then writes the flat gather row -- the two other vertices of
//            every corner, in row order -- and the pinned flag).
//   passes   sm_pass, one lane per vertex, the row loop inside the lane: the sum of the definition in its order, in
//            registers, no atomics.  Positions ping-pong between two arrays; a pass follows one indirection (gather row ->
//            position).  Vertices of an extraction are numbered in cell raster order, so a row's ids are near v and the
//            gathers mostly hit L2; the mesh is not reordered.
//   normals  mesh_normals.hip's two kernels, through the table built above.
// No float atomics anywhere.  "smoothpad" 1 keeps the positions of the passes at 16 bytes per vertex (one dwordx4
// gather) instead of 12 (three dword gathers); the results are the same bits.
#include <algorithm>

#include "mesh_ops.h"
#include "mesh_rows.h"
#include "vcy_internal.h"

namespace vcy {
namespace sm {

constexpr int kShortRow = 12;  // corners a row is sorted with in registers (a marching-cubes row holds 4 - 12)

// the two ids a pass gathers for corner c = 3f + j: faces[3f + (j+1)%3], faces[3f + (j+2)%3]
__device__ __forceinline__ void corner_others(const int* __restrict__ faces, int c, int* a, int* b) {
  const int f = c / 3, j = c - 3 * f;
  const int j1 = j == 2 ? 0 : j + 1, j2 = j == 0 ? 2 : j - 1;
  *a = faces[3 * f + j1];
  *b = faces[3 * f + j2];
}

// t: the corners 3f + j by vertex faces[3f + j], filled; gather: [2 * corners] rows of vertex ids; pinned: [vertices]
template <bool PIN>
__global__ __launch_bounds__(256) void sm_rows_kernel(rows::Table t, int* gather, uint8_t* pinned) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= t.n_rows) return;
  const int* faces = t.key;
  const int b = t.off[v], len = t.off[v + 1] - b;
  int* row = t.items + b;
  int* grow = gather + 2 * (int64_t)b;
  bool pin = false;
  if (len <= kShortRow) {
    int r[kShortRow];
    rows::load_sorted<kShortRow>(row, len, r);
    int g[2 * kShortRow];
#pragma unroll
    for (int k = 0; k < kShortRow; ++k) {
      g[2 * k] = g[2 * k + 1] = (int)v;  // (padding: v itself never pins)
      if (k < len) {
        row[k] = r[k];
        corner_others(faces, r[k], &g[2 * k], &g[2 * k + 1]);
        *reinterpret_cast<int2*>(grow + 2 * k) = make_int2(g[2 * k], g[2 * k + 1]);
      }
    }
    if (PIN) {
#pragma unroll
      for (int i = 0; i < 2 * kShortRow; ++i) {
        int same = 0;
#pragma unroll
        for (int j = 0; j < 2 * kShortRow; ++j) same += g[j] == g[i] ? 1 : 0;
        pin = pin || (same == 1 && g[i] != (int)v);
      }
    }
  } else {
    // a long row (a fan): sorted in place in global memory by this thread; correct, not fast
    rows::heap_sort(row, len);
    for (int k = 0; k < len; ++k) corner_others(faces, row[k], &grow[2 * k], &grow[2 * k + 1]);
    if (PIN) {
      rows::heap_sort(grow, 2 * len);  // (the ids in ascending order: a run of one is an edge that one face uses)
      for (int k = 0; k < 2 * len; ++k) {
        const int id = grow[k];
        const bool single = (k == 0 || grow[k - 1] != id) && (k + 1 == 2 * len || grow[k + 1] != id);
        pin = pin || (single && id != (int)v);
      }
      for (int k = 0; k < len; ++k) corner_others(faces, row[k], &grow[2 * k], &grow[2 * k + 1]);
    }
  }
  pinned[v] = pin ? 1 : 0;
}

// ---- one pass ------------------------------------------------------------------------------------------------
template <int STRIDE>
__device__ __forceinline__ void load_pos(const float* __restrict__ p, int64_t v, float (&o)[3]) {
  if (STRIDE == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + 4 * v);
    o[0] = q.x, o[1] = q.y, o[2] = q.z;
  } else {
    o[0] = p[3 * v], o[1] = p[3 * v + 1], o[2] = p[3 * v + 2];
  }
}

template <int STRIDE>
__global__ __launch_bounds__(256) void sm_pass_kernel(int n, const int* __restrict__ off, const int* __restrict__ gather,
                                                      const uint8_t* __restrict__ pinned, const float* __restrict__ p,
                                                      float* __restrict__ q, float s) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int b = off[v], e = off[v + 1];
  float pv[3];
  load_pos<STRIDE>(p, v, pv);
  float out[3] = {pv[0], pv[1], pv[2]};
  if (b != e && !pinned[v]) {
    float sum[3] = {0.0f, 0.0f, 0.0f};
    const int2* g = reinterpret_cast<const int2*>(gather) + b;  // one corner: the two ids behind it
    int k = 0;
    const int len = e - b;
    for (; k + 2 <= len; k += 2) {  // four independent gathers in flight, added in row order
      const int2 i0 = g[k], i1 = g[k + 1];
      float a0[3], a1[3], a2[3], a3[3];
      load_pos<STRIDE>(p, i0.x, a0);
      load_pos<STRIDE>(p, i0.y, a1);
      load_pos<STRIDE>(p, i1.x, a2);
      load_pos<STRIDE>(p, i1.y, a3);
#pragma unroll
      for (int c = 0; c < 3; ++c) sum[c] = ((sum[c] + a0[c]) + a1[c]) + a2[c], sum[c] = sum[c] + a3[c];
    }
    if (k < len) {
      const int2 i0 = g[k];
      float a0[3], a1[3];
      load_pos<STRIDE>(p, i0.x, a0);
      load_pos<STRIDE>(p, i0.y, a1);
#pragma unroll
      for (int c = 0; c < 3; ++c) sum[c] = (sum[c] + a0[c]) + a1[c];
    }
    const float cnt = (float)(2 * (int64_t)len);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float m = sum[c] / cnt;
      const float d = m - pv[c];
      const float t = s * d;
      out[c] = pv[c] + t;
    }
  }
  if (STRIDE == 4) {
    *reinterpret_cast<float4*>(q + 4 * v) = make_float4(out[0], out[1], out[2], 0.0f);
  } else {
    q[3 * v] = out[0], q[3 * v + 1] = out[1], q[3 * v + 2] = out[2];
  }
}

// 12-byte positions <-> 16-byte positions
__global__ __launch_bounds__(256) void sm_pad_kernel(int n, const float* __restrict__ p3, float* __restrict__ p4) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  *reinterpret_cast<float4*>(p4 + 4 * v) = make_float4(p3[3 * v], p3[3 * v + 1], p3[3 * v + 2], 0.0f);
}
__global__ __launch_bounds__(256) void sm_unpad_kernel(int n, const float* __restrict__ p4, float* __restrict__ p3) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const float4 q = *reinterpret_cast<const float4*>(p4 + 4 * v);
  p3[3 * v] = q.x, p3[3 * v + 1] = q.y, p3[3 * v + 2] = q.z;
}

}  // namespace sm

// The pool, the input into it, and every launch: see mesh_ops.h.  With the caller's host arrays the layout and the launches
// are what vcy_smooth_mesh has always had; a mesh on the device brings its faces and its table, which take no room here.
int smooth_launch(vcy_ctx* c, int64_t n64, int64_t nf64, const float* vertices, const int32_t* faces, const SmoothInput* in,
                  const vcy_smooth_option& o, bool vertex_normals, bool face_normals, SmoothResult* res) {
  VCY_HIP_CHECK(hipSetDevice(c->device));
  for (vcy::Event& e : c->ev_sm) VCY_HIP_CHECK(e.ensure());
  const size_t n = (size_t)n64, nf = (size_t)nf64, nc = 3 * nf;
  const bool normals = vertex_normals || face_normals;
  const int n_passes = 2 * o.iterations;
  const bool pad = c->smooth_pad != 0 && n_passes > 0;
  const size_t stride = pad ? 4 : 3;
  const bool own = in == nullptr;  // (faces and table in this pool)

  // [faces | positions as given (and the result) | the passes' arrays | deg, scan scratch, total | off | cursor | corners |
  //  gather | pinned | face normals | vertex normals]
  PoolLayout at;
  const size_t at_faces = at.take(own ? 4 * nc : 0), at_p3 = at.take(12 * n),
               at_a = at.take(pad ? 16 * n : 0),  // (pad only; otherwise the passes start from p3)
               at_b = at.take(4 * stride * n), at_deg = at.take(own ? 8 * (n + 1) : 0),
               at_scan = at.take(own ? 8 * scan_scratch_words(n + 1) : 0), at_total = at.take(own ? 8 : 0),
               at_off = at.take(own ? 4 * (n + 1) : 0), at_cursor = at.take(own ? 4 * n : 0), at_corners = at.take(own ? 4 * nc : 0),
               at_gather = at.take(8 * nc), at_pinned = at.take(n), at_fn = at.take(normals ? 12 * nf : 0),
               at_vn = at.take(normals ? 12 * n : 0);
  VCY_HIP_CHECK(c->d_sm_buf.grow(at.total(), c->stream));
  char* base = (char*)c->d_sm_buf;
  hipStream_t s = c->stream;

  const rows::Table t = own ? rows::Table{(int)n, (int)nc, (const int*)(base + at_faces), (rows::u64*)(base + at_deg),
                                          (int*)(base + at_off), (int*)(base + at_cursor), (int*)(base + at_corners)}
                            : *in->table;
  int* gather = (int*)(base + at_gather);
  uint8_t* pinned = (uint8_t*)(base + at_pinned);
  float* p3 = (float*)(base + at_p3);

  if (own) {
    VCY_HIP_CHECK(hipMemcpyAsync(p3, vertices, 12 * n, hipMemcpyHostToDevice, s));
    if (nc > 0) VCY_HIP_CHECK(hipMemcpyAsync(base + at_faces, faces, 4 * nc, hipMemcpyHostToDevice, s));
  } else {
    VCY_HIP_CHECK(hipMemcpyAsync(p3, in->vertices, 12 * n, hipMemcpyDeviceToDevice, s));
  }

  const dim3 blk(256), grid_v((unsigned)((n + 255) / 256));

  // ---- build
  VCY_HIP_CHECK(hipEventRecord(c->ev_sm[0], s));
  if (own) { const int rc = rows::fill(s, t, (rows::u64*)(base + at_total), (rows::u64*)(base + at_scan)); if (rc != VCY_OK) return rc; }
  if (o.pin_boundary) hipLaunchKernelGGL(sm::sm_rows_kernel<true>, grid_v, blk, 0, s, t, gather, pinned);
  else hipLaunchKernelGGL(sm::sm_rows_kernel<false>, grid_v, blk, 0, s, t, gather, pinned);
  VCY_HIP_CHECK(hipGetLastError());

  // ---- passes: lambda, mu, lambda, mu ... from `src` to `dst` and back; an even number of them ends where it began
  VCY_HIP_CHECK(hipEventRecord(c->ev_sm[1], s));
  float* src = pad ? (float*)(base + at_a) : p3;
  float* dst = (float*)(base + at_b);
  if (pad) hipLaunchKernelGGL(sm::sm_pad_kernel, grid_v, blk, 0, s, (int)n, p3, src);
  for (int pass = 0; pass < n_passes; ++pass) {
    const float f = (pass & 1) ? o.mu : o.lambda;
    if (pad) hipLaunchKernelGGL(sm::sm_pass_kernel<4>, grid_v, blk, 0, s, (int)n, t.off, gather, pinned, src, dst, f);
    else hipLaunchKernelGGL(sm::sm_pass_kernel<3>, grid_v, blk, 0, s, (int)n, t.off, gather, pinned, src, dst, f);
    std::swap(src, dst);
  }
  // (the result is in `src`)
  if (pad) hipLaunchKernelGGL(sm::sm_unpad_kernel, grid_v, blk, 0, s, (int)n, src, p3);
  else if (src != p3) VCY_HIP_CHECK(hipMemcpyAsync(p3, src, 12 * n, hipMemcpyDeviceToDevice, s));
  VCY_HIP_CHECK(hipGetLastError());

  // ---- normals
  VCY_HIP_CHECK(hipEventRecord(c->ev_sm[2], s));
  float* fn = (float*)(base + at_fn);
  float* vn = (float*)(base + at_vn);
  if (normals) { const int rc = launch_mesh_normals(s, n64, nf64, p3, t.key, t.off, t.items, fn, vertex_normals ? vn : nullptr); if (rc != VCY_OK) return rc; }
  VCY_HIP_CHECK(hipEventRecord(c->ev_sm[3], s));
  *res = SmoothResult{p3, normals ? fn : nullptr, vertex_normals ? vn : nullptr};
  return VCY_OK;
}

int smooth_read_times(vcy_ctx* c, bool normals) {
  for (int k = 0; k < 3; ++k) VCY_HIP_CHECK(hipEventElapsedTime(&c->last_smooth_ms[k], c->ev_sm[k], c->ev_sm[k + 1]));
  if (!normals) c->last_smooth_ms[2] = 0.0f;
  return VCY_OK;
}

namespace {

// vcy_smooth_mesh: the input from the caller's arrays into the pool, the launches, the results into the caller's arrays
int smooth_device(vcy_ctx* c, int64_t n64, int64_t nf64, const float* vertices, const int32_t* faces,
                  const vcy_smooth_option& o, float* vertices_out, float* vertex_normals_out, float* face_normals_out) {
  const size_t n = (size_t)n64, nf = (size_t)nf64;
  hipStream_t s = c->stream;
  SmoothResult r{};
  { const int rc = smooth_launch(c, n64, nf64, vertices, faces, nullptr, o, vertex_normals_out != nullptr, face_normals_out != nullptr, &r); if (rc != VCY_OK) return rc; }
  VCY_HIP_CHECK(hipMemcpyAsync(vertices_out, r.vertices, 12 * n, hipMemcpyDeviceToHost, s));
  if (vertex_normals_out) VCY_HIP_CHECK(hipMemcpyAsync(vertex_normals_out, r.vertex_normals, 12 * n, hipMemcpyDeviceToHost, s));
  if (face_normals_out && nf > 0) VCY_HIP_CHECK(hipMemcpyAsync(face_normals_out, r.face_normals, 12 * nf, hipMemcpyDeviceToHost, s));
  VCY_HIP_CHECK(hipStreamSynchronize(s));  // (the host arrays are read and written until here)
  return smooth_read_times(c, vertex_normals_out || face_normals_out);
}

}  // namespace

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_smooth_mesh(vcy_ctx* c, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                    const vcy_smooth_option* option, float* vertices_out, float* vertex_normals_out, float* face_normals_out) {
  { const int rc = smooth_check_args("vcy_smooth_mesh", n_vertices, n_faces, vertices, faces, option, vertices_out); if (rc != VCY_OK) return rc; }
  if (!c) {  // (behind the argument checks: those need no context)
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (n_vertices == 0) return VCY_OK;
  c->last_smooth_ms[0] = c->last_smooth_ms[1] = c->last_smooth_ms[2] = 0.0f;
  const int rc = smooth_device(c, n_vertices, n_faces, vertices, faces, *option, vertices_out, vertex_normals_out, face_normals_out);
  if (rc != VCY_OK) (void)hipStreamSynchronize(c->stream);  // (queued copies still name the caller's arrays)
  return rc;
}

int vcy_last_smooth_ms(const vcy_ctx* c, float* build_ms, float* passes_ms, float* normals_ms) {
  if (!c) return VCY_ERR_INVALID_ARG;
  if (build_ms) *build_ms = c->last_smooth_ms[0];
  if (passes_ms) *passes_ms = c->last_smooth_ms[1];
  if (normals_ms) *normals_ms = c->last_smooth_ms[2];
  return VCY_OK;
}

}  // extern "C"
