// K-smooth: Taubin smoothing of an indexed mesh and Mesh::CalcNormal of the result, on the device (vcy_smooth_mesh; the
// definition is the section "mesh smoothing" of vacancy_hip.h, the serial statement mesh_smooth_host.hip).
//
// All launches go to the context's stream with no host wait between them, in three groups:
//   build    the vertex -> incident-corner table of the mesh: sm_count (one thread per corner, integer atomicAdd into
//            deg[v] -- counts do not depend on the order of the adds), the exclusive scan of mc_kernels.hip over the
//            n_vertices + 1 entries (row offsets), sm_fill (one thread per corner takes a slot of its vertex's row with an
//            atomicAdd on a cursor -- slots come out in arbitrary order), sm_rows (one thread per vertex sorts its row
//            ascending: the canonical row of the definition whatever order the atomics ran in; then writes the flat gather
//            row -- the two other vertices of every corner, in row order -- and the pinned flag).
//   passes   sm_pass, one lane per vertex, the row loop inside the lane: the sum of the definition in its order, in
//            registers, no atomics.  Positions ping-pong between two arrays; a pass follows one indirection (gather row ->
//            position).  Vertices of an extraction are numbered in cell raster order, so a row's ids are near v and the
//            gathers mostly hit L2; the mesh is not reordered.
//   normals  sm_face_normals (one thread per face, face_normal.h's Mesh::CalcFaceNormal), sm_vertex_normals (one lane per
//            vertex sums the face normals of its row in row order, divides by the row length, normalises).
// No float atomics anywhere.  "smoothpad" 1 keeps the positions of the passes at 16 bytes per vertex (one dwordx4
// gather) instead of 12 (three dword gathers); the results are the same bits.
#include <algorithm>
#include <climits>
#include <cstring>

#include "face_normal.h"
#include "mesh_rows.h"
#include "vcy_internal.h"

namespace vcy {
namespace sm {

typedef unsigned long long u64;

constexpr int kShortRow = 12;  // corners a row is sorted with in registers (a marching-cubes row holds 4 - 12)

struct Table {
  int n, nc;            // vertices, corners (3 * faces)
  const int* faces;
  u64* deg;             // [n + 1] counts, scanned in place
  int* off;             // [n + 1] row offsets
  int* cursor;          // [n]
  int* corners;         // [nc] rows of corner ids 3f + j
  int* gather;          // [2 * nc] rows of vertex ids
  uint8_t* pinned;      // [n]
};

__global__ __launch_bounds__(256) void sm_count_kernel(Table t) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= t.nc) return;
  atomicAdd(&t.deg[t.faces[c]], 1ull);
}

__global__ __launch_bounds__(256) void sm_offsets_kernel(Table t) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v > t.n) return;
  const int o = (int)t.deg[v];
  t.off[v] = o;
  if (v < t.n) t.cursor[v] = o;
}

__global__ __launch_bounds__(256) void sm_fill_kernel(Table t) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= t.nc) return;
  const int slot = atomicAdd(&t.cursor[t.faces[c]], 1);  // (< off[v + 1]: the row has a slot per corner counted)
  t.corners[slot] = (int)c;
}

// the two ids a pass gathers for corner c = 3f + j: faces[3f + (j+1)%3], faces[3f + (j+2)%3]
__device__ __forceinline__ void corner_others(const int* __restrict__ faces, int c, int* a, int* b) {
  const int f = c / 3, j = c - 3 * f;
  const int j1 = j == 2 ? 0 : j + 1, j2 = j == 0 ? 2 : j - 1;
  *a = faces[3 * f + j1];
  *b = faces[3 * f + j2];
}

template <bool PIN>
__global__ __launch_bounds__(256) void sm_rows_kernel(Table t) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= t.n) return;
  const int b = t.off[v], len = t.off[v + 1] - b;
  int* row = t.corners + b;
  int* grow = t.gather + 2 * (int64_t)b;
  bool pin = false;
  if (len <= kShortRow) {
    int r[kShortRow];
#pragma unroll
    for (int k = 0; k < kShortRow; ++k) r[k] = k < len ? row[k] : INT_MAX;
    // odd-even transposition sort: kShortRow rounds, every index static
#pragma unroll
    for (int round = 0; round < kShortRow; ++round) {
#pragma unroll
      for (int i = round & 1; i + 1 < kShortRow; i += 2) {
        const int lo = min(r[i], r[i + 1]), hi = max(r[i], r[i + 1]);
        r[i] = lo;
        r[i + 1] = hi;
      }
    }
    int g[2 * kShortRow];
#pragma unroll
    for (int k = 0; k < kShortRow; ++k) {
      g[2 * k] = g[2 * k + 1] = (int)v;  // (padding: v itself never pins)
      if (k < len) {
        row[k] = r[k];
        corner_others(t.faces, r[k], &g[2 * k], &g[2 * k + 1]);
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
    heap_sort(row, len);
    for (int k = 0; k < len; ++k) corner_others(t.faces, row[k], &grow[2 * k], &grow[2 * k + 1]);
    if (PIN) {
      heap_sort(grow, 2 * len);  // (the ids in ascending order: a run of one is an edge that one face uses)
      for (int k = 0; k < 2 * len; ++k) {
        const int id = grow[k];
        const bool single = (k == 0 || grow[k - 1] != id) && (k + 1 == 2 * len || grow[k + 1] != id);
        pin = pin || (single && id != (int)v);
      }
      for (int k = 0; k < len; ++k) corner_others(t.faces, row[k], &grow[2 * k], &grow[2 * k + 1]);
    }
  }
  t.pinned[v] = pin ? 1 : 0;
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

// ---- normals ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sm_face_normals_kernel(int nf, const int* __restrict__ faces,
                                                              const float* __restrict__ verts, float* __restrict__ fn_out) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int i0 = faces[3 * f + 0], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  float q[3][3], fn[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    q[0][k] = verts[3 * (int64_t)i0 + k];
    q[1][k] = verts[3 * (int64_t)i1 + k];
    q[2][k] = verts[3 * (int64_t)i2 + k];
  }
  mc::face_normal(q[0], q[1], q[2], fn);
  fn_out[3 * f + 0] = fn[0];
  fn_out[3 * f + 1] = fn[1];
  fn_out[3 * f + 2] = fn[2];
}

// Mesh::CalcNormal (mesh.cc:213-221): the row is the order in which the serial walk meets the vertex
__global__ __launch_bounds__(256) void sm_vertex_normals_kernel(int n, const int* __restrict__ off,
                                                                const int* __restrict__ corners,
                                                                const float* __restrict__ fn, float* __restrict__ vn) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int b = off[v], e = off[v + 1];
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int k = b; k < e; ++k) {
    const int64_t f = corners[k] / 3;
    acc[0] += fn[3 * f + 0];
    acc[1] += fn[3 * f + 1];
    acc[2] += fn[3 * f + 2];
  }
  const float d = (float)(e - b);  // (a vertex no face names: 0 / 0, as in the reference)
  acc[0] = acc[0] / d;
  acc[1] = acc[1] / d;
  acc[2] = acc[2] / d;
  mc::normalize3(acc);
  vn[3 * v + 0] = acc[0];
  vn[3 * v + 1] = acc[1];
  vn[3 * v + 2] = acc[2];
}

}  // namespace sm

namespace {

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The vertex -> incident-corner table of t.faces: counts, row offsets, rows sorted ascending, gather rows, pinned flags.
// `total`: one word, `scratch`: the scan's chunk sums, ((n + 1) / 1024 + 64) * 2 words.
int build_table(hipStream_t s, const sm::Table& t, sm::u64* total, sm::u64* scratch, bool pin) {
  const size_t n = (size_t)t.n, nc = (size_t)t.nc;
  const dim3 blk(256), grid_v((unsigned)((n + 255) / 256)), grid_v1((unsigned)((n + 256) / 256)), grid_c((unsigned)((nc + 255) / 256));
  VCY_HIP_CHECK(hipMemsetAsync(t.deg, 0, 8 * (n + 1), s));
  if (nc > 0) hipLaunchKernelGGL(sm::sm_count_kernel, grid_c, blk, 0, s, t);
  VCY_HIP_CHECK(hipGetLastError());
  { const int rc = device_exclusive_scan_u64(t.deg, (int64_t)n + 1, total, scratch, s); if (rc != VCY_OK) return rc; }
  hipLaunchKernelGGL(sm::sm_offsets_kernel, grid_v1, blk, 0, s, t);
  if (nc > 0) hipLaunchKernelGGL(sm::sm_fill_kernel, grid_c, blk, 0, s, t);
  if (pin) hipLaunchKernelGGL(sm::sm_rows_kernel<true>, grid_v, blk, 0, s, t);
  else hipLaunchKernelGGL(sm::sm_rows_kernel<false>, grid_v, blk, 0, s, t);
  VCY_HIP_CHECK(hipGetLastError());
  return VCY_OK;
}

// Mesh::CalcNormal of (verts, t.faces) through the table: face normals into fn, vertex normals into vn unless it is null.
int launch_normals(hipStream_t s, const sm::Table& t, const float* verts, float* fn, float* vn) {
  const size_t n = (size_t)t.n, nf = (size_t)t.nc / 3;
  const dim3 blk(256), grid_v((unsigned)((n + 255) / 256)), grid_f((unsigned)((nf + 255) / 256));
  if (nf > 0) hipLaunchKernelGGL(sm::sm_face_normals_kernel, grid_f, blk, 0, s, (int)nf, t.faces, verts, fn);
  if (vn) hipLaunchKernelGGL(sm::sm_vertex_normals_kernel, grid_v, blk, 0, s, (int)n, t.off, t.corners, fn, vn);
  VCY_HIP_CHECK(hipGetLastError());
  return VCY_OK;
}

int smooth_device(vcy_ctx* c, int64_t n64, int64_t nf64, const float* vertices, const int32_t* faces,
                  const vcy_smooth_option& o, float* vertices_out, float* vertex_normals_out, float* face_normals_out) {
  VCY_HIP_CHECK(hipSetDevice(c->device));
  for (vcy::Event& e : c->ev_sm) VCY_HIP_CHECK(e.ensure());
  const size_t n = (size_t)n64, nf = (size_t)nf64, nc = 3 * nf;
  const bool normals = vertex_normals_out || face_normals_out;
  const int n_passes = 2 * o.iterations;
  const bool pad = c->smooth_pad != 0 && n_passes > 0;
  const size_t stride = pad ? 4 : 3;

  // [faces | positions as given (and the result) | the passes' arrays | deg, scan scratch, total | off | cursor | corners |
  //  gather | pinned | face normals | vertex normals]
  const size_t at_faces = 0;
  const size_t at_p3 = at_faces + align256(4 * nc);
  const size_t at_a = at_p3 + align256(12 * n);   // (pad only; otherwise the passes start from p3)
  const size_t at_b = at_a + (pad ? align256(16 * n) : 0);
  const size_t at_deg = at_b + align256(4 * stride * n);
  const size_t scan_words = ((n + 1) / 1024 + 64) * 2;
  const size_t at_scan = at_deg + align256(8 * (n + 1));
  const size_t at_total = at_scan + align256(8 * scan_words);
  const size_t at_off = at_total + 256;
  const size_t at_cursor = at_off + align256(4 * (n + 1));
  const size_t at_corners = at_cursor + align256(4 * n);
  const size_t at_gather = at_corners + align256(4 * nc);
  const size_t at_pinned = at_gather + align256(8 * nc);
  const size_t at_fn = at_pinned + align256(n);
  const size_t at_vn = at_fn + (normals ? align256(12 * nf) : 0);
  const size_t total = at_vn + (normals ? align256(12 * n) : 0);
  VCY_HIP_CHECK(c->d_sm_buf.grow(total, c->stream));
  char* base = (char*)c->d_sm_buf;
  hipStream_t s = c->stream;

  sm::Table t{};
  t.n = (int)n, t.nc = (int)nc;
  t.faces = (const int*)(base + at_faces);
  t.deg = (sm::u64*)(base + at_deg);
  t.off = (int*)(base + at_off);
  t.cursor = (int*)(base + at_cursor);
  t.corners = (int*)(base + at_corners);
  t.gather = (int*)(base + at_gather);
  t.pinned = (uint8_t*)(base + at_pinned);
  float* p3 = (float*)(base + at_p3);

  VCY_HIP_CHECK(hipMemcpyAsync(p3, vertices, 12 * n, hipMemcpyHostToDevice, s));
  if (nc > 0) VCY_HIP_CHECK(hipMemcpyAsync(base + at_faces, faces, 4 * nc, hipMemcpyHostToDevice, s));

  const dim3 blk(256), grid_v((unsigned)((n + 255) / 256)), grid_v1((unsigned)((n + 256) / 256)),
      grid_c((unsigned)((nc + 255) / 256)), grid_f((unsigned)((nf + 255) / 256));

  // ---- build
  VCY_HIP_CHECK(hipEventRecord(c->ev_sm[0], s));
  { const int rc = build_table(s, t, (sm::u64*)(base + at_total), (sm::u64*)(base + at_scan), o.pin_boundary != 0); if (rc != VCY_OK) return rc; }

  // ---- passes: lambda, mu, lambda, mu ... from `src` to `dst` and back; an even number of them ends where it began
  VCY_HIP_CHECK(hipEventRecord(c->ev_sm[1], s));
  float* src = pad ? (float*)(base + at_a) : p3;
  float* dst = (float*)(base + at_b);
  if (pad) hipLaunchKernelGGL(sm::sm_pad_kernel, grid_v, blk, 0, s, (int)n, p3, src);
  for (int pass = 0; pass < n_passes; ++pass) {
    const float f = (pass & 1) ? o.mu : o.lambda;
    if (pad) hipLaunchKernelGGL(sm::sm_pass_kernel<4>, grid_v, blk, 0, s, (int)n, t.off, t.gather, t.pinned, src, dst, f);
    else hipLaunchKernelGGL(sm::sm_pass_kernel<3>, grid_v, blk, 0, s, (int)n, t.off, t.gather, t.pinned, src, dst, f);
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
  if (normals) { const int rc = launch_normals(s, t, p3, fn, vertex_normals_out ? vn : nullptr); if (rc != VCY_OK) return rc; }
  VCY_HIP_CHECK(hipEventRecord(c->ev_sm[3], s));

  VCY_HIP_CHECK(hipMemcpyAsync(vertices_out, p3, 12 * n, hipMemcpyDeviceToHost, s));
  if (vertex_normals_out) VCY_HIP_CHECK(hipMemcpyAsync(vertex_normals_out, vn, 12 * n, hipMemcpyDeviceToHost, s));
  if (face_normals_out && nf > 0) VCY_HIP_CHECK(hipMemcpyAsync(face_normals_out, fn, 12 * nf, hipMemcpyDeviceToHost, s));
  VCY_HIP_CHECK(hipStreamSynchronize(s));  // (the host arrays are read and written until here)
  for (int k = 0; k < 3; ++k) VCY_HIP_CHECK(hipEventElapsedTime(&c->last_smooth_ms[k], c->ev_sm[k], c->ev_sm[k + 1]));
  if (!normals) c->last_smooth_ms[2] = 0.0f;
  return VCY_OK;
}

}  // namespace

// Mesh::CalcNormal of a mesh that lies in device memory, for the other mesh operators (mesh_decimate.hip): the table and
// the normals in the smoothing's pool (vcy_ctx::d_sm_buf), launched on the context's stream, not waited for.
int mesh_normals_device(vcy_ctx* c, int64_t n64, int64_t nf64, const float* d_vertices, const int32_t* d_faces, bool vertex_normals,
                        float** d_face_normals, float** d_vertex_normals) {
  const size_t n = (size_t)n64, nf = (size_t)nf64, nc = 3 * nf;
  const size_t scan_words = ((n + 1) / 1024 + 64) * 2;
  const size_t at_deg = 0;
  const size_t at_scan = at_deg + align256(8 * (n + 1));
  const size_t at_total = at_scan + align256(8 * scan_words);
  const size_t at_off = at_total + 256;
  const size_t at_cursor = at_off + align256(4 * (n + 1));
  const size_t at_corners = at_cursor + align256(4 * n);
  const size_t at_gather = at_corners + align256(4 * nc);
  const size_t at_pinned = at_gather + align256(8 * nc);
  const size_t at_fn = at_pinned + align256(n);
  const size_t at_vn = at_fn + align256(12 * nf);
  const size_t total = at_vn + align256(12 * n);
  VCY_HIP_CHECK(c->d_sm_buf.grow(total, c->stream));
  char* base = (char*)c->d_sm_buf;
  sm::Table t{};
  t.n = (int)n, t.nc = (int)nc;
  t.faces = d_faces;
  t.deg = (sm::u64*)(base + at_deg);
  t.off = (int*)(base + at_off);
  t.cursor = (int*)(base + at_cursor);
  t.corners = (int*)(base + at_corners);
  t.gather = (int*)(base + at_gather);
  t.pinned = (uint8_t*)(base + at_pinned);
  *d_face_normals = (float*)(base + at_fn);
  *d_vertex_normals = (float*)(base + at_vn);
  if (vertex_normals) { const int rc = build_table(c->stream, t, (sm::u64*)(base + at_total), (sm::u64*)(base + at_scan), false); if (rc != VCY_OK) return rc; }
  return launch_normals(c->stream, t, d_vertices, *d_face_normals, vertex_normals ? *d_vertex_normals : nullptr);
}

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
