// Mesh::CalcNormal of an indexed mesh in device memory, for the mesh operators (mesh_smooth.hip, mesh_decimate.hip):
//   mn_face_normals    one thread per face, face_normal.h's Mesh::CalcFaceNormal;
//   mn_vertex_normals  one lane per vertex sums the face normals of its row of the vertex -> incident-corner table in row
//                      order (ascending corner, so ascending face: the order of the serial walk), divides by the row
//                      length, normalises.  No float atomics.
// The smoothing hands in the table it has built (launch_mesh_normals); mesh_normals_device builds the table of the mesh
// it is given -- mesh_rows.h's five steps, nothing else -- in a pool of its own (vcy_ctx::d_mn_buf).
#include "face_normal.h"
#include "mesh_rows.h"
#include "vcy_internal.h"

namespace vcy {

namespace {

constexpr int kShortRow = 12;  // corners a row is sorted with in registers (a marching-cubes row holds 4 - 12)

__global__ __launch_bounds__(256) void mn_face_normals_kernel(int nf, const int* __restrict__ faces,
                                                              const float* __restrict__ verts, float* __restrict__ fn_out) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int i0 = faces[3 * f + 0], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  float fn[3];
  mc::face_normal_of(verts, i0, i1, i2, fn);
  fn_out[3 * f + 0] = fn[0];
  fn_out[3 * f + 1] = fn[1];
  fn_out[3 * f + 2] = fn[2];
}

// Mesh::CalcNormal (mesh.cc:213-221): the row is the order in which the serial walk meets the vertex
__global__ __launch_bounds__(256) void mn_vertex_normals_kernel(int n, const int* __restrict__ off,
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

}  // namespace

// Face normals of (verts, faces) into fn; vertex normals into vn, unless it is null, through the sorted rows
// (off, corners) of the mesh's vertex -> incident-corner table.
int launch_mesh_normals(hipStream_t s, int64_t n, int64_t nf, const float* verts, const int32_t* faces, const int* off,
                        const int* corners, float* fn, float* vn) {
  const dim3 blk(256), grid_v((unsigned)((n + 255) / 256)), grid_f((unsigned)((nf + 255) / 256));
  if (nf > 0) hipLaunchKernelGGL(mn_face_normals_kernel, grid_f, blk, 0, s, (int)nf, faces, verts, fn);
  if (vn) hipLaunchKernelGGL(mn_vertex_normals_kernel, grid_v, blk, 0, s, (int)n, off, corners, fn, vn);
  VCY_HIP_CHECK(hipGetLastError());
  return VCY_OK;
}

int mesh_normals_device(vcy_ctx* c, int64_t n64, int64_t nf64, const float* d_vertices, const int32_t* d_faces, bool vertex_normals,
                        float** d_face_normals, float** d_vertex_normals) {
  const size_t n = (size_t)n64, nf = (size_t)nf64, nc = 3 * nf;
  // [deg, scan scratch, total | off | cursor | corners | face normals | vertex normals]
  PoolLayout at;
  const size_t at_deg = at.take(8 * (n + 1)), at_scan = at.take(8 * scan_scratch_words(n + 1)), at_total = at.take(8),
               at_off = at.take(4 * (n + 1)), at_cursor = at.take(4 * n), at_corners = at.take(4 * nc),
               at_fn = at.take(12 * nf), at_vn = at.take(12 * n);
  VCY_HIP_CHECK(c->d_mn_buf.grow(at.total(), c->stream));
  char* base = (char*)c->d_mn_buf;
  hipStream_t s = c->stream;
  const rows::Table t{(int)n, (int)nc, d_faces, (rows::u64*)(base + at_deg), (int*)(base + at_off), (int*)(base + at_cursor),
                      (int*)(base + at_corners)};
  *d_face_normals = (float*)(base + at_fn);
  *d_vertex_normals = (float*)(base + at_vn);
  if (vertex_normals) {
    { const int rc = rows::fill(s, t, (rows::u64*)(base + at_total), (rows::u64*)(base + at_scan)); if (rc != VCY_OK) return rc; }
    hipLaunchKernelGGL(rows::rows_sort_kernel<kShortRow>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t);
  }
  return launch_mesh_normals(s, n64, nf64, d_vertices, d_faces, t.off, t.items, *d_face_normals, vertex_normals ? *d_vertex_normals : nullptr);
}

}  // namespace vcy
