// K5: normals of the marching-cubes mesh, Mesh::CalcFaceNormal + Mesh::CalcNormal (reference
// src/vacancy/mesh.cc:197-240), as the last stage of the extraction chain.
//
// The reference sums, for every vertex, the normals of the faces that use it in ASCENDING FACE INDEX (a float sum:
// the order is part of the result), divides by the count and normalises.  A marching-cubes vertex sits on one grid
// edge; the faces that use it belong to the at most four cells around that edge, faces are numbered in cell raster
// order and, inside a cell, in kTriTable order.  So one thread -- the cell that OWNS the edge, as in mc_emit -- visits
// those cells in raster order, walks each one's triangle row and adds the normal of every triangle that names the
// edge: the reference's sum in the reference's order, in registers, no atomics, no sorting, one 12-byte store.
//
// The corner positions of those triangles are recomputed from the state with the chain's own VertexInterp (fp64, the
// 1e-5 snaps, the cast to float), in the argument order of the cell that owns the corner's edge -- the first active
// cell around it -- so they are the emitted positions to the bit without a lookup of vertex ids.  The loads hit lines
// the chain has just touched: 8 corner values per visited cell, 2 per recomputed position, ACT words for the owners.
//
// The face normals are one thread per face over the emitted arrays (device staging), 12 bytes out each.
//
// Arithmetic: include/vacancy/linalg.h's, i.e. squaredNorm = x*x + (y*y + z*z), normalized() = n2 > 0 ? v / sqrt(n2) : v,
// true division per component; no contraction, correctly rounded sqrt and division, denormals kept (Makefile).
#include "face_normal.h"
#include "mc_common.h"
#include "vcy_internal.h"

namespace vcy {
namespace mc {

namespace {

// The four cells around a grid edge in raster order (z, then y, then x), relative to the first, and the number the
// edge has in each; per axis of the edge.  kGrp[e] = (axis, position of the cell that calls the edge e).
__device__ const int8_t kGrpOff[3][4][3] = {{{0, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 1, 1}},
                                            {{0, 0, 0}, {1, 0, 0}, {0, 0, 1}, {1, 0, 1}},
                                            {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}}};
__device__ const int8_t kGrpEdge[3][4] = {{6, 4, 2, 0}, {5, 7, 1, 3}, {10, 11, 9, 8}};
__device__ const int8_t kGrp[12][2] = {{0, 3}, {1, 2}, {0, 2}, {1, 3}, {0, 1}, {1, 0},
                                       {0, 0}, {1, 1}, {2, 3}, {2, 2}, {2, 0}, {2, 1}};
// edges whose interpolation runs against their axis (kEdgeA -> kEdgeB): e2, e3, e6, e7
constexpr int kEdgeReversed = 0xCC;

// kCornerOff without the table
__device__ __forceinline__ int corner_dx(int c) { return ((c ^ (c >> 1)) & 1) - 1; }
__device__ __forceinline__ int corner_dy(int c) { return ((c >> 1) & 1) - 1; }
__device__ __forceinline__ int corner_dz(int c) { return (c >> 2) - 1; }

struct Cell {
  int li, cy, x;
};

// SLAB: the ghost layer (li = 0, the last cell layer of the slab below) counts as well -- its cells own corners on the
// lower seam plane, and with them the argument order of VertexInterp there.
template <bool SLAB>
__device__ __forceinline__ bool cell_active(const McParams& p, const u64* __restrict__ act, const Cell& s) {
  if (s.li < ((SLAB && p.has_ghost) ? 0 : 1) || s.li > p.L || s.cy < 0 || s.cy >= p.Y || s.x < 1 || s.x >= p.nx) return false;
  return (act[word_index(p, s.li, s.cy, s.x >> 6)] >> (s.x & 63)) & 1ull;
}

__device__ __forceinline__ Cell group_cell(const Cell& s, int axis, int from, int to) {
  Cell r;
  r.x = s.x + kGrpOff[axis][to][0] - kGrpOff[axis][from][0];
  r.cy = s.cy + kGrpOff[axis][to][1] - kGrpOff[axis][from][1];
  r.li = s.li + kGrpOff[axis][to][2] - kGrpOff[axis][from][2];
  return r;
}

__device__ __forceinline__ float corner_value(const McParams& p, const Cell& s, int c) {
  const int z = p.zc0 + s.li - 1 + corner_dz(c), y = s.cy + 1 + corner_dy(c), x = s.x + corner_dx(c);
  return p.sdf[((int64_t)(z - p.zs0) * p.ny + y) * (int64_t)p.nx + x];
}

// cube index (marching_cubes.cc:121-128)
__device__ __forceinline__ int cell_case(const McParams& p, const Cell& s) {
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = corner_value(p, s, c);
  int code = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) code |= ((double)v[c] < p.iso ? 1 : 0) << c;
  return code;
}

// The emitted position of the vertex on edge e of the ACTIVE cell s: VertexInterp with the arguments in the order of
// the first active cell around the edge (the owner, where the reference's map insert happens).
template <bool SLAB>
__device__ __forceinline__ void edge_position(const McParams& p, const u64* __restrict__ act, const Cell& s, int e,
                                              float out[3]) {
  const int axis = kGrp[e][0], me = kGrp[e][1];
  int oe = e;
  for (int k = me - 1; k >= 0; --k)
    if (cell_active<SLAB>(p, act, group_cell(s, axis, me, k))) oe = kGrpEdge[axis][k];
  const bool flip = (((kEdgeReversed >> oe) ^ (kEdgeReversed >> e)) & 1) != 0;
  const int ca = flip ? kEdgeB[e] : kEdgeA[e], cb = flip ? kEdgeA[e] : kEdgeB[e];
  const int y = s.cy + 1, z = p.zc0 + s.li - 1;
  const float pa[3] = {p.px[s.x + corner_dx(ca)], p.py[y + corner_dy(ca)], p.pz[z + corner_dz(ca)]};
  const float pb[3] = {p.px[s.x + corner_dx(cb)], p.py[y + corner_dy(cb)], p.pz[z + corner_dz(cb)]};
  vertex_interp(p.iso, pa, pb, corner_value(p, s, ca), corner_value(p, s, cb), p.linear != 0, out);
}

// normalize3, face_normal, face_normal_of: face_normal.h

// the counts of the chain, and whether mc_emit has written a mesh at all (it has not when a capacity was too small:
// the host then runs the chain again with room, and these kernels with it)
__device__ __forceinline__ bool chain_fits(const NormalsLaunch& a, int64_t* ncells, int64_t* nv, int64_t* nf) {
  const u64 nc = *a.ncells_dev, gt = *a.grand_total_dev;
  *ncells = (int64_t)nc;
  *nv = (int64_t)(gt >> 32);
  *nf = (int64_t)(gt & 0xFFFFFFFFull);
  return *ncells <= a.cap_cells && *nv <= a.cap_verts && *nf <= a.cap_faces;
}

// ---- face normals: one thread per face over the emitted arrays ------------------------------------------------
__global__ __launch_bounds__(256) void mc_face_normals_kernel(NormalsLaunch a) {
  int64_t ncells, nv, nf;
  if (!chain_fits(a, &ncells, &nv, &nf)) return;
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int i0 = a.faces[3 * f + 0], i1 = a.faces[3 * f + 1], i2 = a.faces[3 * f + 2];
  float fn[3] = {0.0f, 0.0f, 0.0f};
  if ((int64_t)(unsigned)i0 < nv && (int64_t)(unsigned)i1 < nv && (int64_t)(unsigned)i2 < nv)  // (always, for a mesh of mc_emit)
    face_normal_of(a.verts, i0, i1, i2, fn);
  a.face_normals[3 * f + 0] = fn[0];
  a.face_normals[3 * f + 1] = fn[1];
  a.face_normals[3 * f + 2] = fn[2];
}

// ---- vertex normals: one thread per active cell, the edges it owns ---------------------------------------------
// SLAB (a context that owns z [z_begin, z_end) of the grid): a vertex on an x- or y-axis edge in the plane below the
// slab's first cell layer or -- when z_end < nz -- in its top plane has faces in two slabs; the host finishes those
// (vcy_mesh_normals_host_seam), here their slots get zeros.  The former are the vertices of the ghost cells, the latter
// those of e4..e7 of the last own layer.  Every other vertex has all its faces in this slab and is final: the corners of
// first-layer triangles that lie on the lower seam plane take their owners from the ghost layer's ACT bits.
template <bool SLAB>
__global__ __launch_bounds__(256) void mc_vertex_normals_kernel(McParams p, NormalsLaunch a) {
  int64_t ncells, nv, nf;
  if (!chain_fits(a, &ncells, &nv, &nf)) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ncells) return;
  const int64_t slot = (int64_t)a.cell_list[i];
  Cell c;
  int w;
  decode_word(p, slot >> 6, &c.li, &c.cy, &w);
  c.x = w * 64 + (int)(slot & 63);
  const uint32_t inf = a.info[i];
  const int owned = inf & 0xFFF, code = (inf >> 12) & 0xFF;
  if (owned == 0 || (!SLAB && c.li < 1)) return;
  const int64_t v0 = (int64_t)(a.block_offs[i >> 8] >> 32) + (int64_t)(inf >> 20);  // first vertex of this cell
  for (int e = 0; e < 12; ++e) {
    if (!((owned >> e) & 1)) continue;
    const int axis = kGrp[e][0], me = kGrp[e][1];
    float n[3] = {0.0f, 0.0f, 0.0f};
    int count = 0;
    const bool seam = SLAB && (c.li < 1 || (a.open_top != 0 && c.li == p.L && e >= 4 && e < 8));
    // this cell owns the edge: the cells before it around the edge are not active
    for (int k = seam ? 4 : me; k < 4; ++k) {
      const Cell s = group_cell(c, axis, me, k);
      if (k > me && !cell_active<SLAB>(p, a.act, s)) continue;
      const int se = kGrpEdge[axis][k];
      const int scode = k == me ? code : cell_case(p, s);
      const uint4 trow = *reinterpret_cast<const uint4*>(&a.T->tri[scode][0]);
      const int ntri = a.T->ntri[scode];
      auto entry = [&](int idx) -> int {
        const uint32_t word = (idx < 4) ? trow.x : (idx < 8) ? trow.y : (idx < 12) ? trow.z : trow.w;
        return (int)((word >> (8 * (idx & 3))) & 0xFFu);
      };
      for (int t = 0; t < ntri; ++t) {
        // corner j of the face reads entry 3t + (2 - j) (marching_cubes.cc:199-206)
        const int e0 = entry(3 * t + 2), e1 = entry(3 * t + 1), e2 = entry(3 * t);
        const int hits = (e0 == se ? 1 : 0) + (e1 == se ? 1 : 0) + (e2 == se ? 1 : 0);
        if (hits == 0) continue;
        float q0[3], q1[3], q2[3], fn[3];
        edge_position<SLAB>(p, a.act, s, e0, q0);
        edge_position<SLAB>(p, a.act, s, e1, q1);
        edge_position<SLAB>(p, a.act, s, e2, q2);
        face_normal(q0, q1, q2, fn);
        for (int h = 0; h < hits; ++h) {  // (mesh.cc:215-219: once per corner that names the vertex)
          n[0] += fn[0];
          n[1] += fn[1];
          n[2] += fn[2];
          ++count;
        }
      }
    }
    if (!seam) {
      const float d = (float)count;  // (>= 1: the owner's own triangle row names every edge it cuts)
      n[0] = n[0] / d;
      n[1] = n[1] / d;
      n[2] = n[2] / d;
      normalize3(n);
    }
    const int64_t vid = v0 + __popc(owned & (int)a.T->prec[code][e]);
    if (vid < nv) {
      a.vertex_normals[3 * vid + 0] = n[0];
      a.vertex_normals[3 * vid + 1] = n[1];
      a.vertex_normals[3 * vid + 2] = n[2];
    }
  }
}

// ---- how many faces the first and the last own cell layer have: one workgroup -----------------------------------
// In the merged face array of a grid cut into slabs, the faces of a slab's last layer and of the next slab's first
// layer are one contiguous range that holds every face of the seam vertices between them.  Faces are numbered in list
// order, so a layer's faces start at the face offset of its first cell: the block's offset (block_offs) plus the
// triangles of the cells before it in its block of 256 (the case of each is in info).  The list index of the first
// cell of a cell word comes from the offsets mc_compact used.
__global__ __launch_bounds__(256) void mc_layer_faces_kernel(McParams p, NormalsLaunch a) {
  __shared__ int sm[4];
  int64_t ncells, nv, nf;
  if (!chain_fits(a, &ncells, &nv, &nf)) return;
  const int64_t nghost = (int64_t)*a.ghost_cells_dev;
  const int64_t layer_words = (int64_t)p.Yc * p.Wr;
  u64 before[2];
  for (int q = 0; q < 2; ++q) {  // (uniform) faces before layer 2, faces before layer L
    const int64_t cw = p.G + (q == 0 ? 1 : (int64_t)p.L - 1) * layer_words;
    const int64_t i = cw < p.nwords ? (int64_t)a.block_cell_offs[cw >> 8] + a.word_cell_off[cw] : ncells;
    int tot = 0;
    int ntri = 0;
    if (i < ncells) {
      const int64_t j = (i >> 8 << 8) + threadIdx.x;
      if (j < i && j >= nghost) ntri = a.T->ntri[(a.info[j] >> 12) & 0xFF];  // (ghost cells have no faces)
    }
    (void)block_exclusive_scan(ntri, &tot, sm);
    before[q] = i < ncells ? (a.block_offs[i >> 8] & 0xFFFFFFFFull) + (u64)tot : (u64)nf;
  }
  if (threadIdx.x == 0) {
    a.report[0] = before[0];
    a.report[1] = (u64)nf - before[1];
  }
}

// ---- the vertex -> incident-corner table from the cells (CornerRowsLaunch, mc_common.h) ---------------------------
// The first face of every active cell, as mc_emit numbers them: the offset of the cell's block of 256 list entries plus the
// triangles of the cells before it in the block.  Precondition: a WHOLE grid.  A z-slab's list begins with its ghost cells,
// which are active and have a case but no faces (mc_emit: `li > 0`); they are not told apart here, and mc_corner_rows below
// does not walk the ghost layer either.  vcy_extract_iso_chain refuses a slab before it gets here.
__global__ __launch_bounds__(256) void mc_face_base_kernel(CornerRowsLaunch a) {
  __shared__ int sm[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int ntri = i < a.n_cells ? a.T->ntri[(a.info[i] >> 12) & 0xFF] : 0;
  int tot;
  const int before = block_exclusive_scan(ntri, &tot, sm);
  if (i < a.n_cells) a.face_base[i] = (uint32_t)(a.block_offs[i >> 8] & 0xFFFFFFFFull) + (uint32_t)before;
}

// One thread per active cell, the edges it owns, the walk of mc_vertex_normals_kernel: the cells around the edge in raster
// order -- so ascending face index --, in each the triangles that name the edge, in each triangle the corners in ascending j.
// FILL false: the number of corners into deg[vertex]; true: the corners 3 (face base + t) + j into the vertex's row.  No
// positions, no case recomputed: a neighbour's case and face base come from its list entry, found through its ACT word as
// mc_emit finds an owner.  As compiled for gfx950: see DESIGN.md, "extraction chain".
template <bool FILL>
__global__ __launch_bounds__(256) void mc_corner_rows_kernel(McParams p, CornerRowsLaunch a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_cells) return;
  const int64_t slot = (int64_t)a.cell_list[i];
  Cell c;
  int w;
  decode_word(p, slot >> 6, &c.li, &c.cy, &w);
  c.x = w * 64 + (int)(slot & 63);
  const uint32_t inf = a.info[i];
  const int owned = inf & 0xFFF, code = (inf >> 12) & 0xFF;
  if (owned == 0 || c.li < 1) return;
  const int64_t v0 = (int64_t)(a.block_offs[i >> 8] >> 32) + (int64_t)(inf >> 20);  // first vertex of this cell
  const int64_t n_items = 3 * a.n_faces;
  for (int e = 0; e < 12; ++e) {
    if (!((owned >> e) & 1)) continue;
    const int64_t vid = v0 + __popc(owned & (int)a.T->prec[code][e]);
    if (vid >= a.n_vertices) continue;  // (never, for the mesh these arrays describe)
    const int axis = kGrp[e][0], me = kGrp[e][1];
    const int64_t row = FILL ? (int64_t)a.off[vid] : 0;
    int count = 0;
    // this cell owns the edge: the cells before it around the edge are not active
    for (int k = me; k < 4; ++k) {
      int scode = code;
      int64_t si = i;
      if (k > me) {
        const Cell s = group_cell(c, axis, me, k);
        if (s.li < 1 || s.li > p.L || s.cy < 0 || s.cy >= p.Y || s.x < 1 || s.x >= p.nx) continue;
        const int64_t cw = word_index(p, s.li, s.cy, s.x >> 6);
        const u64 aw = a.act[cw];
        if (!((aw >> (s.x & 63)) & 1ull)) continue;
        si = (int64_t)a.block_cell_offs[cw >> 8] + a.word_cell_off[cw] + __popcll(aw & ((1ull << (s.x & 63)) - 1ull));
        if (si >= a.n_cells) continue;  // (never)
        scode = (a.info[si] >> 12) & 0xFF;
      }
      const int se = kGrpEdge[axis][k];
      const uint4 trow = *reinterpret_cast<const uint4*>(&a.T->tri[scode][0]);
      const int ntri = a.T->ntri[scode];
      const int64_t fb = FILL ? (int64_t)a.face_base[si] : 0;
      for (int t = 0; t < ntri; ++t) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          // corner j of the face reads entry 3t + (2 - j) (marching_cubes.cc:199-206)
          const int idx = 3 * t + (2 - j);
          const uint32_t word = (idx < 4) ? trow.x : (idx < 8) ? trow.y : (idx < 12) ? trow.z : trow.w;
          if ((int)((word >> (8 * (idx & 3))) & 0xFFu) != se) continue;
          if (FILL && row + count < n_items) a.items[row + count] = (int)(3 * (fb + t) + j);
          ++count;
        }
      }
    }
    if (!FILL) a.deg[vid] = (u64)count;
  }
}

}  // namespace

hipError_t launch_corner_rows_count(hipStream_t stream, const McParams& p, const CornerRowsLaunch& a) {
  if (a.n_cells <= 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cells + 255) / 256));
  hipLaunchKernelGGL(mc_face_base_kernel, grid, dim3(256), 0, stream, a);
  hipLaunchKernelGGL(mc_corner_rows_kernel<false>, grid, dim3(256), 0, stream, p, a);
  return hipGetLastError();
}

hipError_t launch_corner_rows_fill(hipStream_t stream, const McParams& p, const CornerRowsLaunch& a) {
  if (a.n_cells <= 0) return hipSuccess;
  hipLaunchKernelGGL(mc_corner_rows_kernel<true>, dim3((unsigned)((a.n_cells + 255) / 256)), dim3(256), 0, stream, p, a);
  return hipGetLastError();
}

hipError_t launch_normals(hipStream_t stream, const McParams& p, const NormalsLaunch& a) {
  if (a.face_normals != nullptr && a.cap_faces > 0)
    hipLaunchKernelGGL(mc_face_normals_kernel, dim3((unsigned)((a.cap_faces + 255) / 256)), dim3(256), 0, stream, a);
  if (a.vertex_normals != nullptr && a.cap_cells > 0) {
    const dim3 grid((unsigned)((a.cap_cells + 255) / 256));
    if (a.slab) hipLaunchKernelGGL(mc_vertex_normals_kernel<true>, grid, dim3(256), 0, stream, p, a);
    else hipLaunchKernelGGL(mc_vertex_normals_kernel<false>, grid, dim3(256), 0, stream, p, a);
  }
  if (a.report != nullptr) hipLaunchKernelGGL(mc_layer_faces_kernel, dim3(1), dim3(256), 0, stream, p, a);
  return hipGetLastError();
}

}  // namespace mc
}  // namespace vcy
