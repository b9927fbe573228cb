// What the marching-cubes translation units share (mc_kernels.hip: the kernels of the extraction chain and their
// launches; mc_normals.hip: the normals behind it; mc_extract.hip: the host driver of both): the cell-word layout,
// the case tables' shape, VertexInterp, the block scan, and the launch structs the driver fills.  The device code
// here has internal linkage or is inline, so each translation unit gets its own copy and no relocatable device
// code is needed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

struct vcy_ctx;
namespace vcy {
namespace mc {

typedef unsigned long long u64;

struct McTables {
  int8_t tri[256][16];     // edge numbers, -1 terminated (reference kTriTable)
  uint8_t ntri[256];
  uint16_t prec[256][12];  // prec[c][e] = edges whose vertex the serial scan creates before e's
};

// corner offsets relative to the cell's max corner (x,y,z), marching_cubes.cc:93-101
static __device__ const int8_t kCornerOff[8][3] = {{-1, -1, -1}, {0, -1, -1}, {0, 0, -1}, {-1, 0, -1},
                                            {-1, -1, 0},  {0, -1, 0},  {0, 0, 0},  {-1, 0, 0}};
// interpolation argument order per edge (:138-197) and key order (always lower id first)
static __device__ const int8_t kEdgeA[12] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3};
static __device__ const int8_t kEdgeB[12] = {1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7};

// Cell (x, y, z) is named by its max corner; bit b of word w of a row is x = 64*w + b.
// Cell rows: layer li = 0 is the ghost layer (z = zc0-1), li = l+1 the slab's own layer l;
// word index of (li, cy = y-1, w):  li == 0 ? cy*Wr + w : G + ((li-1)*Yc + cy)*Wr + w,
// Yc >= Y = rows a layer takes in the cell-word arrays (the sweep pads a layer to whole row groups, so that
// a group is a whole number of 256-word blocks; padding rows hold no active cell),
// G = ghost words rounded up to a whole block so that own cells start on a block boundary.
// Exact n / d for 32-bit unsigned n (Granlund-Montgomery): three integer instructions instead of the
// long 64-bit division sequence.
struct FastDiv {
  uint32_t d, m, s1, s2;
};

struct McParams {
  const float* sdf;   // slab incl. halo slices
  const void* cnt;
  const float* px;
  const float* py;
  const float* pz;
  const u64* in;      // bit planes [slice][y][Wr]
  const u64* ok;
  const u64* tc;
  int nx, ny;
  int nslices;        // stored voxel slices
  int Wr;             // 64-bit words per row
  int Y;              // cell rows per layer = ny-1
  int Yc;             // rows per layer in the cell-word arrays (>= Y)
  int L;              // own cell layers
  int zc0;            // global z of own layer 0
  int zs0;            // global z of stored slice 0
  int has_ghost;
  int64_t G;          // words reserved for the ghost layer
  int64_t nwords;     // G + L*Yc*Wr
  double iso;
  int linear;
  FastDiv div_row, div_layer;  // by Wr and by Yc * Wr; used when small32 (every word index < 2^32)
  int small32;
};

constexpr int kWordsPerBlock = 256;

__device__ __forceinline__ uint32_t fast_div(uint32_t n, const FastDiv& f) {
  const uint32_t t = __umulhi(n, f.m);
  return (t + ((n - t) >> f.s1)) >> f.s2;
}

__device__ __forceinline__ bool decode_word(const McParams& p, int64_t cw, int* li, int* cy, int* w) {
  if (p.small32) {
    uint32_t r;
    if (cw < p.G) {
      if (cw >= (int64_t)p.Yc * p.Wr) return false;  // padding
      *li = 0;
      r = (uint32_t)cw;
    } else {
      const uint32_t q = (uint32_t)(cw - p.G);
      const uint32_t layer = fast_div(q, p.div_layer);
      *li = (int)layer + 1;
      r = q - layer * p.div_layer.d;
    }
    const uint32_t row = fast_div(r, p.div_row);
    *cy = (int)row;
    *w = (int)(r - row * p.div_row.d);
    return *cy < p.Y;  // (rows Y .. Yc-1 are padding)
  }
  int64_t r;
  if (cw < p.G) {
    if (cw >= (int64_t)p.Yc * p.Wr) return false;  // padding
    *li = 0;
    r = cw;
  } else {
    const int64_t q = cw - p.G;
    const int64_t layer = q / ((int64_t)p.Yc * p.Wr);
    *li = (int)layer + 1;
    r = q - layer * ((int64_t)p.Yc * p.Wr);
  }
  *cy = (int)(r / p.Wr);
  *w = (int)(r - (int64_t)(*cy) * p.Wr);
  return *cy < p.Y;
}

__device__ __forceinline__ int64_t word_index(const McParams& p, int li, int cy, int w) {
  return (li == 0 ? 0 : p.G + (int64_t)(li - 1) * p.Yc * p.Wr) + (int64_t)cy * p.Wr + w;
}

__device__ __forceinline__ bool neighbour_active(const McParams& p, const u64* __restrict__ act, int li,
                                                 int cy, int x, int dx, int dy, int dl) {
  const int nl = li + dl, ncy = cy + dy, nxx = x + dx;
  if (nl < 0 || ncy < 0 || ncy >= p.Y || nxx < 1 || nxx >= p.nx) return false;
  return (act[word_index(p, nl, ncy, nxx >> 6)] >> (nxx & 63)) & 1ull;
}

// ---- block-level exclusive scan (256 threads = 4 waves) ---------------------------------------
__device__ __forceinline__ int wave_inclusive_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

__device__ __forceinline__ int block_exclusive_scan(int v, int* total, int* sm /*[4]*/) {
  const int incl = wave_inclusive_scan(v);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 63) sm[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int s = sm[w];
    if (w < wave) base += s;
    tot += s;
  }
  *total = tot;
  return base + incl - v;
}

// VertexInterp, marching_cubes.cc:25-57 (fp64, then cast)
__device__ __forceinline__ void vertex_interp(double iso, const float pa[3], const float pb[3], float va,
                                              float vb, bool linear, float out[3]) {
  if (!linear) {
    out[0] = pa[0]; out[1] = pa[1]; out[2] = pa[2];
    return;
  }
  const double v1 = va, v2 = vb;
  if (fabs(iso - v1) < 0.00001) { out[0] = pa[0]; out[1] = pa[1]; out[2] = pa[2]; return; }
  if (fabs(iso - v2) < 0.00001) { out[0] = pb[0]; out[1] = pb[1]; out[2] = pb[2]; return; }
  if (fabs(v1 - v2) < 0.00001) { out[0] = pa[0]; out[1] = pa[1]; out[2] = pa[2]; return; }
  const double mu = (iso - v1) / (v2 - v1);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = (float)((double)pa[k] + mu * ((double)pb[k] - (double)pa[k]));
}

// ---- mc_kernels.hip: the launches of the extraction chain, in the order the driver enqueues them ----------------
// Every pointer is device memory unless said otherwise.  Each launch returns VCY_OK or a VCY_ERR_* with the error set.
void build_tables(McTables* t);  // (host) the case tables the kernels read

// mc_sweep_kernel's geometry (see the kernel), planned by the driver because it shapes the cell-word arrays (Yc)
struct SweepParams {
  int R;           // cell rows per workgroup
  int K;           // 256-word blocks per step = R * Wr / 256
  int groups;      // row groups per layer = Yc / R
  int layers;      // cell layers per workgroup
  int dl;          // cells whose max corner lies in stored slice s form layer li = s + dl
  int cnt_slices;  // READS_CNT: update_num is read for the stored slices below this one (all of them)
  int wshift;      // log2 Wr
};
constexpr int kSweepMaxK = 4;
#ifndef VCY_SWEEP_TARGET_WGS
#define VCY_SWEEP_TARGET_WGS 1024
#endif

// What a chained scan needs from its caller: the publication flags of ONE scan slot (kChainedScanMaxChunks words), the
// slot's ticket counter and how many tickets have been drawn from it so far (advanced by the launch).
constexpr int kChainedScanMaxChunks = 1024;
struct ChainedScanSlot {
  uint32_t* flags;
  uint32_t* ticket;
  uint32_t* tickets_drawn;  // (host)
  uint32_t epoch;
};

// What the three launches take.  launch_cell_search: the bit planes (mc_bits_kernel, or mc_bits_bricks_kernel over the
// owned slices when the context's brick minima allow) and mc_active_kernel -- or, with `sweep`, mc_sweep_kernel alone -- then the scan
// of the per-block cell counts; it sets p->in / ok / tc to the planes the later passes read (a whole grid whose state
// implies TC == OK gets no third plane: p->tc == p->ok).  launch_owners: mc_compact, mc_owner and the scan of their
// per-block counts.  launch_emit: mc_emit.  The kernels behind the search read the number of cells and the totals from
// device memory and stay inside the three capacities.
struct ChainLaunch {
  const McTables* T;
  const SweepParams* sweep;                    // null: bit planes in memory
  u64 *in, *ok, *tc, *ghost;                   // planes [slice][y][Wr]; the sweep: `in` and IN / OK / TC of one slice in `ghost`
  u64* act;                                    // [nwords]
  uint32_t* word_cell_off;                     // [nwords]
  u64* block_cells;                            // [nblocks + 1] per block of kWordsPerBlock cell words, scanned in place
  unsigned nblocks;
  u64 *scan_scratch, *ncells_dev;              // ncells_dev receives the number of active cells
  int64_t cap_cells, cap_verts, cap_faces;     // (the last two: mc_emit only, like verts .. report)
  unsigned cell_blocks;                        // blocks of 256 list entries = (cap_cells + 255) / 256
  u64* cell_list;                              // the three below: [cap_cells]
  uint32_t* info;
  uint16_t* nbr_active;
  u64* block_offs;                             // [cell_blocks + 1] (vertices << 32 | triangles), scanned in place
  u64 *cell_scan_scratch, *grand_total_dev;
  float* verts;                                // verts / keys / faces: device staging, or page-locked HOST arrays (the
  long long* keys;                             // direct path); keys may be null
  int* faces;
  u64* report;  // 64 page-locked host bytes: cells, ghost cells, (vertices << 32 | triangles), foreign vertices
};
int launch_cell_search(const vcy_ctx* c, McParams* p, const ChainLaunch& a, const ChainedScanSlot& slot);  // on c->stream
int launch_owners(hipStream_t stream, const McParams& p, const ChainLaunch& a, const ChainedScanSlot& slot);
int launch_emit(hipStream_t stream, const McParams& p, const ChainLaunch& a);

// mc_normals.hip: Mesh::CalcFaceNormal + Mesh::CalcNormal (reference mesh.cc:197-240) of the mesh mc_emit has just
// been enqueued for, behind it on the same stream.  Every pointer is device memory; `verts` / `faces` are the DEVICE
// staging of the mesh.  vertex_normals / face_normals may be null.  The kernels read the counts where the chain left
// them and return without a store when a capacity is exceeded, exactly as mc_emit does.
// `slab` != 0 (a context that owns a z-slab, vcy_extract_iso_normals_slab): the vertex kernel's slab instance, which
// reads the ghost layer's ACT bits and leaves the seam vertices -- those of ghost cells, and with `open_top` those on
// the slab's top plane -- at zero for the host's seam finish.  `report` != null: one more small launch writes the
// numbers of faces of the slab's first and last own cell layer to report[0], report[1] (page-locked host memory).
struct NormalsLaunch {
  const McTables* T;
  const u64* act;
  const u64* cell_list;
  const u64* ncells_dev;
  int64_t cap_cells;
  const uint32_t* info;
  const u64* block_offs;
  const u64* grand_total_dev;
  int64_t cap_verts, cap_faces;
  const float* verts;
  const int* faces;
  float* vertex_normals;
  float* face_normals;
  int slab, open_top;
  const uint32_t* word_cell_off;  // the three below: read by the layer count only (`report` != null)
  const u64* block_cell_offs;
  const u64* ghost_cells_dev;
  u64* report;
};
hipError_t launch_normals(hipStream_t stream, const McParams& p, const NormalsLaunch& a);

// mc_normals.hip: the vertex -> incident-corner table of the mesh an extraction of a WHOLE grid has left (rows of corner
// ids 3 f + j by vertex faces[3 f + j], every row ascending: mesh_rows.h's table after its sort) from the cells instead of
// from the faces.  The thread that owns a grid edge walks the cells around it as mc_vertex_normals_kernel does, so a row
// comes out in ascending corner id without atomics and without a sort.  The counts are the host's (the extraction has been
// waited for and fitted its capacities).  Three launches the caller puts its scan between:
//   launch_corner_rows_count  mc_face_base (the first face of every active cell: the block's offset plus mc_emit's block
//                             scan of the triangle counts) into `face_base`, and the row lengths into `deg`
//   -- the caller: exclusive scan of deg[0 .. n_vertices], row offsets into `off` --
//   launch_corner_rows_fill   the rows into `items`
struct CornerRowsLaunch {
  const McTables* T;
  const u64* act;
  const u64* cell_list;
  int64_t n_cells, n_vertices, n_faces;
  const uint32_t* info;
  const u64* block_offs;
  const uint32_t* word_cell_off;
  const u64* block_cell_offs;
  uint32_t* face_base;  // [n_cells]
  u64* deg;             // [n_vertices + 1], cleared by the caller
  const int* off;       // [n_vertices + 1]
  int* items;           // [3 n_faces]
};
hipError_t launch_corner_rows_count(hipStream_t stream, const McParams& p, const CornerRowsLaunch& a);
hipError_t launch_corner_rows_fill(hipStream_t stream, const McParams& p, const CornerRowsLaunch& a);

}  // namespace mc

// mc_extract.hip: extract_iso with the mesh left where mc_emit wrote it, the device staging vcy_ctx::d_mc_out, whatever
// "mcdirect" says (valid until the context next extracts): a whole-grid context without edge keys.  The first stage of the
// extraction chain (mesh_chain.hip).  The counts are those of the extraction's own wait.
struct StagedMesh {
  const float* vertices;  // device, 3 floats per vertex; null when the mesh is empty
  const int32_t* faces;   // device, 3 ints per face
  int64_t n_vertices, n_faces;
  mc::McParams p;             // the cell-word layout of the extraction ...
  mc::CornerRowsLaunch cells; // ... and its cell arrays (face_base .. items are the caller's to fill in)
};
int extract_iso_staged(vcy_ctx* ctx, double iso, int linear_interp, StagedMesh* staged);

}  // namespace vcy
