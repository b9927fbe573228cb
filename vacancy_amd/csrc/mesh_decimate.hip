// K-decimate: vertex-clustering decimation of an indexed mesh and Mesh::CalcNormal of the result, on the device
// (vcy_decimate_mesh; the definition is the section "mesh decimation" of vacancy_hip.h, the serial statement
// mesh_decimate_host.hip, the arithmetic the two share mesh_decimate.h).
//
// All launches go to the context's stream with no host wait between them, in three groups:
//   cluster  dc_keys (one lane per vertex: its cell, and the flag of the cell rule), dc_vinsert (an open-addressing table of
//            int32 slots, a power of two >= 2 n, a slot holds a vertex index: atomicCAS claims an empty slot; a taken slot
//            names a vertex whose cell is compared with the lane's own -- only vertices of one cell ever share a slot, so
//            the answer does not depend on who is there at the moment --; a match ends in atomicMin of the lane's index, a
//            mismatch moves to the next slot), dc_vflag (a vertex is a representative iff its slot holds its own index),
//            the exclusive scan of mc_kernels.hip over the flags (cluster numbers by ascending lowest member),
//            dc_vcluster (cluster of every vertex; for MEAN and NEAREST an integer atomicAdd counts the members: the
//            count of mesh_rows.h's row table of the vertices by cluster, whose scan, offsets and fill follow), dc_rows
//            (one lane per cluster sorts its row ascending -- the order of the definition's sum whatever order the
//            atomics ran in --, in registers up to 48 members, in global memory up to 256 --, then the sum in registers,
//            the mean, the nearest member; a row of more than 256 members goes on a list),
//            dc_long_rows (one workgroup per listed row: see there).  FIRST needs no rows.
//            Quadric representatives (vcy_decimate_mesh_quadric; "mesh decimation, quadric representatives", the
//            arithmetic: mesh_quadric.h) are MEAN plus one stage behind the rows: mesh_rows.h's table of the input mesh's
//            corners by vertex, built with its checked kernels -- the verdict on the face indices is not read yet, so a
//            corner with a bad index is left out and raises the face flag --, dc_qv (one lane per vertex sorts its corner
//            row and adds the quadrics of its faces, seen from its cluster's mean, in registers: nine doubles per vertex),
//            dc_qsolve (one lane per cluster adds its members' nine doubles in row order -- every row is sorted by now,
//            the long ones too --, solves, and overwrites the mean unless the fallback rule holds; a byte per cluster
//            says which, and dc_emit_v counts the bytes of the clusters it emits: a ballot and one integer add per wave).
//   faces    dc_fmap (one lane per face: index check, corners -> clusters, collapsed faces flagged, the canonical triple),
//            dc_finsert (the same table trick, a slot holds a face index, canonical triples compared), dc_fflag (a face
//            survives iff its slot holds its own index; survivors mark their clusters with a plain store of 1), two scans
//            (output faces, output vertices).
//   emit     dc_emit_v (vertex_map, positions), dc_emit_f (faces, face_source).
// Then the one wait for these launches: the host reads the three flags and the three counts.  Behind it the normals of the
// output mesh, still in device memory (mesh_normals.hip's mesh_normals_device), and the
// copies into the caller's arrays, sized by the counts; a refused call copies nothing.
// Integer atomics only; no float atomics anywhere.  Every probe loop is bounded by the table size and raises a flag if it
// runs out.  Both tables are cleared on the stream at the start of every call.
#include <algorithm>

#include "mesh_decimate.h"
#include "mesh_ops.h"
#include "mesh_quadric.h"
#include "mesh_rows.h"
#include "vcy_internal.h"

namespace vcy {
namespace dc {

typedef unsigned long long u64;

constexpr int kShortRow = 16;   // members a row is sorted with in registers ...
constexpr int kMidRow = 48;     // ... and by a second, wider network (cells of 4 voxels hold about 18 vertices, at most a few dozen)
constexpr int kLongRow = 256;   // members from which on a row goes to a workgroup of its own (dc_long_rows_kernel)
constexpr int kShortCorners = 12;  // corners a vertex's row is sorted with in registers (a marching-cubes row holds 4 - 12)
enum { kErrVertex = 0, kErrTable = 1, kErrFace = 2, kLongCount = 3 };  // words of Dec::err

struct Dec {
  int n, nf, mode;
  float cell, origin[3];
  const float* pos;     // [3 n]
  const int* faces;     // [3 nf]
  int* key;             // [3 n] cells
  int* vslot;           // [n] the slot of every vertex's cell
  int* vtable;          // [vmask + 1]
  unsigned vmask;
  u64* vflag;           // [n + 1] representative flags, scanned in place
  int* cluster;         // [n] cluster number of every vertex
  int* rep;             // [n] lowest member of every cluster
  u64* deg;             // [n + 1] member counts, scanned in place
  int* off;             // [n + 1] row offsets
  int* cursor;          // [n]
  int* member;          // [n] rows of vertex ids
  float* cpos;          // [3 n] position of every cluster (MEAN, NEAREST)
  int* longlist;        // [long_cap] clusters with more than kLongRow members; their number: err[kLongCount]
  int long_cap;
  int* fcanon;          // [3 nf] canonical triple of every face
  int* fslot;           // [nf] the slot of every face's triple, -1: collapsed
  int* ftable;          // [fmask + 1]
  unsigned fmask;
  u64* fflag;           // [nf + 1] survivor flags, scanned in place
  u64* used;            // [n + 1] per cluster: some survivor names it; scanned in place
  float* pos_out;       // [3 n]
  int* faces_out;       // [3 nf]
  int* vmap;            // [n]
  int* fsrc;            // [nf]
  int* err;             // [4]
  const u64* totals;    // clusters, output faces, output vertices
  // quadric representatives
  float regularize;
  int* coff;            // [n + 1] offsets of the corner rows
  int* corner;          // [3 nf] rows of corners 3 f + j by vertex
  double* qv;           // [9 n] Qv of every vertex
  unsigned char* fell;  // [n] per cluster: it keeps the mean
  u64* fallbacks;       // the output vertices that keep the mean
};

__global__ __launch_bounds__(256) void dc_keys_kernel(Dec d) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= d.n) return;
  const float p[3] = {d.pos[3 * v], d.pos[3 * v + 1], d.pos[3 * v + 2]};
  int32_t k[3];
  if (!cell_key(p, d.origin, d.cell, k)) d.err[kErrVertex] = 1;
  d.key[3 * v] = k[0], d.key[3 * v + 1] = k[1], d.key[3 * v + 2] = k[2];
}

// The slot whose entry `id` shares, or -1 after mask + 1 probes.  `triple`: three ints per entry, written by an earlier
// kernel; a slot holds the lowest id of the entries with its triple once every lane has returned.
__device__ __forceinline__ int table_insert(int* table, unsigned mask, const int* __restrict__ triple, int id) {
  const int a = triple[3 * (int64_t)id], b = triple[3 * (int64_t)id + 1], c = triple[3 * (int64_t)id + 2];
  unsigned h = hash3((uint32_t)a, (uint32_t)b, (uint32_t)c) & mask;
  for (unsigned probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
    int cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur < 0) {
      cur = atomicCAS(&table[h], -1, id);
      if (cur < 0) return (int)h;  // claimed
    }
    // (cur is an entry's id: nothing else is ever stored)
    if (triple[3 * (int64_t)cur] == a && triple[3 * (int64_t)cur + 1] == b && triple[3 * (int64_t)cur + 2] == c) {
      atomicMin(&table[h], id);
      return (int)h;
    }
  }
  return -1;
}

__global__ __launch_bounds__(256) void dc_vinsert_kernel(Dec d) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= d.n) return;
  int slot = table_insert(d.vtable, d.vmask, d.key, (int)v);
  if (slot < 0) d.err[kErrTable] = 1, slot = 0;
  d.vslot[v] = slot;
}

// the representative of v's cell; v itself where the table failed (the flag is up: the results are thrown away)
__device__ __forceinline__ int representative(const Dec& d, int64_t v) {
  const int r = d.vtable[d.vslot[v]];
  return (r < 0 || r >= d.n) ? (int)v : r;
}

__global__ __launch_bounds__(256) void dc_vflag_kernel(Dec d) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v > d.n) return;
  d.vflag[v] = (v < d.n && representative(d, v) == (int)v) ? 1ull : 0ull;
}

template <bool ROWS>
__global__ __launch_bounds__(256) void dc_vcluster_kernel(Dec d) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= d.n) return;
  const int r = representative(d, v);
  const int cl = (int)min(d.vflag[r], (u64)(d.n - 1));  // (the clamp only ever acts where the table failed)
  d.cluster[v] = cl;
  if (r == (int)v) d.rep[cl] = (int)v;
  if (ROWS) atomicAdd(&d.deg[cl], 1ull);
}

template <bool NEAREST>
__global__ __launch_bounds__(256) void dc_rows_kernel(Dec d) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= (int64_t)min(d.totals[0], (u64)d.n)) return;
  const int b = d.off[c], len = d.off[c + 1] - b;
  if (len <= 0) return;  // (only where the table failed)
  int* row = d.member + b;
  if (len > kLongRow) {  // (at most n / kLongRow of them: the list has room)
    const int w = atomicAdd(&d.err[kLongCount], 1);
    if (w < d.long_cap) d.longlist[w] = (int)c;
    return;
  }
  rows::sort_row<kShortRow, kMidRow>(row, len);  // (beyond kMidRow, up to kLongRow members: in place in global memory)
  float m[3];
  row_mean(d.pos, row, len, m);
  if (NEAREST) {
    const int64_t best = row_nearest(d.pos, row, len, m);
    m[0] = d.pos[3 * best], m[1] = d.pos[3 * best + 1], m[2] = d.pos[3 * best + 2];
  }
  d.cpos[3 * c] = m[0], d.cpos[3 * c + 1] = m[1], d.cpos[3 * c + 2] = m[2];
}

// A crowded cell, one workgroup per row.  The row is written again in ascending index by a walk over the vertices from the
// cluster's lowest member on (a ballot and a prefix per 256 vertices: no sort, work bounded by n per row and rows by
// n / kLongRow).  The sums of the definition are serial, so ONE lane adds, in row order, from tiles of 256 positions the
// workgroup gathers into LDS; NEAREST computes d(i) one lane per member and lets the same lane pick, in row order.
template <bool NEAREST>
__global__ __launch_bounds__(256) void dc_long_rows_kernel(Dec d) {
  __shared__ int wave_hits[4];
  __shared__ float tile[3 * 256];
  __shared__ float mean[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int count = min(d.err[kLongCount], d.long_cap);
  for (int w = blockIdx.x; w < count; w += gridDim.x) {
    const int c = d.longlist[w];
    const int b = d.off[c], len = d.off[c + 1] - b;
    int* row = d.member + b;
    int run = 0;
    const int lowest = d.rep[c];  // (in range unless the table failed)
    for (int64_t v0 = (lowest >= 0 && lowest < d.n) ? lowest & ~255 : 0; v0 < d.n && run < len; v0 += 256) {
      const int64_t v = v0 + tid;
      const bool hit = v < d.n && d.cluster[v] == c;
      const u64 bal = __ballot(hit);
      if (lane == 0) wave_hits[wave] = __popcll(bal);
      __syncthreads();
      int before = run;
      for (int k = 0; k < wave; ++k) before += wave_hits[k];
      const int at = before + __popcll(bal & ((1ull << lane) - 1ull));
      if (hit && at < len) row[at] = (int)v;  // (exactly len vertices are in cluster c: the bound never acts)
      run += wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
      __syncthreads();
    }
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int j0 = 0; j0 < len; j0 += 256) {
      if (j0 + tid < len) {
        const int64_t i = row[j0 + tid];
        tile[3 * tid] = d.pos[3 * i], tile[3 * tid + 1] = d.pos[3 * i + 1], tile[3 * tid + 2] = d.pos[3 * i + 2];
      }
      __syncthreads();
      if (tid == 0) {
        const int m = min(256, len - j0);
        for (int k = 0; k < m; ++k) {
          s[0] = s[0] + tile[3 * k];
          s[1] = s[1] + tile[3 * k + 1];
          s[2] = s[2] + tile[3 * k + 2];
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const float cnt = (float)len;
      mean[0] = s[0] / cnt, mean[1] = s[1] / cnt, mean[2] = s[2] / cnt;
    }
    __syncthreads();
    const float m[3] = {mean[0], mean[1], mean[2]};
    if (!NEAREST) {
      if (tid == 0) d.cpos[3 * (int64_t)c] = m[0], d.cpos[3 * (int64_t)c + 1] = m[1], d.cpos[3 * (int64_t)c + 2] = m[2];
    } else {
      int best = 0;  // position in the row
      float dbest = 0.0f;
      for (int j0 = 0; j0 < len; j0 += 256) {
        if (j0 + tid < len) tile[tid] = dist2(d.pos + 3 * (int64_t)row[j0 + tid], m);
        __syncthreads();
        if (tid == 0) {
          const int cnt = min(256, len - j0);
          for (int k = 0; k < cnt; ++k) {
            const float dk = tile[k];
            if (j0 + k == 0) dbest = dk;
            else if (dk < dbest) best = j0 + k, dbest = dk;
          }
        }
        __syncthreads();
      }
      if (tid == 0) {
        const int64_t i = row[best];
        d.cpos[3 * (int64_t)c] = d.pos[3 * i], d.cpos[3 * (int64_t)c + 1] = d.pos[3 * i + 1], d.cpos[3 * (int64_t)c + 2] = d.pos[3 * i + 2];
      }
    }
    __syncthreads();  // (mean and the tile are written again for the next row)
  }
}

// Qv of every vertex: the quadrics of the faces around it in corner order, seen from the mean of its cluster.  Nine double
// accumulators and one face's temporaries per lane.  A face in the row may still name a bad index at another corner (the
// face flag is up then and the call refused): it is left out, never read through.  As compiled for gfx950: 54 VGPRs, no
// scratch, 8 waves per SIMD (dc_qsolve_kernel: 52, none, 8) -- launch bounds beyond the block size would buy nothing.
__global__ __launch_bounds__(256) void dc_qv_kernel(Dec d) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= d.n) return;
  const int b = d.coff[v], len = d.coff[v + 1] - b;
  double Q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (len > 0) {
    int* row = d.corner + b;
    rows::sort_row<kShortCorners>(row, len);
    const float* mp = d.cpos + 3 * (int64_t)d.cluster[v];
    const float m[3] = {mp[0], mp[1], mp[2]};
    for (int k = 0; k < len; ++k) {
      const int64_t f = row[k] / 3;
      const int i0 = d.faces[3 * f], i1 = d.faces[3 * f + 1], i2 = d.faces[3 * f + 2];
      if (i0 < 0 || i0 >= d.n || i1 < 0 || i1 >= d.n || i2 < 0 || i2 >= d.n) continue;
      double q[9];
      face_quadric(d.pos + 3 * (int64_t)i0, d.pos + 3 * (int64_t)i1, d.pos + 3 * (int64_t)i2, m, q);
      quadric_add(Q, q);
    }
  }
  double* out = d.qv + 9 * v;
#pragma unroll
  for (int k = 0; k < 9; ++k) out[k] = Q[k];
}

// The position of every cluster: its members' Qv added in row order, the solve, the fallback rule.
__global__ __launch_bounds__(256) void dc_qsolve_kernel(Dec d) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= (int64_t)min(d.totals[0], (u64)d.n)) return;
  const int b = d.off[c], len = d.off[c + 1] - b;
  const int lowest = d.rep[c];
  if (len <= 0 || lowest < 0 || lowest >= d.n) return;  // (only where the table failed)
  const int* row = d.member + b;
  double Q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < len; ++j) quadric_add(Q, d.qv + 9 * (int64_t)row[j]);  // (a long row: serial, as its mean is)
  const float m[3] = {d.cpos[3 * c], d.cpos[3 * c + 1], d.cpos[3 * c + 2]};
  float P[3];
  const bool fell = solve_or_mean(Q, m, d.regularize, d.origin, d.cell, d.key + 3 * (int64_t)lowest, P);
  d.fell[c] = fell ? 1 : 0;
  if (!fell) d.cpos[3 * c] = P[0], d.cpos[3 * c + 1] = P[1], d.cpos[3 * c + 2] = P[2];
}

__global__ __launch_bounds__(256) void dc_fmap_kernel(Dec d) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= d.nf) return;
  const int i0 = d.faces[3 * f], i1 = d.faces[3 * f + 1], i2 = d.faces[3 * f + 2];
  int32_t t[3] = {-1, -1, -1};
  if (i0 < 0 || i0 >= d.n || i1 < 0 || i1 >= d.n || i2 < 0 || i2 >= d.n) {
    d.err[kErrFace] = 1;
  } else {
    const int a = d.cluster[i0], b = d.cluster[i1], c = d.cluster[i2];
    if (a != b && b != c && c != a) canonical(a, b, c, t);
  }
  d.fcanon[3 * f] = t[0], d.fcanon[3 * f + 1] = t[1], d.fcanon[3 * f + 2] = t[2];  // (-1: collapsed)
}

__global__ __launch_bounds__(256) void dc_finsert_kernel(Dec d) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= d.nf) return;
  int slot = -1;
  if (d.fcanon[3 * f] >= 0) {
    slot = table_insert(d.ftable, d.fmask, d.fcanon, (int)f);
    if (slot < 0) d.err[kErrTable] = 1;
  }
  d.fslot[f] = slot;
}

__global__ __launch_bounds__(256) void dc_fflag_kernel(Dec d) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f > d.nf) return;
  const int slot = f < d.nf ? d.fslot[f] : -1;
  const bool survives = slot >= 0 && d.ftable[slot] == (int)f;
  d.fflag[f] = survives ? 1ull : 0ull;
  if (survives) {
    d.used[d.fcanon[3 * f]] = 1ull;  // (cluster numbers, all < n)
    d.used[d.fcanon[3 * f + 1]] = 1ull;
    d.used[d.fcanon[3 * f + 2]] = 1ull;
  }
}

template <bool FIRST, bool QUADRIC>
__global__ __launch_bounds__(256) void dc_emit_v_kernel(Dec d) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= d.n) return;
  const int cl = d.cluster[v];
  const u64 o = d.used[cl];
  d.vmap[v] = d.used[cl + 1] != o ? (int)o : -1;
  // the same lane as cluster v
  bool emits = v < (int64_t)min(d.totals[0], (u64)d.n);
  u64 g = 0;
  if (emits) {
    g = d.used[v];
    emits = d.used[v + 1] != g;
  }
  if (emits) {
    const float* src = FIRST ? d.pos + 3 * (int64_t)d.rep[v] : d.cpos + 3 * v;
    d.pos_out[3 * g] = src[0], d.pos_out[3 * g + 1] = src[1], d.pos_out[3 * g + 2] = src[2];
  }
  if (QUADRIC) {  // (every lane with v < n is here: one integer add per wave)
    const u64 kept = __ballot(emits && d.fell[v] != 0);
    if (kept != 0 && (int)(threadIdx.x & 63) == __ffsll((long long)kept) - 1) atomicAdd(d.fallbacks, (u64)__popcll(kept));
  }
}

__global__ __launch_bounds__(256) void dc_emit_f_kernel(Dec d) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= d.nf) return;
  const u64 g = d.fflag[f];
  if (d.fflag[f + 1] == g) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) d.faces_out[3 * g + j] = (int)d.used[d.cluster[d.faces[3 * f + j]]];  // (a survivor's indices are valid)
  d.fsrc[g] = (int)f;
}

}  // namespace dc

namespace {

// slots of an open-addressing table for n entries: a power of two >= 2 n, so a load of at most 1/2
size_t table_slots(size_t n) {
  size_t s = 1024;
  while (s < 2 * n) s <<= 1;
  return s;
}

struct Report {
  int err[4];
  dc::u64 totals[4];  // clusters, output faces, output vertices
  dc::u64 corners;    // quadric representatives: the corner table's total,
  dc::u64 fallbacks;  // the output vertices that keep the mean
};

}  // namespace

// The pool, the input, the three groups of launches, the wait for flags and counts, the normals: see mesh_ops.h.  With the
// caller's host arrays the layout and the launches are what the entry points have always had; a mesh on the device is read
// where it lies, and a corner table it brings takes the place of the quadric stage's own.
int decimate_launch(const char* who, vcy_ctx* c, int64_t n64, int64_t nf64, const float* vertices, const int32_t* faces,
                    const DecimateInput* in, const vcy_decimate_option& o, const float* regularize, bool vertex_normals,
                    bool face_normals, DecimateResult* res) {
  VCY_HIP_CHECK(hipSetDevice(c->device));
  for (vcy::Event& e : c->ev_dc) VCY_HIP_CHECK(e.ensure());
  const bool quadric = regularize != nullptr;
  if (quadric)
    for (vcy::Event& e : c->ev_dq) VCY_HIP_CHECK(e.ensure());
  const size_t n = (size_t)n64, nf = (size_t)nf64, nc = 3 * nf;
  const bool normals = vertex_normals || face_normals;
  const bool own = in == nullptr;  // (positions and faces in this pool)
  const bool own_corners = own || in->corner == nullptr;
  const bool rows = o.mode != VCY_DECIMATE_FIRST;
  const size_t vslots = table_slots(n), fslots = table_slots(nf);

  // [report | faces | positions | keys | vslot | vtable | vflag | cluster | rep | deg | off | cursor | member | cpos | fcanon |
  //  fslot | ftable | fflag | used | scan scratch | the four outputs]: 108 bytes and 8 to 16 of table per vertex, 52 and 8 to
  //  16 per face; quadric representatives add [coff | corners | Qv | fell]: 77 bytes per vertex and 12 per face (the corner
  //  table's counts and cursors are the member table's, free again by then)
  PoolLayout at;
  const size_t at_report = at.take(sizeof(Report)), at_faces = at.take(own ? 4 * nc : 0), at_pos = at.take(own ? 12 * n : 0), at_key = at.take(12 * n),
               at_vslot = at.take(4 * n), at_vtable = at.take(4 * vslots), at_vflag = at.take(8 * (n + 1)), at_cluster = at.take(4 * n),
               at_rep = at.take(4 * n), at_deg = at.take(8 * (n + 1)), at_off = at.take(4 * (n + 1)), at_cursor = at.take(4 * n),
               at_member = at.take(4 * n), at_cpos = at.take(12 * n), at_long = at.take(4 * (n / dc::kLongRow + 1)), at_fcanon = at.take(4 * nc), at_fslot = at.take(4 * nf),
               at_ftable = at.take(4 * fslots), at_fflag = at.take(8 * (nf + 1)), at_used = at.take(8 * (n + 1)),
               at_scan = at.take(8 * scan_scratch_words(std::max(n, nf) + 1)), at_pos_out = at.take(12 * n),
               at_faces_out = at.take(4 * nc), at_vmap = at.take(4 * n), at_fsrc = at.take(4 * nf);
  const size_t at_coff = at.take(quadric && own_corners ? 4 * (n + 1) : 0), at_corner = at.take(quadric && own_corners ? 4 * nc : 0),
               at_qv = at.take(quadric ? 72 * n : 0), at_fell = at.take(quadric ? n : 0);
  VCY_HIP_CHECK(c->d_dc_buf.grow(at.total(), c->stream));
  char* base = (char*)c->d_dc_buf;
  hipStream_t s = c->stream;
  Report* d_report = (Report*)(base + at_report);
  dc::u64* scan = (dc::u64*)(base + at_scan);

  dc::Dec d{};
  d.n = (int)n, d.nf = (int)nf, d.mode = o.mode;
  d.cell = o.cell, d.origin[0] = o.origin[0], d.origin[1] = o.origin[1], d.origin[2] = o.origin[2];
  d.pos = own ? (const float*)(base + at_pos) : in->vertices, d.faces = own ? (const int*)(base + at_faces) : in->faces;
  d.key = (int*)(base + at_key), d.vslot = (int*)(base + at_vslot);
  d.vtable = (int*)(base + at_vtable), d.vmask = (unsigned)(vslots - 1);
  d.vflag = (dc::u64*)(base + at_vflag), d.cluster = (int*)(base + at_cluster), d.rep = (int*)(base + at_rep);
  d.deg = (dc::u64*)(base + at_deg), d.off = (int*)(base + at_off), d.cursor = (int*)(base + at_cursor);
  d.member = (int*)(base + at_member), d.cpos = (float*)(base + at_cpos);
  d.longlist = (int*)(base + at_long), d.long_cap = (int)(n / dc::kLongRow + 1);
  d.fcanon = (int*)(base + at_fcanon), d.fslot = (int*)(base + at_fslot);
  d.ftable = (int*)(base + at_ftable), d.fmask = (unsigned)(fslots - 1);
  d.fflag = (dc::u64*)(base + at_fflag), d.used = (dc::u64*)(base + at_used);
  d.pos_out = (float*)(base + at_pos_out), d.faces_out = (int*)(base + at_faces_out);
  d.vmap = (int*)(base + at_vmap), d.fsrc = (int*)(base + at_fsrc);
  d.err = d_report->err, d.totals = d_report->totals;
  d.regularize = quadric ? *regularize : 0.0f;
  d.coff = own_corners ? (int*)(base + at_coff) : in->coff, d.corner = own_corners ? (int*)(base + at_corner) : in->corner, d.qv = (double*)(base + at_qv);
  d.fell = (unsigned char*)(base + at_fell), d.fallbacks = &d_report->fallbacks;

  if (own) {
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_pos, vertices, 12 * n, hipMemcpyHostToDevice, s));
    VCY_HIP_CHECK(hipMemcpyAsync(base + at_faces, faces, 4 * nc, hipMemcpyHostToDevice, s));
  }

  const dim3 blk(256), grid_v((unsigned)((n + 255) / 256)), grid_v1((unsigned)((n + 256) / 256)),
      grid_f((unsigned)((nf + 255) / 256)), grid_f1((unsigned)((nf + 256) / 256));

  // ---- cluster
  VCY_HIP_CHECK(hipEventRecord(c->ev_dc[0], s));
  VCY_HIP_CHECK(hipMemsetAsync(d_report, 0, sizeof(Report), s));
  VCY_HIP_CHECK(hipMemsetAsync(d.vtable, 0xFF, 4 * vslots, s));  // (contexts are reused: every call starts from empty tables)
  VCY_HIP_CHECK(hipMemsetAsync(d.ftable, 0xFF, 4 * fslots, s));
  VCY_HIP_CHECK(hipMemsetAsync(d.deg, 0, 8 * (n + 1), s));
  VCY_HIP_CHECK(hipMemsetAsync(d.used, 0, 8 * (n + 1), s));
  hipLaunchKernelGGL(dc::dc_keys_kernel, grid_v, blk, 0, s, d);
  hipLaunchKernelGGL(dc::dc_vinsert_kernel, grid_v, blk, 0, s, d);
  hipLaunchKernelGGL(dc::dc_vflag_kernel, grid_v1, blk, 0, s, d);
  VCY_HIP_CHECK(hipGetLastError());
  { const int rc = device_exclusive_scan_u64(d.vflag, (int64_t)n + 1, d_report->totals + 0, scan, s); if (rc != VCY_OK) return rc; }
  if (rows) {
    hipLaunchKernelGGL(dc::dc_vcluster_kernel<true>, grid_v, blk, 0, s, d);
    VCY_HIP_CHECK(hipGetLastError());
    const rows::Table members{d.n, d.n, d.cluster, d.deg, d.off, d.cursor, d.member};  // (counted by dc_vcluster)
    { const int rc = rows::fill(s, members, d_report->totals + 3, scan, true); if (rc != VCY_OK) return rc; }
    const dim3 grid_long((unsigned)std::min<size_t>(n / dc::kLongRow + 1, 1024));  // (workgroups loop over the list)
    if (o.mode == VCY_DECIMATE_NEAREST) {
      hipLaunchKernelGGL(dc::dc_rows_kernel<true>, grid_v, blk, 0, s, d);
      hipLaunchKernelGGL(dc::dc_long_rows_kernel<true>, grid_long, blk, 0, s, d);
    } else {
      hipLaunchKernelGGL(dc::dc_rows_kernel<false>, grid_v, blk, 0, s, d);
      hipLaunchKernelGGL(dc::dc_long_rows_kernel<false>, grid_long, blk, 0, s, d);
    }
    if (quadric) {
      VCY_HIP_CHECK(hipGetLastError());
      VCY_HIP_CHECK(hipEventRecord(c->ev_dq[0], s));
      if (own_corners) {
        const rows::Table corners{d.n, (int)nc, d.faces, d.deg, d.coff, d.cursor, d.corner, d.err + dc::kErrFace};
        const int rc = rows::fill<true>(s, corners, &d_report->corners, scan);
        if (rc != VCY_OK) return rc;
      }
      hipLaunchKernelGGL(dc::dc_qv_kernel, grid_v, blk, 0, s, d);
      hipLaunchKernelGGL(dc::dc_qsolve_kernel, grid_v, blk, 0, s, d);
      VCY_HIP_CHECK(hipEventRecord(c->ev_dq[1], s));
    }
  } else {
    hipLaunchKernelGGL(dc::dc_vcluster_kernel<false>, grid_v, blk, 0, s, d);
  }
  VCY_HIP_CHECK(hipGetLastError());

  // ---- faces
  VCY_HIP_CHECK(hipEventRecord(c->ev_dc[1], s));
  hipLaunchKernelGGL(dc::dc_fmap_kernel, grid_f, blk, 0, s, d);
  hipLaunchKernelGGL(dc::dc_finsert_kernel, grid_f, blk, 0, s, d);
  hipLaunchKernelGGL(dc::dc_fflag_kernel, grid_f1, blk, 0, s, d);
  VCY_HIP_CHECK(hipGetLastError());
  { const int rc = device_exclusive_scan_u64(d.fflag, (int64_t)nf + 1, d_report->totals + 1, scan, s); if (rc != VCY_OK) return rc; }
  { const int rc = device_exclusive_scan_u64(d.used, (int64_t)n + 1, d_report->totals + 2, scan, s); if (rc != VCY_OK) return rc; }

  // ---- emit
  VCY_HIP_CHECK(hipEventRecord(c->ev_dc[2], s));
  if (quadric) hipLaunchKernelGGL((dc::dc_emit_v_kernel<false, true>), grid_v, blk, 0, s, d);
  else if (rows) hipLaunchKernelGGL((dc::dc_emit_v_kernel<false, false>), grid_v, blk, 0, s, d);
  else hipLaunchKernelGGL((dc::dc_emit_v_kernel<true, false>), grid_v, blk, 0, s, d);
  hipLaunchKernelGGL(dc::dc_emit_f_kernel, grid_f, blk, 0, s, d);
  VCY_HIP_CHECK(hipGetLastError());
  VCY_HIP_CHECK(hipEventRecord(c->ev_dc[3], s));

  // ---- the one wait for the launches: flags and counts
  Report r;
  VCY_HIP_CHECK(hipMemcpyAsync(&r, d_report, sizeof(Report), hipMemcpyDeviceToHost, s));
  VCY_HIP_CHECK(hipStreamSynchronize(s));
  if (r.err[dc::kErrFace]) {
    set_error("%s: a face names a vertex outside 0 .. %lld", who, (long long)n64 - 1);
    return VCY_ERR_INVALID_ARG;
  }
  if (r.err[dc::kErrVertex]) {
    set_error("%s: a vertex is not finite or lies 2^30 cells or more from the origin", who);
    return VCY_ERR_INVALID_ARG;
  }
  if (r.err[dc::kErrTable] || (size_t)r.err[dc::kLongCount] > n / dc::kLongRow + 1 || r.totals[0] > n || r.totals[1] > nf || r.totals[2] > r.totals[0]) {
    set_error("%s: a table ran out of slots (%llu clusters, %llu faces, %llu vertices)", who, r.totals[0], r.totals[1], r.totals[2]);
    return VCY_ERR_INTERNAL;
  }
  const size_t nvo = (size_t)r.totals[2], nfo = (size_t)r.totals[1];

  // ---- normals of the output mesh, launched behind the wait
  float *d_fn = nullptr, *d_vn = nullptr;
  VCY_HIP_CHECK(hipEventRecord(c->ev_dc[4], s));
  if (normals && nfo > 0) {
    const int rc = mesh_normals_device(c, (int64_t)nvo, (int64_t)nfo, d.pos_out, d.faces_out, vertex_normals, &d_fn, &d_vn);
    if (rc != VCY_OK) return rc;
  }
  VCY_HIP_CHECK(hipEventRecord(c->ev_dc[5], s));
  *res = DecimateResult{(int64_t)nvo, (int64_t)nfo, (int64_t)r.fallbacks, d.pos_out, d.faces_out, d.vmap, d.fsrc, d_fn,
                        vertex_normals ? d_vn : nullptr};
  return VCY_OK;
}

int decimate_read_times(vcy_ctx* c, bool normals, bool quadric) {
  for (int k = 0; k < 3; ++k) VCY_HIP_CHECK(hipEventElapsedTime(&c->last_decimate_ms[k], c->ev_dc[k], c->ev_dc[k + 1]));
  c->last_decimate_ms[3] = 0.0f;
  if (normals) VCY_HIP_CHECK(hipEventElapsedTime(&c->last_decimate_ms[3], c->ev_dc[4], c->ev_dc[5]));
  if (quadric) VCY_HIP_CHECK(hipEventElapsedTime(&c->last_quadric_ms, c->ev_dq[0], c->ev_dq[1]));
  return VCY_OK;
}

namespace {

// vcy_decimate_mesh[_quadric]: the input from the caller's arrays into the pool, the launches, the results into the
// caller's arrays, sized by the counts; a refused call copies nothing.  `regularize` non-NULL: quadric representatives
// (MEAN, then the quadric stage), their fallbacks into `n_fallback`
int decimate_device(const char* who, vcy_ctx* c, int64_t n64, int64_t nf64, const float* vertices, const int32_t* faces,
                    const vcy_decimate_option& o, const float* regularize, float* vertices_out, int32_t* faces_out,
                    int64_t* n_vertices_out, int64_t* n_faces_out, int32_t* vertex_map, int32_t* face_source,
                    float* vertex_normals_out, float* face_normals_out, int64_t* n_fallback) {
  const size_t n = (size_t)n64;
  hipStream_t s = c->stream;
  DecimateResult r{};
  { const int rc = decimate_launch(who, c, n64, nf64, vertices, faces, nullptr, o, regularize, vertex_normals_out != nullptr, face_normals_out != nullptr, &r); if (rc != VCY_OK) return rc; }
  const size_t nvo = (size_t)r.n_vertices, nfo = (size_t)r.n_faces;
  if (nfo > 0) {
    VCY_HIP_CHECK(hipMemcpyAsync(vertices_out, r.vertices, 12 * nvo, hipMemcpyDeviceToHost, s));
    VCY_HIP_CHECK(hipMemcpyAsync(faces_out, r.faces, 12 * nfo, hipMemcpyDeviceToHost, s));
    if (face_source) VCY_HIP_CHECK(hipMemcpyAsync(face_source, r.face_source, 4 * nfo, hipMemcpyDeviceToHost, s));
    if (vertex_normals_out && r.vertex_normals) VCY_HIP_CHECK(hipMemcpyAsync(vertex_normals_out, r.vertex_normals, 12 * nvo, hipMemcpyDeviceToHost, s));
    if (face_normals_out && r.face_normals) VCY_HIP_CHECK(hipMemcpyAsync(face_normals_out, r.face_normals, 12 * nfo, hipMemcpyDeviceToHost, s));
  }
  if (vertex_map) VCY_HIP_CHECK(hipMemcpyAsync(vertex_map, r.vertex_map, 4 * n, hipMemcpyDeviceToHost, s));
  VCY_HIP_CHECK(hipStreamSynchronize(s));  // (the host arrays are written until here)
  { const int rc = decimate_read_times(c, vertex_normals_out || face_normals_out, regularize != nullptr); if (rc != VCY_OK) return rc; }
  *n_vertices_out = r.n_vertices;
  *n_faces_out = r.n_faces;
  if (n_fallback) *n_fallback = r.n_fallback;
  return VCY_OK;
}

}  // namespace

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_decimate_mesh(vcy_ctx* c, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                      const vcy_decimate_option* option, float* vertices_out, int32_t* faces_out, int64_t* n_vertices_out,
                      int64_t* n_faces_out, int32_t* vertex_map, int32_t* face_source, float* vertex_normals_out,
                      float* face_normals_out) {
  { const int rc = decimate_check_args("vcy_decimate_mesh", n_vertices, n_faces, vertices, faces, option, vertices_out, faces_out, n_vertices_out, n_faces_out); if (rc != VCY_OK) return rc; }
  if (!c) {  // (behind the argument checks: those need no context)
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  for (float& ms : c->last_decimate_ms) ms = 0.0f;
  if (n_vertices == 0 || n_faces == 0) {
    *n_vertices_out = *n_faces_out = 0;
    return VCY_OK;
  }
  const int rc = decimate_device("vcy_decimate_mesh", c, n_vertices, n_faces, vertices, faces, *option, nullptr, vertices_out,
                                 faces_out, n_vertices_out, n_faces_out, vertex_map, face_source, vertex_normals_out,
                                 face_normals_out, nullptr);
  if (rc != VCY_OK) (void)hipStreamSynchronize(c->stream);  // (queued copies still name the caller's arrays)
  return rc;
}

int vcy_decimate_mesh_quadric(vcy_ctx* c, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                              const vcy_decimate_option* option, float regularize, float* vertices_out, int32_t* faces_out,
                              int64_t* n_vertices_out, int64_t* n_faces_out, int32_t* vertex_map, int32_t* face_source,
                              float* vertex_normals_out, float* face_normals_out, int64_t* n_fallback) {
  const char* who = "vcy_decimate_mesh_quadric";
  { const int rc = decimate_check_args(who, n_vertices, n_faces, vertices, faces, option, vertices_out, faces_out, n_vertices_out, n_faces_out, &regularize); if (rc != VCY_OK) return rc; }
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  for (float& ms : c->last_decimate_ms) ms = 0.0f;
  c->last_quadric_ms = 0.0f;
  if (n_vertices == 0 || n_faces == 0) {
    *n_vertices_out = *n_faces_out = 0;
    if (n_fallback) *n_fallback = 0;
    return VCY_OK;
  }
  const int rc = decimate_device(who, c, n_vertices, n_faces, vertices, faces, *option, &regularize, vertices_out, faces_out,
                                 n_vertices_out, n_faces_out, vertex_map, face_source, vertex_normals_out, face_normals_out,
                                 n_fallback);
  if (rc != VCY_OK) (void)hipStreamSynchronize(c->stream);
  return rc;
}

int vcy_last_quadric_ms(const vcy_ctx* c, float* device_ms) {
  if (!c) return VCY_ERR_INVALID_ARG;
  if (device_ms) *device_ms = c->last_quadric_ms;
  return VCY_OK;
}

int vcy_last_decimate_ms(const vcy_ctx* c, float* cluster_ms, float* faces_ms, float* emit_ms, float* normals_ms) {
  if (!c) return VCY_ERR_INVALID_ARG;
  if (cluster_ms) *cluster_ms = c->last_decimate_ms[0];
  if (faces_ms) *faces_ms = c->last_decimate_ms[1];
  if (emit_ms) *emit_ms = c->last_decimate_ms[2];
  if (normals_ms) *normals_ms = c->last_decimate_ms[3];
  return VCY_OK;
}

}  // extern "C"
