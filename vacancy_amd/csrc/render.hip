// Ray-cast of the carved hull into a view: per pixel the first solid voxel on the pixel's ray -- depth, voxel id, entry
// axis -- and the comparison of the hull's silhouette with the input silhouettes (vcy_render_hull / vcy_hull_agreement;
// no reference counterpart -- the definitions are in vacancy_hip.h and restated in numpy in tests/render_ref.py).
//
// The chain, all on the context's stream:
//   1. solid bits     one bit per voxel, 64-voxel words along x: launch_solid_bits, the labelling's first kernel
//   2. rn_occupancy   one bit per 8 x 8 x 8 brick, set when a voxel of the brick is solid; a lane per brick over the bit
//                     words, a wave's 64 answers stored as one ballot
//   3. rn_cast        one lane per pixel, one wave per 8 x 8 pixel tile (neighbouring rays take neighbouring paths), four
//                     tiles per workgroup, the view in blockIdx.z: a batch is one launch.  The plane tables sit in LDS
//                     when they fit.  No atomics: every pixel has one writer.  For vcy_hull_agreement the same kernel ends
//                     in three ballots per wave and one 64-bit atomic add per counter per wave.
// 1 and 2 are kept on the context and redone when StateFlags::epoch or the iso level has moved.
//
// The walk.  The path of a ray is the merge by (t, axis) of three monotone sequences t_a(k) = (P_a[k] - o_a) * inv_a, each
// computed from the integer k.  A lane holds its cell (i_x, i_y, i_z) and the t of the next plane on every axis, and a
// step takes the smallest.  Two shortcuts leave the path's states untouched ("rayskip", on by default):
//   brick    inside a brick without a solid voxel, the next BRICK plane of every axis (k % 8 == 0, or the grid's last
//            plane) is looked up, the earliest of them by (t, axis) is the event E the flat walk would reach with nothing
//            solid before it, and the cell on each other axis after E is the count of that axis' planes that sort before
//            E -- a binary search over the at most 7 planes left in the brick, with the exact comparison of the merge;
//   entry    outside the grid, E is the LATEST of the planes through which the out-of-range axes come into range; no
//            state before E lies inside the grid, and the other axes are counted up to E in the same way.
// Both compare the same floats as the flat walk, so "rayskip" 0 and 1 give the same bits.
//
// z-slabs (vcy_render_hull_slab, the SLAB instances of rn_cast).  A context that owns the slices [z0, z1) renders the
// whole-grid image of the state in which no voxel outside its slices is solid: the ray walks the GLOBAL path -- global
// plane tables, plane indices and start cells --, "inside" is narrowed to z0 <= i_z < z1, the entry jump takes plane z0
// or z1 as the plane through which z comes into range, and the bricks are counted from z0 (brick planes at z0 + 8k,
// capped at z1), as the bit planes and the occupancy bits of a slab are.  The halo slices are never read.  The same
// instances pack one hit bit per pixel: a wave's ballot is its tile's eight row bytes, stored by eight lanes.  The
// images of the slabs are merged on the host (render_merge.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "vcy_internal.h"

namespace vcy {
namespace rn {

typedef unsigned long long u64;

struct Grid {
  int n[3];
  int off[3];        // where an axis' planes start in the table
  int total;         // nx + ny + nz + 3
  int Wr;            // bit words per voxel row
  int nbx, nby;      // bricks along x and y
  int empty;         // nothing has been carved: every ray is a miss, no bit plane exists
  int z0, z1;        // the owned slices (SLAB instances only; bits and occ start at slice z0)
  const u64* bits;
  const u64* occ;
  const float* planes;
};

struct View {          // one per view of a launch, in device memory
  float R[9], t[3];    // w2c
  float fx, fy, cx, cy;
  int ortho, w, h;
  int rx0, ry0, rx1, ry1;
  float* depth;        // any of the three may be null
  long long* voxel;
  uint8_t* axis;
  const uint8_t* mask;  // agreement only
  uint8_t* hits;        // SLAB instances only, may be null: rows of (w + 63) / 64 64-bit words, bit u & 63 of word u >> 6
};

__global__ __launch_bounds__(256) void rn_occupancy_kernel(const u64* __restrict__ bits, int ny, int nz, int Wr, int nbx,
                                                           int nby, int64_t nbricks, u64* __restrict__ occ) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (a wave covers 64 consecutive bricks: one word)
  bool any = false;
  if (b < nbricks) {
    const int bx = (int)(b % nbx);
    const int64_t q = b / nbx;
    const int by = (int)(q % nby), bz = (int)(q / nby);
    const int y1 = min(by * 8 + 8, ny), z1 = min(bz * 8 + 8, nz);
    u64 acc = 0;
    for (int z = bz * 8; z < z1; ++z)
      for (int y = by * 8; y < y1; ++y) acc |= bits[((int64_t)z * ny + y) * Wr + (bx >> 3)];
    any = ((acc >> ((bx & 7) * 8)) & 0xffull) != 0ull;  // (bits past the end of a row are zero)
  }
  const u64 m = __ballot(any);
  if ((threadIdx.x & 63) == 0 && (b >> 6) < ((nbricks + 63) >> 6)) occ[b >> 6] = m;
}

// One axis of one ray.
struct Axis {
  int i;      // cell, -1 .. n
  int s;      // direction of travel, 0: no crossings
  float o, inv;
  float tn;   // t of the next plane, +inf when there is none
};

__device__ __forceinline__ float cross_t(const float* P, int off, int k, const Axis& a) { return (P[off + k] - a.o) * a.inv; }

// the next plane ahead of cell i, or -1
__device__ __forceinline__ int next_plane(const Axis& a, int n) {
  const int k = a.s > 0 ? a.i + 1 : a.i;
  return a.s == 0 || k < 0 || k > n ? -1 : k;
}

__device__ __forceinline__ void set_next(const float* P, int off, int n, Axis& a) {
  const int k = next_plane(a, n);
  a.tn = k < 0 ? INFINITY : cross_t(P, off, k, a);
}

// the start cell: the first k of 0 .. n at which the planes stop lying "on the low side" of the start, minus one
__device__ __forceinline__ void init_axis(const float* P, int off, int n, float o, float d, Axis& a) {
  a.o = o;
  const float inv = 1.0f / d;
  const bool moves = d != 0.0f && isfinite(inv);
  a.inv = moves ? inv : 0.0f;
  a.s = !moves ? 0 : (d > 0.0f ? 1 : -1);
  int lo = 0, hi = n + 1;  // first k in [0, n + 1] where low(k) fails
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float p = P[off + mid];
    const float t = (p - o) * a.inv;
    const bool low = a.s > 0 ? t < 0.0f : (a.s < 0 ? !(t < 0.0f) : p <= o);
    if (low) lo = mid + 1;
    else hi = mid;
  }
  a.i = lo - 1;
  set_next(P, off, n, a);
}

// how many of the next m planes of axis b sort before the event (tE, aE) in the merge
__device__ __forceinline__ int count_before(const float* P, int off, const Axis& a, int m, float tE, bool axis_first) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const int k = a.s > 0 ? a.i + mid : a.i - mid + 1;
    const float t = cross_t(P, off, k, a);
    if (t < tE || (t == tE && axis_first)) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Moves the ray to just behind the event on plane kE[aE] of axis aE; m[b]: the planes of axis b that may lie before it.
__device__ __forceinline__ void jump(const float* P, const Grid& g, Axis (&ax)[3], int aE, float tE, const int (&kE)[3],
                                     const int (&m)[3]) {
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    if (b == aE) {
      ax[b].i = ax[b].s > 0 ? kE[b] : kE[b] - 1;
    } else if (ax[b].s != 0 && m[b] > 0) {
      ax[b].i += ax[b].s * count_before(P, g.off[b], ax[b], m[b], tE, b < aE);
    }
    set_next(P, g.off[b], g.n[b], ax[b]);
  }
}

template <bool LDS, bool SKIP, bool AGREE, bool SLAB>
__global__ __launch_bounds__(256) void rn_cast_kernel(Grid g, const View* __restrict__ views, u64* __restrict__ counts) {
  static_assert(!(AGREE && SLAB), "the slabs' silhouettes are compared on the host, from their hit bits");
  const int zlo = SLAB ? g.z0 : 0, zhi = SLAB ? g.z1 : g.n[2];  // the slices a voxel can be hit in
  extern __shared__ float s_planes[];
  const View& v = views[blockIdx.z];
  if ((int)blockIdx.x * 16 >= v.w || (int)blockIdx.y * 16 >= v.h) return;  // (uniform: the launch is sized for the largest view)
  const float* P = g.planes;
  if (LDS) {
    for (int k = threadIdx.x; k < g.total; k += 256) s_planes[k] = g.planes[k];
    __syncthreads();
    P = s_planes;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), w = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool in_img = u < v.w && w < v.h;
  const bool in_roi = in_img && u >= v.rx0 && u <= v.rx1 && w >= v.ry0 && w <= v.ry1;

  float depth = INFINITY;
  long long voxel = -1;
  int axis = 255;
  if (in_roi && !g.empty) {
    float oc0 = 0.0f, oc1 = 0.0f, dc0 = 0.0f, dc1 = 0.0f;
    if (v.ortho) {
      oc0 = (float)u;
      oc1 = (float)w;
    } else {
      dc0 = ((float)u - v.cx) / v.fx;
      dc1 = ((float)w - v.cy) / v.fy;
    }
    const float q0 = oc0 - v.t[0], q1 = oc1 - v.t[1], q2 = 0.0f - v.t[2];
    Axis ax[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float o = v.R[a] * q0 + v.R[3 + a] * q1 + v.R[6 + a] * q2;
      const float d = v.R[a] * dc0 + v.R[3 + a] * dc1 + v.R[6 + a] * 1.0f;
      finite = finite && isfinite(o) && isfinite(d);
      ax[a].o = o;
      ax[a].inv = d;  // (kept until init_axis below)
    }
    if (finite) {
#pragma unroll
      for (int a = 0; a < 3; ++a) init_axis(P, g.off[a], g.n[a], ax[a].o, ax[a].inv, ax[a]);
      float t_in = 0.0f;
      int a_in = 3;
      int64_t brick_seen = -1;
      bool brick_live = false;
      for (;;) {
        const bool inside = ax[0].i >= 0 && ax[0].i < g.n[0] && ax[1].i >= 0 && ax[1].i < g.n[1] && ax[2].i >= zlo && ax[2].i < zhi;
        if (inside) {
          const int zl = ax[2].i - zlo;  // (slice within the bit planes)
          if (SKIP) {
            const int64_t b = ((int64_t)(zl >> 3) * g.nby + (ax[1].i >> 3)) * g.nbx + (ax[0].i >> 3);
            if (b != brick_seen) {
              brick_seen = b;
              brick_live = (g.occ[b >> 6] >> (b & 63)) & 1ull;
            }
            if (!brick_live) {
              // the brick planes ahead, and the earliest of them
              int kE[3], m[3], aE = -1;
              float tE = INFINITY;
#pragma unroll
              for (int a = 0; a < 3; ++a) {
                if (SLAB && a == 2) kE[a] = ax[a].s > 0 ? min(zlo + (zl | 7) + 1, zhi) : zlo + (zl & ~7);  // bricks from z0
                else kE[a] = ax[a].s > 0 ? min((ax[a].i | 7) + 1, g.n[a]) : (ax[a].i & ~7);
                m[a] = ax[a].s > 0 ? kE[a] - 1 - ax[a].i : ax[a].i - kE[a];
                if (ax[a].s != 0) {
                  const float t = cross_t(P, g.off[a], kE[a], ax[a]);
                  if (t < tE) tE = t, aE = a;  // (ties: the lower axis stays)
                }
              }
              if (aE < 0) break;  // nothing ahead but t = +inf
              jump(P, g, ax, aE, tE, kE, m);
              t_in = tE;
              a_in = aE;
              continue;
            }
          }
          const u64 word = g.bits[((int64_t)zl * g.n[1] + ax[1].i) * g.Wr + (ax[0].i >> 6)];
          if ((word >> (ax[0].i & 63)) & 1ull) {
            depth = t_in == 0.0f ? 0.0f : t_in;
            voxel = ((long long)ax[2].i * g.n[1] + ax[1].i) * g.n[0] + ax[0].i;
            axis = a_in;
            break;
          }
        } else {
          bool gone = false, waiting = false;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const bool below = ax[a].i < (a == 2 ? zlo : 0), above = ax[a].i >= (a == 2 ? zhi : g.n[a]);
            gone = gone || (below && ax[a].s <= 0) || (above && ax[a].s >= 0);
            waiting = waiting || below || above;
          }
          if (gone) break;
          if (SKIP && waiting) {
            // the planes through which the out-of-range axes come into range, and the latest of them
            int kE[3], m[3], aE = -1;
            float tE = -INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              const int lo = a == 2 ? zlo : 0, hi = a == 2 ? zhi : g.n[a];
              kE[a] = ax[a].s > 0 ? lo : hi;
              m[a] = ax[a].s > 0 ? g.n[a] - ax[a].i : ax[a].i + 1;  // (every plane ahead: an axis that is not E may be far past its own entry)
              if (ax[a].i < lo || ax[a].i >= hi) {
                const float t = cross_t(P, g.off[a], kE[a], ax[a]);
                if (t >= tE) tE = t, aE = a;  // (ties: the higher axis is the later one)
              }
            }
            if (aE < 0 || tE == INFINITY) break;
            jump(P, g, ax, aE, tE, kE, m);
            t_in = tE;
            a_in = aE;
            continue;
          }
        }
        // one crossing: the smallest (t, axis)
        int a = 0;
        float t = ax[0].tn;
        if (ax[1].tn < t) t = ax[1].tn, a = 1;
        if (ax[2].tn < t) t = ax[2].tn, a = 2;
        if (t == INFINITY) break;
#pragma unroll
        for (int b = 0; b < 3; ++b)
          if (b == a) {
            ax[b].i += ax[b].s;
            set_next(P, g.off[b], g.n[b], ax[b]);
          }
        t_in = t;
        a_in = a;
      }
    }
  }
  if (in_img) {
    const int64_t px = (int64_t)w * v.w + u;
    if (v.depth) v.depth[px] = depth;
    if (v.voxel) v.voxel[px] = voxel;
    if (v.axis) v.axis[px] = (uint8_t)axis;
  }
  if (SLAB) {
    // the tile's hit bits: byte r of the ballot is row r, bit c of it column c; lanes 0 .. 7 store a row byte each, and
    // behind the last tile of a row of tiles the lanes 8 j + r clear byte j of what is left of the row's last word
    const u64 hb = __ballot(in_roi && voxel >= 0);
    if (v.hits) {
      const int x0 = blockIdx.x * 16 + (wave & 1) * 8, y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane & 7), j = lane >> 3;
      const int row_bytes = ((v.w + 63) >> 6) * 8, at = (x0 >> 3) + j;
      if (x0 < v.w && y < v.h && at < row_bytes && (j == 0 || x0 + 8 >= v.w))
        v.hits[(int64_t)y * row_bytes + at] = j == 0 ? (uint8_t)(hb >> ((lane & 7) * 8)) : (uint8_t)0;
    }
  }
  if (AGREE) {
    const bool mask = in_roi && v.mask[(int64_t)w * v.w + u] != 0;
    const bool hull = voxel >= 0;
    const u64 both = __ballot(mask && hull), only_mask = __ballot(mask && !hull), only_hull = __ballot(in_roi && !mask && hull);
    if (lane == 0) {
      u64* c = counts + 3 * (size_t)blockIdx.z;
      if (both) atomicAdd(c + 0, (u64)__builtin_popcountll(both));
      if (only_mask) atomicAdd(c + 1, (u64)__builtin_popcountll(only_mask));
      if (only_hull) atomicAdd(c + 2, (u64)__builtin_popcountll(only_hull));
    }
  }
}

constexpr int kMaxViewsPerLaunch = 64;
constexpr int kLdsPlanes = 12288;  // floats: the three tables of up to 4095 voxels per axis, 48 KiB

}  // namespace rn

namespace {

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

size_t hit_bytes(const vcy_view& v) { return (((size_t)v.width + 63) / 64) * 8 * (size_t)v.height; }  // packed hit bits of a view

int cell_planes(const float bb_min[3], const float bb_max[3], float resolution, int axis, int n, float* out) {
  std::vector<float> p((size_t)n);
  { const int rc = vcy_axis_positions(bb_min, bb_max, resolution, axis, p.data()); if (rc != VCY_OK) return rc; }
  const double lo = n > 1 ? ((double)p[1] - (double)p[0]) * 0.5 : (double)resolution * 0.5;
  const double hi = n > 1 ? ((double)p[(size_t)n - 1] - (double)p[(size_t)n - 2]) * 0.5 : (double)resolution * 0.5;
  out[0] = (float)((double)p[0] - lo);
  for (int k = 1; k < n; ++k) out[k] = (float)(((double)p[(size_t)k - 1] + (double)p[(size_t)k]) * 0.5);
  out[n] = (float)((double)p[(size_t)n - 1] + hi);
  for (int k = 0; k < n; ++k)
    if (!(out[k] < out[k + 1])) {
      set_error("vcy_cell_planes: the planes %d and %d of axis %d are not increasing (%g, %g)", k, k + 1, axis, (double)out[k],
                (double)out[k + 1]);
      return VCY_ERR_INVALID_ARG;
    }
  return VCY_OK;
}

// Bit planes of the current state at `iso`, when the kept ones describe another state.
int ensure_bits(vcy_ctx* c, double iso) {
  if (c->rn_bits_valid && c->rn_epoch == c->st.epoch && c->rn_iso == iso) return VCY_OK;
  c->rn_bits_valid = false;
  const int Wr = (c->nx + 63) / 64;
  const int nzl = c->nz_local();  // (launch_solid_bits covers the owned slices; bricks are counted from z0)
  const int64_t nwords = (int64_t)Wr * c->ny * nzl;
  const int nbx = (c->nx + 7) / 8, nby = (c->ny + 7) / 8, nbz = (nzl + 7) / 8;
  const int64_t nbricks = (int64_t)nbx * nby * nbz, nocc = (nbricks + 63) / 64;
  VCY_HIP_CHECK(c->d_rn_bits.grow(sizeof(rn::u64) * (size_t)(nwords + nocc), c->stream, false));
  rn::u64* bits = (rn::u64*)c->d_rn_bits;
  { const int rc = launch_solid_bits(c, iso, bits); if (rc != VCY_OK) return rc; }
  hipLaunchKernelGGL(rn::rn_occupancy_kernel, dim3((unsigned)((nocc * 64 + 255) / 256)), dim3(256), 0, c->stream, bits, c->ny,
                     nzl, Wr, nbx, nby, nbricks, bits + nwords);
  VCY_HIP_CHECK(hipGetLastError());
  c->rn_bits_valid = true;
  c->rn_epoch = c->st.epoch;
  c->rn_iso = iso;
  return VCY_OK;
}

int ensure_planes(vcy_ctx* c) {
  if (c->d_rn_planes) return VCY_OK;
  const int n[3] = {c->nx, c->ny, c->nz};
  std::vector<float> all((size_t)(c->nx + c->ny + c->nz + 3));
  size_t at = 0;
  for (int a = 0; a < 3; ++a) {
    const int rc = cell_planes(c->opt.bb_min, c->opt.bb_max, c->opt.resolution, a, n[a], all.data() + at);
    if (rc != VCY_OK) return rc;
    at += (size_t)n[a] + 1;
  }
  DeviceBuf<float> d;
  VCY_HIP_CHECK(d.alloc(sizeof(float) * all.size()));
  if (hipMemcpy(d, all.data(), sizeof(float) * all.size(), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("vcy_render_hull: the copy of the plane tables failed");
    return VCY_ERR_HIP;
  }
  c->d_rn_planes = std::move(d);
  return VCY_OK;
}

// vcy_render_hull (masks == null), vcy_hull_agreement (masks, counts) and vcy_render_hull_slab (slab: any context, hit
// bits) behind their argument checks; depth_dev (render_depth_device: one launch's views): the depth image of every view
// stays in vcy_ctx::d_rn_out, is not copied to the host, and its device address is handed back
int render(vcy_ctx* c, double iso, int n_views, const vcy_view* views, float* const* depth, int64_t* const* voxel,
           uint8_t* const* axis, const uint8_t* const* masks, int64_t* counts, const char* who, bool slab = false,
           uint64_t* const* hits = nullptr, const float** depth_dev = nullptr) {
  if (n_views <= 0 || !views || (masks && !counts) || (depth_dev && (depth || n_views > rn::kMaxViewsPerLaunch))) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_views; ++i) {
    const int rc = check_render_view(&views[i], i);
    if (rc != VCY_OK) return rc;
    if (masks && !masks[i]) {
      set_error("%s: null silhouette", who);
      return VCY_ERR_INVALID_ARG;
    }
  }
  if (!c) {  // (behind the argument checks: those need no context)
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!slab && !(c->z0 == 0 && c->z1 == c->nz && c->halo_lo == 0)) {
    // (the slabs' images are merged by vcy_render_merge_host; these two entry points keep to the whole grid)
    set_error("%s: the context owns z [%d, %d) of %d slices; the ray-cast needs the whole grid in one context", who, c->z0,
              c->z1, c->nz);
    return VCY_ERR_UNSUPPORTED;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  c->last_render_device_ms = 0.0f;
  { const int rc = flush_pending(c); if (rc != VCY_OK) return rc; }
  { const int rc = ensure_planes(c); if (rc != VCY_OK) return rc; }
  VCY_HIP_CHECK(c->ev_rn_begin.ensure());
  VCY_HIP_CHECK(c->ev_rn_end.ensure());

  rn::Grid g{};
  g.n[0] = c->nx, g.n[1] = c->ny, g.n[2] = c->nz;
  g.off[0] = 0, g.off[1] = c->nx + 1, g.off[2] = c->nx + c->ny + 2;
  g.total = c->nx + c->ny + c->nz + 3;
  g.Wr = (c->nx + 63) / 64;
  g.nbx = (c->nx + 7) / 8, g.nby = (c->ny + 7) / 8;
  g.empty = c->st.fresh ? 1 : 0;  // nothing carved since the fill: no voxel is solid, and the lazy fill stays lazy
  g.z0 = c->z0, g.z1 = c->z1;
  g.planes = c->d_rn_planes;
  const bool lds = g.total <= rn::kLdsPlanes;
  const bool skip = c->ray_skip != 0;

  // One launch.  Its copies read `rec` and the caller's silhouettes and write the caller's images asynchronously until the
  // wait at its end: a failure in between is returned through the loop below, which waits before anything is destroyed.
  auto chunk = [&](int first, float* ms_out) -> int {
    const int m = std::min(rn::kMaxViewsPerLaunch, n_views - first);
    // [view records | counters | per view: depth, voxel ids, axes, silhouette]
    std::vector<rn::View> rec((size_t)m);
    std::vector<size_t> at_depth((size_t)m, 0), at_voxel((size_t)m, 0), at_axis((size_t)m, 0), at_mask((size_t)m, 0),
        at_hits((size_t)m, 0);
    size_t bytes = align16(sizeof(rn::View) * (size_t)m);
    const size_t at_counts = bytes;
    bytes += align16(sizeof(rn::u64) * 3 * (size_t)m);
    int wmax = 0, hmax = 0;
    for (int i = 0; i < m; ++i) {
      const vcy_view& v = views[first + i];
      const size_t px = (size_t)v.width * (size_t)v.height;
      if ((depth && depth[first + i]) || depth_dev) at_depth[(size_t)i] = bytes, bytes += align16(px * sizeof(float));
      if (voxel && voxel[first + i]) at_voxel[(size_t)i] = bytes, bytes += align16(px * sizeof(int64_t));
      if (axis && axis[first + i]) at_axis[(size_t)i] = bytes, bytes += align16(px);
      if (masks) at_mask[(size_t)i] = bytes, bytes += align16(px);
      if (hits && hits[first + i]) at_hits[(size_t)i] = bytes, bytes += align16(hit_bytes(v));
      wmax = std::max(wmax, v.width), hmax = std::max(hmax, v.height);
    }
    VCY_HIP_CHECK(c->d_rn_out.grow(bytes, c->stream, false));
    char* base = (char*)c->d_rn_out;
    for (int i = 0; i < m; ++i) {
      const vcy_view& v = views[first + i];
      rn::View& r = rec[(size_t)i];
      for (int row = 0; row < 3; ++row) {
        for (int col = 0; col < 3; ++col) r.R[row * 3 + col] = v.w2c[row * 4 + col];
        r.t[row] = v.w2c[row * 4 + 3];
      }
      r.fx = v.fx, r.fy = v.fy, r.cx = v.cx, r.cy = v.cy;
      r.ortho = v.is_ortho != 0, r.w = v.width, r.h = v.height;
      r.rx0 = v.roi_min[0], r.ry0 = v.roi_min[1], r.rx1 = v.roi_max[0], r.ry1 = v.roi_max[1];
      r.depth = at_depth[(size_t)i] ? (float*)(base + at_depth[(size_t)i]) : nullptr;
      r.voxel = at_voxel[(size_t)i] ? (long long*)(base + at_voxel[(size_t)i]) : nullptr;
      r.axis = at_axis[(size_t)i] ? (uint8_t*)(base + at_axis[(size_t)i]) : nullptr;
      r.mask = masks ? (const uint8_t*)(base + at_mask[(size_t)i]) : nullptr;
      r.hits = at_hits[(size_t)i] ? (uint8_t*)(base + at_hits[(size_t)i]) : nullptr;
      if (masks)
        VCY_HIP_CHECK(hipMemcpyAsync(base + at_mask[(size_t)i], masks[first + i], (size_t)v.width * (size_t)v.height,
                                     hipMemcpyHostToDevice, c->stream));
    }
    VCY_HIP_CHECK(hipMemcpyAsync(base, rec.data(), sizeof(rn::View) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    rn::u64* d_counts = (rn::u64*)(base + at_counts);
    if (masks) VCY_HIP_CHECK(hipMemsetAsync(d_counts, 0, sizeof(rn::u64) * 3 * (size_t)m, c->stream));

    VCY_HIP_CHECK(hipEventRecord(c->ev_rn_begin, c->stream));
    if (!g.empty) {
      const int rc = ensure_bits(c, iso);
      if (rc != VCY_OK) return rc;
      g.bits = (const rn::u64*)c->d_rn_bits;
      g.occ = g.bits + (int64_t)g.Wr * c->ny * c->nz_local();
    }
    const dim3 grid((unsigned)((wmax + 15) / 16), (unsigned)((hmax + 15) / 16), (unsigned)m);
    const size_t shmem = lds ? sizeof(float) * (size_t)g.total : 0;
    const rn::View* d_views = (const rn::View*)base;
#define VCY_RN_CAST(L, S, A) \
  hipLaunchKernelGGL((rn::rn_cast_kernel<L, S, A, false>), grid, dim3(256), shmem, c->stream, g, d_views, d_counts)
#define VCY_RN_CAST_SLAB(L, S) \
  hipLaunchKernelGGL((rn::rn_cast_kernel<L, S, false, true>), grid, dim3(256), shmem, c->stream, g, d_views, d_counts)
    if (slab) {
      if (lds) { if (skip) VCY_RN_CAST_SLAB(true, true); else VCY_RN_CAST_SLAB(true, false); }
      else { if (skip) VCY_RN_CAST_SLAB(false, true); else VCY_RN_CAST_SLAB(false, false); }
    } else if (masks) {
      if (lds) { if (skip) VCY_RN_CAST(true, true, true); else VCY_RN_CAST(true, false, true); }
      else { if (skip) VCY_RN_CAST(false, true, true); else VCY_RN_CAST(false, false, true); }
    } else {
      if (lds) { if (skip) VCY_RN_CAST(true, true, false); else VCY_RN_CAST(true, false, false); }
      else { if (skip) VCY_RN_CAST(false, true, false); else VCY_RN_CAST(false, false, false); }
    }
#undef VCY_RN_CAST
#undef VCY_RN_CAST_SLAB
    VCY_HIP_CHECK(hipGetLastError());
    VCY_HIP_CHECK(hipEventRecord(c->ev_rn_end, c->stream));

    for (int i = 0; i < m; ++i) {
      const vcy_view& v = views[first + i];
      const size_t px = (size_t)v.width * (size_t)v.height;
      if (depth_dev) depth_dev[first + i] = (const float*)(base + at_depth[(size_t)i]);
      else if (at_depth[(size_t)i])
        VCY_HIP_CHECK(hipMemcpyAsync(depth[first + i], base + at_depth[(size_t)i], px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
      if (at_voxel[(size_t)i])
        VCY_HIP_CHECK(hipMemcpyAsync(voxel[first + i], base + at_voxel[(size_t)i], px * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
      if (at_axis[(size_t)i])
        VCY_HIP_CHECK(hipMemcpyAsync(axis[first + i], base + at_axis[(size_t)i], px, hipMemcpyDeviceToHost, c->stream));
      if (at_hits[(size_t)i])
        VCY_HIP_CHECK(hipMemcpyAsync(hits[first + i], base + at_hits[(size_t)i], hit_bytes(v), hipMemcpyDeviceToHost, c->stream));
    }
    if (masks)
      VCY_HIP_CHECK(hipMemcpyAsync(counts + 3 * (size_t)first, d_counts, sizeof(rn::u64) * 3 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    VCY_HIP_CHECK(hipStreamSynchronize(c->stream));  // (the host arrays above are read and written until here)
    VCY_HIP_CHECK(hipEventElapsedTime(ms_out, c->ev_rn_begin, c->ev_rn_end));
    return VCY_OK;
  };
  float ms_total = 0.0f;
  for (int first = 0; first < n_views; first += rn::kMaxViewsPerLaunch) {
    float ms = 0.0f;
    const int rc = chunk(first, &ms);
    if (rc != VCY_OK) {
      (void)hipStreamSynchronize(c->stream);  // (queued copies still name host memory of this call and of the caller)
      return rc;
    }
    ms_total += ms;
  }
  c->last_render_device_ms = ms_total;
  return VCY_OK;
}

}  // namespace

int render_depth_device(vcy_ctx* c, double iso, int n_views, const vcy_view* views, const float** depth_dev, const char* who) {
  return render(c, iso, n_views, views, nullptr, nullptr, nullptr, nullptr, nullptr, who, false, nullptr, depth_dev);
}

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_cell_planes(const float bb_min[3], const float bb_max[3], float resolution, int axis, float* out) {
  if (!bb_min || !bb_max || !out || axis < 0 || axis > 2) {
    set_error("vcy_cell_planes: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  int32_t n[3];
  { const int rc = vcy_compute_dims(bb_min, bb_max, resolution, n); if (rc != VCY_OK) return rc; }
  if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0) {
    set_error("vcy_cell_planes: grid has an empty axis (%d,%d,%d)", n[0], n[1], n[2]);
    return VCY_ERR_INVALID_ARG;
  }
  return cell_planes(bb_min, bb_max, resolution, axis, n[axis], out);
}

int vcy_render_hull(vcy_ctx* c, double iso_level, int n_views, const vcy_view* views, float* const* depth_host,
                    int64_t* const* voxel_host, uint8_t* const* axis_host) {
  return render(c, iso_level, n_views, views, depth_host, voxel_host, axis_host, nullptr, nullptr, "vcy_render_hull");
}

int vcy_render_hull_slab(vcy_ctx* c, double iso_level, int n_views, const vcy_view* views, float* const* depth_host,
                         int64_t* const* voxel_host, uint8_t* const* axis_host, uint64_t* const* hits_host) {
  return render(c, iso_level, n_views, views, depth_host, voxel_host, axis_host, nullptr, nullptr, "vcy_render_hull_slab", true,
                hits_host);
}

int vcy_hull_agreement(vcy_ctx* c, double iso_level, int n_views, const vcy_view* views, const uint8_t* const* masks_host,
                       int64_t* counts) {
  if (!masks_host || !counts) {
    set_error("vcy_hull_agreement: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  return render(c, iso_level, n_views, views, nullptr, nullptr, nullptr, masks_host, counts, "vcy_hull_agreement");
}

int vcy_last_render_ms(const vcy_ctx* c, float* device_ms) {
  if (!c || !device_ms) return VCY_ERR_INVALID_ARG;
  *device_ms = c->last_render_device_ms;
  return VCY_OK;
}

}  // extern "C"
