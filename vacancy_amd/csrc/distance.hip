// The Euclidean distance field of the hull on the device (vcy_distance_field, vcy_redistance, vcy_last_distance_ms; the
// definitions are in the section "distance field of the hull" of vacancy_hip.h, the serial statement in distance_host.hip).
//
// The chain, all on the context's stream, integers throughout:
//   1. cc_bits   one bit per voxel, 64-voxel words along x (launch_solid_bits, the labelling's and the ray-cast's)
//   2. df_x      one wave per word, a lane per voxel: the distance along the row to the nearest voxel of the other class
//                by clz / ctz on the word and at most two words to either side (R <= 127) -- no search loop.  The bits of
//                a row's last word beyond nx belong to no voxel and are masked out of every word before it is searched.
//                One byte per voxel: the class in bit 7, the distance (1 .. R; 0 = none within R) below it.
//   3. df_axis   along y, then along z.  Lanes run along x, so every global access is a coalesced row segment.  A workgroup
//                stages a tile of 64 x `tile` voxels with its +-R halo in LDS as 16-bit values (class in bit 15, squared
//                distance below it; consecutive lanes read consecutive halves of consecutive banks: no conflicts), then
//                every lane walks d = 1 .. R outward from its voxel and stops as soon as d*d cannot win -- exact, because
//                candidates only grow with d.  Slices beyond the grid are neither staged nor read: the walk is bounded.
//                The y pass writes 16 bits per voxel (2 * 127^2 + 1 fits 15); the z pass writes the result itself:
//                the signed int32 field, or sdf = +-phi where update_num >= 1 (phi from the table the host built with the
//                one formula of distance_field.h), counting the voxels it rewrote: a wave adds up its rows and issues one
//                integer atomic, into one of 1024 counters the host sums (16 M atomics on ONE address cost 195 ms at 1024^3).
// Scratch per voxel: 1 bit + 1 byte + 2 bytes (and the 4 bytes of the field for vcy_distance_field), one grow-only pool.
//
// A z-slab (vcy_distance_slab_begin, vcy_distance_slab_planes, vcy_distance_field_slab, vcy_redistance_slab) runs steps 1, 2
// and the y pass over its own slices alone and KEEPS the y pass's 16-bit values, with room for min(R, what the grid has
// there) planes in front and behind (vcy_ctx::d_df_h, tagged with the iso level, the radius and the state's epoch).  The
// finishing calls copy the neighbours' planes into the two ends and run the z pass as df_window_kernel: the same tile body
// over the longer column, tiles counted from the slab's first slice, results for the slab's slices alone.  The ends hold
// exactly what the grid has within R, so the walk's bounds are the whole grid's own and the results are the whole-grid
// call's, bit for bit.
#include <algorithm>
#include <vector>

#include "distance_field.h"
#include "vcy_internal.h"

namespace vcy {
namespace df {

typedef unsigned long long u64;

constexpr int kLanes = 64;  // a tile's extent along x
constexpr int kCountSlots = 1024;  // counters of rewritten voxels, summed by the host (a power of two)

__global__ __launch_bounds__(256) void df_x_kernel(const u64* __restrict__ bits, int nx, int Wr, int64_t nwords, int R,
                                                   uint8_t* __restrict__ gx) {
  const int lane = threadIdx.x & 63;
  for (int64_t wi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); wi < nwords; wi += (int64_t)gridDim.x * 4) {
    const int64_t row = wi / Wr;
    const int w = (int)(wi - row * Wr);
    const int x = w * 64 + lane;
    if (x >= nx) continue;
    const u64* rb = bits + row * Wr;
    const int c = (int)((rb[w] >> lane) & 1ull);
    const u64 flip = c ? ~0ull : 0ull;
    // the voxels of word k of this row that are of the other class (k in [0, Wr)); padding bits are nobody's
    auto other = [&](int k) -> u64 {
      const int valid = nx - k * 64;
      const u64 m = rb[k] ^ flip;
      return valid < 64 ? m & ((1ull << valid) - 1ull) : m;
    };
    const u64 own = other(w);
    int dl = R + 1, dr = R + 1;
    const u64 lo = own & ((1ull << lane) - 1ull);
    if (lo) {
      dl = lane - (63 - __builtin_clzll(lo));
    } else {
      int base = lane + 1;  // the distance to the last voxel of the word before
      for (int k = w - 1; k >= 0 && base <= R; --k, base += 64) {
        const u64 o = other(k);
        if (o) {
          dl = base + __builtin_clzll(o);
          break;
        }
      }
    }
    const u64 hi = lane == 63 ? 0ull : own & ~((2ull << lane) - 1ull);
    if (hi) {
      dr = __builtin_ctzll(hi) - lane;
    } else {
      int base = 64 - lane;  // the distance to the first voxel of the word behind
      for (int k = w + 1; k < Wr && base <= R; ++k, base += 64) {
        const u64 o = other(k);
        if (o) {
          dr = base + __builtin_ctzll(o);
          break;
        }
      }
    }
    const int d = min(dl, dr);
    gx[row * nx + x] = (uint8_t)((c << 7) | (d <= R ? d : 0));
  }
}

enum Pass { kPassY, kPassField, kPassSdf };

// One workgroup per tile of 64 (x) by `tile` (along the axis) voxels of one line bundle: blockIdx.x the tile along x,
// blockIdx.y along the axis, blockIdx.z the remaining coordinate.  `stride`: voxels between two steps along the axis,
// `outer_stride`: between two values of the remaining coordinate.  LDS: (tile + 2 R) * 64 uint16.  n_written
// (kPassSdf): kCountSlots counters.
// The axis holds n_axis values of `in`; results are emitted for its window [w0, w1) alone, with `out` and `cnt` indexed
// from the window's start, and the tiles are counted from w0.  The whole-grid kernel is the window [0, n_axis); a z-slab's
// z pass (df_window_kernel) the slab's own slices between the planes of its neighbours.
template <int PASS, typename CountT>
__device__ __forceinline__ void df_axis_tile(const void* __restrict__ in, void* __restrict__ out, int nx, int n_axis, int w0,
                                             int w1, int64_t stride, int64_t outer_stride, int tile, int R,
                                             const float* __restrict__ phi, const CountT* __restrict__ cnt,
                                             u64* __restrict__ n_written) {
  extern __shared__ uint16_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = blockIdx.x * kLanes + lane;
  const int a0 = w0 + blockIdx.y * tile;
  const bool live = x < nx;
  const int64_t base = (int64_t)blockIdx.z * outer_stride + x;
  const int far = R * R + 1;
  const int lo = max(a0 - R, 0), hi = min(a0 + tile + R, n_axis);  // (uniform)
  if (live) {
    for (int a = lo + wave; a < hi; a += 4) {
      uint16_t v;
      if (PASS == kPassY) {
        const uint8_t b = ((const uint8_t*)in)[base + (int64_t)a * stride];
        const int d = b & 127;
        v = (uint16_t)(((b >> 7) << 15) | (d ? d * d : far));
      } else {
        v = ((const uint16_t*)in)[base + (int64_t)a * stride];
      }
      lds[(a - a0 + R) * kLanes + lane] = v;
    }
  }
  __syncthreads();
  unsigned int rewritten = 0;  // by this wave (uniform)
  for (int j = wave; j < tile && a0 + j < w1; j += 4) {  // (the bounds are uniform per wave)
    const int a = a0 + j;
    bool wrote = false;
    if (live) {
      const uint16_t* col = lds + (j + R) * kLanes + lane;
      const int mine = col[0];
      const int c = mine >> 15;
      int best = mine & 0x7fff;
      for (int d = 1; d <= R && d * d < best; ++d) {
        if (a - d >= 0) {  // (>= lo: staged)
          const int u = col[-d * kLanes];
          best = min(best, ((u >> 15) != c ? 0 : (u & 0x7fff)) + d * d);
        }
        if (a + d < n_axis) {  // (< hi: staged)
          const int u = col[d * kLanes];
          best = min(best, ((u >> 15) != c ? 0 : (u & 0x7fff)) + d * d);
        }
      }
      const int64_t v = base + (int64_t)(a - w0) * stride;
      if (PASS == kPassY) {
        ((uint16_t*)out)[v] = (uint16_t)((c << 15) | best);  // (best <= the row's own value <= FAR)
      } else {
        if (best > R * R) best = far;
        if (PASS == kPassField) {
          ((int32_t*)out)[v] = c ? -best : best;
        } else if (cnt[v] >= 1) {
          const float p = phi[min(best, R * R)];
          ((float*)out)[v] = c ? -p : p;
          wrote = true;
        }
      }
    }
    if (PASS == kPassSdf) rewritten += (unsigned int)__builtin_popcountll(__ballot(wrote));
  }
  if (PASS == kPassSdf && lane == 0 && rewritten) {
    const unsigned int slot = ((blockIdx.x + 3u * blockIdx.y + 7u * blockIdx.z) * 4u + (unsigned int)wave) & (kCountSlots - 1);
    atomicAdd(n_written + slot, (u64)rewritten);
  }
}

template <int PASS, typename CountT>
__global__ __launch_bounds__(256) void df_axis_kernel(const void* __restrict__ in, void* __restrict__ out, int nx, int n_axis,
                                                      int64_t stride, int64_t outer_stride, int tile, int R,
                                                      const float* __restrict__ phi, const CountT* __restrict__ cnt,
                                                      u64* __restrict__ n_written) {
  df_axis_tile<PASS, CountT>(in, out, nx, n_axis, 0, n_axis, stride, outer_stride, tile, R, phi, cnt, n_written);
}

// The z pass of a z-slab: `in` is the slab's y-pass output with w0 planes of the neighbours below in front and
// n_axis - w1 of those above behind (min(R, what the grid has there) each, so the walk's bounds are the whole grid's own).
template <int PASS, typename CountT>
__global__ __launch_bounds__(256) void df_window_kernel(const uint16_t* __restrict__ in, void* __restrict__ out, int nx,
                                                        int n_axis, int w0, int w1, int64_t stride, int64_t outer_stride,
                                                        int tile, int R, const float* __restrict__ phi,
                                                        const CountT* __restrict__ cnt, u64* __restrict__ n_written) {
  df_axis_tile<PASS, CountT>(in, out, nx, n_axis, w0, w1, stride, outer_stride, tile, R, phi, cnt, n_written);
}

namespace {

int check_call(const vcy_ctx* c, const char* who, int radius) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  { const int rc = check_radius(who, radius); if (rc != VCY_OK) return rc; }
  if (c->z0 == 0 && c->z1 == c->nz && c->halo_lo == 0) return VCY_OK;
  set_error("%s: the context owns z [%d, %d) of %d slices; the distance field needs the whole grid in one context "
            "(a z-slab would need %d slices of its neighbours per seam)", who, c->z0, c->z1, c->nz, radius);
  return VCY_ERR_UNSUPPORTED;
}

template <int PASS, typename CountT>
void launch_axis(vcy_ctx* c, const void* in, void* out, bool along_z, int R, const float* phi, const void* cnt, u64* n_written) {
  // the larger tile where the halo is long: (tile + 2 R) rows are staged for `tile` rows of results
  const int tile = R <= 32 ? 64 : 128;
  const int n_axis = along_z ? c->nz : c->ny, n_outer = along_z ? c->ny : c->nz;
  const int64_t stride = along_z ? c->slice : (int64_t)c->nx, outer_stride = along_z ? (int64_t)c->nx : c->slice;
  const dim3 grid((unsigned)((c->nx + kLanes - 1) / kLanes), (unsigned)((n_axis + tile - 1) / tile), (unsigned)n_outer);
  const size_t lds_bytes = (size_t)(tile + 2 * R) * kLanes * sizeof(uint16_t);  // at most 48 896 bytes
  hipLaunchKernelGGL((df_axis_kernel<PASS, CountT>), grid, dim3(256), lds_bytes, c->stream, in, out, c->nx, n_axis, stride,
                     outer_stride, tile, R, phi, (const CountT*)cnt, n_written);
}

// The chain.  PASS kPassField: the field into the pool, copied to d2_host after the end event; kPassSdf: into the state,
// *n_rewritten from the device's counter.  The state is stored (not fresh) and the caller has declared a write.
int run_chain(vcy_ctx* c, double iso, int R, int pass, int32_t* d2_host, int64_t* n_rewritten) {
  const int nx = c->nx, Wr = (nx + 63) / 64;
  const int64_t n = c->slab_voxels(), nwords = (int64_t)Wr * c->ny * c->nz;
  if (c->ny > 65535 || c->nz > 65535) {  // (a grid dimension of the axis launches)
    set_error("distance field: ny = %d, nz = %d: more than 65535 rows or slices", c->ny, c->nz);
    return VCY_ERR_TOO_MANY_VOXELS;
  }
  const std::vector<float> phi = phi_table(R, c->opt.resolution);
  PoolLayout pool;
  const size_t at_bits = pool.take(sizeof(u64) * (size_t)nwords), at_gx = pool.take((size_t)n);
  const size_t at_h = pool.take(sizeof(uint16_t) * (size_t)n), at_phi = pool.take(sizeof(float) * phi.size());
  const size_t at_count = pool.take(sizeof(u64) * kCountSlots);
  const size_t at_field = pass == kPassField ? pool.take(sizeof(int32_t) * (size_t)n) : 0;
  VCY_HIP_CHECK(c->d_df_buf.grow(pool.total(), c->stream));
  char* p = (char*)c->d_df_buf;
  u64* bits = (u64*)(p + at_bits);
  uint8_t* gx = (uint8_t*)(p + at_gx);
  uint16_t* h = (uint16_t*)(p + at_h);
  float* d_phi = (float*)(p + at_phi);
  u64* d_count = (u64*)(p + at_count);
  VCY_HIP_CHECK(c->ev_df_begin.ensure());
  VCY_HIP_CHECK(c->ev_df_end.ensure());
  VCY_HIP_CHECK(hipMemcpyAsync(d_phi, phi.data(), sizeof(float) * phi.size(), hipMemcpyHostToDevice, c->stream));
  VCY_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(u64) * kCountSlots, c->stream));

  VCY_HIP_CHECK(hipEventRecord(c->ev_df_begin, c->stream));
  { const int rc = launch_solid_bits(c, iso, bits); if (rc != VCY_OK) return rc; }
  hipLaunchKernelGGL(df_x_kernel, dim3((unsigned)std::min<int64_t>((nwords + 3) / 4, 1 << 20)), dim3(256), 0, c->stream, bits, nx,
                     Wr, nwords, R, gx);
  VCY_HIP_CHECK(hipGetLastError());
  launch_axis<kPassY, uint8_t>(c, gx, h, false, R, nullptr, nullptr, nullptr);
  VCY_HIP_CHECK(hipGetLastError());
  if (pass == kPassField) launch_axis<kPassField, uint8_t>(c, h, p + at_field, true, R, nullptr, nullptr, nullptr);
  else if (c->cnt_bytes == 1) launch_axis<kPassSdf, uint8_t>(c, h, c->owned_slab_sdf(), true, R, d_phi, c->owned_slab_cnt(), d_count);
  else if (c->cnt_bytes == 2) launch_axis<kPassSdf, uint16_t>(c, h, c->owned_slab_sdf(), true, R, d_phi, c->owned_slab_cnt(), d_count);
  else launch_axis<kPassSdf, uint32_t>(c, h, c->owned_slab_sdf(), true, R, d_phi, c->owned_slab_cnt(), d_count);
  VCY_HIP_CHECK(hipGetLastError());
  VCY_HIP_CHECK(hipEventRecord(c->ev_df_end, c->stream));
  VCY_HIP_CHECK(hipEventSynchronize(c->ev_df_end));  // (`phi` has been read)
  VCY_HIP_CHECK(hipEventElapsedTime(&c->last_distance_device_ms, c->ev_df_begin, c->ev_df_end));
  if (pass == kPassField) {
    VCY_HIP_CHECK(hipMemcpy(d2_host, p + at_field, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  } else if (n_rewritten) {
    std::vector<u64> counts(kCountSlots);
    VCY_HIP_CHECK(hipMemcpy(counts.data(), d_count, sizeof(u64) * kCountSlots, hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (u64 k : counts) total += (int64_t)k;
    *n_rewritten = total;
  }
  return VCY_OK;
}

// ---- a z-slab: the x and the y pass over its own slices now, the z pass once the neighbours' planes are there ----------

struct SlabHalo {
  int below, above;  // planes of the neighbours in front of and behind the slab's own in vcy_ctx::d_df_h
};

SlabHalo halo_of(const vcy_ctx* c, int R) { return {halo_below(R, c->z0), halo_above(R, c->z1, c->nz)}; }

// the kept planes describe the state as it is, and no queued view is about to change it
bool slab_tag_current(const vcy_ctx* c) { return c->df_epoch >= 0 && c->df_epoch == c->st.epoch && c->pending.empty(); }

int check_slab_ctx(const vcy_ctx* c) {
  if (c) return VCY_OK;
  set_error("voxel grid has not been initialized");
  return VCY_ERR_NOT_INITIALIZED;
}

int check_slab_tag(const vcy_ctx* c, const char* who) {
  if (slab_tag_current(c)) return VCY_OK;
  set_error(c->df_epoch < 0 ? "%s: no vcy_distance_slab_begin on this context"
                            : "%s: the voxel state has been written since vcy_distance_slab_begin", who);
  return VCY_ERR_INVALID_ARG;
}

int slab_begin(vcy_ctx* c, double iso, int R) {
  const int nx = c->nx, ny = c->ny, nzl = c->nz_local(), Wr = (nx + 63) / 64;
  if (ny > 65535 || nzl > 65535) {  // (a grid dimension of the axis launches)
    set_error("vcy_distance_slab_begin: ny = %d, %d slices: more than 65535 rows or slices", ny, nzl);
    return VCY_ERR_TOO_MANY_VOXELS;
  }
  const int64_t n = c->slab_voxels(), nwords = (int64_t)Wr * ny * nzl;
  const SlabHalo halo = halo_of(c, R);
  c->df_epoch = -1;
  VCY_HIP_CHECK(c->d_df_h.grow(sizeof(uint16_t) * (size_t)(c->slice * (halo.below + nzl + halo.above)), c->stream));
  uint16_t* h = (uint16_t*)(void*)c->d_df_h + (int64_t)halo.below * c->slice;
  VCY_HIP_CHECK(c->ev_df_begin.ensure());
  VCY_HIP_CHECK(c->ev_df_end.ensure());
  if (c->st.fresh) {  // nothing carved since the fill: class 0, FAR everywhere, and the lazy fill stays lazy
    VCY_HIP_CHECK(hipEventRecord(c->ev_df_begin, c->stream));
    VCY_HIP_CHECK(hipMemsetD16Async((hipDeviceptr_t)h, (unsigned short)far_of(R), (size_t)n, c->stream));
  } else {
    PoolLayout pool;
    const size_t at_bits = pool.take(sizeof(u64) * (size_t)nwords), at_gx = pool.take((size_t)n);
    VCY_HIP_CHECK(c->d_df_buf.grow(pool.total(), c->stream));
    char* p = (char*)c->d_df_buf;
    u64* bits = (u64*)(p + at_bits);
    uint8_t* gx = (uint8_t*)(p + at_gx);
    VCY_HIP_CHECK(hipEventRecord(c->ev_df_begin, c->stream));
    { const int rc = launch_solid_bits(c, iso, bits); if (rc != VCY_OK) return rc; }
    hipLaunchKernelGGL(df_x_kernel, dim3((unsigned)std::min<int64_t>((nwords + 3) / 4, 1 << 20)), dim3(256), 0, c->stream, bits,
                       nx, Wr, nwords, R, gx);
    VCY_HIP_CHECK(hipGetLastError());
    const int tile = R <= 32 ? 64 : 128;
    const dim3 grid((unsigned)((nx + kLanes - 1) / kLanes), (unsigned)((ny + tile - 1) / tile), (unsigned)nzl);
    hipLaunchKernelGGL((df_axis_kernel<kPassY, uint8_t>), grid, dim3(256), (size_t)(tile + 2 * R) * kLanes * sizeof(uint16_t),
                       c->stream, (const void*)gx, (void*)h, nx, ny, (int64_t)nx, c->slice, tile, R, (const float*)nullptr,
                       (const uint8_t*)nullptr, (u64*)nullptr);
    VCY_HIP_CHECK(hipGetLastError());
  }
  VCY_HIP_CHECK(hipEventRecord(c->ev_df_end, c->stream));
  VCY_HIP_CHECK(hipEventSynchronize(c->ev_df_end));
  VCY_HIP_CHECK(hipEventElapsedTime(&c->last_distance_device_ms, c->ev_df_begin, c->ev_df_end));
  c->df_epoch = c->st.epoch, c->df_iso = iso, c->df_radius = R;
  return VCY_OK;
}

template <int PASS, typename CountT>
void launch_window(vcy_ctx* c, const SlabHalo& halo, void* out, int R, const float* phi, const void* cnt, u64* n_written) {
  const int tile = R <= 32 ? 64 : 128, nzl = c->nz_local();
  // tiles are counted from the window's start: every one of them holds slices of the slab
  const dim3 grid((unsigned)((c->nx + kLanes - 1) / kLanes), (unsigned)((nzl + tile - 1) / tile), (unsigned)c->ny);
  const size_t lds_bytes = (size_t)(tile + 2 * R) * kLanes * sizeof(uint16_t);  // at most 48 896 bytes
  hipLaunchKernelGGL((df_window_kernel<PASS, CountT>), grid, dim3(256), lds_bytes, c->stream,
                     (const uint16_t*)(void*)c->d_df_h, out, c->nx, halo.below + nzl + halo.above, halo.below, halo.below + nzl,
                     c->slice, (int64_t)c->nx, tile, R, phi, (const CountT*)cnt, n_written);
}

// The neighbours' planes into the ends of the kept column, then the z pass over the window.  The tag is current, the
// counts have been checked, and for kPassSdf the state is stored and the caller has declared a write.
int slab_finish(vcy_ctx* c, const uint16_t* below, const uint16_t* above, int pass, int32_t* d2_host, int64_t* n_rewritten) {
  const int R = c->df_radius, nzl = c->nz_local();
  const SlabHalo halo = halo_of(c, R);
  const int64_t n = c->slab_voxels();
  const std::vector<float> phi = phi_table(R, c->opt.resolution);
  PoolLayout pool;
  const size_t at_phi = pool.take(sizeof(float) * phi.size()), at_count = pool.take(sizeof(u64) * kCountSlots);
  const size_t at_field = pass == kPassField ? pool.take(sizeof(int32_t) * (size_t)n) : 0;
  VCY_HIP_CHECK(c->d_df_buf.grow(pool.total(), c->stream));
  char* p = (char*)c->d_df_buf;
  float* d_phi = (float*)(p + at_phi);
  u64* d_count = (u64*)(p + at_count);
  uint16_t* ext = (uint16_t*)(void*)c->d_df_h;
  const size_t plane = sizeof(uint16_t) * (size_t)c->slice;
  if (halo.below) VCY_HIP_CHECK(hipMemcpyAsync(ext, below, plane * halo.below, hipMemcpyHostToDevice, c->stream));
  if (halo.above)
    VCY_HIP_CHECK(hipMemcpyAsync(ext + c->slice * (halo.below + nzl), above, plane * halo.above, hipMemcpyHostToDevice, c->stream));
  VCY_HIP_CHECK(hipMemcpyAsync(d_phi, phi.data(), sizeof(float) * phi.size(), hipMemcpyHostToDevice, c->stream));
  VCY_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(u64) * kCountSlots, c->stream));
  VCY_HIP_CHECK(hipEventRecord(c->ev_df_begin, c->stream));
  if (pass == kPassField) launch_window<kPassField, uint8_t>(c, halo, p + at_field, R, nullptr, nullptr, nullptr);
  else if (c->cnt_bytes == 1) launch_window<kPassSdf, uint8_t>(c, halo, c->owned_slab_sdf(), R, d_phi, c->owned_slab_cnt(), d_count);
  else if (c->cnt_bytes == 2) launch_window<kPassSdf, uint16_t>(c, halo, c->owned_slab_sdf(), R, d_phi, c->owned_slab_cnt(), d_count);
  else launch_window<kPassSdf, uint32_t>(c, halo, c->owned_slab_sdf(), R, d_phi, c->owned_slab_cnt(), d_count);
  VCY_HIP_CHECK(hipGetLastError());
  VCY_HIP_CHECK(hipEventRecord(c->ev_df_end, c->stream));
  VCY_HIP_CHECK(hipEventSynchronize(c->ev_df_end));  // (`phi` and the planes have been read)
  VCY_HIP_CHECK(hipEventElapsedTime(&c->last_distance_device_ms, c->ev_df_begin, c->ev_df_end));
  if (pass == kPassField) {
    VCY_HIP_CHECK(hipMemcpy(d2_host, p + at_field, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  } else if (n_rewritten) {
    std::vector<u64> counts(kCountSlots);
    VCY_HIP_CHECK(hipMemcpy(counts.data(), d_count, sizeof(u64) * kCountSlots, hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (u64 k : counts) total += (int64_t)k;
    *n_rewritten = total;
  }
  return VCY_OK;
}

// what the two finishing calls check alike, nothing touched on a refusal
int check_finish(vcy_ctx* c, const char* who, const uint16_t* below, int n_below, const uint16_t* above, int n_above) {
  { const int rc = check_slab_ctx(c); if (rc != VCY_OK) return rc; }
  { const int rc = check_slab_tag(c, who); if (rc != VCY_OK) return rc; }
  return check_halo(who, c->df_radius, c->z0, c->z1, c->nz, n_below, n_above, below, above);
}

}  // namespace

}  // namespace df
}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_distance_field(vcy_ctx* c, double iso_level, int radius, int32_t* d2_host) {
  { const int rc = df::check_call(c, "vcy_distance_field", radius); if (rc != VCY_OK) return rc; }
  if (!d2_host) {
    set_error("vcy_distance_field: null pointer");
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  c->last_distance_device_ms = 0.0f;
  { const int rc = flush_pending(c); if (rc != VCY_OK) return rc; }
  if (c->st.fresh) {  // nothing carved since the fill: no voxel is solid, and the lazy fill stays lazy
    std::fill(d2_host, d2_host + c->slab_voxels(), (int32_t)df::far_of(radius));
    return VCY_OK;
  }
  return df::run_chain(c, iso_level, radius, df::kPassField, d2_host, nullptr);
}

int vcy_redistance(vcy_ctx* c, double iso_level, int radius, int64_t* n_rewritten) {
  if (n_rewritten) *n_rewritten = 0;
  { const int rc = df::check_call(c, "vcy_redistance", radius); if (rc != VCY_OK) return rc; }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  c->last_distance_device_ms = 0.0f;
  { const int rc = flush_pending(c); if (rc != VCY_OK) return rc; }
  // views_carved bounds every update_num: no voxel is touched, nothing is launched, nothing declared
  if (c->st.fresh || c->st.views_carved == 0) return VCY_OK;
  // touched voxels get a new sdf; the final kernel works on columns along z and does not reduce the brick minima again
  c->st.written(StateWrite::redistance());
  return df::run_chain(c, iso_level, radius, df::kPassSdf, nullptr, n_rewritten);
}

int vcy_distance_slab_begin(vcy_ctx* c, double iso_level, int radius) {
  const char* who = "vcy_distance_slab_begin";
  { const int rc = df::check_slab_ctx(c); if (rc != VCY_OK) return rc; }
  { const int rc = df::check_radius(who, radius); if (rc != VCY_OK) return rc; }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  c->last_distance_device_ms = 0.0f;
  { const int rc = flush_pending(c); if (rc != VCY_OK) return rc; }
  return df::slab_begin(c, iso_level, radius);
}

int vcy_distance_slab_planes(const vcy_ctx* c, int z_begin, int z_end, uint16_t* h_host) {
  const char* who = "vcy_distance_slab_planes";
  { const int rc = df::check_slab_ctx(c); if (rc != VCY_OK) return rc; }
  { const int rc = df::check_slab_tag(c, who); if (rc != VCY_OK) return rc; }
  if ((!h_host && z_begin != z_end) || z_begin < c->z0 || z_end > c->z1 || z_begin > z_end) {
    set_error("%s: slices [%d, %d) are not among the context's own [%d, %d), or a null pointer", who, z_begin, z_end, c->z0, c->z1);
    return VCY_ERR_INVALID_ARG;
  }
  if (z_begin == z_end) return VCY_OK;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const uint16_t* h = (const uint16_t*)(void*)c->d_df_h + c->slice * (df::halo_below(c->df_radius, c->z0) + (z_begin - c->z0));
  // (vcy_distance_slab_begin has waited for its launches)
  VCY_HIP_CHECK(hipMemcpy(h_host, h, sizeof(uint16_t) * (size_t)(c->slice * (z_end - z_begin)), hipMemcpyDeviceToHost));
  return VCY_OK;
}

int vcy_distance_field_slab(vcy_ctx* c, const uint16_t* below, int n_below, const uint16_t* above, int n_above,
                            int32_t* d2_host) {
  const char* who = "vcy_distance_field_slab";
  { const int rc = df::check_finish(c, who, below, n_below, above, n_above); if (rc != VCY_OK) return rc; }
  if (!d2_host) {
    set_error("%s: null pointer", who);
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  c->last_distance_device_ms = 0.0f;
  return df::slab_finish(c, below, above, df::kPassField, d2_host, nullptr);
}

int vcy_redistance_slab(vcy_ctx* c, const uint16_t* below, int n_below, const uint16_t* above, int n_above,
                        int64_t* n_rewritten) {
  if (n_rewritten) *n_rewritten = 0;
  { const int rc = df::check_finish(c, "vcy_redistance_slab", below, n_below, above, n_above); if (rc != VCY_OK) return rc; }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  c->last_distance_device_ms = 0.0f;
  // views_carved bounds every update_num: no voxel is touched, nothing is launched, nothing declared
  if (c->st.fresh || c->st.views_carved == 0) return VCY_OK;
  c->st.written(StateWrite::redistance());  // (the kept planes describe the state before: the tag no longer matches)
  return df::slab_finish(c, below, above, df::kPassSdf, nullptr, n_rewritten);
}

int vcy_last_distance_ms(const vcy_ctx* c, float* device_ms) {
  if (!c || !device_ms) return VCY_ERR_INVALID_ARG;
  *device_ms = c->last_distance_device_ms;
  return VCY_OK;
}

}  // extern "C"
