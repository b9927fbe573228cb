// The voxel state of a context behind the C ABI: the counter widths, the lazy fill, reset, download and upload (whole
// slab, positions, single voxels), the comparison of two slabs, and the halo slices of a z-slab.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vcy_internal.h"

namespace vcy {

// sdf = lowest(), update_num = 0 over slab + halo (reference voxel_carver.cc:339, Voxel ctor)
__global__ void fill_f32_kernel(float* __restrict__ p, float v, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

// update_num from one counter width to another (lazy widening of vcy_ctx::d_cnt; halo packs travel in the final
// width).  Narrowing saturates: it only happens to the two halo slices a slab receives, whose counters are read as
// `update_num >= 1` and nothing else (marching_cubes.cc:88-90, extract_voxel.cc:283-286).
template <typename S, typename D>
__global__ __launch_bounds__(256) void convert_counts_kernel(const S* __restrict__ src, D* __restrict__ dst, int64_t n) {
  int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  constexpr unsigned cap = sizeof(D) == 1 ? 255u : (sizeof(D) == 2 ? 65535u : 0xffffffffu);
  for (; i < n; i += stride) {
    if (i + 4 <= n) {
      S v[4];
      __builtin_memcpy(v, src + i, sizeof(v));  // (both arrays are 16-byte aligned and i is a multiple of 4)
      D o[4];
      for (int k = 0; k < 4; ++k) o[k] = (D)min((unsigned)v[k], cap);
      __builtin_memcpy(dst + i, o, sizeof(o));
    } else {
      for (int64_t k = i; k < n; ++k) dst[k] = (D)min((unsigned)src[k], cap);
    }
  }
}

int convert_counts(hipStream_t stream, const void* src, int sb, void* dst, int db, int64_t n) {
  if (n <= 0) return VCY_OK;
  if (sb == db) {
    VCY_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)n * sb, hipMemcpyDeviceToDevice, stream));
    return VCY_OK;
  }
  const dim3 grid((unsigned)std::min<int64_t>((n + 1023) / 1024, 256 * 32));
#define VCY_CONV(S, D) hipLaunchKernelGGL((convert_counts_kernel<S, D>), grid, dim3(256), 0, stream, (const S*)src, (D*)dst, n)
  if (sb == 1 && db == 2) VCY_CONV(uint8_t, uint16_t);
  else if (sb == 1 && db == 4) VCY_CONV(uint8_t, uint32_t);
  else if (sb == 2 && db == 4) VCY_CONV(uint16_t, uint32_t);
  else if (sb == 2 && db == 1) VCY_CONV(uint16_t, uint8_t);
  else if (sb == 4 && db == 1) VCY_CONV(uint32_t, uint8_t);
  else if (sb == 4 && db == 2) VCY_CONV(uint32_t, uint16_t);
  else {
    set_error("convert_counts: unsupported widths %d -> %d", sb, db);
    return VCY_ERR_INTERNAL;
  }
#undef VCY_CONV
  VCY_HIP_CHECK(hipGetLastError());
  return VCY_OK;
}

// Bytes a counter needs to hold values up to max_count (never more than the final width of the options).
int count_width_for(const vcy_ctx* c, int64_t max_count) {
  if (!c->lazy_count) return c->cnt_bytes_wire;
  const int64_t cap = (int64_t)c->opt.update_option.voxel_max_update_num + 1;  // voxel_carver.cc:447-450
  const int64_t m = std::min(max_count, cap);
  const int w = m <= 255 ? 1 : (m <= 65535 ? 2 : 4);
  return std::min(w, c->cnt_bytes_wire);
}

// Switches d_cnt to `bytes` per counter, converting what it holds: everything, on a fresh slab only a valid halo, and
// nothing at all when the caller is about to overwrite every counter (`keep_contents` false: the robust carve).  The array
// of the other width is KEPT (d_cnt_spare) once both exist: a vcy_reset followed by a carve across the 256th view used to
// pay two allocations of 1 - 2 GB, two device-wide synchronisations (hipFree) and a pipeline stall per cycle.  The
// conversion is ordered on the context's stream like every other access to the counters, so nothing waits here either.
int set_count_width(vcy_ctx* c, int bytes, bool keep_contents) {
  if (bytes == c->cnt_bytes) return VCY_OK;
  const int64_t nvox = c->slice * (int64_t)(c->halo_lo + c->nz_local());
  const size_t need = (size_t)nvox * bytes;
  DeviceBuf<> d_new;
  if (c->d_cnt_spare && c->d_cnt_spare.bytes() >= need) {
    d_new = std::move(c->d_cnt_spare);
  } else {
    VCY_HIP_CHECK(d_new.alloc(need));
  }
  const int64_t keep = !keep_contents ? 0 : !c->st.fresh ? nvox : c->st.halo_valid ? c->slice * (int64_t)c->halo_lo : 0;
  const int rc = convert_counts(c->stream, c->d_cnt, c->cnt_bytes, d_new, bytes, keep);  // (nothing to keep: no launch)
  if (rc != VCY_OK) {
    (void)hipStreamSynchronize(c->stream);
    return rc;  // (d_new goes back to the allocator)
  }
  // the old array becomes the spare (a smaller spare that was passed over goes back to the allocator)
  if (c->d_cnt_spare) {
    (void)hipStreamSynchronize(c->stream);
    (void)c->d_cnt_spare.reset();
  }
  c->d_cnt_spare = std::move(c->d_cnt);
  c->d_cnt = std::move(d_new);
  c->cnt_bytes = bytes;
  return VCY_OK;
}

int ensure_count_width(vcy_ctx* c, int64_t max_count) {
  const int w = count_width_for(c, max_count);
  if (w <= c->cnt_bytes) return VCY_OK;
  return set_count_width(c, w);
}

static void discard_pending(vcy_ctx* c) {
  for (auto& t : c->pending) c->sdf_pool.push_back(std::move(t.d_sdf));
  c->pending.clear();
}

int fill_state(vcy_ctx* c) {
  discard_pending(c);  // whatever they would have carved is wiped
  c->deferred_rc = VCY_OK;
  c->deferred_msg.clear();
  c->st.filled();
  c->fused.forget_live_hint();
  // counters start over at one byte (fresh: nothing to convert; the wide array is kept as the spare)
  if (c->d_cnt && c->cnt_bytes != count_width_for(c, 0)) return set_count_width(c, count_width_for(c, 0));
  return VCY_OK;
}

int materialize(vcy_ctx* c) {
  {
    const int rcf = flush_pending(c);  // every reader of the state comes through here
    if (rcf != VCY_OK) return rcf;
  }
  if (!c->st.fresh) return VCY_OK;
  // only the owned slab: halo slices are written by vcy_halo_install / _unpack
  const int64_t n = c->slab_voxels();
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(fill_f32_kernel, dim3(grid), dim3(256), 0, c->stream, c->owned_slab_sdf(), kInvalidSdf, n);
  VCY_HIP_CHECK(hipGetLastError());
  VCY_HIP_CHECK(hipMemsetAsync(c->owned_slab_cnt(), 0, (size_t)n * c->cnt_bytes, c->stream));
  c->st.stored();
  return VCY_OK;
}

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_reset(vcy_ctx* c) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  return fill_state(c);
}

/* ---- state access ------------------------------------------------------- */

int vcy_download(vcy_ctx* c, float* sdf, int32_t* update_num) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  { int rcm = materialize(c); if (rcm != VCY_OK) return rcm; }
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  const int64_t n = c->slab_voxels();
  if (sdf)
    VCY_HIP_CHECK(hipMemcpy(sdf, c->owned_slab_sdf(), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  if (update_num) {
    std::vector<uint8_t> raw((size_t)n * c->cnt_bytes);
    VCY_HIP_CHECK(hipMemcpy(raw.data(), c->owned_slab_cnt(), raw.size(), hipMemcpyDeviceToHost));
    if (c->cnt_bytes == 1) {
      for (int64_t i = 0; i < n; ++i) update_num[i] = raw[i];
    } else if (c->cnt_bytes == 2) {
      const uint16_t* r = (const uint16_t*)raw.data();
      for (int64_t i = 0; i < n; ++i) update_num[i] = r[i];
    } else {
      std::memcpy(update_num, raw.data(), raw.size());
    }
  }
  return VCY_OK;
}

int vcy_upload(vcy_ctx* c, const float* sdf, const int32_t* update_num) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  // refused before anything is touched: a bad counter leaves the state and everything kept beside it as they were
  const int64_t n = c->slab_voxels();
  int64_t mx = 0;
  if (update_num) {
    const int64_t cap = (int64_t)c->opt.update_option.voxel_max_update_num + 1;
    for (int64_t i = 0; i < n; ++i) {
      const int32_t v = update_num[i];
      if (v < 0 || v > cap) {
        set_error("update_num[%lld]=%d outside [0, voxel_max_update_num+1]", (long long)i, v);
        return VCY_ERR_INVALID_ARG;
      }
      mx = v > mx ? v : mx;
    }
  }
  { int rcm = materialize(c); if (rcm != VCY_OK) return rcm; }
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  // arbitrary state from outside: nothing kept beside it survives
  c->st.written(StateWrite::upload(std::max(c->st.views_carved, mx)));
  if (sdf)
    VCY_HIP_CHECK(hipMemcpy(c->owned_slab_sdf(), sdf, sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
  if (update_num) {
    { const int rcw = ensure_count_width(c, c->st.views_carved); if (rcw != VCY_OK) return rcw; }
    // (a widening converts the old counters on the context's stream; the copy below is not ordered behind that stream and
    // must not be overtaken by it)
    VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<uint8_t> raw((size_t)n * c->cnt_bytes);
    for (int64_t i = 0; i < n; ++i) {
      const int32_t v = update_num[i];
      if (c->cnt_bytes == 1) raw[i] = (uint8_t)v;
      else if (c->cnt_bytes == 2) ((uint16_t*)raw.data())[i] = (uint16_t)v;
      else ((int32_t*)raw.data())[i] = v;
    }
    VCY_HIP_CHECK(hipMemcpy(c->owned_slab_cnt(), raw.data(), raw.size(), hipMemcpyHostToDevice));
  }
  return VCY_OK;
}

int vcy_download_positions(vcy_ctx* c, float* pos) {
  if (!c || !pos) return VCY_ERR_INVALID_ARG;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  std::vector<float> px(c->nx), py(c->ny), pz(c->nz);
  VCY_HIP_CHECK(hipMemcpy(px.data(), c->d_px, sizeof(float) * c->nx, hipMemcpyDeviceToHost));
  VCY_HIP_CHECK(hipMemcpy(py.data(), c->d_py, sizeof(float) * c->ny, hipMemcpyDeviceToHost));
  VCY_HIP_CHECK(hipMemcpy(pz.data(), c->d_pz, sizeof(float) * c->nz, hipMemcpyDeviceToHost));
  int64_t i = 0;
  for (int z = c->z0; z < c->z1; ++z)
    for (int y = 0; y < c->ny; ++y)
      for (int x = 0; x < c->nx; ++x, ++i) {
        pos[3 * i + 0] = px[x];
        pos[3 * i + 1] = py[y];
        pos[3 * i + 2] = pz[z];
      }
  return VCY_OK;
}

/* ---- halo --------------------------------------------------------------- */
// Each rank contributes the LAST two xy-slices of its slab: [sdf slice z1-2][sdf slice
// z1-1][cnt slice z1-2][cnt slice z1-1].  Rank r installs rank r-1's contribution as its
// two halo slices z0-2, z0-1 (cells of layer z0 need slice z0-1; deciding which rank owns
// the marching-cubes vertices on plane z0-1 needs the validity of layer z0-1, i.e. slice
// z0-2 as well).

int64_t vcy_halo_bytes(const vcy_ctx* c) {
  if (!c) return 0;
  // (counters travel at their final width: a pack's size and layout do not depend on how many views a slab has seen)
  return 2 * c->slice * (int64_t)(sizeof(float) + c->cnt_bytes_wire);
}

int vcy_halo_pack(vcy_ctx* c, void* send) {
  if (!c || !send) return VCY_ERR_INVALID_ARG;
  if (c->nz_local() < 2) {
    set_error("a slab needs at least 2 slices to exchange halos");
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  { int rcm = materialize(c); if (rcm != VCY_OK) return rcm; }
  const int64_t s = c->slice;
  const float* sdf_src = c->owned_slab_sdf() + (int64_t)(c->nz_local() - 2) * s;
  const char* cnt_src = (const char*)c->owned_slab_cnt() + (int64_t)(c->nz_local() - 2) * s * c->cnt_bytes;
  VCY_HIP_CHECK(hipMemcpyAsync(send, sdf_src, 2 * s * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return convert_counts(c->stream, cnt_src, c->cnt_bytes, (char*)send + 2 * s * sizeof(float), c->cnt_bytes_wire, 2 * s);
}

int vcy_halo_install(vcy_ctx* c, const void* prev_pack) {
  if (!c) return VCY_ERR_INVALID_ARG;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  if (c->halo_lo == 0) {
    c->st.halo_installed();  // first slab: nothing below
    return VCY_OK;
  }
  if (!prev_pack) return VCY_ERR_INVALID_ARG;
  const int64_t s = c->slice;
  const char* src = (const char*)prev_pack;
  VCY_HIP_CHECK(hipMemcpyAsync(c->d_sdf, src, 2 * s * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  { const int rcc = convert_counts(c->stream, src + 2 * s * sizeof(float), c->cnt_bytes_wire, c->d_cnt, c->cnt_bytes, 2 * s);
    if (rcc != VCY_OK) return rcc; }
  c->st.halo_installed();
  return VCY_OK;
}

int vcy_halo_copy_from(vcy_ctx* c, vcy_ctx* below) {
  if (!c) return VCY_ERR_INVALID_ARG;
  if (c->halo_lo == 0) {
    c->st.halo_installed();
    return VCY_OK;
  }
  if (!below || below->z1 != c->z0 || below->nx != c->nx || below->ny != c->ny ||
      below->cnt_bytes_wire != c->cnt_bytes_wire || below->nz_local() < 2) {
    set_error("vcy_halo_copy_from: `below` is not the slab that ends at z_begin (with >= 2 slices)");
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(below->device));
  { int rcm = materialize(below); if (rcm != VCY_OK) return rcm; }
  VCY_HIP_CHECK(hipStreamSynchronize(below->stream));  // its carve must have finished
  VCY_HIP_CHECK(hipSetDevice(c->device));
  { int rcm = flush_pending(c); if (rcm != VCY_OK) return rcm; }
  const int64_t s = c->slice;
  const float* sdf_src = below->owned_slab_sdf() + (int64_t)(below->nz_local() - 2) * s;
  const char* cnt_src = (const char*)below->owned_slab_cnt() + (int64_t)(below->nz_local() - 2) * s * below->cnt_bytes;
  VCY_HIP_CHECK(hipMemcpyPeerAsync(c->d_sdf, c->device, sdf_src, below->device, 2 * s * sizeof(float), c->stream));
  if (below->cnt_bytes == c->cnt_bytes) {
    VCY_HIP_CHECK(hipMemcpyPeerAsync(c->d_cnt, c->device, cnt_src, below->device, 2 * s * c->cnt_bytes, c->stream));
  } else {
    // Slabs that have not seen the same number of views hold counters of different widths.  Neither array is
    // re-allocated for the exchange (the neighbour's would be, from THIS caller's thread, while its own driver thread may
    // be using it): its two slices travel as they are into a staging buffer of this context and are converted into this
    // slab's width behind the copy -- widening is exact, narrowing saturates, and halo counters are only ever read as
    // `update_num >= 1` (convert_counts_kernel).
    const size_t tmp_need = (size_t)(2 * s) * below->cnt_bytes;
    VCY_HIP_CHECK(c->d_halo_tmp.grow(tmp_need, c->stream));
    VCY_HIP_CHECK(hipMemcpyPeerAsync(c->d_halo_tmp, c->device, cnt_src, below->device, tmp_need, c->stream));
    const int rcc = convert_counts(c->stream, c->d_halo_tmp, below->cnt_bytes, c->d_cnt, c->cnt_bytes, 2 * s);
    if (rcc != VCY_OK) return rcc;
  }
  c->st.halo_installed();
  return VCY_OK;
}

int vcy_halo_unpack(vcy_ctx* c, const void* gathered, int rank, int world) {
  if (!c || !gathered || rank < 0 || rank >= world) return VCY_ERR_INVALID_ARG;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  if (c->halo_lo == 0) {
    c->st.halo_installed();
    return VCY_OK;
  }
  if (rank == 0) {
    set_error("rank 0 must own z_begin == 0");
    return VCY_ERR_INVALID_ARG;
  }
  const int64_t s = c->slice;
  const char* src = (const char*)gathered + (int64_t)(rank - 1) * vcy_halo_bytes(c);
  VCY_HIP_CHECK(hipMemcpyAsync(c->d_sdf, src, 2 * s * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  { const int rcc = convert_counts(c->stream, src + 2 * s * sizeof(float), c->cnt_bytes_wire, c->d_cnt, c->cnt_bytes, 2 * s);
    if (rcc != VCY_OK) return rcc; }
  c->st.halo_installed();
  return VCY_OK;
}

// Voxel state at arbitrary voxel ids (global ids of this slab), gathered on the device.
__global__ void gather_state_kernel(const float* __restrict__ sdf, const void* __restrict__ cnt, int cnt_bytes,
                                    const long long* __restrict__ ids, int64_t n, long long first_id,
                                    float* __restrict__ out_sdf, int* __restrict__ out_cnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long local = ids[i] - first_id;
  out_sdf[i] = sdf[local];
  out_cnt[i] = cnt_bytes == 1 ? (int)((const uint8_t*)cnt)[local]
             : cnt_bytes == 2 ? (int)((const uint16_t*)cnt)[local] : ((const int*)cnt)[local];
}

int vcy_download_voxels(vcy_ctx* c, int64_t n, const int64_t* voxel_ids, float* sdf, int32_t* update_num) {
  if (!c || n < 0 || (n > 0 && (!voxel_ids || !sdf || !update_num))) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  if (n == 0) return VCY_OK;
  const int64_t first = (int64_t)c->z0 * c->slice, last = (int64_t)c->z1 * c->slice;
  for (int64_t i = 0; i < n; ++i)
    if (voxel_ids[i] < first || voxel_ids[i] >= last) {
      set_error("voxel id %lld outside this slab", (long long)voxel_ids[i]);
      return VCY_ERR_INVALID_ARG;
    }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  { int rcm = materialize(c); if (rcm != VCY_OK) return rcm; }
  DeviceBuf<char> d;
  VCY_HIP_CHECK(d.alloc((size_t)n * 16));
  long long* d_ids = (long long*)d;
  float* d_s = (float*)(d + (size_t)n * 8);
  int* d_n = (int*)(d + (size_t)n * 12);
  hipError_t e = hipMemcpyAsync(d_ids, voxel_ids, (size_t)n * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(gather_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       c->owned_slab_sdf(), c->owned_slab_cnt(), c->cnt_bytes, d_ids, n, (long long)first, d_s, d_n);
    e = hipMemcpyAsync(sdf, d_s, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(update_num, d_n, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    set_error("vcy_download_voxels: %s", hipGetErrorString(e));
    return VCY_ERR_HIP;
  }
  return VCY_OK;
}

// Counts voxels whose state differs between two slabs (bit compare of sdf, value compare of update_num).
__device__ __forceinline__ int load_count(const void* cnt, int cnt_bytes, int64_t i) {
  return cnt_bytes == 1 ? (int)((const uint8_t*)cnt)[i]
       : cnt_bytes == 2 ? (int)((const uint16_t*)cnt)[i] : ((const int*)cnt)[i];
}

__global__ __launch_bounds__(256) void state_diff_kernel(const float* __restrict__ sa, const void* __restrict__ ca,
                                                         int cba, const float* __restrict__ sb,
                                                         const void* __restrict__ cb, int cbb, int64_t n,
                                                         unsigned long long* __restrict__ n_diff) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  unsigned local = 0;
  for (; i < n; i += stride) {
    const bool diff = __float_as_uint(sa[i]) != __float_as_uint(sb[i]) || load_count(ca, cba, i) != load_count(cb, cbb, i);
    local += diff ? 1u : 0u;
  }
  const unsigned long long m = __ballot(local != 0);
  if (m) {  // rare: serialise only when something differs
    for (int d = 32; d > 0; d >>= 1) local += __shfl_down(local, d, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(n_diff, (unsigned long long)local);
  }
}

int vcy_state_equal(vcy_ctx* a, vcy_ctx* b, int64_t* n_diff) {
  if (!a || !b || !n_diff) return VCY_ERR_INVALID_ARG;
  if (a->device != b->device || a->nx != b->nx || a->ny != b->ny || a->z0 != b->z0 || a->z1 != b->z1) {
    set_error("vcy_state_equal: the contexts do not own the same slab on the same device");
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(a->device));
  { int rcm = materialize(a); if (rcm != VCY_OK) return rcm; }
  { int rcm = materialize(b); if (rcm != VCY_OK) return rcm; }
  VCY_HIP_CHECK(hipStreamSynchronize(b->stream));
  DeviceBuf<unsigned long long> d;
  unsigned long long h = 0;
  VCY_HIP_CHECK(d.alloc(sizeof(unsigned long long)));
  hipError_t e = hipMemsetAsync(d, 0, sizeof(unsigned long long), a->stream);
  if (e == hipSuccess) {
    const int64_t n = a->slab_voxels();
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(state_diff_kernel, dim3(grid), dim3(256), 0, a->stream, a->owned_slab_sdf(), a->owned_slab_cnt(),
                       a->cnt_bytes, b->owned_slab_sdf(), b->owned_slab_cnt(), b->cnt_bytes, n, d);
    e = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, a->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
  if (e != hipSuccess) {
    set_error("vcy_state_equal: %s", hipGetErrorString(e));
    return VCY_ERR_HIP;
  }
  *n_diff = (int64_t)h;
  return VCY_OK;
}

}  // extern "C"
