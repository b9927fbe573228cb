// Device helpers shared by carve_fused_kernel (carve_fused_kernel.h) and the pre-pass kernels (carve_fused.hip): the
// short divisions, the sample and update sequences, tile staging, and the footprint of a brick in a view.  Every unit
// that includes this file gets its own copies (anonymous namespace).
#pragma once
#include "carve_fused.h"

namespace vcy {
namespace {

// Wave priority: everything but the runs over the voxels is short and ends in a memory request (view records,
// window lookups, the next tile, the state) whose latency nothing of this wave can cover; it runs at raised
// priority so that those requests leave as early as possible while the other waves of the SIMD are in their
// runs.  +2 ... 3 % in every mode.
#define VCY_SETPRIO(n) __builtin_amdgcn_s_setprio(n)

// Development build only (-DVCY_PHASE_TIMING, profiles/tools/phase_timing.py): s_memtime ticks of every wave,
// accumulated per phase of the fused kernel.  Slots 0-6: prologue + state load, tile staging, select-free
// view, sure view, checked view, re-bounding after a change, write-back; 7-9: views taken by the three
// loops; 10: waves; 11: views that changed their brick; 12-14: parts of slot 0 (until the kernel arguments
// and axis tables are there, brick_footprints, state + first live set).
#ifdef VCY_PHASE_TIMING
__device__ unsigned long long g_phase_ticks[256][16];
#define VCY_PT_DECL unsigned long long pt_last = __builtin_amdgcn_s_memtime(), pt_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define VCY_PT(slot)                                                  \
  do {                                                                \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();       \
    pt_acc[slot] += t_ - pt_last;                                     \
    pt_last = t_;                                                     \
  } while (0)
#define VCY_PT_COUNT(slot) pt_acc[slot] += 1
#define VCY_PT_FLUSH(lane_)                                                                         \
  do {                                                                                              \
    if ((lane_) == 0)                                                                               \
      for (int q_ = 0; q_ < 16; ++q_) atomicAdd(&g_phase_ticks[blockIdx.x & 255][q_], pt_acc[q_]);  \
  } while (0)
#else
#define VCY_PT_DECL
#define VCY_PT(slot)
#define VCY_PT_COUNT(slot)
#define VCY_PT_FLUSH(lane_)
#endif

// Correctly rounded n/d for normal operands away from the exponent limits: v_rcp_f32 plus the
// refinement steps of the standard fp32 division expansion (without v_div_scale/v_div_fixup).
__device__ __forceinline__ float div_fast(float n, float d) {
  float r = __builtin_amdgcn_rcpf(d);
  const float e = __builtin_fmaf(-d, r, 1.0f);
  r = __builtin_fmaf(e, r, r);
  float q = n * r;
  const float e2 = __builtin_fmaf(-d, q, n);
  q = __builtin_fmaf(e2, r, q);
  const float e3 = __builtin_fmaf(-d, q, n);
  return __builtin_fmaf(e3, r, q);
}

// Shorter sequences for n / d.  They are NOT correct for every pair of floats, but for a given numerator
// they usually are for EVERY denominator: the host checks that exhaustively on the device, once per
// focal length (div_level, carve_fused.hip: all 2^23 significands in each of the 121 binades [2^-60, 2^61) the fast
// path admits), and only then selects the variant.  DIV 2: v_rcp_f32, one multiply, one correction;
// DIV 1: Newton step on the reciprocal first; DIV 0: the full IEEE expansion (div_fast).
// Plain (unpacked) fp32 throughout: on MI355X v_pk_*_f32 issue at half rate AND slow the scalar
// fp32 instructions around them (profiles/r02/valu_ubench.txt), while v_mul/v_fma_f32 issue every 2 cycles.
template <int DIV>
__device__ __forceinline__ float div_view(float n, float d) {
  if (DIV == 0) return div_fast(n, d);
  float r = __builtin_amdgcn_rcpf(d);
  if (DIV == 1) {
    const float e = __builtin_fmaf(-d, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
  }
  const float q = n * r;
  const float e2 = __builtin_fmaf(-d, q, n);
  return __builtin_fmaf(e2, r, q);
}

__device__ __forceinline__ float div_view1(int div, float n, float d) {  // scalar twin, for the checker
  float r = __builtin_amdgcn_rcpf(d);
  if (div == 1) {
    const float e = __builtin_fmaf(-d, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
  }
  const float q = n * r;
  const float e2 = __builtin_fmaf(-d, q, n);
  return __builtin_fmaf(e2, r, q);
}

// 2^-60 <= z <= 2^60 (also false for negative z, NaN, inf, 0)
__device__ __forceinline__ bool in_fast_div_range(float z) {
  const unsigned lo = 0x21800000u;  // 2^-60
  const unsigned hi = 0x5d800000u;  // 2^60
  return (__float_as_uint(z) - lo) <= (hi - lo);
}

typedef const float __attribute__((address_space(1))) * gfloat_ptr;  // known-global loads
// base[idx] for idx < 2^30 with the BYTE offset formed in 32 bits: where `base` is uniform the load then takes a scalar
// base and one 32-bit vector offset (global_load_dword v, v, s[..]) instead of a 64-bit vector address
__device__ __forceinline__ float load_u32_index(gfloat_ptr base, unsigned idx) {
  typedef const char __attribute__((address_space(1))) * gchar_ptr;
  return *(gfloat_ptr)((gchar_ptr)base + (idx << 2));
}
typedef const float __attribute__((address_space(4))) * cfloat_ptr;  // read-only: scalar loads
// Generic sample for a voxel the staged tile does not cover (rare): global-memory taps and the
// full ROI / outside-image semantics of carve_common.h.  Kept out of line so that the hot loop
// stays small.
__device__ __attribute__((noinline)) bool sample_generic(const ViewParams* v, ModeParams m, float px,
                                                         float py, float pz, float* dist) {
  return view_distance<true, 0, 0, false, false>(*v, m, px, py, pz, dist);
}

// LDS traffic inside one wave needs ordering against the compiler only (DS ops of a wave are
// executed in issue order).
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Correctly rounded 1.0f / m for the integers m = 1 .. 65536 (update_num + 1 of a u8 / u16 counter):
// v_rcp_f32 and ONE Newton step.  Unlike div_fast this is not correct for every float; that it is for
// every m in the range is checked exhaustively on the device by vcy_selftest (and by the GPU tests).
__device__ __forceinline__ float rcp_count(float m) {
  const float r = __builtin_amdgcn_rcpf(m);
  const float e = __builtin_fmaf(-m, r, 1.0f);
  return __builtin_fmaf(e, r, r);
}

// Branch-free voxel update (select form of fuse() in carve_common.h): first touch
// (voxel_carver.cc:482-486), UpdateVoxelMax (:78-86) or UpdateVoxelWeightedAverage (:88-95).
template <int UPDATE>
__device__ __forceinline__ bool apply_sample(bool ok, float dist, float wgt, float& s, int& n) {
  if (UPDATE == VCY_UPDATE_MAX) {
    const bool take = ok && (n < 1 || dist > s);
    s = take ? dist : s;
    n += take ? 1 : 0;
    return take;
  } else if (UPDATE == kUpdateWaUnitWeight) {
    // voxel_update_weight == 1: w * x == x exactly, and the denominator is the integer n + 1
    const float inv_denom = rcp_count((float)(n + 1));
    const float avg = ((float)n * s + dist) * inv_denom;
    const float ns = (n < 1) ? dist : avg;
    s = ok ? ns : s;
    n += ok ? 1 : 0;
  } else {
    const float inv_denom = div_fast(1.0f, wgt * (float)(n + 1));
    const float avg = (wgt * (float)n * s + wgt * dist) * inv_denom;
    const float ns = (n < 1) ? dist : avg;
    s = ok ? ns : s;
    n += ok ? 1 : 0;
  }
  return ok;
}

// ---- update sequences of the fast path ---------------------------------------------------------
// Measured on MI355X (profiles/r02/valu_ubench.txt): a compare / select / carry chain through VCC (the
// VOPC / VOP2 encodings) issues in about 3.5 cycles per instruction and overlaps with full-rate fp32
// instructions of other voxels; the same chain through an arbitrary SGPR pair (VOP3 encodings, what the
// compiler picks once several voxels are in flight) takes 7 per instruction, and an EXEC-masked variant
// (v_cmpx) more.  The chains are therefore written out with VCC.
//
// UpdateVoxelMax for a voxel that has been touched before (voxel_carver.cc:78-86):
//   if (dist > sdf) { sdf = dist; ++update_num; }      -- NaN compares false, -0 == +0 stay put
// `took` accumulates the lanes that changed.
__device__ __forceinline__ void update_max_touched(float dist, float& s, int& n, unsigned long long& took) {
  asm("v_cmp_gt_f32_e32 vcc, %[d], %[s]\n\t"
      "s_or_b64 %[took], %[took], vcc\n\t"
      "v_cndmask_b32_e32 %[s], %[s], %[d], vcc\n\t"
      "v_addc_co_u32_e32 %[n], vcc, 0, %[n], vcc"
      : [s] "+v"(s), [n] "+v"(n), [took] "+s"(took)
      : [d] "v"(dist)
      : "vcc");
}

// UpdateVoxelWeightedAverage with voxel_update_weight == 1 (voxel_carver.cc:88-95) behind the truncation
// skip (:478), for a voxel whose counter is kept as a float `fn` (exact below 2^24):
//   if (!(dist < -1)) { sdf = (fn * sdf + dist) * (1 / (fn + 1)); fn += 1; }
// 1 / (fn + 1) is rcp_count() -- v_rcp_f32 and one Newton step, the correctly rounded quotient for every
// count a u8 / u16 counter can hold (vcy_selftest).  Requires "update_num == 0 implies sdf == lowest()"
// (state only ever written by the fill and the carve kernels): then the first touch needs no special
// case, (0 * sdf + dist) * 1 == dist bit for bit (0 * lowest() = -0, -0 + dist = dist).
template <bool TRUNC>
__device__ __forceinline__ void update_wa_unit(float dist, float& s, float& fn, unsigned long long& took) {
  const float f1 = fn + 1.0f;
  const float avg = (fn * s + dist) * rcp_count(f1);
  if (TRUNC) {
    asm("v_cmp_ngt_f32_e32 vcc, -1.0, %[d]\n\t"   // !(-1 > d)  ==  !(d < -1), true for NaN like the reference
        "s_or_b64 %[took], %[took], vcc\n\t"
        "v_cndmask_b32_e32 %[s], %[s], %[avg], vcc\n\t"
        "v_cndmask_b32_e32 %[fn], %[fn], %[f1], vcc"
        : [s] "+v"(s), [fn] "+v"(fn), [took] "+s"(took)
        : [d] "v"(dist), [avg] "v"(avg), [f1] "v"(f1)
        : "vcc");
  } else {
    s = avg;
    fn = f1;
  }
}

typedef float f4 __attribute__((ext_vector_type(4)));
typedef f4 __attribute__((address_space(3))) lds_float4;

// The weighted-average kernels keep update_num as a float in registers (exact below 2^24; it is converted
// at the load and the store of the brick): (float)n and (float)(n + 1) of the reference's formula are
// then fn and fn + 1 without conversions.
template <int UPDATE>
__device__ __forceinline__ bool apply_sample(bool ok, float dist, float wgt, float& s, float& fn) {
  const float f1 = fn + 1.0f;
  float avg;
  if (UPDATE == kUpdateWaUnitWeight) {
    avg = (fn * s + dist) * rcp_count(f1);
  } else {
    avg = (wgt * fn * s + wgt * dist) * div_fast(1.0f, wgt * f1);
  }
  const float ns = (fn < 1.0f) ? dist : avg;
  s = ok ? ns : s;
  fn = ok ? f1 : fn;
  return ok;
}

// q / d for 0 <= q < 4096, 1 <= d <= 1024, given inv = 1.0f / d: (q + 0.5) / d is never within
// 0.5 / d of an integer, far more than the float rounding of the product.
__device__ __forceinline__ int div_small(int q, float inv) { return (int)(((float)q + 0.5f) * inv); }

typedef float __attribute__((address_space(3))) lds_float;
typedef uint32_t __attribute__((address_space(3))) lds_u32;

// Raw tile of view `v` into the wave-private LDS buffer `buf` (256 floats): pixel (i, j) of the tile =
// image pixel (min(tx0 + i, roi_max.x), min(ty0 + j, roi_max.y)), for the th + 1 <= 16 rows the taps reach.
// Asynchronous: the data is in LDS once the wave's vmcnt has drained (raw_tile_wait).
// raw_prefetch_rows: the requests, given the tile's uniform origin and height.
__device__ __forceinline__ void raw_prefetch_rows(const ViewParams& v, int th, int tx0, int ty0, int lane, float* buf) {
  gfloat_ptr img = (gfloat_ptr)v.sdf;
  const unsigned width = (unsigned)v.width;
  lds_float* dst = (lds_float*)buf;
  if (tx0 + 15 <= v.roi_max_xi && ty0 + 15 <= v.roi_max_yi) {
    // The usual case (uniform test): the whole 16 x 16 window lies inside the ROI, nothing is clamped.  The
    // address is a scalar base per group of four rows plus one per-lane offset that only depends on the
    // image width: one vector instruction per load.
    const unsigned lane_off = __umul24(width, (unsigned)lane >> 4) + ((unsigned)lane & 15u);
    gfloat_ptr base = img + (__umul24(width, (unsigned)ty0) + (unsigned)tx0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (4 * r <= th)  // uniform: rows 4 r .. 4 r + 3 hold a tap row (taps reach rows 0 .. th)
        __builtin_amdgcn_global_load_lds(base + (size_t)(4 * r) * width + lane_off, dst + 64 * r, 4, 0, 0);
    }
    return;
  }
  const unsigned xx = (unsigned)min(tx0 + (lane & 15), v.roi_max_xi);
  const int yl = ty0 + (lane >> 4);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (4 * r <= th) {
      const unsigned yy = (unsigned)min(yl + 4 * r, v.roi_max_yi);
      __builtin_amdgcn_global_load_lds(img + (__umul24(width, yy) + xx), dst + 64 * r, 4, 0, 0);
    }
  }
}
__device__ __forceinline__ void raw_prefetch(const ViewParams& v, const TileInfo& ti, int lane, float* buf) {
#ifdef VCY_FLOOR_NO_TILE_LOADS  // development build (issue floor, profiles/tools/issue_floor.sh): the taps read whatever LDS holds
  return;
#endif
  // (opaque: lane >> 4 and lane & 15 are formed here, every time -- hoisted out of the view loop they were two more
  // registers live through every view, and the weighted-average kernels spilled exactly those to scratch)
  asm volatile("" : "+v"(lane));
  const int nq = __builtin_amdgcn_readfirstlane(ti.nq);
  if (nq == 0) return;
  const int th = __builtin_amdgcn_readfirstlane(ti.th);
  const int tx0 = __builtin_amdgcn_readfirstlane(ti.tx0);
  const int ty0 = __builtin_amdgcn_readfirstlane(ti.ty0);
  raw_prefetch_rows(v, th, tx0, ty0, lane, buf);
}
// ... for a wave that holds the record's fields as scalars (unpack_footprint_scalar): nothing to make uniform
__device__ __forceinline__ void raw_prefetch(const ViewParams& v, const FootprintFields& f, int lane, float* buf) {
#ifdef VCY_FLOOR_NO_TILE_LOADS
  return;
#endif
  asm volatile("" : "+v"(lane));  // (as above)
  if (f.nq == 0) return;
  // The same requests as raw_prefetch_rows makes -- one per group of four rows that holds a tap row (taps reach rows
  // 0 .. th) -- entered at the last group and falling through to the first: one forward branch on the uniform group
  // count instead of a test in front of every request.  (Requests complete in order whichever is issued first.)
  gfloat_ptr img = (gfloat_ptr)v.sdf;
  const unsigned width = (unsigned)v.width;
  lds_float* dst = (lds_float*)buf;
  const int groups = (f.th >> 2) + 1;
  if (f.tx0 + 15 <= v.roi_max_xi && f.ty0 + 15 <= v.roi_max_yi) {  // (uniform) nothing is clamped
    const unsigned lane_off = __umul24(width, (unsigned)lane >> 4) + ((unsigned)lane & 15u);
    gfloat_ptr base = img + (__umul24(width, (unsigned)f.ty0) + (unsigned)f.tx0);
    switch (groups) {
      default: __builtin_amdgcn_global_load_lds(base + (size_t)12 * width + lane_off, dst + 192, 4, 0, 0); [[fallthrough]];
      case 3: __builtin_amdgcn_global_load_lds(base + (size_t)8 * width + lane_off, dst + 128, 4, 0, 0); [[fallthrough]];
      case 2: __builtin_amdgcn_global_load_lds(base + (size_t)4 * width + lane_off, dst + 64, 4, 0, 0); [[fallthrough]];
      case 1: __builtin_amdgcn_global_load_lds(base + lane_off, dst, 4, 0, 0);
    }
    return;
  }
  const unsigned xx = (unsigned)min(f.tx0 + (lane & 15), v.roi_max_xi);
  const int yl = f.ty0 + (lane >> 4);
  auto row = [&](int r) {
    const unsigned yy = (unsigned)min(yl + 4 * r, v.roi_max_yi);
    __builtin_amdgcn_global_load_lds(img + (__umul24(width, yy) + xx), dst + 64 * r, 4, 0, 0);
  };
  switch (groups) {
    default: row(3); [[fallthrough]];
    case 3: row(2); [[fallthrough]];
    case 2: row(1); [[fallthrough]];
    case 1: row(0);
  }
}

// ... for the view step of the instances that keep their records (carve_fused_kernel, kRecRegs): the two words of the
// record as scalars, a record that HAS a tile (footprint_has_tile), and the view through the constant address space.
// What differs from the form above is what it costs the scalar unit, not what it requests:
//  - the view's four fields are read into locals before the first test, so they are ONE batch of scalar loads behind one
//    wait (behind the `&&` of the clamp test the second bound was a scalar-cache round trip of its own);
//  - the clamp test is one comparison (footprint_window_unclamped);
//  - every request takes ONE scalar base, the tile's origin in the image, and a 32-bit vector offset in bytes: the
//    lane's own, plus four image rows per row group (one vector add where the scalar unit widened a product and added
//    a 64-bit pair per group; an image is at most 2^28 bytes: fused_eligible).
typedef const ViewParams __attribute__((address_space(4))) * cview_ptr;
__device__ __forceinline__ void raw_prefetch_step(cview_ptr v, uint32_t ub_word, uint32_t tile_word, int lane, float* buf) {
#ifdef VCY_FLOOR_NO_TILE_LOADS
  return;
#endif
  asm volatile("" : "+v"(lane));  // (as above)
  typedef const char __attribute__((address_space(1))) * gchar_ptr;
  const int roi_max_xi = v->roi_max_xi, roi_max_yi = v->roi_max_yi;
  const unsigned width = (unsigned)v->width;
  gchar_ptr img = (gchar_ptr)v->sdf;
  const int tx0 = footprint_tx0(tile_word), ty0 = footprint_ty0(tile_word);
  const int groups = footprint_row_groups(ub_word);
  lds_float* dst = (lds_float*)buf;
  if (footprint_window_unclamped(tx0, ty0, roi_max_xi, roi_max_yi)) {  // (uniform) nothing is clamped
    gchar_ptr origin = img + tile_origin_bytes(width, tx0, ty0);
    const unsigned four_rows = width * 16u;  // (bytes)
    unsigned off = (__umul24(width, (unsigned)lane >> 4) + ((unsigned)lane & 15u)) << 2;  // this lane's pixel of group 0
    auto request = [&](unsigned r) {
      if (r > 0) off += four_rows;
      __builtin_amdgcn_global_load_lds((gfloat_ptr)(origin + off), dst + 64 * r, 4, 0, 0);
    };
    // (nested tests instead of a switch that falls through, which came out of the compiler as lane-mask flags tested in
    // front of every request; first group first, so that no request is shared with the clamped form below -- merged,
    // the shared one took a 64-bit vector address)
    request(0);
    if (groups > 1) {
      request(1);
      if (groups > 2) {
        request(2);
        if (groups > 3) request(3);
      }
    }
    return;
  }
  const unsigned xx = (unsigned)min(tx0 + (lane & 15), roi_max_xi);
  const int yl = ty0 + (lane >> 4);
  auto row = [&](int r) {
    const unsigned yy = (unsigned)min(yl + 4 * r, roi_max_yi);
    __builtin_amdgcn_global_load_lds((gfloat_ptr)img + (__umul24(width, yy) + xx), dst + 64 * r, 4, 0, 0);
  };
  switch (groups) {
    default: row(3); [[fallthrough]];
    case 3: row(2); [[fallthrough]];
    case 2: row(1); [[fallthrough]];
    case 1: row(0);
  }
}

__device__ __forceinline__ void raw_tile_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// min over the wave (NaN operands are ignored, like the `dist > s` test ignores them): six DPP
// v_min_f32 (row reduction, then row_bcast 15 / 31) and one readlane.  Written in assembly because
// the compiler expands a DPP move + canonicalise + min per step.  ONE block: the s_nop 1 in front of every
// step is the VALU-write -> DPP-read hazard (two wait states), which the assembler does not see inside an
// asm block -- and as six blocks the compiler, which does not see into them either, put an s_nop of its own
// around every one.
__device__ __forceinline__ float wave_min(float v) {
#define VCY_DPP_MIN(CTRL) "s_nop 1\n\tv_min_f32_dpp %0, %0, %0 " CTRL "\n\t"
  asm volatile(VCY_DPP_MIN("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
               VCY_DPP_MIN("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
               VCY_DPP_MIN("row_half_mirror row_mask:0xf bank_mask:0xf")
               VCY_DPP_MIN("row_mirror row_mask:0xf bank_mask:0xf")      // every lane of a 16-lane row holds the row minimum
               VCY_DPP_MIN("row_bcast:15 row_mask:0xa bank_mask:0xf")    // rows 1, 3 <- min(own, row 0 / 2)
               VCY_DPP_MIN("row_bcast:31 row_mask:0xc bank_mask:0xf")    // rows 2, 3 <- min(own, row 1): lane 63 = all
               : "+v"(v));
#undef VCY_DPP_MIN
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 63));
}

// Fills a whole (big) tile in place: pixel (i, j) of the (tw + 1) x (th + 1) window = image pixel
// (min(tx0 + i, roi_max.x), min(ty0 + j, roi_max.y)).  Every group of 64 consecutive tile pixels is one
// LDS-direct request (lane L -> tile element 64 r + L); all requests are issued before the one wait.
__device__ __forceinline__ void tile_fill(const ViewParams& v, const TileInfo& ti, int lane, float* tile) {
  const int nq = __builtin_amdgcn_readfirstlane(ti.nq);
  if (nq == 0) return;
  const int tw = __builtin_amdgcn_readfirstlane(ti.tw), th = __builtin_amdgcn_readfirstlane(ti.th);
  const int tx0 = __builtin_amdgcn_readfirstlane(ti.tx0);
  const int ty0 = __builtin_amdgcn_readfirstlane(ti.ty0);
  const float inv_pitch = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(ti.inv_tw)));
  const int pitch = tw + 1, npx = pitch * (th + 1);
  gfloat_ptr img = (gfloat_ptr)v.sdf;
  const unsigned width = (unsigned)v.width;
  lds_float* dst = (lds_float*)tile;
  for (int q0 = 0; q0 < npx; q0 += 64) {  // (uniform)
    const int q = q0 + lane;
    if (q < npx) {  // lanes beyond the window request nothing (and write nothing)
      const int j = div_small(q, inv_pitch), i = q - j * pitch;
      const unsigned xx = (unsigned)min(tx0 + i, v.roi_max_xi), yy = (unsigned)min(ty0 + j, v.roi_max_yi);
      __builtin_amdgcn_global_load_lds(img + (__umul24(width, yy) + xx), dst + q0, 4, 0, 0);
    }
  }
  raw_tile_wait();
}

// ---- the upper bound of a footprint's samples, from the window-maximum planes ------------------------------------------
// Two callers make these lookups: footprint_of (the pre-pass, the kernel prologues that bound their footprints
// themselves, the slab planner) and the prologue of the carve kernels that keep their records, where a launch reuses the
// records of an earlier one and only their bounds are stale (kStateStaleBounds).  Both go through the helpers below --
// which pixels a tap of the tile can read, how the windows are placed over them, the lookups, the bound and (carve_fused.h:
// pack_footprint_ub) its truncation into the record -- so what the second caller finds IS what the pre-pass would write.
//
// The pixels a tap of the tile [tx0, tx1] x [ty0, ty1] can read are pw x ph (one more column and row, up to the ROI's
// last); window maxima of side k = 8 when both sides reach 8, else 4; nxw x nyw windows placed inside that rectangle (a
// side shorter than k gets one window that sticks out of it: a maximum over more pixels is still an upper bound, and the
// planes are filled well beyond any footprint, FusedView::wrect).
struct FootprintWindows {
  int pw, ph;
  int L;         // log2 of the windows' side: 3 or 2
  int nxw, nyw;  // windows along x and y
};
__device__ __forceinline__ FootprintWindows footprint_windows(int tx0, int ty0, int tx1, int ty1, int roi_max_xi,
                                                              int roi_max_yi) {
  FootprintWindows fw;
  fw.pw = min(tx1 + 1, roi_max_xi) - tx0 + 1;
  fw.ph = min(ty1 + 1, roi_max_yi) - ty0 + 1;
  fw.L = min(fw.pw, fw.ph) >= 8 ? 3 : 2;
  const int k = 1 << fw.L;
  fw.nxw = (fw.pw + k - 1) >> fw.L, fw.nyw = (fw.ph + k - 1) >> fw.L;
  return fw;
}
// The lookups: t[0..9) receive window maxima whose maximum is the maximum over the rectangle (entries that are not
// requested hold -inf).  `plane_off`: the plane's offset from `wm` in elements, folded into a 32-bit index (images are at
// most 8192 x 8192 and there are four planes: < 2^28 elements; where `wm` is uniform -- the pre-pass -- the loads take a
// scalar base and one vector offset.  Width and rows are below 2^24: full-rate 24-bit multiplies).  Nothing here waits for
// the loads: a caller with other requests to make puts them between this and footprint_window_max.
// EXACT_COUNTS (the pre-pass: every thread has a pair, the view is uniform): as many lookups as the widest footprint of
// the wave needs, each behind a uniform test.  Without it (the carve kernel's prologue: one lane per VIEW, half the wave
// idle, and every instruction of it is paid by a wave that is short of issue slots, not of memory): 2 x 2 lookups in a
// straight line, or all 3 x 3 when some lane needs a third window -- one test instead of nine.  A window that a lane does
// not need repeats its last one, so the maximum is the same either way.
template <bool EXACT_COUNTS = true>
__device__ __forceinline__ void footprint_window_requests(gfloat_ptr wm, unsigned width, unsigned plane_off, int tx0, int ty0,
                                                          const FootprintWindows& fw, float t[9]) {
  const int L = fw.L, k = 1 << L, pw = fw.pw, ph = fw.ph;
  const unsigned origin = __umul24(width, (unsigned)ty0) + (unsigned)tx0 + plane_off;
#pragma unroll
  for (int q = 0; q < 9; ++q) t[q] = -INFINITY;
  // the largest window counts (up to 3) among the lanes that take the 3 x 3 path below: wave-uniform
  const bool small = fw.nxw <= 3 && fw.nyw <= 3;
  int ux, uy;
  if (EXACT_COUNTS) {
    ux = __any(small && fw.nxw >= 3) ? 3 : (__any(small && fw.nxw >= 2) ? 2 : 1);
    uy = __any(small && fw.nyw >= 3) ? 3 : (__any(small && fw.nyw >= 2) ? 2 : 1);
  } else {
    ux = uy = __any(small && (fw.nxw >= 3 || fw.nyw >= 3)) ? 3 : 2;
  }
  if (small) {
    // the usual case (footprints up to 24 pixels wide): as many lookups as the widest footprint among
    // the wave's lanes needs (uniform counts ux x uy, typically 2 x 2; narrower ones repeat their last
    // window), all requested before the first is used.  As a per-lane loop each load waited for the one
    // before; nine unconditional ones cost the memory system twice what is needed (measured at
    // 2048^3 x 64: 157 ms instead of 108).
    auto look = [&](int aq, int bq) {
      const unsigned ro = origin + __umul24(width, (unsigned)min(bq << L, max(ph - k, 0)));
      t[3 * bq + aq] = load_u32_index(wm, ro + (unsigned)min(aq << L, max(pw - k, 0)));
    };
    if (EXACT_COUNTS) {
#pragma unroll
      for (int bq = 0; bq < 3; ++bq) {
#pragma unroll
        for (int aq = 0; aq < 3; ++aq)
          if (aq < ux && bq < uy) look(aq, bq);
      }
    } else {
      // (the four first, the other five behind ONE uniform test: as two alternatives the compiler merged them behind a
      // flag, and the wait it then put in front of the second alternative's requests -- for registers the first one
      // loads into -- covered the tile requested in front of these lookups)
      look(0, 0), look(1, 0), look(0, 1), look(1, 1);
      if (ux == 3) look(2, 0), look(2, 1), look(0, 2), look(1, 2), look(2, 2);
    }
  } else {  // (rare: a long thin footprint, 4 windows along one side)
    float m = -INFINITY;
    for (int bq = 0; bq < fw.nyw; ++bq) {
      const unsigned ro = origin + __umul24(width, (unsigned)min(bq << L, max(ph - k, 0)));
      for (int aq = 0; aq < fw.nxw; ++aq) m = fmaxf(m, load_u32_index(wm, ro + (unsigned)min(aq << L, max(pw - k, 0))));
    }
    t[0] = m;
  }
}
__device__ __forceinline__ float footprint_window_max(const float t[9]) {
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < 9; ++q) m = fmaxf(m, t[q]);
  return m;
}
// TileInfo::ub from the maximum `m` over every pixel a tap can read (`has_nan`: a non-finite pixel was seen -- only the
// scan of a launch without planes says so; the planes hold +inf there).  Voxels projecting outside the ROI sample max_sdf
// instead (voxel_carver.cc:469-471) -- not in a `sure` tile: every sample of the brick lies inside it, hence inside the ROI.
__device__ __forceinline__ float footprint_upper_bound(float m, int has_nan, bool outside_max, bool sure, float max_sdf) {
  if (outside_max && !sure) {
    has_nan |= !(fabsf(max_sdf) <= 3.402823466e+38f);
    m = fmaxf(m, max_sdf);
  }
  return has_nan ? INFINITY : (__builtin_fmaf(fabsf(m), 0x1p-20f, m) + 1.0e-30f);
}

// Footprint of one brick in one view: the tile of SDF pixels its samples read, whether every sample provably
// lies inside it (`sure`), and bounds of those samples (TileInfo).
// The brick is convex, so the exact projections of its voxels lie in the hull of the exact
// projections of its 8 corners.  Corners and voxels are both COMPUTED with a few float operations;
// the rectangle is only trusted when an explicit first-order bound of those errors (err_u, err_w
// below) is well inside the margin added around the corner hull.  Nothing here needs the exact
// arithmetic of the samples: corners come from the linear form p000 + {0,ax} + {0,ay} + {0,az} and
// an approximate reciprocal.
template <bool SAMEF, int TQ, bool GEN>
__device__ __forceinline__ TileInfo footprint_of(const FusedView& fv, float xl, float xh, float yl, float yh, float zl_,
                                                 float zh, bool is_ortho, bool outside_max, bool want_bound,
                                                 bool want_lower, float* lower_out = nullptr) {
  const ViewParams& v = fv.v;
  const float xa = fmaxf(fabsf(xl), fabsf(xh)), ya = fmaxf(fabsf(yl), fabsf(yh)), za = fmaxf(fabsf(zl_), fabsf(zh));
  const bool ortho = GEN && is_ortho;
  float p0[3], ax[3], ay[3], az[3], mag[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    p0[i] = v.t[i] + (v.r[i][0] * xl + (v.r[i][1] * yl + v.r[i][2] * zl_));
    ax[i] = v.r[i][0] * (xh - xl);
    ay[i] = v.r[i][1] * (yh - yl);
    az[i] = v.r[i][2] * (zh - zl_);
    // magnitude of the terms of pc[i]: its computed value is within ~2^-21 * mag[i] of the exact one
    mag[i] = fabsf(v.t[i]) + (fabsf(v.r[i][0]) * xa + (fabsf(v.r[i][1]) * ya + fabsf(v.r[i][2]) * za));
  }
  float umin = INFINITY, umax = -INFINITY, wmin = INFINITY, wmax_ = -INFINITY, zmin = INFINITY, zmax = -INFINITY;
  int bad = 0;
  const float fx = v.fx, fy = SAMEF ? v.fx : v.fy;
  float pxy[4][3];  // p0, p0 + ax, p0 + ay, p0 + ax + ay
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    pxy[0][i] = p0[i];
    pxy[1][i] = p0[i] + ax[i];
    pxy[2][i] = p0[i] + ay[i];
    pxy[3][i] = pxy[1][i] + ay[i];
  }
#pragma unroll
  for (int corner = 0; corner < 8; ++corner) {
    float pc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pc[i] = (corner & 4) ? pxy[corner & 3][i] + az[i] : pxy[corner & 3][i];
    float u = pc[0], w = pc[1];
    if (!ortho) {
      const float rz = __builtin_amdgcn_rcpf(pc[2]);  // (its operand range is checked on zmin / zmax below)
      u = __builtin_fmaf(fx * rz, pc[0], v.cx);
      w = __builtin_fmaf(fy * rz, pc[1], v.cy);
    }
    umin = fminf(umin, u);
    umax = fmaxf(umax, u);
    wmin = fminf(wmin, w);
    wmax_ = fmaxf(wmax_, w);
    zmin = fminf(zmin, pc[2]);
    zmax = fmaxf(zmax, pc[2]);
  }
  // in front of the camera, reciprocals finite and normal: every corner depth inside div_fast's range -- tested on the
  // smallest and the largest (a NaN depth would slip through fminf / fmaxf, but NaN / huge inputs end up in mag, next line)
  if (!ortho) bad |= !in_fast_div_range(zmin) || !in_fast_div_range(zmax);
  // finite inputs (NaN / huge values anywhere end up in mag), image coordinates of sane size
  bad |= !(mag[0] < 0x1p60f) || !(mag[1] < 0x1p60f) || !(mag[2] < 0x1p60f);
  bad |= !(umin > -1.0e6f) || !(umax < 1.0e6f) || !(wmin > -1.0e6f) || !(wmax_ < 1.0e6f);
  const float uabs = fmaxf(fabsf(umin), fabsf(umax)), wabs = fmaxf(fabsf(wmin), fabsf(wmax_));
  // |computed - exact| of an image coordinate, corner or voxel (first order, constants rounded up):
  //   pinhole  u = fx * X / Z + cx:  fx * dX / Z + |u - cx| * dZ / Z + rounding of the last operations,
  //            with dX <= 2^-21 mag_x, dZ <= 2^-21 mag_z and Z >= zmin;
  //   ortho    u = X:                dX.
  float err_u, err_w;
  if (ortho) {
    err_u = 0x1p-21f * mag[0];
    err_w = 0x1p-21f * mag[1];
  } else {
    bad |= !(zmin * 4.0f >= zmax);
    const float iz = 0x1p-21f * __builtin_amdgcn_rcpf(zmin) * 1.0001f;
    err_u = iz * (fx * mag[0] + (uabs + fabsf(v.cx)) * mag[2]) + 0x1p-21f * (uabs + fabsf(v.cx));
    err_w = iz * (fy * mag[1] + (wabs + fabsf(v.cy)) * mag[2]) + 0x1p-21f * (wabs + fabsf(v.cy));
  }
  const float margin = 0.125f;
  bad |= !(err_u <= 0.03125f) || !(err_w <= 0.03125f);  // corner error + voxel error <= margin / 2
  TileInfo ti;
  ti.lo_x = ti.lo_y = INFINITY;  // nothing passes the tile test
  ti.hi_x = ti.hi_y = -INFINITY;
  ti.pitchf = 0.0f;
  ti.base = 0;
  ti.tx0 = ti.ty0 = ti.tw = ti.nq = ti.th = 0;
  ti.inv_tw = 1.0f;
  ti.ub = INFINITY;  // never dropped
  ti.sure = 0;
  if (!bad) {
    const int tx0 = max((int)floorf(umin - margin), v.roi_min_xi);
    const int ty0 = max((int)floorf(wmin - margin), v.roi_min_yi);
    const int tx1 = min((int)floorf(umax + margin), v.roi_max_xi);
    const int ty1 = min((int)floorf(wmax_ + margin), v.roi_max_yi);
    const int tw = tx1 - tx0 + 1, th = ty1 - ty0 + 1;
    constexpr bool kRaw = TQ == kTileRaw;
    if (tw > 0 && th > 0 && (kRaw ? (tw <= 15 && th <= 15) : ((tw + 1) * (th + 1) <= kBigPixels))) {
      // Every computed (u, w) of the brick is within corner error + voxel error < margin of the corner
      // hull, so when the ROI clipped nothing it lies in [tx0, tx1 + 1) x [ty0, ty1 + 1); the depth
      // guard keeps every computed pc.z within a factor 2 of the corner range, inside div_fast's.
      const bool unclipped = (int)floorf(umin - margin) >= v.roi_min_xi && (int)floorf(wmin - margin) >= v.roi_min_yi &&
                             (int)floorf(umax + margin) < v.roi_max_xi && (int)floorf(wmax_ + margin) < v.roi_max_yi;
      const bool depth_ok = 0x1p-20f * mag[2] <= 0.25f * zmin && zmin >= 0x1p-58f && zmax <= 0x1p58f;
      // (|16 base| < 2^22: the fast path forms LDS addresses in the float pipeline, carve_view_fast)
      const int pitch = kRaw ? 16 : tw + 1;  // pixels per tile row
      const bool small_base = ty0 * pitch + tx0 < (1 << 18);
      // orthographic: no division, and the only depth test is the reference's `pc.z < 0` skip
      // (voxel_carver.cc:456): every computed pc.z of the brick is >= zmin - 2^-20 mag_z
      const bool depth_ok_ortho = zmin > 0x1p-20f * mag[2];
      ti.sure = (unclipped && (ortho ? depth_ok_ortho : depth_ok) && small_base) ? 1 : 0;
      ti.tx0 = tx0;
      ti.ty0 = ty0;
      ti.tw = tw;
      ti.th = th;
      ti.nq = tw * th;
      ti.inv_tw = 1.0f / (float)pitch;
      ti.pitchf = (float)pitch;
      ti.base = -(ty0 * pitch + tx0);
      ti.lo_x = (float)tx0;
      ti.lo_y = (float)ty0;
      // taps exist for floor(u) in [tx0, tx1]; at the ROI edge u == roi_max is still inside
      ti.hi_x = (tx1 == v.roi_max_xi) ? v.roi_max_x
                                      : __uint_as_float(__float_as_uint((float)(tx1 + 1)) - 1u);
      ti.hi_y = (ty1 == v.roi_max_yi) ? v.roi_max_y
                                      : __uint_as_float(__float_as_uint((float)(ty1 + 1)) - 1u);
      if (want_bound) {
        // maximum over every pixel a tap of this tile can read (the lookups: footprint_window_requests above)
        const FootprintWindows fw = footprint_windows(tx0, ty0, tx1, ty1, v.roi_max_xi, v.roi_max_yi);
        const int L = fw.L;
        float m = -INFINITY;
        int has_nan = 0;
        gfloat_ptr wm = (gfloat_ptr)fv.wmax;
        if (wm != nullptr) {
          float t[9];
          footprint_window_requests(wm, (unsigned)v.width, L == 3 ? (unsigned)fv.wmax_plane : 0u, tx0, ty0, fw, t);
          m = footprint_window_max(t);
        } else {  // no planes (out of memory for them): scan the rectangle
          gfloat_ptr img = (gfloat_ptr)v.sdf;
          for (int j = 0; j < fw.ph; ++j) {
            gfloat_ptr row = img + ((unsigned)v.width * (unsigned)(ty0 + j) + (unsigned)tx0);
            for (int i = 0; i < fw.pw; ++i) {
              const float t = row[i];
              has_nan |= !(fabsf(t) <= 3.402823466e+38f);  // NaN or +-inf: 0 * inf = NaN samples
              m = fmaxf(m, t);
            }
          }
        }
        ti.ub = footprint_upper_bound(m, has_nan, outside_max, ti.sure != 0, v.max_sdf);
        // Lower bound of the samples, by the mirrored argument: with every tap >= mn the sample is
        // >= mn - 2^-22 |mn|.  If that is >= -1 no voxel of this tile is skipped by the truncation test
        // (`dist < -1`, voxel_carver.cc:478) and the test is compiled out of the run over it (sure bit 1).
        // Voxels outside the ROI are not an issue: a `sure` tile has none.
        // (not looked up for a tile the upper bound already drops: `ub < -1`, the view is never processed)
        if (want_lower && ti.sure && !(ti.ub < -1.0f) && wm != nullptr && fv.has_lower && fw.nxw <= 3 && fw.nyw <= 3) {
          float t[9];  // planes 2 / 3: of the negated image -- max of -g = -(min of g)
          footprint_window_requests(wm, (unsigned)v.width, (L == 3 ? 3u : 2u) * (unsigned)fv.wmax_plane, tx0, ty0, fw, t);
          const float mneg = footprint_window_max(t);
          const float neg_lb = __builtin_fmaf(fabsf(mneg), 0x1p-20f, mneg);  // -(lower bound); +inf: none
          if (neg_lb <= 1.0f) ti.sure |= 2;
          if (lower_out) *lower_out = -neg_lb;  // (the slab planner, plan_cost_kernel)
        }
      }
    }
  }
  return ti;
}

// The whole FusedView record of view `vi` at once (ten 16-byte loads in flight, one wait): fields fetched where
// they are first needed cost a memory round trip each, behind every branch of footprint_of.
// (Pinned by the empty asm: the compiler would otherwise sink every load to its first use again.)
__device__ __forceinline__ FusedView load_fused_view(const FusedView* __restrict__ views, int vi) {
  static_assert(sizeof(FusedView) % 4 == 0, "FusedView is fetched dword by dword");
  constexpr int kViewDwords = (int)(sizeof(FusedView) / 4);
  typedef const uint32_t __attribute__((address_space(1))) * gu32_ptr;
  gu32_ptr src = (gu32_ptr)views + (size_t)vi * kViewDwords;
  uint32_t raw[kViewDwords];
#pragma unroll
  for (int q = 0; q < kViewDwords; ++q) raw[q] = src[q];
#pragma unroll
  for (int q = 0; q < kViewDwords; ++q) asm volatile("" : "+v"(raw[q]));
  FusedView fv;
  __builtin_memcpy(&fv, raw, sizeof(FusedView));
  return fv;
}

// What lane `vi` needs of its view to bound the footprint of a kept record (kStateStaleBounds): the planes, the image
// width, the ROI's last column and row, and the view's current max_sdf.  Per-lane loads; the caller pins them next to
// its record's load so that they are one batch behind one wait.
struct BoundView {
  gfloat_ptr wmax;
  unsigned wmax_plane, width;
  int roi_max_xi, roi_max_yi;
  float max_sdf;
};
__device__ __forceinline__ BoundView load_bound_view(const FusedView* __restrict__ views, int vi) {
  // (a 32-bit byte offset from the uniform base, view_byte_offset: one vector offset instead of a 64-bit address)
  typedef const char __attribute__((address_space(1))) * gchar_ptr;
  typedef const FusedView __attribute__((address_space(1))) * gview_ptr;
  const FusedView __attribute__((address_space(1)))& fv = *(gview_ptr)((gchar_ptr)views + view_byte_offset(vi));
  BoundView b;
  b.wmax = (gfloat_ptr)fv.wmax;
  b.wmax_plane = (unsigned)fv.wmax_plane, b.width = (unsigned)fv.v.width;
  b.roi_max_xi = fv.v.roi_max_xi, b.roi_max_yi = fv.v.roi_max_yi;
  b.max_sdf = fv.v.max_sdf;
  return b;
}

// (through an LDS-typed pointer: ds_write_b128, not flat stores)
__device__ __forceinline__ void store_tile_info(lds_u32* tinfo_lds, int vi, const TileInfo& ti) {
  static_assert(sizeof(TileInfo) % 4 == 0, "TileInfo is stored dword by dword");
  uint32_t w32[sizeof(TileInfo) / 4];
  __builtin_memcpy(w32, &ti, sizeof(TileInfo));
  lds_u32* dst = tinfo_lds + vi * (int)(sizeof(TileInfo) / 4);
#pragma unroll
  for (int q = 0; q < (int)(sizeof(TileInfo) / 4); ++q) dst[q] = w32[q];
}

// Prologue of the fused kernels that bound their footprints themselves (the big tile), out of line so that its
// registers do not add to the main loop's: lane vi handles view vi of the wave brick.
template <bool SAMEF, int TQ, bool GEN>
__device__ __attribute__((noinline)) float brick_footprints(const FusedView* __restrict__ views, int nviews, int lane,
                                                            float xl, float xh, float yl, float yh, float zl_, float zh,
                                                            bool is_ortho, bool outside_max, bool want_bound,
                                                            bool want_lower, lds_u32* tinfo_lds) {
  float ub_lane = INFINITY;
  if (lane < nviews) {
    const FusedView fv = load_fused_view(views, lane);
    const TileInfo ti = footprint_of<SAMEF, TQ, GEN>(fv, xl, xh, yl, yh, zl_, zh, is_ortho, outside_max, want_bound,
                                                     want_lower);
    store_tile_info(tinfo_lds, lane, ti);
    ub_lane = ti.ub;
  }
  return ub_lane;
}

// The same for the raw-tile kernels that keep their footprints as packed records in registers: lane vi returns the record
// the pre-pass would have written for view vi (footprint_records_kernel), a lane without a view "no tile, no bound".
template <bool SAMEF, bool GEN>
__device__ __attribute__((noinline)) FootprintRecord brick_footprint_records(const FusedView* __restrict__ views, int nviews,
                                                                             int lane, float xl, float xh, float yl, float yh,
                                                                             float zl_, float zh, bool is_ortho,
                                                                             bool outside_max, bool want_bound,
                                                                             bool want_lower) {
  FootprintRecord rec;
  rec.w0 = 0x7f800000u, rec.w1 = 0u;
  if (lane < nviews) {
    const FusedView fv = load_fused_view(views, lane);
    const TileInfo ti = footprint_of<SAMEF, kTileRaw, GEN>(fv, xl, xh, yl, yh, zl_, zh, is_ortho, outside_max, want_bound,
                                                            want_lower);
    rec = pack_footprint(ti, fv.v);
  }
  return rec;
}

}  // namespace
}  // namespace vcy
