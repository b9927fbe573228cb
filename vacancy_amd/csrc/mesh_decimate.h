// The arithmetic of the mesh decimation -- the section "mesh decimation" of vacancy_hip.h: the cell of a vertex, the
// canonical form of a face, the mean of a member row and its nearest member -- in ONE place, compiled for the kernels
// (mesh_decimate.hip) and for the serial host function (mesh_decimate_host.hip).  The library's flags (no FMA contraction,
// correctly rounded division, denormals kept) make host and device agree to the bit.  Also the hash of the two
// open-addressing tables, which both sides use (any hash gives the same results; this one spreads lattice keys).
#pragma once

#include <cmath>
#include <cstdint>

#include "vacancy_hip.h"

#if defined(__HIPCC__)
#define VCY_DC_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define VCY_DC_FN inline
#endif

namespace vcy {
namespace dc {

// k_c = floor((p_c - origin_c) / cell); false (and k_c = 0) for a non-finite p_c or |t_c| >= 2^30
VCY_DC_FN bool cell_key(const float* p, const float* origin, float cell, int32_t* k) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float d = p[c] - origin[c];
    const float t = d / cell;
    const bool in = fabsf(p[c]) <= 3.402823466e+38f && fabsf(t) < 1073741824.0f;  // (false for NaN)
    k[c] = in ? (int32_t)floorf(t) : 0;
    ok = ok && in;
  }
  return ok;
}

// three 32-bit words -> 32 bits (multiply-xorshift finaliser over a sum of odd multiples: neighbouring lattice cells and
// neighbouring cluster numbers land far apart, so probe chains at a load of at most 1/2 stay short)
VCY_DC_FN uint32_t hash3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t h = a * 0x9E3779B1u + b * 0x85EBCA77u + c * 0xC2B2AE3Du;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  h *= 0x297A2D39u;
  h ^= h >> 15;
  return h;
}

// the rotation of (a, b, c), three different numbers, that puts the smallest first
VCY_DC_FN void canonical(int32_t a, int32_t b, int32_t c, int32_t* out) {
  if (a < b && a < c) out[0] = a, out[1] = b, out[2] = c;
  else if (b < c) out[0] = b, out[1] = c, out[2] = a;
  else out[0] = c, out[1] = a, out[2] = b;
}

// MEAN of the members row[0 .. len), in row order
VCY_DC_FN void row_mean(const float* p, const int32_t* row, int64_t len, float* m) {
  float s[3] = {0.0f, 0.0f, 0.0f};
  for (int64_t j = 0; j < len; ++j) {
    const float* q = p + 3 * (int64_t)row[j];
    s[0] = s[0] + q[0];
    s[1] = s[1] + q[1];
    s[2] = s[2] + q[2];
  }
  const float n = (float)len;
  m[0] = s[0] / n;
  m[1] = s[1] / n;
  m[2] = s[2] / n;
}

// d(i) of NEAREST for the member at q
VCY_DC_FN float dist2(const float* q, const float* m) {
  const float dx = q[0] - m[0], dy = q[1] - m[1], dz = q[2] - m[2];
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float xy = xx + yy;
  return xy + zz;
}

// NEAREST: the member closest to m, the lower index on a tie; a NaN distance never wins
VCY_DC_FN int32_t row_nearest(const float* p, const int32_t* row, int64_t len, const float* m) {
  int32_t best = row[0];
  float dbest = 0.0f;
  for (int64_t j = 0; j < len; ++j) {
    const float d = dist2(p + 3 * (int64_t)row[j], m);
    if (j == 0) dbest = d;
    else if (d < dbest) best = row[j], dbest = d;
  }
  return best;
}

}  // namespace dc
}  // namespace vcy
