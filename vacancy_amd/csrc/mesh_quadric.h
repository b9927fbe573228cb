// The arithmetic of the quadric-error representative -- the section "mesh decimation, quadric representatives" of
// vacancy_hip.h: the quadric of a face seen from a cluster's mean, the componentwise sum, the regularised 3x3 solve with
// its fallback to the mean -- in ONE place, compiled for the kernels (mesh_decimate.hip) and for the serial host function
// (mesh_decimate_host.hip).  All of it is double, one rounding per operation (no FMA contraction: the library's flags);
// fp64 division is correctly rounded on both sides without a further flag.
#pragma once

#include "mesh_decimate.h"

namespace vcy {
namespace dc {

// q(f) of the face (p0, p1, p2) seen from the mean m
VCY_DC_FN void face_quadric(const float* p0, const float* p1, const float* p2, const float* m, double* q) {
  const double mx = (double)m[0], my = (double)m[1], mz = (double)m[2];
  const double ax = (double)p0[0] - mx, ay = (double)p0[1] - my, az = (double)p0[2] - mz;
  const double bx = (double)p1[0] - mx, by = (double)p1[1] - my, bz = (double)p1[2] - mz;
  const double cx = (double)p2[0] - mx, cy = (double)p2[1] - my, cz = (double)p2[2] - mz;
  const double ex = bx - ax, ey = by - ay, ez = bz - az;
  const double gx = cx - ax, gy = cy - ay, gz = cz - az;
  const double nx = ey * gz - ez * gy;
  const double ny = ez * gx - ex * gz;
  const double nz = ex * gy - ey * gx;
  const double d = -((nx * ax + ny * ay) + nz * az);
  q[0] = nx * nx, q[1] = nx * ny, q[2] = nx * nz;
  q[3] = ny * ny, q[4] = ny * nz, q[5] = nz * nz;
  q[6] = nx * d, q[7] = ny * d, q[8] = nz * d;
}

// Q = Q + q, componentwise
VCY_DC_FN void quadric_add(double* Q, const double* q) {
#pragma unroll
  for (int k = 0; k < 9; ++k) Q[k] = Q[k] + q[k];
}

// The position of a cluster with quadric Q, mean m and cell `key`: P of the definition into `out` and false, or the bits of
// m and true where the fallback rule holds.
VCY_DC_FN bool solve_or_mean(const double* Q, const float* m, float regularize, const float* origin, float cell,
                             const int32_t* key, float* out) {
  out[0] = m[0], out[1] = m[1], out[2] = m[2];
  const double big = 1.7976931348623157e308;
  const double t = (Q[0] + Q[3]) + Q[5];
  if (!(t > 0.0) || !(t <= big)) return true;  // (NaN fails both)
  const double w = (double)regularize * t;
  const double A00 = Q[0] + w, A11 = Q[3] + w, A22 = Q[5] + w, A01 = Q[1], A02 = Q[2], A12 = Q[4];
  const double r0 = -Q[6], r1 = -Q[7], r2 = -Q[8];
  const double d0 = A00;
  if (!(d0 > 0.0)) return true;
  const double l10 = A01 / d0, l20 = A02 / d0;
  const double d1 = A11 - l10 * A01;
  if (!(d1 > 0.0)) return true;
  const double u = A12 - l20 * A01;
  const double l21 = u / d1;
  const double d2 = (A22 - l20 * A02) - l21 * u;
  if (!(d2 > 0.0)) return true;
  const double y0 = r0;
  const double y1 = r1 - l10 * y0;
  const double y2 = (r2 - l20 * y0) - l21 * y1;
  const double z0 = y0 / d0, z1 = y1 / d1, z2 = y2 / d2;
  const double x2 = z2;
  const double x1 = z1 - l21 * x2;
  const double x0 = (z0 - l10 * x1) - l20 * x2;
  const double s[3] = {(double)m[0] + x0, (double)m[1] + x1, (double)m[2] + x2};
  float P[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (!(fabs(s[c]) < 0x1.ffffffp+127)) return true;  // (NaN, or 2^128 - 2^103 and beyond: P would not be finite)
    P[c] = (float)s[c];                                // to nearest even
  }
  int32_t k[3];
  if (!cell_key(P, origin, cell, k)) return true;  // (refuses a non-finite P as well)
  if (k[0] != key[0] || k[1] != key[1] || k[2] != key[2]) return true;
  out[0] = P[0], out[1] = P[1], out[2] = P[2];
  return false;
}

}  // namespace dc
}  // namespace vcy
