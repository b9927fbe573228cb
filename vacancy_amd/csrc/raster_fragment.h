// The rasteriser's arithmetic of one (face, view, pixel) fragment -- the section "rasterising an indexed mesh" of
// vacancy_hip.h, steps 1 to 8 -- compiled for the kernel (raster.hip) and for the serial host function (raster_host.hip):
// the projection of a vertex (rs::project), the canonical edge function (rs::edge_value), what a face keeps per view
// (rs::setup_face) and the key of a fragment (rs::fragment_key).  The library's flags (no FMA contraction, correctly rounded
// division, denormals kept) make host and device agree to the bit; the per-pixel part is double by definition.
#pragma once

#include <cmath>
#include <cstdint>

#include "vacancy_hip.h"

#if defined(__HIPCC__)
#define VCY_RS_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define VCY_RS_FN inline
#endif

namespace vcy {
namespace rs {

constexpr int kMaxViewsPerLaunch = 64;
constexpr unsigned long long kMissKey = ~0ull;  // no fragment: above every key, the face index being below 2^31

struct View {  // one per view of a launch, in device memory (the host function: one per view of the call)
  float R[9], t[3];  // w2c
  float fx, fy, cx, cy;
  int rx0, ry0, rx1, ry1;
  int ortho, w, h;
};

inline void fill_view(const vcy_view& v, View* r) {
  for (int row = 0; row < 3; ++row) {
    for (int col = 0; col < 3; ++col) r->R[row * 3 + col] = v.w2c[row * 4 + col];
    r->t[row] = v.w2c[row * 4 + 3];
  }
  r->fx = v.fx, r->fy = v.fy, r->cx = v.cx, r->cy = v.cy;
  r->rx0 = v.roi_min[0], r->ry0 = v.roi_min[1], r->rx1 = v.roi_max[0], r->ry1 = v.roi_max[1];
  r->ortho = v.is_ortho != 0, r->w = v.width, r->h = v.height;
}

VCY_RS_FN bool finite_f(float x) { return x - x == 0.0f; }  // (false for NaN and both infinities)

// Step 1: a vertex in a view.  A pure function of (vertex, view): every face that names the vertex sees these bits.
struct Point {
  float u, w, z;
  bool usable;
};
VCY_RS_FN Point project(const View& v, const float (&p)[3]) {
  float pc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float c0 = v.R[3 * r + 0] * p[0];
    const float c1 = v.R[3 * r + 1] * p[1];
    const float c2 = v.R[3 * r + 2] * p[2];
    pc[r] = v.t[r] + (c0 + (c1 + c2));
  }
  Point q;
  q.z = pc[2];
  q.usable = finite_f(pc[0]) && finite_f(pc[1]) && finite_f(pc[2]) && (v.ortho ? !(pc[2] < 0.0f) : pc[2] > 0.0f);
  if (v.ortho) {
    q.u = pc[0];
    q.w = pc[1];
  } else {
    q.u = v.fx / pc[2] * pc[0] + v.cx;
    q.w = v.fy / pc[2] * pc[1] + v.cy;
  }
  q.usable = q.usable && finite_f(q.u) && finite_f(q.w);
  return q;
}

// Step 3: the face's value at (px, py) for its directed edge from vertex `from` (at a) to vertex `to` (at b): the edge
// function of the edge's lower index towards its higher one, negated when the face runs the other way.  from != to.
VCY_RS_FN double edge_value(int from, int to, const Point& a, const Point& b, double px, double py) {
  const bool forward = from < to;
  const double ax = forward ? (double)a.u : (double)b.u, ay = forward ? (double)a.w : (double)b.w;
  const double bx = forward ? (double)b.u : (double)a.u, by = forward ? (double)b.w : (double)a.w;
  const double m0 = (bx - ax) * (py - ay);
  const double m1 = (by - ay) * (px - ax);
  const double e = m0 - m1;
  return forward ? e : -e;
}

// Steps 2, 4 and 5: what a face keeps in a view.
enum { kDrawn = -1, kDropUnusable = 0, kDropDegenerate = 1 };
struct Face {
  int id[3];
  Point p[3];
  double area;     // A
  double sign;     // s
  int x0, y0, x1, y1;  // candidate pixels, inside the ROI; empty when x0 > x1 or y0 > y1
};

VCY_RS_FN float min3(float a, float b, float c) { return fminf(a, fminf(b, c)); }
VCY_RS_FN float max3(float a, float b, float c) { return fmaxf(a, fmaxf(b, c)); }

// The class the face is dropped in, or kDrawn with `f` filled.
VCY_RS_FN int setup_face(const View& v, const int (&id)[3], const Point (&p)[3], Face& f) {
#pragma unroll
  for (int k = 0; k < 3; ++k) f.id[k] = id[k], f.p[k] = p[k];
  f.area = 0.0, f.sign = 0.0;
  f.x0 = f.y0 = 0, f.x1 = f.y1 = -1;
  if (!(p[0].usable && p[1].usable && p[2].usable)) return kDropUnusable;
  if (id[0] == id[1] || id[1] == id[2] || id[2] == id[0]) return kDropDegenerate;
  f.area = edge_value(id[0], id[1], p[0], p[1], (double)p[2].u, (double)p[2].w);
  if (!(f.area > 0.0) && !(f.area < 0.0)) return kDropDegenerate;  // (0 and NaN)
  if (!(f.area - f.area == 0.0)) return kDropDegenerate;              // (infinite)
  f.sign = f.area > 0.0 ? 1.0 : -1.0;
  // the box, clamped while still float: a coordinate may lie far outside what an int holds
  const float bx0 = fmaxf(ceilf(min3(p[0].u, p[1].u, p[2].u)), (float)v.rx0);
  const float bx1 = fminf(floorf(max3(p[0].u, p[1].u, p[2].u)), (float)v.rx1);
  const float by0 = fmaxf(ceilf(min3(p[0].w, p[1].w, p[2].w)), (float)v.ry0);
  const float by1 = fminf(floorf(max3(p[0].w, p[1].w, p[2].w)), (float)v.ry1);
  if (bx0 <= bx1 && by0 <= by1) f.x0 = (int)bx0, f.x1 = (int)bx1, f.y0 = (int)by0, f.y1 = (int)by1;
  return kDrawn;
}

VCY_RS_FN long long box_pixels(const Face& f) {
  return f.x0 > f.x1 || f.y0 > f.y1 ? 0 : (long long)(f.x1 - f.x0 + 1) * (long long)(f.y1 - f.y0 + 1);
}

VCY_RS_FN uint32_t float_bits(float x) {
  union { float f; uint32_t u; } c;
  c.f = x;
  return c.u;
}
VCY_RS_FN float bits_float(uint32_t u) {
  union { float f; uint32_t u; } c;
  c.u = u;
  return c.f;
}

// Steps 6 to 8: the key (depth bits << 32 | face index) of the face's fragment at pixel (x, y), kMissKey when the pixel
// is not covered or the fragment is discarded.  Keys compare as the definition's (depth bits, face index).
VCY_RS_FN unsigned long long fragment_key(const View& v, const Face& f, int face, int x, int y) {
  const double px = (double)x, py = (double)y;
  const double e0 = edge_value(f.id[1], f.id[2], f.p[1], f.p[2], px, py);
  const double e1 = edge_value(f.id[2], f.id[0], f.p[2], f.p[0], px, py);
  const double e2 = edge_value(f.id[0], f.id[1], f.p[0], f.p[1], px, py);
  if (!(f.sign * e0 >= 0.0 && f.sign * e1 >= 0.0 && f.sign * e2 >= 0.0)) return kMissKey;
  const double l0 = e0 / f.area, l1 = e1 / f.area, l2 = e2 / f.area;
  const double z0 = (double)f.p[0].z, z1 = (double)f.p[1].z, z2 = (double)f.p[2].z;
  double z;
  if (v.ortho) {
    const double t0 = l0 * z0, t1 = l1 * z1, t2 = l2 * z2;
    z = (t0 + t1) + t2;
  } else {
    const double t0 = l0 * (1.0 / z0), t1 = l1 * (1.0 / z1), t2 = l2 * (1.0 / z2);
    z = 1.0 / ((t0 + t1) + t2);
  }
  float d = (float)z;
  if (!finite_f(d) || d < 0.0f) return kMissKey;
  if (d == 0.0f) d = 0.0f;  // (-0 is stored as +0)
  return ((unsigned long long)float_bits(d) << 32) | (unsigned long long)(uint32_t)face;
}

}  // namespace rs
}  // namespace vcy
