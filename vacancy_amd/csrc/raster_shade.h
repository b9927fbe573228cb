// The shading arithmetic of one pixel -- the section "shading a rasterised mesh" of vacancy_hip.h, steps 9 to 11 --
// compiled for the kernel (raster_shade.hip) and for the serial host function (shade_host.hip).  The weights come from
// rs::project, rs::setup_face and rs::edge_value (raster_fragment.h): they are the rasteriser's bits by construction, and
// the T of a pinhole is the sum whose reciprocal rs::fragment_key rounds to the depth.
#pragma once

#include "raster_fragment.h"

namespace vcy {
namespace rs {

// Steps 1, 2 and 4 again for the face that won a pixel: its corners in the view.  `vertices`, `faces`: the mesh.
VCY_RS_FN void winner_face(const View& v, const float* vertices, const int32_t* faces, int64_t face, Face& f) {
  int id[3];
  Point p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    id[k] = faces[3 * face + k];
    const float* at = vertices + 3 * (int64_t)id[k];
    const float xyz[3] = {at[0], at[1], at[2]};
    p[k] = project(v, xyz);
  }
  (void)setup_face(v, id, p, f);  // (drawn: it won a pixel)
}

// Step 9: b_0, b_1, b_2 of the face at pixel (x, y).
VCY_RS_FN void weights(const View& v, const Face& f, int x, int y, double (&b)[3]) {
  const double px = (double)x, py = (double)y;
  const double e0 = edge_value(f.id[1], f.id[2], f.p[1], f.p[2], px, py);
  const double e1 = edge_value(f.id[2], f.id[0], f.p[2], f.p[0], px, py);
  const double e2 = edge_value(f.id[0], f.id[1], f.p[0], f.p[1], px, py);
  const double l0 = e0 / f.area, l1 = e1 / f.area, l2 = e2 / f.area;
  if (v.ortho) {
    b[0] = l0, b[1] = l1, b[2] = l2;
  } else {
    const double z0 = (double)f.p[0].z, z1 = (double)f.p[1].z, z2 = (double)f.p[2].z;
    const double t0 = l0 * (1.0 / z0), t1 = l1 * (1.0 / z1), t2 = l2 * (1.0 / z2);
    const double T = (t0 + t1) + t2;
    b[0] = t0 / T, b[1] = t1 / T, b[2] = t2 / T;
  }
}

// Step 10: one channel.
VCY_RS_FN float blend(const double (&b)[3], float a0, float a1, float a2) {
  const double m0 = b[0] * (double)a0, m1 = b[1] * (double)a1, m2 = b[2] * (double)a2;
  return (float)((m0 + m1) + m2);
}

// Step 10 for the winner of a pixel: `channels` values from the per-vertex attributes.
template <int C>
VCY_RS_FN void shade(const Face& f, const double (&b)[3], const float* attributes, float (&value)[C]) {
  const float* a0 = attributes + (int64_t)C * f.id[0];
  const float* a1 = attributes + (int64_t)C * f.id[1];
  const float* a2 = attributes + (int64_t)C * f.id[2];
#pragma unroll
  for (int c = 0; c < C; ++c) value[c] = blend(b, a0[c], a1[c], a2[c]);
}

// Step 11: q.
VCY_RS_FN uint8_t quantize(float v) {
  if (!(v > 0.0f)) return 0;  // (NaN as well)
  if (v >= 255.0f) return 255;
  return (uint8_t)floorf(v + 0.5f);
}

enum { kSums = 7 };  // step 12: n, sad[3], ssd[3]

}  // namespace rs
}  // namespace vcy
