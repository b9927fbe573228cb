// Mesh::CalcFaceNormal on the device, shared by the normals of the extraction chain (mc_normals.hip) and the normals of a
// general indexed mesh (mesh_normals.hip).  Arithmetic: include/vacancy/linalg.h's, i.e. squaredNorm = x*x + (y*y + z*z),
// normalized() = n2 > 0 ? v / sqrt(n2) : v, true division per component; no contraction, correctly rounded sqrt and
// division, denormals kept (Makefile).  The host's statement of the same is mesh_host.hip's.
#pragma once

#include <hip/hip_runtime.h>

namespace vcy {
namespace mc {

// Eigen::Vector3f::normalize() as include/vacancy/linalg.h evaluates it
__device__ __forceinline__ void normalize3(float v[3]) {
  const float n2 = v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]);
  if (n2 > 0.0f) {
    const float n = sqrtf(n2);
    v[0] = v[0] / n;
    v[1] = v[1] / n;
    v[2] = v[2] / n;
  }
}

// Mesh::CalcFaceNormal for one face (mesh.cc:231-240)
__device__ __forceinline__ void face_normal(const float p0[3], const float p1[3], const float p2[3], float fn[3]) {
  float v1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  float v2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  normalize3(v1);
  normalize3(v2);
  fn[0] = v1[1] * v2[2] - v1[2] * v2[1];
  fn[1] = v1[2] * v2[0] - v1[0] * v2[2];
  fn[2] = v1[0] * v2[1] - v1[1] * v2[0];
  normalize3(fn);
}

// ... of the face (i0, i1, i2) of an indexed mesh: nine position loads, then the above
__device__ __forceinline__ void face_normal_of(const float* verts, int i0, int i1, int i2, float fn[3]) {
  float q[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    q[0][k] = verts[3 * (int64_t)i0 + k];
    q[1][k] = verts[3 * (int64_t)i1 + k];
    q[2][k] = verts[3 * (int64_t)i2 + k];
  }
  face_normal(q[0], q[1], q[2], fn);
}

}  // namespace mc
}  // namespace vcy
