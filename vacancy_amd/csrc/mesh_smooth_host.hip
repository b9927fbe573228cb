// Taubin smoothing of an indexed mesh, serially on the host (vcy_smooth_mesh_host; the definition is the section "mesh
// smoothing" of vacancy_hip.h, restated in numpy in tests/smooth_ref.py).  Host code only -- no GPU, no context, nothing
// of the HIP runtime --, like mesh_host.hip, whose vcy_mesh_normals_host gives the normals of the result.  Also the
// argument checks the device entry point (mesh_smooth.hip) shares.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_shared.h"
#include "vacancy_hip.h"

namespace vcy {

void set_error(const char* fmt, ...);

// Everything the definition refuses, before anything is written.
int smooth_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                      const vcy_smooth_option* o, const float* vertices_out) {
  if (n_vertices < 0 || n_faces < 0 || !o || (n_vertices > 0 && (!vertices || !vertices_out)) || (n_faces > 0 && !faces)) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  if (o->iterations < 0 || o->iterations > 10000) {
    set_error("%s: iterations %d outside 0 .. 10000", who, o->iterations);
    return VCY_ERR_INVALID_ARG;
  }
  if (!std::isfinite(o->lambda) || !std::isfinite(o->mu)) {
    set_error("%s: lambda and mu must be finite (%g, %g)", who, (double)o->lambda, (double)o->mu);
    return VCY_ERR_INVALID_ARG;
  }
  if (o->pin_boundary != 0 && o->pin_boundary != 1) {
    set_error("%s: pin_boundary %d is neither 0 nor 1", who, o->pin_boundary);
    return VCY_ERR_INVALID_ARG;
  }
  { const int rc = mesh_index_limits(who, n_vertices, n_faces); if (rc != VCY_OK) return rc; }
  for (int64_t i = 0; i < 3 * n_faces; ++i)
    if (faces[i] < 0 || faces[i] >= n_vertices) {
      set_error("%s: face %lld names vertex %d of %lld", who, (long long)(i / 3), faces[i], (long long)n_vertices);
      return VCY_ERR_INVALID_ARG;
    }
  return VCY_OK;
}

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_smooth_mesh_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                         const vcy_smooth_option* option, float* vertices_out, float* vertex_normals_out,
                         float* face_normals_out) {
  { const int rc = smooth_check_args("vcy_smooth_mesh_host", n_vertices, n_faces, vertices, faces, option, vertices_out); if (rc != VCY_OK) return rc; }
  if (n_vertices == 0) return VCY_OK;
  const size_t nv = (size_t)n_vertices;
  const int64_t n_corners = 3 * n_faces;

  // rows: corners in ascending id behind off[v] (a counting sort is stable), then the ids a pass gathers, two per corner
  std::vector<int64_t> off(nv + 1, 0);
  for (int64_t c = 0; c < n_corners; ++c) ++off[(size_t)faces[c] + 1];
  for (size_t v = 0; v < nv; ++v) off[v + 1] += off[v];
  std::vector<int32_t> gather(2 * (size_t)n_corners);
  {
    std::vector<int64_t> cursor(off.begin(), off.end() - 1);
    for (int64_t c = 0; c < n_corners; ++c) {
      const int64_t f = c / 3, j = c - 3 * f;
      const int64_t slot = cursor[(size_t)faces[c]]++;
      gather[2 * (size_t)slot] = faces[3 * f + (j + 1) % 3];
      gather[2 * (size_t)slot + 1] = faces[3 * f + (j + 2) % 3];
    }
  }
  std::vector<uint8_t> pinned(nv, 0);
  if (option->pin_boundary) {
    std::vector<int32_t> ids;
    for (size_t v = 0; v < nv; ++v) {
      ids.assign(gather.begin() + 2 * off[v], gather.begin() + 2 * off[v + 1]);
      std::sort(ids.begin(), ids.end());
      for (size_t k = 0; k < ids.size(); ++k) {
        const bool single = (k == 0 || ids[k - 1] != ids[k]) && (k + 1 == ids.size() || ids[k + 1] != ids[k]);
        if (single && ids[k] != (int32_t)v) pinned[v] = 1;
      }
    }
  }

  std::vector<float> a(vertices, vertices + 3 * nv), b(3 * nv);
  float *p = a.data(), *q = b.data();
  for (int pass = 0; pass < 2 * option->iterations; ++pass) {
    const float s = (pass & 1) ? option->mu : option->lambda;
    for (size_t v = 0; v < nv; ++v) {
      const int64_t k0 = 2 * off[v], k1 = 2 * off[v + 1];
      if (k0 == k1 || pinned[v]) {
        q[3 * v] = p[3 * v], q[3 * v + 1] = p[3 * v + 1], q[3 * v + 2] = p[3 * v + 2];
        continue;
      }
      float sum[3] = {0.0f, 0.0f, 0.0f};
      for (int64_t k = k0; k < k1; ++k) {
        const float* g = p + 3 * (size_t)gather[(size_t)k];
        sum[0] = sum[0] + g[0];
        sum[1] = sum[1] + g[1];
        sum[2] = sum[2] + g[2];
      }
      const float cnt = (float)(k1 - k0);
      for (int c = 0; c < 3; ++c) {
        const float m = sum[c] / cnt;
        const float d = m - p[3 * v + c];
        const float t = s * d;
        q[3 * v + c] = p[3 * v + c] + t;
      }
    }
    std::swap(p, q);
  }
  std::memcpy(vertices_out, p, sizeof(float) * 3 * nv);  // (memcpy: the input bits, whatever they are)
  if (vertex_normals_out || face_normals_out)
    return vcy_mesh_normals_host(n_vertices, n_faces, vertices_out, faces, vertex_normals_out, face_normals_out);
  return VCY_OK;
}

}  // extern "C"
