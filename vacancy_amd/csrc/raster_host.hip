// Rasterising an indexed mesh into views, serially on the host (vcy_raster_mesh_host; the definition is the section
// "rasterising an indexed mesh" of vacancy_hip.h, restated in numpy in tests/raster_ref.py).  Host code only -- no GPU, no
// context, nothing of the HIP runtime --, like render_merge.hip, whose check_render_view refuses the views.  The
// arithmetic of a fragment is raster_fragment.h, shared with the kernel (raster.hip).  Also the argument checks the device
// entry points share.
#include <cmath>
#include <cstdint>
#include <vector>

#include "host_shared.h"
#include "raster_fragment.h"
#include "vacancy_hip.h"

namespace vcy {

void set_error(const char* fmt, ...);
int check_render_view(const vcy_view* v, int i);  // render_merge.hip

// Everything the definition refuses, before anything is written.
int raster_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                      int n_views, const vcy_view* views) {
  if (n_vertices < 0 || n_faces < 0 || n_views <= 0 || !views || (n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_views; ++i) {
    const int rc = check_render_view(&views[i], i);
    if (rc != VCY_OK) return rc;
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

int vcy_raster_mesh_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces, int n_views,
                         const vcy_view* views, float* const* depth, int32_t* const* face, uint64_t* const* hits,
                         int64_t* n_dropped) {
  { const int rc = raster_check_args("vcy_raster_mesh_host", n_vertices, n_faces, vertices, faces, n_views, views); if (rc != VCY_OK) return rc; }
  std::vector<unsigned long long> keys;
  for (int i = 0; i < n_views; ++i) {
    rs::View v;
    rs::fill_view(views[i], &v);
    const int64_t w = v.w, h = v.h, words = (w + 63) / 64;
    keys.assign((size_t)(w * h), rs::kMissKey);
    int64_t dropped[2] = {0, 0};
    for (int64_t fi = 0; fi < n_faces; ++fi) {
      const int id[3] = {faces[3 * fi], faces[3 * fi + 1], faces[3 * fi + 2]};
      rs::Point p[3];
      for (int k = 0; k < 3; ++k) {
        const float* at = vertices + 3 * (int64_t)id[k];
        const float xyz[3] = {at[0], at[1], at[2]};
        p[k] = rs::project(v, xyz);
      }
      rs::Face f;
      const int cls = rs::setup_face(v, id, p, f);
      if (cls != rs::kDrawn) {
        ++dropped[cls];
        continue;
      }
      for (int y = f.y0; y <= f.y1; ++y)
        for (int x = f.x0; x <= f.x1; ++x) {
          const unsigned long long key = rs::fragment_key(v, f, (int)fi, x, y);
          unsigned long long& at = keys[(size_t)(w * y + x)];
          if (key < at) at = key;
        }
    }
    if (n_dropped) n_dropped[2 * i] = dropped[0], n_dropped[2 * i + 1] = dropped[1];
    float* d = depth ? depth[i] : nullptr;
    int32_t* fo = face ? face[i] : nullptr;
    uint64_t* hb = hits ? hits[i] : nullptr;
    if (hb)
      for (int64_t k = 0; k < words * h; ++k) hb[k] = 0;
    for (int64_t y = 0; y < h; ++y)
      for (int64_t x = 0; x < w; ++x) {
        const unsigned long long key = keys[(size_t)(w * y + x)];
        const bool hit = key != rs::kMissKey;
        if (d) d[w * y + x] = hit ? rs::bits_float((uint32_t)(key >> 32)) : INFINITY;
        if (fo) fo[w * y + x] = hit ? (int32_t)(uint32_t)key : -1;
        if (hb && hit) hb[y * words + (x >> 6)] |= 1ull << (x & 63);
      }
  }
  return VCY_OK;
}

}  // extern "C"
