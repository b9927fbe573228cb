// Shading a rasterised mesh, serially on the host (vcy_shade_mesh_host, vcy_mesh_photo_error_host; the definition is the
// section "shading a rasterised mesh" of vacancy_hip.h, restated in numpy in tests/shade_ref.py).  Host code only -- no GPU,
// no context, nothing of the HIP runtime.  The winners come from vcy_raster_mesh_host's face image, the arithmetic of a
// pixel is raster_shade.h, shared with the kernel (raster_shade.hip).  Also the argument checks the device entry points
// share.
#include <cstdint>
#include <vector>

#include "raster_shade.h"
#include "vacancy_hip.h"

namespace vcy {

void set_error(const char* fmt, ...);
int raster_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                      int n_views, const vcy_view* views);  // raster_host.hip

// Everything the definition refuses, before anything is written.
int shade_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                     const float* attributes, int n_views, const vcy_view* views, const vcy_shade_option* option) {
  if (!option || option->channels < 1 || option->channels > 4 || (n_vertices > 0 && !attributes)) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  return raster_check_args(who, n_vertices, n_faces, vertices, faces, n_views, views);
}

int photo_error_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                           const float* colors, int n_views, const vcy_view* views, const uint8_t* const* photos,
                           const uint8_t* const* masks, const int64_t* sums) {
  if (!photos || !sums || (n_vertices > 0 && !colors)) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  { const int rc = raster_check_args(who, n_vertices, n_faces, vertices, faces, n_views, views); if (rc != VCY_OK) return rc; }
  for (int i = 0; i < n_views; ++i)
    if (!photos[i] || (masks && !masks[i])) {
      set_error("%s: null %s of view %d", who, !photos[i] ? "photograph" : "silhouette", i);
      return VCY_ERR_INVALID_ARG;
    }
  return VCY_OK;
}

namespace {

// the face image of view i (vcy_raster_mesh_host: the rasteriser's host code decides the winners)
int winners(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces, const vcy_view& view,
            std::vector<int32_t>* face) {
  face->assign((size_t)view.width * (size_t)view.height, -1);
  int32_t* at = face->data();
  return vcy_raster_mesh_host(n_vertices, n_faces, vertices, faces, 1, &view, nullptr, &at, nullptr, nullptr);
}

template <int C>
void shade_view(const rs::View& v, const float* vertices, const int32_t* faces, const float* attributes, const int32_t* face,
                const float* background, float* value, uint8_t* value8, float* bary) {
  for (int y = 0; y < v.h; ++y)
    for (int x = 0; x < v.w; ++x) {
      const int64_t px = (int64_t)v.w * y + x;
      float val[C];
      double b[3] = {0.0, 0.0, 0.0};
      for (int c = 0; c < C; ++c) val[c] = background[c];
      if (face[px] >= 0) {
        rs::Face f;
        rs::winner_face(v, vertices, faces, face[px], f);
        rs::weights(v, f, x, y, b);
        rs::shade<C>(f, b, attributes, val);
      }
      for (int c = 0; c < C; ++c) {
        if (value) value[C * px + c] = val[c];
        if (value8) value8[C * px + c] = rs::quantize(val[c]);
      }
      if (bary)
        for (int k = 0; k < 3; ++k) bary[3 * px + k] = (float)b[k];
    }
}

}  // namespace

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_shade_mesh_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                        const float* attributes, int n_views, const vcy_view* views, const vcy_shade_option* option,
                        float* const* value, uint8_t* const* value8, float* const* bary) {
  { const int rc = shade_check_args("vcy_shade_mesh_host", n_vertices, n_faces, vertices, faces, attributes, n_views, views, option); if (rc != VCY_OK) return rc; }
  std::vector<int32_t> face;
  for (int i = 0; i < n_views; ++i) {
    { const int rc = winners(n_vertices, n_faces, vertices, faces, views[i], &face); if (rc != VCY_OK) return rc; }
    rs::View v;
    rs::fill_view(views[i], &v);
    float* val = value ? value[i] : nullptr;
    uint8_t* val8 = value8 ? value8[i] : nullptr;
    float* br = bary ? bary[i] : nullptr;
    const float* bg = option->background;
    switch (option->channels) {
      case 1: shade_view<1>(v, vertices, faces, attributes, face.data(), bg, val, val8, br); break;
      case 2: shade_view<2>(v, vertices, faces, attributes, face.data(), bg, val, val8, br); break;
      case 3: shade_view<3>(v, vertices, faces, attributes, face.data(), bg, val, val8, br); break;
      default: shade_view<4>(v, vertices, faces, attributes, face.data(), bg, val, val8, br); break;
    }
  }
  return VCY_OK;
}

int vcy_mesh_photo_error_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                              const float* colors, int n_views, const vcy_view* views, const uint8_t* const* photos,
                              const uint8_t* const* masks, int64_t* sums) {
  { const int rc = photo_error_check_args("vcy_mesh_photo_error_host", n_vertices, n_faces, vertices, faces, colors, n_views, views, photos, masks, sums); if (rc != VCY_OK) return rc; }
  std::vector<int32_t> face;
  for (int i = 0; i < n_views; ++i) {
    { const int rc = winners(n_vertices, n_faces, vertices, faces, views[i], &face); if (rc != VCY_OK) return rc; }
    rs::View v;
    rs::fill_view(views[i], &v);
    int64_t s[rs::kSums] = {0, 0, 0, 0, 0, 0, 0};
    for (int y = 0; y < v.h; ++y)
      for (int x = 0; x < v.w; ++x) {
        const int64_t px = (int64_t)v.w * y + x;
        if (face[(size_t)px] < 0 || (masks && masks[i][px] == 0)) continue;
        rs::Face f;
        rs::winner_face(v, vertices, faces, face[(size_t)px], f);
        double b[3];
        rs::weights(v, f, x, y, b);
        float val[3];
        rs::shade<3>(f, b, colors, val);
        s[0] += 1;
        for (int c = 0; c < 3; ++c) {
          const int64_t d = (int64_t)rs::quantize(val[c]) - (int64_t)photos[i][3 * px + c];
          s[1 + c] += d < 0 ? -d : d;
          s[4 + c] += d * d;
        }
      }
    for (int k = 0; k < rs::kSums; ++k) sums[(size_t)rs::kSums * i + k] = s[k];
  }
  return VCY_OK;
}

}  // extern "C"
