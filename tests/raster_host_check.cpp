// Stand-alone check of vcy_raster_mesh_host (vacancy_amd/csrc/raster_host.hip) and the vcy_hull_agreement_host that reads
// its hit bits (render_merge.hip) for a host sanitizer build: no GPU, no HIP runtime, its own vcy::set_error.  `make -C
// vacancy_amd/csrc raster_host_check` builds the three files with AddressSanitizer and UBSan on the host side and runs the
// program (CPU only).  The scenes are generated here and their answers are literals: the tilted lattice quad in an identity
// ortho view, a fronto-parallel triangle in a pinhole, a triangle far larger than the image, coordinates no int holds,
// non-finite vertices, a 130-wide image; every array is exactly as long as the sizes say.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vacancy_hip.h"

namespace vcy {
thread_local char g_error[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}
}  // namespace vcy

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                      \
    }                                                                \
  } while (0)

namespace {

vcy_view identity_view(int w, int h, bool ortho) {
  vcy_view v{};
  v.w2c[0] = v.w2c[5] = v.w2c[10] = 1.0f;
  v.fx = v.fy = ortho ? 1.0f : 32.0f;
  v.cx = ortho ? 0.0f : (float)w / 2, v.cy = ortho ? 0.0f : (float)h / 2;
  v.is_ortho = ortho;
  v.roi_min[0] = v.roi_min[1] = 0;
  v.roi_max[0] = w - 1, v.roi_max[1] = h - 1;
  v.width = w, v.height = h;
  return v;
}

struct Images {
  int w, h;
  std::vector<float> depth;
  std::vector<int32_t> face;
  std::vector<uint64_t> hits;
  int64_t dropped[2];
  Images(int w_, int h_) : w(w_), h(h_), depth((size_t)w_ * h_, 77.0f), face((size_t)w_ * h_, 77), hits((size_t)((w_ + 63) / 64) * h_, 77), dropped{77, 77} {}
  bool hit(int x, int y) const { return (hits[(size_t)y * ((w + 63) / 64) + (x >> 6)] >> (x & 63)) & 1; }
};

int raster(const std::vector<float>& v, const std::vector<int32_t>& f, const vcy_view& view, Images* im) {
  float* d = im->depth.data();
  int32_t* fo = im->face.data();
  uint64_t* hb = im->hits.data();
  return vcy_raster_mesh_host((int64_t)v.size() / 3, (int64_t)f.size() / 3, v.data(), f.data(), 1, &view, &d, &fo, &hb, im->dropped);
}

}  // namespace

int main() {
  // the lattice quad: z = 4 + (x - 2) / 2 + (y - 2) / 4 over [2, 10]^2, the diagonal x + y = 12 shared
  const std::vector<float> quad_v = {2, 2, 4, 10, 2, 8, 2, 10, 6, 10, 10, 10};
  const std::vector<int32_t> quad_f = {0, 1, 2, 1, 3, 2};
  {
    Images im(48, 40);
    CHECK(raster(quad_v, quad_f, identity_view(48, 40, true), &im) == VCY_OK);
    for (int y = 0; y < 40; ++y)
      for (int x = 0; x < 48; ++x) {
        const bool in = x >= 2 && x <= 10 && y >= 2 && y <= 10;
        CHECK(im.hit(x, y) == in);
        CHECK(im.face[(size_t)y * 48 + x] == (!in ? -1 : x + y <= 12 ? 0 : 1));
        const float d = im.depth[(size_t)y * 48 + x];
        CHECK(in ? d == 4.0f + (float)(x - 2) * 0.5f + (float)(y - 2) * 0.25f : std::isinf(d) && d > 0);
      }
    CHECK(im.dropped[0] == 0 && im.dropped[1] == 0);
    // its agreement with a silhouette that covers the columns 0 .. 5
    std::vector<uint8_t> mask((size_t)48 * 40, 0);
    for (int y = 0; y < 40; ++y)
      for (int x = 0; x < 6; ++x) mask[(size_t)y * 48 + x] = 1;
    const vcy_view view = identity_view(48, 40, true);
    const uint64_t* hb = im.hits.data();
    int64_t counts[3] = {0, 0, 0};
    CHECK(vcy_hull_agreement_host(&view, 1, &hb, mask.data(), counts) == VCY_OK);
    CHECK(counts[0] == 36 && counts[1] == 240 - 36 && counts[2] == 45);
  }
  {  // a fronto-parallel triangle at depth 4 in the pinhole: (8, 4), (40, 4), (8, 36) on the image
    Images im(48, 40);
    CHECK(raster({-2, -2, 4, 2, -2, 4, -2, 2, 4}, {0, 1, 2}, identity_view(48, 40, false), &im) == VCY_OK);
    int n = 0;
    for (int y = 0; y < 40; ++y)
      for (int x = 0; x < 48; ++x) {
        const bool in = x >= 8 && y >= 4 && (x - 8) + (y - 4) <= 32;
        CHECK(im.hit(x, y) == in);
        if (in) {
          CHECK(im.depth[(size_t)y * 48 + x] == 4.0f);
          ++n;
        }
      }
    CHECK(n == 33 * 34 / 2);
  }
  {  // a triangle far larger than a 130-wide image, a ROI inside it; NULL outputs one at a time
    vcy_view view = identity_view(130, 7, true);
    view.roi_min[0] = 3, view.roi_min[1] = 1, view.roi_max[0] = 128, view.roi_max[1] = 5;
    Images im(130, 7);
    CHECK(raster({-4000, -3000, 9, 5000, -3000, 9, -4000, 6000, 9}, {0, 1, 2}, view, &im) == VCY_OK);
    for (int y = 0; y < 7; ++y)
      for (int x = 0; x < 192; ++x) {
        const bool in = x >= 3 && x <= 128 && y >= 1 && y <= 5;
        CHECK(((im.hits[(size_t)y * 3 + (x >> 6)] >> (x & 63)) & 1) == (uint64_t)in);  // (the padding of a row is 0)
      }
    const std::vector<float> v = {-4000, -3000, 9, 5000, -3000, 9, -4000, 6000, 9};
    const std::vector<int32_t> f = {0, 1, 2};
    uint64_t* hb = im.hits.data();
    CHECK(vcy_raster_mesh_host(3, 1, v.data(), f.data(), 1, &view, nullptr, nullptr, &hb, nullptr) == VCY_OK);
    float* none = nullptr;
    CHECK(vcy_raster_mesh_host(3, 1, v.data(), f.data(), 1, &view, &none, nullptr, nullptr, nullptr) == VCY_OK);
  }
  {  // coordinates no int holds, non-finite vertices, a vertex behind the camera, degenerate faces, no faces at all
    const float big = 1.0e30f;
    const std::vector<float> v = {-big, -big, 1, big, -big, 1, 0, big, 1, NAN, 0, 1, 0, INFINITY, 1, 5, 5, -1, 3, 3, 2, 6, 6, 2, 9, 9, 2};
    const std::vector<int32_t> f = {0, 1, 2, 0, 1, 3, 0, 1, 4, 0, 1, 5, 6, 7, 8, 6, 6, 7};
    Images im(48, 40);
    CHECK(raster(v, f, identity_view(48, 40, true), &im) == VCY_OK);
    CHECK(im.dropped[0] == 3 && im.dropped[1] == 2);
    for (int y = 0; y < 40; ++y)
      for (int x = 0; x < 48; ++x) CHECK(im.hit(x, y) && im.face[(size_t)y * 48 + x] == 0 && im.depth[(size_t)y * 48 + x] == 1.0f);
    Images empty(48, 40);
    CHECK(raster({1, 2, 3}, {}, identity_view(48, 40, false), &empty) == VCY_OK);
    for (size_t i = 0; i < empty.face.size(); ++i) CHECK(empty.face[i] == -1 && std::isinf(empty.depth[i]));
    for (uint64_t word : empty.hits) CHECK(word == 0);
    CHECK(empty.dropped[0] == 0 && empty.dropped[1] == 0);
  }

  // refusals: nothing is written
  {
    Images im(48, 40);
    const auto untouched = [&] {
      for (float x : im.depth)
        if (x != 77.0f) return false;
      for (int32_t x : im.face)
        if (x != 77) return false;
      for (uint64_t x : im.hits)
        if (x != 77) return false;
      return im.dropped[0] == 77 && im.dropped[1] == 77;
    };
    vcy_view view = identity_view(48, 40, true);
    std::vector<int32_t> bad = quad_f;
    bad[4] = 4;
    CHECK(raster(quad_v, bad, view, &im) == VCY_ERR_INVALID_ARG && untouched());
    CHECK(std::strstr(vcy::g_error, "face 1") != nullptr);
    bad[4] = -1;
    CHECK(raster(quad_v, bad, view, &im) == VCY_ERR_INVALID_ARG && untouched());
    view.roi_max[0] = 48;
    CHECK(raster(quad_v, quad_f, view, &im) == VCY_ERR_INVALID_ARG && untouched());
    view = identity_view(48, 40, false);
    view.fx = 0.0f;
    CHECK(raster(quad_v, quad_f, view, &im) == VCY_ERR_INVALID_ARG && untouched());
    view = identity_view(48, 40, true);
    view.w2c[3] = NAN;
    CHECK(raster(quad_v, quad_f, view, &im) == VCY_ERR_INVALID_ARG && untouched());
    view = identity_view(48, 40, true);
    float* d = im.depth.data();
    CHECK(vcy_raster_mesh_host(4, 2, quad_v.data(), quad_f.data(), 0, &view, &d, nullptr, nullptr, im.dropped) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_raster_mesh_host(4, 2, nullptr, quad_f.data(), 1, &view, &d, nullptr, nullptr, im.dropped) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_raster_mesh_host(4, 2, quad_v.data(), nullptr, 1, &view, &d, nullptr, nullptr, im.dropped) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_raster_mesh_host(4, 2, quad_v.data(), quad_f.data(), 1, nullptr, &d, nullptr, nullptr, im.dropped) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_raster_mesh_host(-1, 2, quad_v.data(), quad_f.data(), 1, &view, &d, nullptr, nullptr, im.dropped) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_raster_mesh_host(4, (int64_t)1 << 30, quad_v.data(), quad_f.data(), 1, &view, &d, nullptr, nullptr, im.dropped) == VCY_ERR_UNSUPPORTED);
    CHECK(untouched());
  }

  std::puts("raster_host_check: ok");
  return 0;
}
