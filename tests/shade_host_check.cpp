// Stand-alone check of vcy_shade_mesh_host and vcy_mesh_photo_error_host (vacancy_amd/csrc/shade_host.hip) with the
// rasteriser's host code behind them (raster_host.hip, render_merge.hip) for a host sanitizer build: no GPU, no HIP runtime,
// its own vcy::set_error.  `make -C vacancy_amd/csrc shade_host_check` builds the files with AddressSanitizer and UBSan on
// the host side and runs the program (CPU only).  The scenes are generated here and their answers are literals: the tilted
// lattice quad in an identity ortho view with an attribute linear in (x, y), a fronto-parallel triangle in a pinhole, a
// triangle far larger than a 130-wide image, non-finite attributes; every array is exactly as long as the sizes say.
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
  int w, h, ch;
  std::vector<float> value, bary;
  std::vector<uint8_t> value8;
  Images(int w_, int h_, int ch_)
      : w(w_), h(h_), ch(ch_), value((size_t)w_ * h_ * ch_, 77.0f), bary((size_t)w_ * h_ * 3, 77.0f), value8((size_t)w_ * h_ * ch_, 77) {}
  bool untouched() const {
    for (float x : value)
      if (x != 77.0f) return false;
    for (float x : bary)
      if (x != 77.0f) return false;
    for (uint8_t x : value8)
      if (x != 77) return false;
    return true;
  }
};

int shade(const std::vector<float>& v, const std::vector<int32_t>& f, const std::vector<float>& a, const vcy_view& view,
          const vcy_shade_option& opt, Images* im) {
  float* val = im->value.data();
  uint8_t* val8 = im->value8.data();
  float* br = im->bary.data();
  return vcy_shade_mesh_host((int64_t)v.size() / 3, (int64_t)f.size() / 3, v.data(), f.data(), a.data(), 1, &view, &opt, &val, &val8, &br);
}

}  // namespace

int main() {
  // the lattice quad over [2, 10]^2 with the attribute (70 + 4 x + 2.5 y, 250 - 8 x - 0.25 y): exact weights
  const std::vector<float> quad_v = {2, 2, 4, 10, 2, 8, 2, 10, 6, 10, 10, 10};
  const std::vector<int32_t> quad_f = {0, 1, 2, 1, 3, 2};
  std::vector<float> quad_a;
  for (int k = 0; k < 4; ++k) {
    const float x = quad_v[3 * k], y = quad_v[3 * k + 1];
    quad_a.push_back(70.0f + 4.0f * x + 2.5f * y);
    quad_a.push_back(250.0f - 8.0f * x - 0.25f * y);
  }
  const vcy_shade_option two{2, {1.0f, 300.0f, 0.0f, 0.0f}};
  {
    Images im(48, 40, 2);
    CHECK(shade(quad_v, quad_f, quad_a, identity_view(48, 40, true), two, &im) == VCY_OK);
    for (int y = 0; y < 40; ++y)
      for (int x = 0; x < 48; ++x) {
        const bool in = x >= 2 && x <= 10 && y >= 2 && y <= 10;
        const size_t px = (size_t)y * 48 + x;
        const float want0 = in ? 70.0f + 4.0f * x + 2.5f * y : 1.0f, want1 = in ? 250.0f - 8.0f * x - 0.25f * y : 300.0f;
        CHECK(im.value[2 * px] == want0 && im.value[2 * px + 1] == want1);
        CHECK(im.value8[2 * px] == (uint8_t)std::floor(want0 + 0.5f) && im.value8[2 * px + 1] == (in ? (uint8_t)std::floor(want1 + 0.5f) : 255));
        const float sum = im.bary[3 * px] + im.bary[3 * px + 1] + im.bary[3 * px + 2];
        CHECK(sum == (in ? 1.0f : 0.0f));
      }
    CHECK(im.bary[3 * ((size_t)2 * 48 + 2)] == 1.0f && im.bary[3 * ((size_t)2 * 48 + 10) + 1] == 1.0f);
  }
  {  // a fronto-parallel triangle at depth 4 in the pinhole: b_k = l_k; one channel; the photometric error of a constant
    const std::vector<float> v = {-2, -2, 4, 2, -2, 4, -2, 2, 4};
    const std::vector<int32_t> f = {0, 1, 2};
    const vcy_view view = identity_view(48, 40, false);
    Images im(48, 40, 1);
    const vcy_shade_option one{1, {0.0f, 0.0f, 0.0f, 0.0f}};
    CHECK(shade(v, f, {64.0f, 96.0f, 128.0f}, view, one, &im) == VCY_OK);
    int n = 0;
    for (int y = 0; y < 40; ++y)
      for (int x = 0; x < 48; ++x) {
        const bool in = x >= 8 && y >= 4 && (x - 8) + (y - 4) <= 32;
        const size_t px = (size_t)y * 48 + x;
        CHECK(im.bary[3 * px + 1] == (in ? (float)(x - 8) / 32.0f : 0.0f) && im.bary[3 * px + 2] == (in ? (float)(y - 4) / 32.0f : 0.0f));
        CHECK(im.value[px] == (in ? 64.0f + (float)(x - 8) + 2.0f * (float)(y - 4) : 0.0f));
        n += in;
      }
    CHECK(n == 33 * 34 / 2);
    const std::vector<float> white(9, 255.0f);
    std::vector<uint8_t> photo((size_t)48 * 40 * 3, 0), mask((size_t)48 * 40, 0);
    for (size_t i = 0; i < photo.size(); i += 3) photo[i + 1] = 255, photo[i + 2] = 250;
    for (int y = 0; y < 40; ++y)
      for (int x = 0; x < 8 + 5; ++x) mask[(size_t)y * 48 + x] = 9;  // the columns 8 .. 12 of the triangle: 33 + 32 + 31 + 30 + 29
    const uint8_t* pp = photo.data();
    const uint8_t* mp = mask.data();
    int64_t sums[7] = {77, 77, 77, 77, 77, 77, 77};
    CHECK(vcy_mesh_photo_error_host(3, 1, v.data(), f.data(), white.data(), 1, &view, &pp, nullptr, sums) == VCY_OK);
    CHECK(sums[0] == n && sums[1] == 255 * n && sums[2] == 0 && sums[3] == 5 * n && sums[4] == 65025 * n && sums[5] == 0 && sums[6] == 25 * n);
    CHECK(vcy_mesh_photo_error_host(3, 1, v.data(), f.data(), white.data(), 1, &view, &pp, &mp, sums) == VCY_OK);
    CHECK(sums[0] == 155 && sums[1] == 255 * 155 && sums[6] == 25 * 155);
    std::fill(mask.begin(), mask.end(), 0);
    CHECK(vcy_mesh_photo_error_host(3, 1, v.data(), f.data(), white.data(), 1, &view, &pp, &mp, sums) == VCY_OK);
    for (int64_t s : sums) CHECK(s == 0);
    // refusals of the error call: nothing is written
    int64_t kept[7] = {77, 77, 77, 77, 77, 77, 77};
    const uint8_t* none = nullptr;
    CHECK(vcy_mesh_photo_error_host(3, 1, v.data(), f.data(), white.data(), 1, &view, nullptr, &mp, kept) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_mesh_photo_error_host(3, 1, v.data(), f.data(), white.data(), 1, &view, &none, &mp, kept) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_mesh_photo_error_host(3, 1, v.data(), f.data(), white.data(), 1, &view, &pp, &none, kept) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_mesh_photo_error_host(3, 1, v.data(), f.data(), nullptr, 1, &view, &pp, &mp, kept) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_mesh_photo_error_host(3, 1, v.data(), f.data(), white.data(), 1, &view, &pp, &mp, nullptr) == VCY_ERR_INVALID_ARG);
    for (int64_t s : kept) CHECK(s == 77);
  }
  {  // a triangle far larger than a 130-wide image, a ROI inside it, four channels with non-finite attributes; NULL outputs
    vcy_view view = identity_view(130, 7, true);
    view.roi_min[0] = 3, view.roi_min[1] = 1, view.roi_max[0] = 128, view.roi_max[1] = 5;
    const std::vector<float> v = {-4000, -3000, 9, 5000, -3000, 9, -4000, 6000, 9};
    const std::vector<int32_t> f = {0, 1, 2};
    const std::vector<float> a = {100, NAN, INFINITY, -5, 100, 3, INFINITY, -5, 100, 3, INFINITY, 400};
    const vcy_shade_option four{4, {NAN, -1.0f, 254.5f, 0.5f}};
    Images im(130, 7, 4);
    CHECK(shade(v, f, a, view, four, &im) == VCY_OK);
    for (int y = 0; y < 7; ++y)
      for (int x = 0; x < 130; ++x) {
        const bool in = x >= 3 && x <= 128 && y >= 1 && y <= 5;
        const size_t px = (size_t)y * 130 + x;
        if (in) {
          CHECK(std::fabs(im.value[4 * px] - 100.0f) < 1e-4f && std::isnan(im.value[4 * px + 1]) && std::isinf(im.value[4 * px + 2]));
          CHECK(im.value8[4 * px] == 100 && im.value8[4 * px + 1] == 0 && im.value8[4 * px + 2] == 255);
        } else {
          CHECK(std::isnan(im.value[4 * px]) && im.value[4 * px + 1] == -1.0f && im.value[4 * px + 3] == 0.5f);
          CHECK(im.value8[4 * px] == 0 && im.value8[4 * px + 1] == 0 && im.value8[4 * px + 2] == 255 && im.value8[4 * px + 3] == 1);
          CHECK(im.bary[3 * px] == 0.0f && im.bary[3 * px + 1] == 0.0f && im.bary[3 * px + 2] == 0.0f);
        }
      }
    uint8_t* v8 = im.value8.data();
    CHECK(vcy_shade_mesh_host(3, 1, v.data(), f.data(), a.data(), 1, &view, &four, nullptr, &v8, nullptr) == VCY_OK);
    float* none = nullptr;
    CHECK(vcy_shade_mesh_host(3, 1, v.data(), f.data(), a.data(), 1, &view, &four, &none, nullptr, &none) == VCY_OK);
    CHECK(vcy_shade_mesh_host(3, 0, v.data(), nullptr, a.data(), 1, &view, &four, nullptr, &v8, nullptr) == VCY_OK);  // no faces
    CHECK(vcy_shade_mesh_host(0, 0, nullptr, nullptr, nullptr, 1, &view, &four, nullptr, &v8, nullptr) == VCY_OK);   // no mesh
    for (size_t i = 0; i < im.value8.size(); i += 4) CHECK(im.value8[i] == 0 && im.value8[i + 2] == 255 && im.value8[i + 3] == 1);
  }

  // refusals: nothing is written
  {
    Images im(48, 40, 2);
    vcy_view view = identity_view(48, 40, true);
    CHECK(shade(quad_v, quad_f, quad_a, view, vcy_shade_option{0, {0, 0, 0, 0}}, &im) == VCY_ERR_INVALID_ARG && im.untouched());
    CHECK(shade(quad_v, quad_f, quad_a, view, vcy_shade_option{5, {0, 0, 0, 0}}, &im) == VCY_ERR_INVALID_ARG && im.untouched());
    std::vector<int32_t> bad = quad_f;
    bad[4] = 4;
    CHECK(shade(quad_v, bad, quad_a, view, two, &im) == VCY_ERR_INVALID_ARG && im.untouched());
    CHECK(std::strstr(vcy::g_error, "face 1") != nullptr);
    view.roi_max[0] = 48;
    CHECK(shade(quad_v, quad_f, quad_a, view, two, &im) == VCY_ERR_INVALID_ARG && im.untouched());
    view = identity_view(48, 40, true);
    float* val = im.value.data();
    CHECK(vcy_shade_mesh_host(4, 2, quad_v.data(), quad_f.data(), quad_a.data(), 1, &view, nullptr, &val, nullptr, nullptr) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_shade_mesh_host(4, 2, quad_v.data(), quad_f.data(), nullptr, 1, &view, &two, &val, nullptr, nullptr) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_shade_mesh_host(4, 2, quad_v.data(), quad_f.data(), quad_a.data(), 0, &view, &two, &val, nullptr, nullptr) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_shade_mesh_host(4, (int64_t)1 << 30, quad_v.data(), quad_f.data(), quad_a.data(), 1, &view, &two, &val, nullptr, nullptr) == VCY_ERR_UNSUPPORTED);
    CHECK(im.untouched());
  }

  std::puts("shade_host_check: ok");
  return 0;
}
