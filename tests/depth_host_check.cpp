// Stand-alone check of vcy_carve_depth_host (vacancy_amd/csrc/carve_depth_host.hip) for a host sanitizer build: no GPU, no
// HIP runtime, its own vcy::set_error.  `make -C vacancy_amd/csrc depth_host_check` builds it from carve_depth_host.hip
// alone with AddressSanitizer and UBSan on the host side and runs it (CPU only).  The case is the 65 x 9 x 17 grid under 70
// views of mixed camera models -- pinhole and orthographic, a shrunk and a one-pixel ROI, a camera that looks away --, with
// images that hold NaN, +-inf, 0, negative values and lowest(), generated here.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
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

constexpr int kW = 48, kH = 40, kViews = 70;

uint32_t g_seed = 12345u;
float uniform() {  // [0, 1)
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)(g_seed >> 8) * (1.0f / 16777216.0f);
}

// A camera at `pos` whose z axis points at the origin (or away from it), rows of w2c from an orthonormal frame.
vcy_view make_view(const float pos[3], bool away, bool ortho, int rx0, int ry0, int rx1, int ry1) {
  float z[3] = {-pos[0], -pos[1], -pos[2]};
  const float len = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
  for (float& c : z) c = (away ? -c : c) / len;
  const float up[3] = {0.0f, 1.0f, 0.1f};
  float x[3] = {up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]};
  const float lx = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  for (float& c : x) c /= lx;
  const float y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
  const float* rows[3] = {x, y, z};
  vcy_view v;
  std::memset(&v, 0, sizeof(v));
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) v.w2c[4 * r + k] = rows[r][k];
    v.w2c[4 * r + 3] = -(rows[r][0] * pos[0] + rows[r][1] * pos[1] + rows[r][2] * pos[2]);
  }
  if (ortho) {  // a pixel is a world unit: the origin in the middle of the image
    v.w2c[3] += kW / 2.0f;
    v.w2c[7] += kH / 2.0f;
  }
  v.fx = 34.0f * len / 65.0f;
  v.fy = v.fx * 1.07f;
  v.cx = kW / 2.0f - 0.3f;
  v.cy = kH / 2.0f + 0.2f;
  v.is_ortho = ortho ? 1 : 0;
  v.roi_min[0] = rx0, v.roi_min[1] = ry0, v.roi_max[0] = rx1, v.roi_max[1] = ry1;
  v.width = kW, v.height = kH;
  return v;
}

}  // namespace

int main() {
  vcy_carver_option opt;
  std::memset(&opt, 0, sizeof(opt));
  const float half[3] = {32.5f, 4.5f, 8.5f};
  for (int a = 0; a < 3; ++a) opt.bb_min[a] = -half[a], opt.bb_max[a] = half[a];
  opt.resolution = 1.0f;
  opt.sdf_minmax_normalize = 1;
  opt.update_option.voxel_update = VCY_UPDATE_WEIGHTED_AVERAGE;
  opt.update_option.sdf_interp = VCY_INTERP_BILINEAR;
  opt.update_option.update_outside = VCY_OUTSIDE_NONE;
  opt.update_option.voxel_max_update_num = 255;
  opt.update_option.voxel_update_weight = 0.7f;
  opt.update_option.truncation_band = 0.1f;
  const int32_t dims[3] = {65, 9, 17};  // (int)(diff / resolution) per axis
  const size_t n = (size_t)dims[0] * dims[1] * dims[2];

  std::vector<vcy_view> views;
  std::vector<std::vector<float>> images;
  const float lowest = std::numeric_limits<float>::lowest(), inf = std::numeric_limits<float>::infinity();
  for (int i = 0; i < kViews; ++i) {
    const float a = 6.2831853f * (float)i / (float)kViews;
    const float pos[3] = {std::cos(a) * 110.0f, 40.0f * std::sin(3.0f * a), std::sin(a) * 110.0f - 20.0f};
    const int k = i % 8;
    const bool ortho = k == 1 || k == 3 || k == 6;
    if (k == 2) views.push_back(make_view(pos, false, false, 5, 4, 40, 33));          // a shrunk ROI
    else if (k == 7) views.push_back(make_view(pos, false, false, 24, 20, 24, 20));    // one pixel
    else views.push_back(make_view(pos, k == 5, ortho, 0, 0, kW - 1, kH - 1));         // k == 5 looks away
    std::vector<float> img((size_t)kW * kH);
    const float dist = std::sqrt(pos[0] * pos[0] + pos[1] * pos[1] + pos[2] * pos[2]);
    for (float& z : img) {
      const float r = uniform();
      z = dist + 70.0f * (uniform() - 0.5f);
      if (r < 0.02f) z = std::nanf("");
      else if (r < 0.04f) z = inf;
      else if (r < 0.06f) z = -inf;
      else if (r < 0.08f) z = 0.0f;
      else if (r < 0.10f) z = -1.0f;
      else if (r < 0.12f) z = lowest;
    }
    images.push_back(std::move(img));
  }
  std::vector<const float*> ptrs;
  for (const std::vector<float>& img : images) ptrs.push_back(img.data());

  std::vector<float> sdf(n, lowest);
  std::vector<int32_t> cnt(n, 0);
  CHECK(vcy_carve_depth_host(&opt, 0, dims[2], kViews, views.data(), ptrs.data(), 1.7f, sdf.data(), cnt.data()) == VCY_OK);
  int64_t touched = 0, most = 0;
  for (size_t i = 0; i < n; ++i) {
    touched += cnt[i] > 0;
    most = cnt[i] > most ? cnt[i] : most;
    CHECK(cnt[i] >= 0 && cnt[i] <= kViews);
    // (a weighted average of samples in [-1, 1] is in [-1, 1] up to the rounding of its products)
    CHECK(cnt[i] > 0 ? (sdf[i] >= -1.001f && sdf[i] <= 1.001f) : sdf[i] == lowest);
  }
  CHECK(touched > (int64_t)n / 4 && most > 3);

  // two slabs, arrays of exactly their size, give the same state
  for (int k : {1, 8, 9}) {
    std::vector<float> s0((size_t)k * dims[0] * dims[1], lowest), s1(n - s0.size(), lowest);
    std::vector<int32_t> c0(s0.size(), 0), c1(s1.size(), 0);
    CHECK(vcy_carve_depth_host(&opt, 0, k, kViews, views.data(), ptrs.data(), 1.7f, s0.data(), c0.data()) == VCY_OK);
    CHECK(vcy_carve_depth_host(&opt, k, dims[2], kViews, views.data(), ptrs.data(), 1.7f, s1.data(), c1.data()) == VCY_OK);
    CHECK(std::memcmp(s0.data(), sdf.data(), s0.size() * sizeof(float)) == 0);
    CHECK(std::memcmp(s1.data(), sdf.data() + s0.size(), s1.size() * sizeof(float)) == 0);
    CHECK(std::memcmp(c0.data(), cnt.data(), c0.size() * sizeof(int32_t)) == 0);
    CHECK(std::memcmp(c1.data(), cnt.data() + c0.size(), c1.size() * sizeof(int32_t)) == 0);
  }

  // refusals: nothing is written
  const std::vector<float> before = sdf;
  CHECK(vcy_carve_depth_host(&opt, 0, dims[2], kViews, views.data(), ptrs.data(), 0.0f, sdf.data(), cnt.data()) == VCY_ERR_INVALID_ARG);
  CHECK(std::strstr(vcy::g_error, "band") != nullptr);
  CHECK(vcy_carve_depth_host(&opt, 0, dims[2], kViews, views.data(), ptrs.data(), std::nanf(""), sdf.data(), cnt.data()) ==
        VCY_ERR_INVALID_ARG);
  CHECK(vcy_carve_depth_host(&opt, 0, dims[2], kViews, views.data(), ptrs.data(), 1e-40f, sdf.data(), cnt.data()) == VCY_ERR_INVALID_ARG);
  CHECK(vcy_carve_depth_host(&opt, 0, dims[2], 0, views.data(), ptrs.data(), 1.7f, sdf.data(), cnt.data()) == VCY_ERR_INVALID_ARG);
  ptrs[35] = nullptr;
  CHECK(vcy_carve_depth_host(&opt, 0, dims[2], kViews, views.data(), ptrs.data(), 1.7f, sdf.data(), cnt.data()) == VCY_ERR_INVALID_ARG);
  CHECK(std::strstr(vcy::g_error, "view 35") != nullptr);
  ptrs[35] = images[35].data();
  views[3].roi_max[0] = kW;
  CHECK(vcy_carve_depth_host(&opt, 0, dims[2], kViews, views.data(), ptrs.data(), 1.7f, sdf.data(), cnt.data()) == VCY_ERR_INVALID_ARG);
  CHECK(vcy_carve_depth_host(&opt, 0, dims[2] + 1, 1, views.data(), ptrs.data(), 1.7f, sdf.data(), cnt.data()) == VCY_ERR_INVALID_ARG);
  CHECK(std::memcmp(before.data(), sdf.data(), n * sizeof(float)) == 0);

  std::puts("depth_host_check: ok");
  return 0;
}
