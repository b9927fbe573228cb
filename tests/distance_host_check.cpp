// Stand-alone check of vcy_distance_field_host (vacancy_amd/csrc/distance_host.hip) for a host sanitizer build: no GPU, no
// HIP runtime, its own vcy::set_error.  `make -C vacancy_amd/csrc distance_host_check` builds it from distance_host.hip alone
// with AddressSanitizer and UBSan on the host side and runs it (CPU only).  Two grids: 65 x 5 x 4 (a row of one whole
// 64-voxel word and one voxel) and 6 x 5 x 4 under a radius larger than every dimension; the states hold untouched voxels,
// NaNs and sdf == iso, generated here, and every result is compared with the definition by brute force over all pairs.
#include <algorithm>
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

uint32_t g_seed = 2024u;
float uniform() {  // [0, 1)
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)(g_seed >> 8) * (1.0f / 16777216.0f);
}

// 0 when every check held.  density: the share of solid voxels among the valid ones (0: nothing is solid, and every voxel
// must be FAR).
int run(const int32_t dims[3], float resolution, float density, double iso, int R) {
  vcy_carver_option opt;
  std::memset(&opt, 0, sizeof(opt));
  for (int a = 0; a < 3; ++a) opt.bb_min[a] = -0.5f * resolution * (float)dims[a], opt.bb_max[a] = 0.5f * resolution * (float)dims[a];
  opt.resolution = resolution;
  const int nx = dims[0], ny = dims[1], nz = dims[2];
  const size_t n = (size_t)nx * ny * nz;
  const float lowest = std::numeric_limits<float>::lowest();
  std::vector<float> sdf(n);
  std::vector<int32_t> cnt(n);
  for (size_t i = 0; i < n; ++i) {
    const float r = uniform();
    sdf[i] = uniform() < density ? -0.5f : 0.5f;
    cnt[i] = 1 + (int32_t)(uniform() * 3.0f);
    if (r < 0.03f) sdf[i] = lowest, cnt[i] = 0;
    else if (r < 0.05f) sdf[i] = std::nanf("");
    else if (r < 0.08f) sdf[i] = (float)iso;
  }
  // arrays of exactly their size: one voxel past the end is the sanitizer's business
  std::vector<int32_t> d2(n);
  std::vector<float> out(n);
  CHECK(vcy_distance_field_host(&opt, sdf.data(), cnt.data(), iso, R, d2.data(), out.data()) == VCY_OK);

  const int far = R * R + 1;
  int64_t exact = 0;
  for (size_t v = 0; v < n; ++v) {
    const bool solid = cnt[v] >= 1 && (double)sdf[v] < iso;
    const int vx = (int)(v % nx), vy = (int)(v / nx % ny), vz = (int)(v / ((size_t)nx * ny));
    int best = far;
    for (size_t u = 0; u < n; ++u) {
      if ((cnt[u] >= 1 && (double)sdf[u] < iso) == solid) continue;
      const int dx = (int)(u % nx) - vx, dy = (int)(u / nx % ny) - vy, dz = (int)(u / ((size_t)nx * ny)) - vz;
      best = std::min(best, dx * dx + dy * dy + dz * dz);
    }
    if (best > R * R) best = far;
    exact += best != far;
    CHECK(d2[v] == (solid ? -best : best));
    if (cnt[v] < 1) {
      CHECK(std::memcmp(&out[v], &sdf[v], sizeof(float)) == 0);
    } else {
      const float root = std::sqrt((float)std::min(best, R * R));
      const float shifted = root - 0.5f;
      const float phi = shifted * resolution;
      const float want = solid ? -phi : phi;
      CHECK(std::memcmp(&out[v], &want, sizeof(float)) == 0);
    }
  }
  if (density > 0.0f) CHECK(exact > 0);
  else CHECK(exact == 0);

  // either output alone, and in place
  std::vector<int32_t> d2b(n);
  CHECK(vcy_distance_field_host(&opt, sdf.data(), cnt.data(), iso, R, d2b.data(), nullptr) == VCY_OK);
  CHECK(d2b == d2);
  std::vector<float> in_place = sdf;
  CHECK(vcy_distance_field_host(&opt, in_place.data(), cnt.data(), iso, R, nullptr, in_place.data()) == VCY_OK);
  CHECK(std::memcmp(in_place.data(), out.data(), n * sizeof(float)) == 0);

  // refusals: nothing is written
  const std::vector<float> before = out;
  CHECK(vcy_distance_field_host(&opt, sdf.data(), cnt.data(), iso, 0, d2.data(), out.data()) == VCY_ERR_INVALID_ARG);
  CHECK(std::strstr(vcy::g_error, "radius") != nullptr);
  CHECK(vcy_distance_field_host(&opt, sdf.data(), cnt.data(), iso, 128, d2.data(), out.data()) == VCY_ERR_INVALID_ARG);
  CHECK(vcy_distance_field_host(&opt, nullptr, cnt.data(), iso, R, d2.data(), out.data()) == VCY_ERR_INVALID_ARG);
  CHECK(std::memcmp(before.data(), out.data(), n * sizeof(float)) == 0 && d2b == d2);
  return 0;
}

}  // namespace

int main() {
  const int32_t wide[3] = {65, 5, 4}, small[3] = {6, 5, 4};
  int failed = 0;
  failed += run(wide, 1.0f, 0.3f, 0.0, 5);
  failed += run(wide, 0.375f, 0.01f, 0.25, 127);  // distances of up to 64 along the row
  failed += run(wide, 1.0f, 0.97f, 0.0, 70);
  failed += run(small, 0.375f, 0.1f, 0.25, 12);   // R beyond the grid
  failed += run(small, 1.0f, 0.0f, 0.0, 9);       // nothing solid: FAR everywhere
  if (failed) return 1;
  std::puts("distance_host_check: ok");
  return 0;
}
