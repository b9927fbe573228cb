// Stand-alone check of the two halves of the distance field of a z-slab on the host (vcy_distance_slab_planes_host,
// vcy_distance_slab_finish_host; vacancy_amd/csrc/distance_host.hip) for a host sanitizer build: no GPU, no HIP runtime,
// its own vcy::set_error.  `make -C vacancy_amd/csrc slab_distance_host_check` builds it from distance_host.hip alone with
// AddressSanitizer and UBSan on the host side and runs it (CPU only).  Grids of 65 x 5 x nz and 6 x 5 x nz cut along z --
// slabs of 2 slices, slabs thinner than the radius so that a slab's planes come from several neighbours, a radius beyond
// the grid --; every array has exactly its size, the planes of a slab's neighbours are cut out of the slabs' own planes as
// the library's callers do it, and the slabs' results, put together, must equal vcy_distance_field_host of the whole grid
// byte for byte.
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

uint32_t g_seed = 4711u;
float uniform() {  // [0, 1)
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)(g_seed >> 8) * (1.0f / 16777216.0f);
}

// 0 when every check held.  `cuts`: the slabs' bounds, 0 first, nz last.
int run(const int32_t dims[3], float resolution, float density, double iso, int R, const std::vector<int>& cuts) {
  vcy_carver_option opt;
  std::memset(&opt, 0, sizeof(opt));
  for (int a = 0; a < 3; ++a) opt.bb_min[a] = -0.5f * resolution * (float)dims[a], opt.bb_max[a] = 0.5f * resolution * (float)dims[a];
  opt.resolution = resolution;
  const int nx = dims[0], ny = dims[1], nz = dims[2];
  const size_t slice = (size_t)nx * ny, n = slice * nz;
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
  std::vector<int32_t> want_d2(n);
  std::vector<float> want_sdf(n);
  CHECK(vcy_distance_field_host(&opt, sdf.data(), cnt.data(), iso, R, want_d2.data(), want_sdf.data()) == VCY_OK);

  // step 1 and 2: every slab's planes, each in an array of its own size
  const size_t n_slabs = cuts.size() - 1;
  std::vector<std::vector<uint16_t>> h(n_slabs);
  for (size_t s = 0; s < n_slabs; ++s) {
    const int z0 = cuts[s], z1 = cuts[s + 1];
    const std::vector<float> s_sdf(sdf.begin() + z0 * slice, sdf.begin() + z1 * slice);
    const std::vector<int32_t> s_cnt(cnt.begin() + z0 * slice, cnt.begin() + z1 * slice);
    h[s].resize(slice * (size_t)(z1 - z0));
    CHECK(vcy_distance_slab_planes_host(&opt, z0, z1, s_sdf.data(), s_cnt.data(), iso, R, h[s].data()) == VCY_OK);
  }
  // the global slice z of the planes, from whichever slab owns it
  auto plane_of = [&](int z) -> const uint16_t* {
    for (size_t s = 0; s < n_slabs; ++s)
      if (z >= cuts[s] && z < cuts[s + 1]) return h[s].data() + (size_t)(z - cuts[s]) * slice;
    return nullptr;
  };
  // step 3
  for (size_t s = 0; s < n_slabs; ++s) {
    const int z0 = cuts[s], z1 = cuts[s + 1];
    const int nb = std::min(R, z0), na = std::min(R, nz - z1);
    std::vector<uint16_t> below(slice * (size_t)nb), above(slice * (size_t)na);
    for (int k = 0; k < nb; ++k) std::memcpy(below.data() + k * slice, plane_of(z0 - nb + k), slice * sizeof(uint16_t));
    for (int k = 0; k < na; ++k) std::memcpy(above.data() + k * slice, plane_of(z1 + k), slice * sizeof(uint16_t));
    const size_t m = slice * (size_t)(z1 - z0);
    const std::vector<float> s_sdf(sdf.begin() + z0 * slice, sdf.begin() + z1 * slice);
    const std::vector<int32_t> s_cnt(cnt.begin() + z0 * slice, cnt.begin() + z1 * slice);
    std::vector<int32_t> d2(m);
    std::vector<float> out(m);
    const uint16_t* pb = nb ? below.data() : nullptr;
    const uint16_t* pa = na ? above.data() : nullptr;
    CHECK(vcy_distance_slab_finish_host(&opt, z0, z1, h[s].data(), pb, nb, pa, na, R, s_cnt.data(), s_sdf.data(), d2.data(),
                                        out.data()) == VCY_OK);
    CHECK(std::memcmp(d2.data(), want_d2.data() + z0 * slice, m * sizeof(int32_t)) == 0);
    CHECK(std::memcmp(out.data(), want_sdf.data() + z0 * slice, m * sizeof(float)) == 0);
    // the field alone without a state, and the sdf in place
    std::vector<int32_t> d2b(m);
    CHECK(vcy_distance_slab_finish_host(&opt, z0, z1, h[s].data(), pb, nb, pa, na, R, nullptr, nullptr, d2b.data(), nullptr) == VCY_OK);
    CHECK(d2b == d2);
    std::vector<float> in_place = s_sdf;
    CHECK(vcy_distance_slab_finish_host(&opt, z0, z1, h[s].data(), pb, nb, pa, na, R, s_cnt.data(), in_place.data(), nullptr,
                                        in_place.data()) == VCY_OK);
    CHECK(std::memcmp(in_place.data(), out.data(), m * sizeof(float)) == 0);
    // refusals: nothing is written
    const std::vector<float> before = out;
    CHECK(vcy_distance_slab_finish_host(&opt, z0, z1, h[s].data(), pb, nb + 1, pa, na, R, s_cnt.data(), s_sdf.data(), d2.data(),
                                        out.data()) == VCY_ERR_INVALID_ARG);
    CHECK(std::strstr(vcy::g_error, "planes") != nullptr);
    CHECK(vcy_distance_slab_finish_host(&opt, z0, z1, h[s].data(), pb, nb, pa, na - 1, R, s_cnt.data(), s_sdf.data(), d2.data(),
                                        out.data()) == VCY_ERR_INVALID_ARG);
    if (nb) CHECK(vcy_distance_slab_finish_host(&opt, z0, z1, h[s].data(), nullptr, nb, pa, na, R, s_cnt.data(), s_sdf.data(),
                                                d2.data(), out.data()) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_distance_slab_finish_host(&opt, z0, z1, h[s].data(), pb, nb, pa, na, 0, s_cnt.data(), s_sdf.data(), d2.data(),
                                        out.data()) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_distance_slab_finish_host(&opt, z0, nz + 1, h[s].data(), pb, nb, pa, na, R, s_cnt.data(), s_sdf.data(), d2.data(),
                                        out.data()) == VCY_ERR_INVALID_ARG);
    CHECK(out == before || std::memcmp(out.data(), before.data(), m * sizeof(float)) == 0);
    CHECK(d2b == d2);
    CHECK(vcy_distance_slab_planes_host(&opt, z1, z0, s_sdf.data(), s_cnt.data(), iso, R, h[s].data()) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_distance_slab_planes_host(&opt, z0, z1, s_sdf.data(), s_cnt.data(), iso, 128, h[s].data()) == VCY_ERR_INVALID_ARG);
  }
  return 0;
}

}  // namespace

int main() {
  const int32_t wide[3] = {65, 5, 9}, small[3] = {6, 5, 12}, tall[3] = {6, 5, 20};
  int failed = 0;
  failed += run(wide, 1.0f, 0.3f, 0.0, 3, {0, 2, 7, 9});          // cuts at z = 2 and z = nz - 2
  failed += run(wide, 0.375f, 0.05f, 0.25, 127, {0, 4, 9});       // R beyond the grid: every slab sees every plane
  failed += run(small, 1.0f, 0.1f, 0.0, 5, {0, 3, 5, 7, 12});     // slabs of 2 slices: planes from three neighbours
  failed += run(small, 0.375f, 0.9f, 0.25, 4, {0, 12});           // one slab: nothing at either end
  failed += run(tall, 1.0f, 0.02f, 0.0, 7, {0, 2, 4, 6, 13, 20});
  failed += run(tall, 1.0f, 0.0f, 0.0, 9, {0, 10, 20});           // nothing solid: FAR everywhere
  if (failed) return 1;
  std::puts("slab_distance_host_check: ok");
  return 0;
}
