// The distance field of the hull on the host (vcy_distance_field_host): the definition of the section "distance field of
// the hull" of vacancy_hip.h run serially -- the row distances by two sweeps, then the y pass and the z pass as they are
// written there.  Host code only -- no GPU, no context, nothing of the HIP runtime --, so a stand-alone program can build
// it under host sanitizers (tests/distance_host_check.cpp, `make distance_host_check`).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "distance_field.h"
#include "host_shared.h"

using namespace vcy;

namespace {

// out[i] = min over |d| <= R, i + d in [0, n), of (cls[i+d] != cls[i] ? 0 : in[i+d]) + d*d, along one line of n
// elements `stride` apart.  Candidates only grow with |d|: the walk ends as soon as d*d cannot win.
void line_pass(const int32_t* in, const uint8_t* cls, int64_t stride, int n, int R, int32_t* out) {
  for (int i = 0; i < n; ++i) {
    const uint8_t c = cls[(int64_t)i * stride];
    int32_t best = in[(int64_t)i * stride];
    for (int d = 1; d <= R && d * d < best; ++d) {
      for (int s = -1; s <= 1; s += 2) {
        const int j = i + s * d;
        if (j < 0 || j >= n) continue;
        const int32_t cand = (cls[(int64_t)j * stride] != c ? 0 : in[(int64_t)j * stride]) + d * d;
        best = std::min(best, cand);
      }
    }
    out[i] = best;
  }
}

}  // namespace

extern "C" int vcy_distance_field_host(const vcy_carver_option* option, const float* sdf, const int32_t* update_num,
                                       double iso_level, int radius, int32_t* d2, float* sdf_out) {
  if (!option || !sdf || !update_num) {
    set_error("vcy_distance_field_host: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  { const int rc = df::check_radius("vcy_distance_field_host", radius); if (rc != VCY_OK) return rc; }
  int32_t dims[3];
  { const int rc = dims_from_option(option->bb_min, option->bb_max, option->resolution, dims); if (rc != VCY_OK) return rc; }
  const int nx = dims[0], ny = dims[1], nz = dims[2], R = radius, far = df::far_of(R);
  const int64_t slice = (int64_t)nx * ny, n = slice * nz;
  std::vector<uint8_t> cls((size_t)n);
  for (int64_t v = 0; v < n; ++v) cls[(size_t)v] = update_num[v] >= 1 && (double)sdf[v] < iso_level ? 1 : 0;

  // x pass: the nearest voxel of the other class to the left, then to the right
  std::vector<int32_t> g((size_t)n), h((size_t)n);
  for (int64_t row = 0; row < (int64_t)ny * nz; ++row) {
    const uint8_t* c = cls.data() + row * nx;
    int32_t* gr = g.data() + row * nx;
    int last[2] = {-1, -1};  // the last voxel of either class seen so far
    for (int x = 0; x < nx; ++x) {
      last[c[x]] = x;
      const int o = last[1 - c[x]];
      gr[x] = o >= 0 ? x - o : R + 1;
    }
    last[0] = last[1] = -1;
    for (int x = nx - 1; x >= 0; --x) {
      last[c[x]] = x;
      const int o = last[1 - c[x]];
      const int d = std::min(gr[x], o >= 0 ? o - x : R + 1);
      gr[x] = d <= R ? d * d : far;
    }
  }
  // y pass, z pass; lines along y are `nx` apart, lines along z a slice
  std::vector<int32_t> line((size_t)std::max(ny, nz));
  for (int z = 0; z < nz; ++z)
    for (int x = 0; x < nx; ++x) {
      const int64_t at = (int64_t)z * slice + x;
      line_pass(g.data() + at, cls.data() + at, nx, ny, R, line.data());
      for (int y = 0; y < ny; ++y) h[(size_t)(at + (int64_t)y * nx)] = line[(size_t)y];
    }
  for (int64_t at = 0; at < slice; ++at) {
    line_pass(h.data() + at, cls.data() + at, slice, nz, R, line.data());
    for (int z = 0; z < nz; ++z) g[(size_t)(at + (int64_t)z * slice)] = line[(size_t)z] > R * R ? far : line[(size_t)z];
  }

  if (d2)
    for (int64_t v = 0; v < n; ++v) d2[v] = cls[(size_t)v] ? -g[(size_t)v] : g[(size_t)v];
  if (sdf_out) {
    const std::vector<float> phi = df::phi_table(R, option->resolution);
    if (sdf_out != sdf) std::memcpy(sdf_out, sdf, sizeof(float) * (size_t)n);
    for (int64_t v = 0; v < n; ++v) {
      if (update_num[v] < 1) continue;
      const float p = phi[(size_t)std::min(g[(size_t)v], R * R)];
      sdf_out[v] = cls[(size_t)v] ? -p : p;
    }
  }
  return VCY_OK;
}
