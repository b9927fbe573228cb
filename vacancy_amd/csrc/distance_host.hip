// The distance field of the hull on the host (vcy_distance_field_host): the definition of the section "distance field of
// the hull" of vacancy_hip.h run serially -- the row distances by two sweeps, then the y pass and the z pass as they are
// written there -- in the two halves a z-slab runs them in: the planes (x and y pass over a range of slices, packed as the
// device packs them: class in bit 15, the capped squared 2-D distance below it) and the finish (the z pass over the
// slab's planes with up to R planes of its neighbours at either end).  vcy_distance_field_host is the two over the whole
// grid with nothing at either end; vcy_distance_slab_planes_host / vcy_distance_slab_finish_host are the halves.
// Host code only -- no GPU, no context, nothing of the HIP runtime --, so a stand-alone program can build it under host
// sanitizers (tests/distance_host_check.cpp, tests/slab_distance_host_check.cpp; `make distance_host_check`,
// `make slab_distance_host_check`).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "distance_field.h"
#include "host_shared.h"
#include "slab_rules.h"

using namespace vcy;

namespace {

// out[i] = min over |d| <= R, i + d in [0, n), of (cls[i+d] != cls[i] ? 0 : in[i+d]) + d*d, along one line of n
// elements `stride` apart, for i in [i0, i1).  Candidates only grow with |d|: the walk ends as soon as d*d cannot win.
void line_pass(const int32_t* in, const uint8_t* cls, int64_t stride, int n, int R, int i0, int i1, int32_t* out) {
  for (int i = i0; i < i1; ++i) {
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
    out[i - i0] = best;
  }
}

// The x pass and the y pass over `nzl` slices of nx * ny voxels: h[v] = class << 15 | the y pass's value (<= FAR).
void planes_of(int nx, int ny, int nzl, const float* sdf, const int32_t* update_num, double iso_level, int R, uint16_t* h) {
  const int far = df::far_of(R);
  const int64_t slice = (int64_t)nx * ny, n = slice * nzl;
  std::vector<uint8_t> cls((size_t)n);
  for (int64_t v = 0; v < n; ++v) cls[(size_t)v] = update_num[v] >= 1 && (double)sdf[v] < iso_level ? 1 : 0;
  // x pass: the nearest voxel of the other class to the left, then to the right
  std::vector<int32_t> g((size_t)n);
  for (int64_t row = 0; row < (int64_t)ny * nzl; ++row) {
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
  // y pass; lines along y are `nx` apart
  std::vector<int32_t> line((size_t)ny);
  for (int z = 0; z < nzl; ++z)
    for (int x = 0; x < nx; ++x) {
      const int64_t at = (int64_t)z * slice + x;
      line_pass(g.data() + at, cls.data() + at, nx, ny, R, 0, ny, line.data());
      for (int y = 0; y < ny; ++y) {
        const int64_t v = at + (int64_t)y * nx;
        h[v] = (uint16_t)((cls[(size_t)v] << 15) | line[(size_t)y]);
      }
    }
}

// The z pass over the columns of [below | h | above] (n_below, nzl, n_above planes of `slice` values), results for the nzl
// planes in the middle: the signed field into d2 and / or sdf = +-phi where update_num >= 1 into sdf_out (either may be
// null; sdf_out may be sdf itself).
void finish_of(int64_t slice, int nzl, const uint16_t* h, const uint16_t* below, int n_below, const uint16_t* above,
               int n_above, int R, float resolution, const int32_t* update_num, const float* sdf, int32_t* d2, float* sdf_out) {
  const int far = df::far_of(R), n_ext = n_below + nzl + n_above;
  const int64_t n = slice * nzl;
  std::vector<float> phi;
  if (sdf_out) {
    phi = df::phi_table(R, resolution);
    if (sdf_out != sdf) std::memcpy(sdf_out, sdf, sizeof(float) * (size_t)n);
  }
  std::vector<int32_t> val((size_t)n_ext), line((size_t)nzl);
  std::vector<uint8_t> cls((size_t)n_ext);
  for (int64_t at = 0; at < slice; ++at) {
    for (int a = 0; a < n_ext; ++a) {
      const uint16_t u = a < n_below ? below[(int64_t)a * slice + at]
                       : a < n_below + nzl ? h[(int64_t)(a - n_below) * slice + at]
                                           : above[(int64_t)(a - n_below - nzl) * slice + at];
      val[(size_t)a] = u & 0x7fff;
      cls[(size_t)a] = (uint8_t)(u >> 15);
    }
    line_pass(val.data(), cls.data(), 1, n_ext, R, n_below, n_below + nzl, line.data());
    for (int z = 0; z < nzl; ++z) {
      const int64_t v = at + (int64_t)z * slice;
      const int32_t k = line[(size_t)z] > R * R ? far : line[(size_t)z];
      const bool solid = cls[(size_t)(n_below + z)] != 0;
      if (d2) d2[v] = solid ? -k : k;
      if (sdf_out && update_num[v] >= 1) {
        const float p = phi[(size_t)std::min(k, R * R)];
        sdf_out[v] = solid ? -p : p;
      }
    }
  }
}

int slab_dims(const char* who, const vcy_carver_option* option, int z_begin, int z_end, int32_t* dims) {
  { const int rc = dims_from_option(option->bb_min, option->bb_max, option->resolution, dims); if (rc != VCY_OK) return rc; }
  if (z_begin < 0 || z_end > dims[2] || z_begin >= z_end) {
    set_error("%s: slices [%d, %d) are no slab of a grid of %d slices", who, z_begin, z_end, dims[2]);
    return VCY_ERR_INVALID_ARG;
  }
  return VCY_OK;
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
  const int64_t slice = (int64_t)dims[0] * dims[1];
  std::vector<uint16_t> h((size_t)(slice * dims[2]));
  planes_of(dims[0], dims[1], dims[2], sdf, update_num, iso_level, radius, h.data());
  finish_of(slice, dims[2], h.data(), nullptr, 0, nullptr, 0, radius, option->resolution, update_num, sdf, d2, sdf_out);
  return VCY_OK;
}

extern "C" int vcy_distance_slab_planes_host(const vcy_carver_option* option, int z_begin, int z_end, const float* sdf_slab,
                                             const int32_t* update_num_slab, double iso_level, int radius, uint16_t* h) {
  const char* who = "vcy_distance_slab_planes_host";
  if (!option || !sdf_slab || !update_num_slab || !h) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  { const int rc = df::check_radius(who, radius); if (rc != VCY_OK) return rc; }
  int32_t dims[3];
  { const int rc = slab_dims(who, option, z_begin, z_end, dims); if (rc != VCY_OK) return rc; }
  planes_of(dims[0], dims[1], z_end - z_begin, sdf_slab, update_num_slab, iso_level, radius, h);
  return VCY_OK;
}

extern "C" int vcy_distance_slab_finish_host(const vcy_carver_option* option, int z_begin, int z_end, const uint16_t* h,
                                             const uint16_t* below, int n_below, const uint16_t* above, int n_above, int radius,
                                             const int32_t* update_num_slab, const float* sdf_slab, int32_t* d2,
                                             float* sdf_out) {
  const char* who = "vcy_distance_slab_finish_host";
  if (!option || !h || (sdf_out && (!sdf_slab || !update_num_slab))) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  { const int rc = df::check_radius(who, radius); if (rc != VCY_OK) return rc; }
  int32_t dims[3];
  { const int rc = slab_dims(who, option, z_begin, z_end, dims); if (rc != VCY_OK) return rc; }
  { const int rc = df::check_halo(who, radius, z_begin, z_end, dims[2], n_below, n_above, below, above); if (rc != VCY_OK) return rc; }
  finish_of((int64_t)dims[0] * dims[1], z_end - z_begin, h, below, n_below, above, n_above, radius, option->resolution,
            update_num_slab, sdf_slab, d2, sdf_out);
  return VCY_OK;
}

/* ---- the host rules of the slabs' front ends (slab_rules.h) ----------------------------------------------------------- */

extern "C" int vcy_close_hull_plan(double radius_voxels, float resolution, double* r, int* big_r) {
  if (!r || !big_r) {
    set_error("vcy_close_hull_plan: null pointer");
    return VCY_ERR_INVALID_ARG;
  }
  long long square = 0;
  switch (slab::close_hull_plan(radius_voxels, resolution, r, big_r, &square)) {
    case slab::kCloseOk: return VCY_OK;
    case slab::kCloseOutOfRange:
      set_error("CloseHull: radius_voxels = %g must be positive and at most 125", radius_voxels);
      break;
    case slab::kCloseTies:
      set_error("CloseHull: radius_voxels = %g ties: (radius + 0.5)^2 = %lld is a squared voxel distance, and the growing "
                "and the shrinking step would treat it alike; pick e.g. %g",
                radius_voxels, square, radius_voxels - 0.2);
      break;
  }
  return VCY_ERR_INVALID_ARG;
}

extern "C" int vcy_distance_halo_host(int n_slabs, const int32_t* z_bounds, int radius, int64_t plane_voxels,
                                      const uint16_t* const* bottoms, const uint16_t* const* tops, int slab, uint16_t* below,
                                      uint16_t* above, int* n_below, int* n_above) {
  const char* who = "vcy_distance_halo_host";
  { const int rc = df::check_radius(who, radius); if (rc != VCY_OK) return rc; }
  switch (plane_voxels < 1 ? slab::kHaloBadArgument
                           : slab::distance_halo(n_slabs, z_bounds, radius, (size_t)plane_voxels, bottoms, tops, slab, below,
                                                 above, n_below, n_above)) {
    case slab::kHaloOk: return VCY_OK;
    case slab::kHaloBadArgument: set_error("%s: invalid argument", who); break;
    case slab::kHaloBadBounds: set_error("%s: the z bounds of the %d slabs do not ascend from 0", who, n_slabs); break;
    case slab::kHaloBadSlab: set_error("%s: slab %d of %d", who, slab, n_slabs); break;
    case slab::kHaloMissingEdge:
      set_error("%s: slab %d needs the edge planes of a neighbour whose pointer is null", who, slab);
      break;
  }
  return VCY_ERR_INVALID_ARG;
}
