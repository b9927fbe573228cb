// The host half of the ray-cast over z-slabs: the merge of the slabs' images and the comparison of their hit bits with a
// silhouette (vcy_render_merge_host / vcy_hull_agreement_host; the definitions are in vacancy_hip.h).  Host code only --
// no GPU, no context, nothing of the HIP runtime --, so the C++ facade, the Python classes and the per-rank driver share
// one statement of the rule.
//
// The rule.  Along a ray the z cell is monotone, so the ray visits the slabs in the order of its direction of travel
// along z, and the whole-grid hit is the hit of the first slab in that order that has one.  Depth is NOT the key: an x
// crossing and a z crossing at the same t are two consecutive states of the path, sorted by axis, and they can lie in two
// slabs.  s_z is formed per pixel as the kernel forms it (render.hip, init_axis), in float, without contraction.
#include <cmath>
#include <cstdint>

#include "vacancy_hip.h"

namespace vcy {
void set_error(const char* fmt, ...);

int check_render_view(const vcy_view* v, int i) {
  if (v->width <= 0 || v->height <= 0) {
    set_error("view %d: invalid image size %d x %d", i, v->width, v->height);
    return VCY_ERR_INVALID_ARG;
  }
  if (v->roi_min[0] < 0 || v->roi_min[1] < 0 || v->roi_max[0] >= v->width || v->roi_max[1] >= v->height ||
      v->roi_min[0] > v->roi_max[0] || v->roi_min[1] > v->roi_max[1]) {
    set_error("view %d: ROI [%d,%d]-[%d,%d] outside the %dx%d image", i, v->roi_min[0], v->roi_min[1], v->roi_max[0],
              v->roi_max[1], v->width, v->height);
    return VCY_ERR_INVALID_ARG;
  }
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(v->w2c[k])) {
      set_error("view %d: w2c is not finite", i);
      return VCY_ERR_INVALID_ARG;
    }
  if (!v->is_ortho && (v->fx == 0.0f || v->fy == 0.0f)) {
    set_error("view %d: a pinhole view needs fx and fy other than 0", i);
    return VCY_ERR_INVALID_ARG;
  }
  return VCY_OK;
}
}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_render_merge_host(const vcy_view* view, int n_slabs, const float* const* depth, const int64_t* const* voxel,
                          const uint8_t* const* axis, float* depth_out, int64_t* voxel_out, uint8_t* axis_out) {
  if (!view || n_slabs <= 0 || !voxel || (depth && !depth_out) || (axis && !axis_out)) {
    set_error("vcy_render_merge_host: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  for (int s = 0; s < n_slabs; ++s)
    if (!voxel[s] || (depth && !depth[s]) || (axis && !axis[s])) {
      set_error("vcy_render_merge_host: slab %d: null image", s);
      return VCY_ERR_INVALID_ARG;
    }
  { const int rc = check_render_view(view, 0); if (rc != VCY_OK) return rc; }
  const int w = view->width, h = view->height;
  const float r0 = view->w2c[2], r1 = view->w2c[6], r2 = view->w2c[10];  // R[0][2], R[1][2], R[2][2]
  for (int v = 0; v < h; ++v) {
    const float dc1 = view->is_ortho ? 0.0f : ((float)v - view->cy) / view->fy;
    for (int u = 0; u < w; ++u) {
      const float dc0 = view->is_ortho ? 0.0f : ((float)u - view->cx) / view->fx;
      const float d = r0 * dc0 + r1 * dc1 + r2 * 1.0f;
      const bool moves = d != 0.0f && std::isfinite(1.0f / d);
      const bool down = moves && !(d > 0.0f);  // s_z < 0: the highest slab comes first
      const int64_t px = (int64_t)v * w + u;
      int from = -1;
      for (int k = 0; k < n_slabs && from < 0; ++k) {
        const int s = down ? n_slabs - 1 - k : k;  // (s_z == 0: at most one slab has a hit)
        if (voxel[s][px] >= 0) from = s;
      }
      if (depth) depth_out[px] = from < 0 ? INFINITY : depth[from][px];
      if (voxel_out) voxel_out[px] = from < 0 ? -1 : voxel[from][px];
      if (axis) axis_out[px] = from < 0 ? (uint8_t)255 : axis[from][px];
    }
  }
  return VCY_OK;
}

int vcy_hull_agreement_host(const vcy_view* view, int n_slabs, const uint64_t* const* hits, const uint8_t* mask,
                            int64_t counts[3]) {
  if (!view || n_slabs <= 0 || !hits || !mask || !counts) {
    set_error("vcy_hull_agreement_host: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  for (int s = 0; s < n_slabs; ++s)
    if (!hits[s]) {
      set_error("vcy_hull_agreement_host: slab %d: null hit bits", s);
      return VCY_ERR_INVALID_ARG;
    }
  { const int rc = check_render_view(view, 0); if (rc != VCY_OK) return rc; }
  const int w = view->width;
  const int64_t words = ((int64_t)w + 63) / 64;
  int64_t both = 0, only_mask = 0, only_hull = 0;
  for (int v = view->roi_min[1]; v <= view->roi_max[1]; ++v)
    for (int u = view->roi_min[0]; u <= view->roi_max[0]; ++u) {
      const int64_t at = (int64_t)v * words + (u >> 6);
      uint64_t word = 0;
      for (int s = 0; s < n_slabs; ++s) word |= hits[s][at];
      const bool hull = (word >> (u & 63)) & 1ull, m = mask[(int64_t)v * w + u] != 0;
      both += m && hull, only_mask += m && !hull, only_hull += !m && hull;
    }
  counts[0] = both, counts[1] = only_mask, counts[2] = only_hull;
  return VCY_OK;
}

}  // extern "C"
