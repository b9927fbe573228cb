// VoxelCarver::RenderMesh / MeshAgreement and the same two of ShardedVoxelCarver differ in whose context names the device:
// the carver's own or the first slab's.  What they do with the Mesh, the cameras and the images is the same and lives here.
#pragma once

#include <array>
#include <cstdint>
#include <limits>
#include <vector>

#include "c_abi_structs.h"
#include "vacancy/camera.h"
#include "vacancy/image.h"
#include "vacancy/log.h"
#include "vacancy/mesh.h"
#include "vacancy_hip.h"

namespace vacancy {
namespace detail {

// vcy_raster_mesh of `mesh` into one camera: depth gets the camera's width x height, silhouette (optional) 255 where a
// face is seen.  false + LOGE on an error.
inline bool RenderMeshWith(vcy_ctx* ctx, const char* who, const Mesh& mesh, const Camera& camera, Image1f* depth,
                           Image1b* silhouette) {
  static_assert(sizeof(Eigen::Vector3f) == 3 * sizeof(float) && sizeof(Eigen::Vector3i) == 3 * sizeof(int32_t), "packed vector layout");
  const int w = camera.width(), h = camera.height();
  bool known = true;
  const vcy_view v = ToView(camera, w, h, &known);
  if (!known) return false;  // (ToView has logged the camera type)
  if (!depth || w <= 0 || h <= 0) {
    LOGE("%s needs a depth image to fill and a camera with a size (%d x %d)\n", who, w, h);
    return false;
  }
  depth->Init(w, h);
  float* dp = depth->data_ptr()->data();
  const int rc = vcy_raster_mesh(ctx, static_cast<int64_t>(mesh.vertices().size()), static_cast<int64_t>(mesh.vertex_indices().size()),
                                 reinterpret_cast<const float*>(mesh.vertices().data()),
                                 reinterpret_cast<const int32_t*>(mesh.vertex_indices().data()), 1, &v, &dp, nullptr, nullptr,
                                 nullptr);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  if (silhouette) {
    silhouette->Init(w, h);
    std::vector<unsigned char>& s = *silhouette->data_ptr();
    for (size_t i = 0; i < s.size(); ++i) s[i] = dp[i] < std::numeric_limits<float>::infinity() ? 255 : 0;
  }
  return true;
}

// vcy_mesh_agreement: per view {mask && mesh, mask && !mesh, !mask && mesh}.  false + LOGE on an error.
inline bool MeshAgreementWith(vcy_ctx* ctx, const char* who, const Mesh& mesh, const std::vector<const Camera*>& cameras,
                              const std::vector<Image1b>& silhouettes, std::vector<std::array<std::int64_t, 3>>* counts) {
  if (!counts || cameras.size() != silhouettes.size() || cameras.empty()) {
    LOGE("%s needs one silhouette per camera, at least one, and a place for the counts (%zu cameras, %zu silhouettes)\n", who,
         cameras.size(), silhouettes.size());
    return false;
  }
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(n);
  std::vector<const uint8_t*> masks(n);
  for (int i = 0; i < n; ++i) {
    const Image1b& s = silhouettes[i];
    bool known = true;
    if (!cameras[i] || s.empty()) {
      LOGE("%s: view %d has no camera or an empty silhouette\n", who, i);
      return false;
    }
    views[i] = ToView(*cameras[i], s.width(), s.height(), &known);
    if (!known) return false;  // (ToView has logged the camera type)
    masks[i] = s.data().data();
  }
  counts->assign(static_cast<size_t>(n), std::array<std::int64_t, 3>{{0, 0, 0}});
  static_assert(sizeof(std::array<std::int64_t, 3>) == 3 * sizeof(std::int64_t), "packed array layout");
  const int rc = vcy_mesh_agreement(ctx, static_cast<int64_t>(mesh.vertices().size()), static_cast<int64_t>(mesh.vertex_indices().size()),
                                    reinterpret_cast<const float*>(mesh.vertices().data()),
                                    reinterpret_cast<const int32_t*>(mesh.vertex_indices().data()), n, views.data(), masks.data(),
                                    (*counts)[0].data());
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  return true;
}

}  // namespace detail
}  // namespace vacancy
