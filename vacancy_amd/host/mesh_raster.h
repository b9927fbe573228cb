// VoxelCarver::RenderMesh / MeshAgreement / ShadeMesh / MeshPhotoError and the same four of ShardedVoxelCarver differ in whose
// context names the device: the carver's own or the first slab's.  What they do with the Mesh, the cameras and the images is the same and lives here.
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

// vcy_shade_mesh of `mesh` into one camera: image gets the camera's width x height, the rounded attribute (vertex colours,
// or with from_normals 127.5 * n + 127.5 of the vertex normals) of the face seen, black where none is.  false + LOGE on an
// error, a mesh without the chosen attribute among them.
inline bool ShadeMeshWith(vcy_ctx* ctx, const char* who, const Mesh& mesh, const Camera& camera, Image3b* image, bool from_normals) {
  static_assert(sizeof(Eigen::Vector3f) == 3 * sizeof(float) && sizeof(Eigen::Vector3i) == 3 * sizeof(int32_t), "packed vector layout");
  const int w = camera.width(), h = camera.height();
  bool known = true;
  const vcy_view v = ToView(camera, w, h, &known);
  if (!known) return false;  // (ToView has logged the camera type)
  if (!image || w <= 0 || h <= 0) {
    LOGE("%s needs an image to fill and a camera with a size (%d x %d)\n", who, w, h);
    return false;
  }
  const std::vector<Eigen::Vector3f>& chosen = from_normals ? mesh.normals() : mesh.vertex_colors();
  if (chosen.empty() || chosen.size() != mesh.vertices().size()) {
    LOGE("%s needs one %s per vertex (%zu for %zu vertices)\n", who, from_normals ? "normal" : "colour", chosen.size(),
         mesh.vertices().size());
    return false;
  }
  std::vector<float> mapped;
  const float* attributes = reinterpret_cast<const float*>(chosen.data());
  if (from_normals) {
    mapped.resize(3 * chosen.size());
    for (size_t i = 0; i < mapped.size(); ++i) mapped[i] = 127.5f * attributes[i] + 127.5f;
    attributes = mapped.data();
  }
  image->Init(w, h);
  uint8_t* px = image->data_ptr()->data();
  const vcy_shade_option option = {3, {0.0f, 0.0f, 0.0f, 0.0f}};
  const int rc = vcy_shade_mesh(ctx, static_cast<int64_t>(mesh.vertices().size()), static_cast<int64_t>(mesh.vertex_indices().size()),
                                reinterpret_cast<const float*>(mesh.vertices().data()),
                                reinterpret_cast<const int32_t*>(mesh.vertex_indices().data()), attributes, 1, &v, &option, nullptr,
                                &px, nullptr);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  return true;
}

// vcy_mesh_photo_error: per view {n, sad r g b, ssd r g b} of the mesh rendered with its vertex colours against the
// photographs, under the silhouettes when there are any (an empty vector: none).  false + LOGE on an error.
inline bool MeshPhotoErrorWith(vcy_ctx* ctx, const char* who, const Mesh& mesh, const std::vector<const Camera*>& cameras,
                               const std::vector<Image3b>& photos, const std::vector<Image1b>& silhouettes,
                               std::vector<std::array<std::int64_t, 7>>* sums) {
  if (!sums || cameras.size() != photos.size() || cameras.empty() || (!silhouettes.empty() && silhouettes.size() != cameras.size())) {
    LOGE("%s needs one photograph per camera, at least one, silhouettes for all or none, and a place for the sums (%zu cameras, "
         "%zu photographs, %zu silhouettes)\n", who, cameras.size(), photos.size(), silhouettes.size());
    return false;
  }
  if (mesh.vertex_colors().empty() || mesh.vertex_colors().size() != mesh.vertices().size()) {
    LOGE("%s needs one colour per vertex (%zu for %zu vertices)\n", who, mesh.vertex_colors().size(), mesh.vertices().size());
    return false;
  }
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(n);
  std::vector<const uint8_t*> pp(n), mp(n);
  for (int i = 0; i < n; ++i) {
    const Image3b& p = photos[i];
    bool known = true;
    if (!cameras[i] || p.empty()) {
      LOGE("%s: view %d has no camera or an empty photograph\n", who, i);
      return false;
    }
    views[i] = ToView(*cameras[i], p.width(), p.height(), &known);
    if (!known) return false;  // (ToView has logged the camera type)
    pp[i] = p.data().data();
    if (!silhouettes.empty()) {
      const Image1b& s = silhouettes[i];
      if (s.width() != p.width() || s.height() != p.height()) {
        LOGE("%s: the silhouette of view %d is %d x %d, its photograph %d x %d\n", who, i, s.width(), s.height(), p.width(), p.height());
        return false;
      }
      mp[i] = s.data().data();
    }
  }
  sums->assign(static_cast<size_t>(n), std::array<std::int64_t, 7>{{0, 0, 0, 0, 0, 0, 0}});
  static_assert(sizeof(std::array<std::int64_t, 7>) == 7 * sizeof(std::int64_t), "packed array layout");
  const int rc = vcy_mesh_photo_error(ctx, static_cast<int64_t>(mesh.vertices().size()), static_cast<int64_t>(mesh.vertex_indices().size()),
                                      reinterpret_cast<const float*>(mesh.vertices().data()),
                                      reinterpret_cast<const int32_t*>(mesh.vertex_indices().data()),
                                      reinterpret_cast<const float*>(mesh.vertex_colors().data()), n, views.data(), pp.data(),
                                      silhouettes.empty() ? nullptr : mp.data(), (*sums)[0].data());
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  return true;
}

}  // namespace detail
}  // namespace vacancy
