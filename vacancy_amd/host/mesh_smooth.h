// Mesh::Smooth, VoxelCarver::SmoothMesh and ShardedVoxelCarver::SmoothMesh differ in who runs the passes: the host function
// or a context's device.  What they do to the Mesh is the same and lives here.
#pragma once

#include <cstdint>
#include <vector>

#include "vacancy/log.h"
#include "vacancy/mesh.h"
#include "vacancy_hip.h"

namespace vacancy {
namespace detail {

// run(n_vertices, n_faces, vertices, faces, &option, vertices_out, vertex_normals_out, face_normals_out) -> vcy status.
// Smooths mesh->vertices() in place.  with_normals: normals(), face_normals() and normal_indices() become
// Mesh::CalcNormal() of the result; otherwise those of them that were filled are refreshed, so that they never describe
// the positions before the call.  false + LOGE on an error, the mesh then stays as it was.
template <class Run>
bool SmoothMeshWith(Mesh* mesh, int iterations, float lambda, float mu, bool pin_boundary, bool with_normals, Run run) {
  static_assert(sizeof(Eigen::Vector3f) == 3 * sizeof(float) && sizeof(Eigen::Vector3i) == 3 * sizeof(int32_t), "packed vector layout");
  const size_t nv = mesh->vertices().size(), nf = mesh->vertex_indices().size();
  const bool had_vertex_normals = nv > 0 && mesh->normals().size() == nv;
  const bool had_face_normals = nf > 0 && mesh->face_normals().size() == nf;
  const bool want_vn = with_normals || had_vertex_normals, want_fn = with_normals || had_face_normals;
  std::vector<Eigen::Vector3f> vn(want_vn ? nv : 0), fn(want_fn ? nf : 0);
  vcy_smooth_option o;
  o.iterations = iterations;
  o.lambda = lambda;
  o.mu = mu;
  o.pin_boundary = pin_boundary ? 1 : 0;
  float* v = reinterpret_cast<float*>(mesh->mutable_vertices()->data());
  const int rc = run(static_cast<int64_t>(nv), static_cast<int64_t>(nf), v,
                     reinterpret_cast<const int32_t*>(mesh->vertex_indices().data()), &o, v,
                     want_vn && nv > 0 ? reinterpret_cast<float*>(vn.data()) : nullptr,
                     want_fn && nf > 0 ? reinterpret_cast<float*>(fn.data()) : nullptr);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  if (want_vn) mesh->mutable_normals()->swap(vn);
  if (want_fn) mesh->mutable_face_normals()->swap(fn);
  if (with_normals || !mesh->normal_indices().empty()) mesh->set_normal_indices(mesh->vertex_indices());
  return true;
}

}  // namespace detail
}  // namespace vacancy
