// Mesh::Decimate, VoxelCarver::DecimateMesh and ShardedVoxelCarver::DecimateMesh differ in who runs the clustering: the host
// function or a context's device.  What they do to the Mesh is the same and lives here.
#pragma once

#include <cstdint>
#include <vector>

#include "vacancy/log.h"
#include "vacancy/mesh.h"
#include "vacancy_hip.h"

namespace vacancy {
namespace detail {

// run(n_vertices, n_faces, vertices, faces, &option, vertices_out, faces_out, &n_vertices_out, &n_faces_out, vertex_map,
// face_source, vertex_normals_out, face_normals_out) -> vcy status.  Replaces vertices() and vertex_indices() by the
// decimated mesh.  with_normals: normals(), face_normals() and normal_indices() become Mesh::CalcNormal() of the result;
// otherwise those of them that were filled are recomputed, so that they never describe the mesh before the call.
// vertex_colors() are not carried (they are cleared: colour the result again).  false + LOGE on an error, the mesh then
// stays as it was.
template <class Run>
bool DecimateMeshWith(Mesh* mesh, float cell, const Eigen::Vector3f& origin, int mode, bool with_normals, Run run) {
  static_assert(sizeof(Eigen::Vector3f) == 3 * sizeof(float) && sizeof(Eigen::Vector3i) == 3 * sizeof(int32_t), "packed vector layout");
  const size_t nv = mesh->vertices().size(), nf = mesh->vertex_indices().size();
  const bool want_vn = with_normals || (nv > 0 && mesh->normals().size() == nv);
  const bool want_fn = with_normals || (nf > 0 && mesh->face_normals().size() == nf);
  std::vector<Eigen::Vector3f> v(nv), vn(want_vn ? nv : 0), fn(want_fn ? nf : 0);
  std::vector<Eigen::Vector3i> f(nf);
  vcy_decimate_option o;
  o.cell = cell;
  o.origin[0] = origin.x(), o.origin[1] = origin.y(), o.origin[2] = origin.z();
  o.mode = mode;
  int64_t nvo = 0, nfo = 0;
  const int rc = run(static_cast<int64_t>(nv), static_cast<int64_t>(nf), reinterpret_cast<const float*>(mesh->vertices().data()),
                     reinterpret_cast<const int32_t*>(mesh->vertex_indices().data()), &o, reinterpret_cast<float*>(v.data()),
                     reinterpret_cast<int32_t*>(f.data()), &nvo, &nfo, static_cast<int32_t*>(nullptr), static_cast<int32_t*>(nullptr),
                     want_vn && nv > 0 ? reinterpret_cast<float*>(vn.data()) : nullptr,
                     want_fn && nf > 0 ? reinterpret_cast<float*>(fn.data()) : nullptr);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  v.resize(static_cast<size_t>(nvo));
  f.resize(static_cast<size_t>(nfo));
  if (want_vn) vn.resize(static_cast<size_t>(nvo));
  if (want_fn) fn.resize(static_cast<size_t>(nfo));
  const bool had_normal_indices = !mesh->normal_indices().empty();
  mesh->mutable_vertices()->swap(v);
  mesh->mutable_vertex_indices()->swap(f);
  mesh->set_vertex_colors(std::vector<Eigen::Vector3f>());
  mesh->mutable_normals()->swap(vn);          // (empty when they were neither asked for nor there)
  mesh->mutable_face_normals()->swap(fn);
  if (with_normals || had_normal_indices) mesh->set_normal_indices(mesh->vertex_indices());
  return true;
}

}  // namespace detail
}  // namespace vacancy
