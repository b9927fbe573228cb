// Triangle mesh container filled by VoxelCarver::ExtractIsoSurface.  Subset of the reference's
// include/vacancy/mesh.h that the carving path uses: Clear, set_vertices, set_vertex_indices,
// accessors and the ASCII PLY writer (byte-compatible with reference mesh.cc:583-631).
#pragma once

#include <string>
#include <vector>

#include "vacancy/common.h"

namespace vacancy {

class Mesh {
 public:
  void Clear() {
    vertices_.clear(); vertex_colors_.clear(); vertex_indices_.clear();
    normals_.clear(); face_normals_.clear(); normal_indices_.clear();
  }
  // Reference mesh.cc:197-240, serial on the host (vcy_mesh_normals_host): face normal = ((p1 - p0).normalized() x
  // (p2 - p0).normalized()).normalized(); vertex normal = its faces' normals summed in ascending face index, divided by
  // their number, normalised; normal_indices = vertex_indices.  VoxelCarver::ExtractIsoSurface(..., with_normals = true)
  // fills the same three vectors from the device, bit for bit.
  void CalcNormal();
  void CalcFaceNormal();
  // `iterations` Taubin iterations over the vertices, serial on the host (vcy_smooth_mesh_host; the rule is in
  // vacancy_hip.h, "mesh smoothing"): a pass with factor lambda, then one with mu (0: plain Laplacian smoothing);
  // pin_boundary keeps the vertices of an edge that one face uses.  normals(), face_normals() and normal_indices() are
  // recomputed if they were filled.  VoxelCarver::SmoothMesh runs the same on the device, bit for bit.  false + LOGE on
  // an error (a face index out of range, a non-finite factor ...), the mesh then stays as it was.
  bool Smooth(int iterations, float lambda = 0.5f, float mu = -0.53f, bool pin_boundary = false);
  // Vertex-clustering decimation, serial on the host (vcy_decimate_mesh_host; the rule is in vacancy_hip.h, "mesh
  // decimation"): the vertices of one cube of edge `cell` of a lattice with a corner at the origin become one vertex --
  // mode 0 their mean, 1 the member nearest to the mean, 2 the first member --, faces that collapse or repeat go, vertices
  // no face names go.  normals(), face_normals() and normal_indices() are recomputed if they were filled; vertex_colors()
  // are cleared.  VoxelCarver::DecimateMesh runs the same on the device, bit for bit, with the lattice at the carver's
  // bb_min.  false + LOGE on an error (a face index out of range, cell <= 0, a non-finite vertex ...), the mesh then stays
  // as it was.
  bool Decimate(float cell, int mode = 0);
  // The same clusters, faces and maps as Decimate(cell, 0), every cluster at its quadric-error representative instead of
  // its mean (vcy_decimate_mesh_quadric_host; vacancy_hip.h, "mesh decimation, quadric representatives"): edges and corners
  // keep their place.  regularize in [0, 1] pulls towards the mean; a cluster whose optimum is undefined or leaves its cell
  // keeps the mean.  VoxelCarver::DecimateMeshQuadric runs the same on the device, bit for bit.
  bool DecimateQuadric(float cell, float regularize = 1e-3f);
  const std::vector<Eigen::Vector3f>& normals() const { return normals_; }
  const std::vector<Eigen::Vector3f>& face_normals() const { return face_normals_; }
  const std::vector<Eigen::Vector3i>& normal_indices() const { return normal_indices_; }
  bool set_normals(const std::vector<Eigen::Vector3f>& n) { normals_ = n; return true; }
  bool set_face_normals(const std::vector<Eigen::Vector3f>& n) { face_normals_ = n; return true; }
  bool set_normal_indices(const std::vector<Eigen::Vector3i>& f) { normal_indices_ = f; return true; }
  std::vector<Eigen::Vector3f>* mutable_normals() { return &normals_; }
  std::vector<Eigen::Vector3f>* mutable_face_normals() { return &face_normals_; }
  const std::vector<Eigen::Vector3f>& vertices() const { return vertices_; }
  const std::vector<Eigen::Vector3f>& vertex_colors() const { return vertex_colors_; }
  const std::vector<Eigen::Vector3i>& vertex_indices() const { return vertex_indices_; }
  bool set_vertices(const std::vector<Eigen::Vector3f>& v) { vertices_ = v; return true; }
  bool set_vertex_colors(const std::vector<Eigen::Vector3f>& c) { vertex_colors_ = c; return true; }
  bool set_vertex_indices(const std::vector<Eigen::Vector3i>& f) { vertex_indices_ = f; return true; }
  // raw adopt (avoids a second copy of multi-million vertex meshes)
  std::vector<Eigen::Vector3f>* mutable_vertices() { return &vertices_; }
  std::vector<Eigen::Vector3i>* mutable_vertex_indices() { return &vertex_indices_; }
  bool WritePly(const std::string& ply_path) const;        // ASCII, reference format
  // binary_little_endian, for large meshes; with nx ny nz after z when normals().size() == vertices().size()
  bool WritePlyBinary(const std::string& ply_path) const;

 private:
  std::vector<Eigen::Vector3f> vertices_;
  std::vector<Eigen::Vector3f> vertex_colors_;
  std::vector<Eigen::Vector3i> vertex_indices_;
  std::vector<Eigen::Vector3f> normals_;
  std::vector<Eigen::Vector3f> face_normals_;
  std::vector<Eigen::Vector3i> normal_indices_;
};

}  // namespace vacancy
