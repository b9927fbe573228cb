// The host half of the meshes of z-slabs: Mesh::CalcNormal on raw arrays, the seam finish of the slabs' normals, and the
// stitch of the slabs' meshes by edge key (vcy_mesh_normals_host*, vcy_mesh_normals_seam_sum, vcy_merge_meshes_host; the
// definitions are in vacancy_hip.h).  Host code only -- no GPU, no context, nothing of the HIP runtime --, so the C++
// facade, the Python classes and the per-rank driver share one statement of each rule.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "vacancy_hip.h"

namespace vcy {
void set_error(const char* fmt, ...);
}  // namespace vcy

using namespace vcy;

extern "C" {

namespace {
// Eigen::Vector3f::normalize() as include/vacancy/linalg.h evaluates it
inline void host_normalize3(float v[3]) {
  const float n2 = v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]);
  if (n2 > 0.0f) {
    const float n = std::sqrt(n2);
    v[0] = v[0] / n;
    v[1] = v[1] / n;
    v[2] = v[2] / n;
  }
}
// Mesh::CalcFaceNormal for one face (mesh.cc:231-240)
inline void host_face_normal(const float* vertices, const int32_t* f, float fn[3]) {
  const float *p0 = vertices + 3 * (int64_t)f[0], *p1 = vertices + 3 * (int64_t)f[1], *p2 = vertices + 3 * (int64_t)f[2];
  float v1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  float v2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  host_normalize3(v1);
  host_normalize3(v2);
  fn[0] = v1[1] * v2[2] - v1[2] * v2[1];
  fn[1] = v1[2] * v2[0] - v1[0] * v2[2];
  fn[2] = v1[0] * v2[1] - v1[1] * v2[0];
  host_normalize3(fn);
}
// Mesh::CalcNormal: one term of a vertex's sum (mesh.cc:213-221), and the division and normalisation behind it
inline void host_add_normal(float* n, int* count, const float fn[3]) {
  n[0] += fn[0];
  n[1] += fn[1];
  n[2] += fn[2];
  ++*count;
}
inline void host_finish_normal(float* n, int count) {
  const float d = static_cast<float>(count);
  n[0] = n[0] / d;
  n[1] = n[1] / d;
  n[2] = n[2] / d;
  host_normalize3(n);
}
}  // namespace

int vcy_mesh_normals_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                          float* vertex_normals, float* face_normals) {
  if (n_vertices < 0 || n_faces < 0 || (n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) {
    set_error("vcy_mesh_normals_host: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  for (int64_t i = 0; i < 3 * n_faces; ++i)
    if (faces[i] < 0 || faces[i] >= n_vertices) {
      set_error("vcy_mesh_normals_host: face %lld names vertex %d of %lld", (long long)(i / 3), faces[i], (long long)n_vertices);
      return VCY_ERR_INVALID_ARG;
    }
  std::vector<int> count;
  if (vertex_normals) {
    count.assign((size_t)n_vertices, 0);
    for (int64_t i = 0; i < 3 * n_vertices; ++i) vertex_normals[i] = 0.0f;
  }
  for (int64_t i = 0; i < n_faces; ++i) {  // Mesh::CalcFaceNormal (mesh.cc:231-240), then the sum of mesh.cc:213-221
    const int32_t* f = faces + 3 * i;
    float fn[3];
    host_face_normal(vertices, f, fn);
    if (face_normals) face_normals[3 * i + 0] = fn[0], face_normals[3 * i + 1] = fn[1], face_normals[3 * i + 2] = fn[2];
    if (vertex_normals)
      for (int j = 0; j < 3; ++j) host_add_normal(vertex_normals + 3 * (int64_t)f[j], &count[(size_t)f[j]], fn);
  }
  if (vertex_normals)
    for (int64_t k = 0; k < n_vertices; ++k)  // (a vertex no face names: 0 / 0, as in the reference)
      host_finish_normal(vertex_normals + 3 * k, count[(size_t)k]);
  return VCY_OK;
}

namespace {
// One term of a vertex's sum as mc_vertex_normals_kernel adds it.  For numbers this is host_add_normal.  Where the sum
// and the term are both NaN (a mesh over NaN voxels) an adder returns one of its operands, and which one is not part of
// the arithmetic: the kernel's add has the term as its first source and returns that one, x86 keeps the sum.  The two
// NaNs can differ in their sign bit, so the seam finish names the kernel's choice.
inline void device_add_normal(float* n, int* count, const float fn[3]) {
  for (int k = 0; k < 3; ++k) n[k] = (std::isnan(n[k]) && std::isnan(fn[k])) ? fn[k] : n[k] + fn[k];
  ++*count;
}

// The seam finish.  face_normals == nullptr: Mesh::CalcFaceNormal of the faces on the host and the host's sum;
// otherwise the given rows (the devices' own face normals) and the device's sum.
int seam_finish(const char* who, int64_t n_vertices, const float* vertices, const int32_t* faces, const float* face_normals,
                int64_t face_begin, int64_t face_end, int64_t n_seam, const int64_t* seam_vertex_ids, float* vertex_normals) {
  if (n_vertices < 0 || n_seam < 0 || face_begin < 0 || face_end < face_begin || (n_seam > 0 && !seam_vertex_ids) ||
      (n_seam > 0 && ((!vertices && !face_normals) || !vertex_normals)) || (n_seam > 0 && face_end > face_begin && !faces)) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  if (n_seam == 0) return VCY_OK;
  // the seam vertices of one plane are a small window of the merged numbering: a slot per id of that window
  int64_t lo = seam_vertex_ids[0], hi = seam_vertex_ids[0];
  for (int64_t k = 0; k < n_seam; ++k) {
    const int64_t id = seam_vertex_ids[k];
    if (id < 0 || id >= n_vertices) {
      set_error("%s: seam vertex %lld of %lld", who, (long long)id, (long long)n_vertices);
      return VCY_ERR_INVALID_ARG;
    }
    lo = std::min(lo, id);
    hi = std::max(hi, id);
  }
  std::vector<int32_t> slot((size_t)(hi - lo + 1), -1);
  for (int64_t k = 0; k < n_seam; ++k) slot[(size_t)(seam_vertex_ids[k] - lo)] = (int32_t)k;  // (a repeated id: one slot)
  for (int64_t i = 3 * face_begin; i < 3 * face_end; ++i)
    if (faces[i] < 0 || faces[i] >= n_vertices) {
      set_error("%s: face %lld names vertex %d of %lld", who, (long long)(i / 3), faces[i], (long long)n_vertices);
      return VCY_ERR_INVALID_ARG;
    }
  std::vector<float> sum(3 * (size_t)n_seam, 0.0f);
  std::vector<int> count((size_t)n_seam, 0);
  for (int64_t i = face_begin; i < face_end; ++i) {  // ascending face index: the order of the reference's sum
    const int32_t* f = faces + 3 * i;
    bool named = false;
    for (int j = 0; j < 3; ++j) named = named || (f[j] >= lo && f[j] <= hi && slot[(size_t)(f[j] - lo)] >= 0);
    if (!named) continue;
    float fn[3];
    if (face_normals)
      fn[0] = face_normals[3 * i], fn[1] = face_normals[3 * i + 1], fn[2] = face_normals[3 * i + 2];
    else
      host_face_normal(vertices, f, fn);
    for (int j = 0; j < 3; ++j) {
      if (f[j] < lo || f[j] > hi) continue;
      const int32_t k = slot[(size_t)(f[j] - lo)];
      if (k < 0) continue;
      if (face_normals)
        device_add_normal(&sum[3 * (size_t)k], &count[(size_t)k], fn);
      else
        host_add_normal(&sum[3 * (size_t)k], &count[(size_t)k], fn);
    }
  }
  for (int64_t k = 0; k < n_seam; ++k) {
    const int32_t q = slot[(size_t)(seam_vertex_ids[k] - lo)];
    float n[3] = {sum[3 * (size_t)q], sum[3 * (size_t)q + 1], sum[3 * (size_t)q + 2]};
    host_finish_normal(n, count[(size_t)q]);
    float* o = vertex_normals + 3 * seam_vertex_ids[k];
    o[0] = n[0], o[1] = n[1], o[2] = n[2];
  }
  return VCY_OK;
}
}  // namespace

int vcy_mesh_normals_host_seam(int64_t n_vertices, const float* vertices, const int32_t* faces, int64_t face_begin,
                               int64_t face_end, int64_t n_seam, const int64_t* seam_vertex_ids, float* vertex_normals) {
  if (n_seam > 0 && !vertices) {
    set_error("vcy_mesh_normals_host_seam: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  return seam_finish("vcy_mesh_normals_host_seam", n_vertices, vertices, faces, nullptr, face_begin, face_end, n_seam,
                     seam_vertex_ids, vertex_normals);
}

int vcy_mesh_normals_seam_sum(int64_t n_vertices, const int32_t* faces, const float* face_normals, int64_t face_begin,
                              int64_t face_end, int64_t n_seam, const int64_t* seam_vertex_ids, float* vertex_normals) {
  if (n_seam > 0 && face_end > face_begin && !face_normals) {
    set_error("vcy_mesh_normals_seam_sum: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  if (n_seam > 0 && face_end == face_begin) {  // (no face: the host's 0 / 0, as vcy_mesh_normals_host_seam)
    static const float none[3] = {0.0f, 0.0f, 0.0f};
    face_normals = none;
  }
  return seam_finish("vcy_mesh_normals_seam_sum", n_vertices, nullptr, faces, face_normals, face_begin, face_end, n_seam,
                     seam_vertex_ids, vertex_normals);
}

namespace {
// an own vertex of the lower slab that a foreign key of the upper slab can name, with its merged id
struct Owner {
  int64_t k0, k1, id;
  bool operator<(const Owner& o) const { return k0 != o.k0 ? k0 < o.k0 : k1 != o.k1 ? k1 < o.k1 : id < o.id; }
};
}  // namespace

int vcy_merge_meshes_host(int n_slabs, const vcy_mesh* slabs, const vcy_mesh_normals* normals, const int64_t* layer_faces,
                          float* vertices, int32_t* faces, int64_t* edge_keys, float* vertex_normals, float* face_normals) {
  static const char who[] = "vcy_merge_meshes_host";
  if (n_slabs < 0 || (n_slabs > 0 && !slabs) || (normals != nullptr) != (layer_faces != nullptr) ||
      (!normals && (vertex_normals || face_normals))) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  // ---- every check that needs no more than a look at the structs, before anything is written ----
  std::vector<int64_t> v0((size_t)n_slabs + 1, 0), f0((size_t)n_slabs + 1, 0);  // first merged vertex / face of a slab
  for (int s = 0; s < n_slabs; ++s) {
    const vcy_mesh& m = slabs[s];
    const int64_t nv = m.n_vertices, nf = m.n_faces, nfo = m.n_foreign_vertices;
    if (nv < 0 || nf < 0 || nfo < 0 || nfo > nv) {
      set_error("%s: slab %d: %lld vertices, %lld of them foreign, %lld faces", who, s, (long long)nv, (long long)nfo, (long long)nf);
      return VCY_ERR_INVALID_ARG;
    }
    if (s == 0 && nfo > 0) {
      set_error("%s: slab 0 has %lld foreign vertices and no slab below it", who, (long long)nfo);
      return VCY_ERR_INVALID_ARG;
    }
    if ((nv > 0 && !m.vertices) || (nf > 0 && !m.faces)) {
      set_error("%s: slab %d: null vertices or faces", who, s);
      return VCY_ERR_INVALID_ARG;
    }
    if (!m.edge_keys && (nfo > 0 || (edge_keys && nv > 0))) {
      set_error("%s: slab %d has no edge keys (vcy_set_param \"meshkeys\" 1)", who, s);
      return VCY_ERR_INVALID_ARG;
    }
    if (normals && ((nv > 0 && !normals[s].vertex_normals) || (nf > 0 && !normals[s].face_normals))) {
      set_error("%s: slab %d has no normals; they are given for every slab or for none", who, s);
      return VCY_ERR_INVALID_ARG;
    }
    if (normals && (layer_faces[2 * s] < 0 || layer_faces[2 * s] > nf || layer_faces[2 * s + 1] < 0 || layer_faces[2 * s + 1] > nf)) {
      set_error("%s: slab %d: layer_faces (%lld, %lld) of %lld faces", who, s, (long long)layer_faces[2 * s],
                (long long)layer_faces[2 * s + 1], (long long)nf);
      return VCY_ERR_INVALID_ARG;
    }
    v0[(size_t)s + 1] = v0[(size_t)s] + (nv - nfo);
    f0[(size_t)s + 1] = f0[(size_t)s] + nf;
    if (v0[(size_t)s + 1] > INT32_MAX) {
      set_error("%s: slab %d: the merged mesh has more than %d vertices", who, s, INT32_MAX);
      return VCY_ERR_INVALID_ARG;
    }
  }
  const int64_t total_v = v0[(size_t)n_slabs], total_f = f0[(size_t)n_slabs];
  if ((total_v > 0 && (!vertices || (normals && !vertex_normals))) || (total_f > 0 && (!faces || (normals && !face_normals)))) {
    set_error("%s: null output array for %lld vertices, %lld faces", who, (long long)total_v, (long long)total_f);
    return VCY_ERR_INVALID_ARG;
  }
  // ---- the owners: owner[s][i] = merged id of slab s's foreign vertex i, by edge key in the slab directly below.  Only
  // own vertices of that slab whose key lies within the range of the foreign keys are entered (those on its top plane,
  // or fewer): entering every vertex made the merge 35 ms for a 600 K-vertex mesh in 8 slabs, where the extraction
  // itself takes 2.  Still nothing is written.
  std::vector<std::vector<int64_t>> owner((size_t)n_slabs);
  std::vector<Owner> table;
  for (int s = 1; s < n_slabs; ++s) {
    const vcy_mesh &m = slabs[s], &below = slabs[s - 1];
    const int64_t nfo = m.n_foreign_vertices;
    if (nfo == 0) continue;
    int64_t lo = m.edge_keys[0], hi = m.edge_keys[1];
    for (int64_t i = 1; i < nfo; ++i) lo = std::min(lo, m.edge_keys[2 * i]), hi = std::max(hi, m.edge_keys[2 * i + 1]);
    table.clear();
    if (below.edge_keys)
      for (int64_t i = below.n_foreign_vertices; i < below.n_vertices; ++i) {
        const int64_t k0 = below.edge_keys[2 * i], k1 = below.edge_keys[2 * i + 1];
        if (k0 >= lo && k1 <= hi) table.push_back(Owner{k0, k1, v0[(size_t)s - 1] + (i - below.n_foreign_vertices)});
      }
    std::sort(table.begin(), table.end());
    owner[(size_t)s].resize((size_t)nfo);
    for (int64_t i = 0; i < nfo; ++i) {
      const int64_t k0 = m.edge_keys[2 * i], k1 = m.edge_keys[2 * i + 1];
      // (a key the lower slab holds twice: its last vertex, as a table filled in order would answer)
      const auto it = std::upper_bound(table.begin(), table.end(), Owner{k0, k1, INT64_MAX});
      if (it == table.begin() || (it - 1)->k0 != k0 || (it - 1)->k1 != k1) {
        set_error("%s: slab %d: foreign vertex %lld with edge key (%lld, %lld) has no owner in slab %d", who, s, (long long)i,
                  (long long)k0, (long long)k1, s - 1);
        return VCY_ERR_INVALID_ARG;
      }
      owner[(size_t)s][(size_t)i] = (it - 1)->id;
    }
  }
  // ---- the merged arrays: own vertices in order, faces re-pointed
  for (int s = 0; s < n_slabs; ++s) {
    const vcy_mesh& m = slabs[s];
    const int64_t nv = m.n_vertices, nfo = m.n_foreign_vertices, nown = nv - nfo, first = v0[(size_t)s];
    if (nown > 0) {
      std::memcpy(vertices + 3 * first, m.vertices + 3 * nfo, sizeof(float) * 3 * (size_t)nown);
      if (edge_keys) std::memcpy(edge_keys + 2 * first, m.edge_keys + 2 * nfo, sizeof(int64_t) * 2 * (size_t)nown);
      if (normals) std::memcpy(vertex_normals + 3 * first, normals[s].vertex_normals + 3 * nfo, sizeof(float) * 3 * (size_t)nown);
    }
    if (m.n_faces == 0) continue;
    if (normals) std::memcpy(face_normals + 3 * f0[(size_t)s], normals[s].face_normals, sizeof(float) * 3 * (size_t)m.n_faces);
    const int64_t* own = owner[(size_t)s].data();
    int32_t* out = faces + 3 * f0[(size_t)s];
    for (int64_t i = 0; i < 3 * m.n_faces; ++i) {
      const int64_t j = m.faces[i];
      if (j < 0 || j >= nv) {
        set_error("%s: slab %d: face %lld names vertex %lld of %lld", who, s, (long long)(i / 3), (long long)j, (long long)nv);
        return VCY_ERR_INVALID_ARG;
      }
      out[i] = (int32_t)(j < nfo ? own[j] : first + (j - nfo));
    }
  }
  // ---- the seams' normals: the vertices the foreign ones were mapped to, over the two cell layers that meet there
  for (int s = 1; normals && s < n_slabs; ++s) {
    const std::vector<int64_t>& ids = owner[(size_t)s];
    if (ids.empty()) continue;
    const int rc = vcy_mesh_normals_seam_sum(total_v, faces, face_normals, f0[(size_t)s] - layer_faces[2 * (s - 1) + 1],
                                             f0[(size_t)s] + layer_faces[2 * s], (int64_t)ids.size(), ids.data(), vertex_normals);
    if (rc != VCY_OK) return rc;
  }
  return VCY_OK;
}

}  // extern "C"
