// The mesh entry points of the C ABI: the page-locked host pool the arrays of a returned mesh come from, the
// extraction wrappers and their timers, and the normals of a mesh on the host (whole meshes and the seams of merged
// slabs).  The extraction itself: mc_extract.hip.
#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "vcy_internal.h"

namespace vcy {

// ---- host buffers of returned meshes ---------------------------------------------------------
// The arrays of a vcy_mesh are page-locked host memory from a small process-wide pool: the mesh download
// (130 MB at 1024^3) is then one DMA at PCIe rate instead of a staged copy into freshly faulted pages, and
// vcy_mesh_free hands the buffers back for the next extraction.  Pageable memory is the fallback when
// pinning fails.
namespace {
struct HostBuf { void* p; size_t bytes; bool pinned; };
std::mutex g_mesh_mutex;
std::vector<HostBuf> g_mesh_live, g_mesh_idle;
constexpr size_t kMeshIdleCap = (size_t)3 << 30;  // idle bytes kept for reuse
}  // namespace

void* mesh_host_alloc(size_t bytes, bool* pinned_out) {
  if (pinned_out) *pinned_out = false;
  if (bytes == 0) bytes = 16;
  std::lock_guard<std::mutex> lock(g_mesh_mutex);
  size_t best = g_mesh_idle.size();
  for (size_t i = 0; i < g_mesh_idle.size(); ++i)
    if (g_mesh_idle[i].bytes >= bytes && g_mesh_idle[i].bytes <= 2 * bytes + 4096 &&
        (best == g_mesh_idle.size() || g_mesh_idle[i].bytes < g_mesh_idle[best].bytes))
      best = i;
  HostBuf b;
  if (best < g_mesh_idle.size()) {
    b = g_mesh_idle[best];
    g_mesh_idle.erase(g_mesh_idle.begin() + (long)best);
  } else {
    b.bytes = bytes + bytes / 8 + 4096;  // headroom: the next view's mesh is usually a little different
    b.p = nullptr;
    // (portable + mapped: the pool is shared by the contexts of every device of the process, and mc_emit writes small
    // meshes into these arrays from whichever device extracts -- "mcdirect")
    b.pinned = hipHostMalloc(&b.p, b.bytes, hipHostMallocPortable | hipHostMallocMapped) == hipSuccess && b.p != nullptr;
    if (!b.pinned) {
      (void)hipGetLastError();
      b.p = std::malloc(b.bytes);
      if (!b.p) return nullptr;
    }
  }
  g_mesh_live.push_back(b);
  if (pinned_out) *pinned_out = b.pinned;  // (page-locked: kernels can write it directly, mc_emit)
  return b.p;
}

void mesh_host_free(void* p) {
  if (!p) return;
  std::lock_guard<std::mutex> lock(g_mesh_mutex);
  for (size_t i = 0; i < g_mesh_live.size(); ++i) {
    if (g_mesh_live[i].p != p) continue;
    const HostBuf b = g_mesh_live[i];
    g_mesh_live.erase(g_mesh_live.begin() + (long)i);
    size_t idle = 0;
    for (const HostBuf& q : g_mesh_idle) idle += q.bytes;
    if (b.pinned && idle + b.bytes <= kMeshIdleCap) {
      g_mesh_idle.push_back(b);
    } else if (b.pinned) {
      (void)hipHostFree(b.p);
    } else {
      std::free(b.p);
    }
    return;
  }
  std::free(p);  // not ours (never happens for meshes this library returned)
}

// idle page-locked mesh buffers are only worth keeping while a context may extract again
void mesh_pool_trim() {
  std::lock_guard<std::mutex> lock(g_mesh_mutex);
  for (const HostBuf& b : g_mesh_idle) (void)hipHostFree(b.p);
  g_mesh_idle.clear();
}

}  // namespace vcy

using namespace vcy;

extern "C" {

// What the extraction entry points share once their arguments are checked: the device, the views still pending, the
// call, empty structs after a failure, and the wall time (call entry -> mesh arrays in host memory).
static int timed_extract(vcy_ctx* c, double iso, int linear_interp, vcy_mesh* out, int which,
                         vcy_mesh_normals* normals_out, int64_t* layer_faces) {
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const auto t0 = std::chrono::steady_clock::now();
  { int rcm = materialize(c); if (rcm != VCY_OK) return rcm; }
  const int rc = extract_iso(c, iso, linear_interp, out, which, normals_out, layer_faces);
  if (rc != VCY_OK) {
    vcy_mesh_free(out);
    if (normals_out) vcy_mesh_normals_free(normals_out);
    if (layer_faces) layer_faces[0] = layer_faces[1] = 0;
  }
  c->last_extract_wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int vcy_extract_iso(vcy_ctx* c, double iso, int linear_interp, vcy_mesh* out) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!out) return VCY_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  return timed_extract(c, iso, linear_interp, out, 0, nullptr, nullptr);
}

int vcy_extract_iso_normals(vcy_ctx* c, double iso, int linear_interp, int which, vcy_mesh* out,
                            vcy_mesh_normals* normals_out) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!out || !normals_out || (which & ~(VCY_NORMALS_VERTEX | VCY_NORMALS_FACE)) != 0) {
    set_error("vcy_extract_iso_normals: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  std::memset(out, 0, sizeof(*out));
  std::memset(normals_out, 0, sizeof(*normals_out));
  if (c->z0 != 0 || c->z1 != c->nz || c->halo_lo != 0) {
    // a vertex on a slab's top or bottom plane has faces in the neighbouring slab
    set_error("vcy_extract_iso_normals: the context owns z [%d, %d) of %d slices; normals need the whole grid "
              "(merge the slabs' meshes and call vcy_mesh_normals_host)", c->z0, c->z1, c->nz);
    return VCY_ERR_UNSUPPORTED;
  }
  if (which == 0) return vcy_extract_iso(c, iso, linear_interp, out);
  return timed_extract(c, iso, linear_interp, out, which, normals_out, nullptr);
}

int vcy_extract_iso_normals_slab(vcy_ctx* c, double iso, int linear_interp, int which, vcy_mesh* out,
                                 vcy_mesh_normals* normals_out, int64_t layer_faces[2]) {
  if (!c) {
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  if (!out || !normals_out || !layer_faces || (which & ~(VCY_NORMALS_VERTEX | VCY_NORMALS_FACE)) != 0) {
    set_error("vcy_extract_iso_normals_slab: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  std::memset(out, 0, sizeof(*out));
  std::memset(normals_out, 0, sizeof(*normals_out));
  layer_faces[0] = layer_faces[1] = 0;
  const bool whole = c->z0 == 0 && c->z1 == c->nz && c->halo_lo == 0;
  if (!whole && !c->mesh_keys) {
    // the seam vertices are found by the edge keys of the slab's foreign vertices
    set_error("vcy_extract_iso_normals_slab: the context owns z [%d, %d) of %d slices; the merge of its normals needs "
              "the edge keys (vcy_set_param \"meshkeys\" 1)", c->z0, c->z1, c->nz);
    return VCY_ERR_INVALID_ARG;
  }
  return timed_extract(c, iso, linear_interp, out, which, normals_out, layer_faces);
}

void vcy_mesh_normals_free(vcy_mesh_normals* n) {
  if (!n) return;
  mesh_host_free(n->vertex_normals);
  mesh_host_free(n->face_normals);
  std::memset(n, 0, sizeof(*n));
}

int vcy_last_normals_ms(const vcy_ctx* c, float* device_ms) {
  if (!c || !device_ms) return VCY_ERR_INVALID_ARG;
  *device_ms = c->last_normals_device_ms;
  return VCY_OK;
}

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

int vcy_last_extract_wall_ms(const vcy_ctx* c, float* wall_ms) {
  if (!c || !wall_ms) return VCY_ERR_INVALID_ARG;
  *wall_ms = c->last_extract_wall_ms;
  return VCY_OK;
}

int vcy_last_extract_ms(const vcy_ctx* c, float* device_ms) {
  if (!c || !device_ms) return VCY_ERR_INVALID_ARG;
  *device_ms = c->last_extract_device_ms;
  return VCY_OK;
}

void vcy_mesh_free(vcy_mesh* m) {
  if (!m) return;
  mesh_host_free(m->vertices);
  mesh_host_free(m->faces);
  mesh_host_free(m->edge_keys);
  std::memset(m, 0, sizeof(*m));
}

}  // extern "C"
