// The mesh entry points of the C ABI: the page-locked host pool the arrays of a returned mesh come from, the
// extraction wrappers and their timers.  The extraction itself: mc_extract.hip; normals and the stitch of z-slab meshes
// on the host: mesh_host.hip.
#include <chrono>
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
