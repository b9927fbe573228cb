// C-ABI entry points of libvacancy_hip.so: the error string, version, lifetime of a context, its parameters, timers,
// the carve log and the device-memory helpers.  State access and halos: vcy_state.hip; the carve entry points:
// vcy_carve.hip and carve_stream.hip; the mesh entry points and the host pool of their arrays: vcy_mesh.hip.
#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <vector>

#include "vcy_internal.h"
#include "build_id.h"  // VCY_SOURCE_HASH, written by the Makefile

namespace vcy {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

// Next slot of the carve timer's event log (vcy_set_param "carvetimer"); the events of a slot are created once and
// re-used after the log has been cleared.  -1 when the log is full (the launch is then simply not recorded) or an
// event cannot be created.
constexpr int kCarveLogMax = 8192;
int carve_log_open(vcy_ctx* c, bool first_chunk) {
  if (first_chunk) c->carve_log_last_dropped = false;
  if (c->carve_log_n >= kCarveLogMax) {
    ++c->carve_log_dropped;
    c->carve_log_last_dropped = true;
    return -1;
  }
  if ((size_t)c->carve_log_n == c->carve_log.size()) {
    vcy_ctx::CarveStamp st{};
    for (int k = 0; k < 3; ++k)
      if (st.ev[k].ensure() != hipSuccess) {
        (void)hipGetLastError();
        return -1;
      }
    c->carve_log.push_back(std::move(st));
  }
  const int i = c->carve_log_n++;
  c->carve_log[(size_t)i].first_chunk = first_chunk;
  if (first_chunk) c->carve_log_last = i;
  return i;
}

// axis_positions and dims_from_option (VoxelGrid::Init, Voxel::pos): host_shared.h

}  // namespace vcy

using namespace vcy;

namespace {
std::mutex g_ctx_count_mutex;
int g_ctx_count = 0;
}  // namespace

extern "C" {

const char* vcy_last_error(void) { return g_last_error.c_str(); }
const char* vcy_version(void) { return "vacancy_amd 0.3 (gfx950) src:" VCY_SOURCE_HASH; }

int vcy_device_count(int* count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
    return VCY_ERR_NO_DEVICE;
  }
  *count = n;
  return VCY_OK;
}

int vcy_compute_dims(const float bb_min[3], const float bb_max[3], float resolution,
                     int32_t dims[3]) {
  return dims_from_option(bb_min, bb_max, resolution, dims, true);
}

int vcy_axis_positions(const float bb_min[3], const float bb_max[3], float resolution, int axis, float* out) {
  if (!bb_min || !bb_max || !out || axis < 0 || axis > 2) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  int32_t n[3];
  const int rc = dims_from_option(bb_min, bb_max, resolution, n);
  if (rc != VCY_OK) return rc;
  axis_positions(bb_min[axis], bb_max[axis], resolution, n[axis], out);
  return VCY_OK;
}

int vcy_create(const vcy_carver_option* o, int device_id, int z_begin, int z_end, vcy_ctx** out) {
  if (!o || !out) {
    set_error("null argument");
    return VCY_ERR_INVALID_ARG;
  }
  *out = nullptr;
  // VoxelCarver::Init, reference voxel_carver.cc:376-389
  if (o->update_option.voxel_max_update_num < 1) {
    set_error("voxel_max_update_num must be positive");
    return VCY_ERR_INVALID_ARG;
  }
  if (o->update_option.voxel_update_weight < std::numeric_limits<float>::min()) {
    set_error("voxel_update_weight must be positive");
    return VCY_ERR_INVALID_ARG;
  }
  if (o->update_option.truncation_band < std::numeric_limits<float>::min()) {
    set_error("truncation_band must be positive");
    return VCY_ERR_INVALID_ARG;
  }
  const vcy_update_option& u = o->update_option;
  if (u.voxel_update < 0 || u.voxel_update > 1 || u.sdf_interp < 0 || u.sdf_interp > 1 ||
      u.update_outside < 0 || u.update_outside > 1) {
    set_error("unknown enum value in update_option");
    return VCY_ERR_INVALID_ARG;
  }
  int32_t n[3];
  int rc = dims_from_option(o->bb_min, o->bb_max, o->resolution, n);
  if (rc != VCY_OK) return rc;
  if (z_end < 0) z_end = n[2];
  if (z_begin < 0 || z_begin >= z_end || z_end > n[2]) {
    set_error("invalid z-slab [%d,%d) for nz=%d", z_begin, z_end, n[2]);
    return VCY_ERR_INVALID_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("no HIP device available (there is no CPU fallback)");
    return VCY_ERR_NO_DEVICE;
  }
  if (device_id < 0 || device_id >= ndev) {
    set_error("device %d out of range (%d devices)", device_id, ndev);
    return VCY_ERR_NO_DEVICE;
  }
  VCY_HIP_CHECK(hipSetDevice(device_id));

  std::unique_ptr<vcy_ctx, void (*)(vcy_ctx*)> owner(new vcy_ctx, vcy_destroy);  // (an early return destroys it)
  vcy_ctx* c = owner.get();
  c->device = device_id;
  c->opt = *o;
  c->nx = n[0];
  c->ny = n[1];
  c->nz = n[2];
  c->z0 = z_begin;
  c->z1 = z_end;
  c->slice = (int64_t)n[0] * n[1];
  c->halo_lo = (z_begin > 0) ? 2 : 0;
  if (c->halo_lo && z_begin < 2) {
    set_error("a non-first slab must start at z >= 2");
    return VCY_ERR_INVALID_ARG;
  }
  // update_num never exceeds voxel_max_update_num + 1 (voxel_carver.cc:447-450)
  const int64_t max_cnt = (int64_t)u.voxel_max_update_num + 1;
  c->cnt_bytes_wire = max_cnt <= 255 ? 1 : (max_cnt <= 65535 ? 2 : 4);
  c->cnt_bytes = 1;  // widened when the views applied (or uploaded counts) need it, ensure_count_width
  {
    const char* e = std::getenv("VCY_MC_TIMING");  // development aid: host-side phases of every extraction on stderr
    if (e && e[0] == '1') c->mc_timing = 1;
  }

  VCY_HIP_CHECK(c->stream.create(hipStreamNonBlocking));
  VCY_HIP_CHECK(c->ev_begin.ensure());
  VCY_HIP_CHECK(c->ev_end.ensure());
  const int64_t nvox = c->slice * (int64_t)(c->halo_lo + c->nz_local());
  VCY_HIP_CHECK(c->d_sdf.alloc((size_t)nvox * sizeof(float)));
  VCY_HIP_CHECK(c->d_cnt.alloc((size_t)nvox * c->cnt_bytes));
  VCY_HIP_CHECK(c->d_px.alloc(sizeof(float) * n[0]));
  VCY_HIP_CHECK(c->d_py.alloc(sizeof(float) * n[1]));
  VCY_HIP_CHECK(c->d_pz.alloc(sizeof(float) * n[2]));

  // Voxel::pos per axis (axis_positions above)
  float* d_axis[3] = {c->d_px, c->d_py, c->d_pz};
  for (int a = 0; a < 3; ++a) {
    std::vector<float> p(n[a]);
    axis_positions(o->bb_min[a], o->bb_max[a], o->resolution, n[a], p.data());
    VCY_HIP_CHECK(hipMemcpy(d_axis[a], p.data(), sizeof(float) * n[a], hipMemcpyHostToDevice));
    if (a == 0) {
      c->h_px = p;
      c->h_px_min = p.front();
      c->h_px_max = p.back();
    } else if (a == 1) {
      c->h_py_min = p.front();
      c->h_py_max = p.back();
    }
    if (a == 2) c->h_pz = p;
  }
  rc = fill_state(c);
  if (rc != VCY_OK) return rc;
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  {
    std::lock_guard<std::mutex> lock(g_ctx_count_mutex);
    ++g_ctx_count;
    c->counted = true;
  }
  *out = owner.release();
  return VCY_OK;
}

// Everything the context holds is a member of an owning type (vcy_resources.h) and goes with it.
void vcy_destroy(vcy_ctx* c) {
  if (!c) return;
  {
    std::lock_guard<std::mutex> lock(g_ctx_count_mutex);
    if (c->counted && --g_ctx_count == 0) mesh_pool_trim();
  }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;
}

int vcy_grid_dims(const vcy_ctx* c, int32_t dims[3]) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  dims[0] = c->nx;
  dims[1] = c->ny;
  dims[2] = c->nz;
  return VCY_OK;
}

int vcy_slab_range(const vcy_ctx* c, int32_t zr[2]) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  zr[0] = c->z0;
  zr[1] = c->z1;
  return VCY_OK;
}

int vcy_set_stream(vcy_ctx* c, void* s) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  { const int rcf = flush_pending(c); if (rcf != VCY_OK) return rcf; }
  if (c->stream) VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  VCY_HIP_CHECK(c->stream.release());
  c->stream.borrow((hipStream_t)s);
  return VCY_OK;
}

int vcy_set_param(vcy_ctx* c, const char* name, int value) {
  if (!c || !name) return VCY_ERR_INVALID_ARG;
  if (std::strcmp(name, "inject_carve_failure") == 0) {  // test hook; does not touch the queue
    c->inject_fail = value > 0 ? value : 0;
    return VCY_OK;
  }
  { const int rcf = flush_pending(c); if (rcf != VCY_OK) return rcf; }  // queued views keep the old setting
  if (std::strcmp(name, "defer") == 0) {
    c->defer = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "fused") == 0) {
    c->use_fused = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "tile") == 0) {
    if (value < 0 || value > 2) return VCY_ERR_INVALID_ARG;
    c->fused.knobs.tile_mode = value;
    return VCY_OK;
  }
  if (std::strcmp(name, "shortdiv") == 0) {
    c->fused.knobs.use_short_div = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "cull") == 0) {
    c->fused.knobs.use_cull = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "mcsweep") == 0) {
    c->mc_sweep = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "carvetimer") == 0) {
    c->time_carve = value != 0;
    c->carve_log_n = c->carve_log_last = c->carve_log_dropped = 0;  // (the log starts over)
    c->carve_log_last_dropped = false;
    return VCY_OK;
  }
  if (std::strcmp(name, "paircount") == 0) {
    c->fused.knobs.count_pairs = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "recordbytes") == 0) {
    c->fused.knobs.record_bytes_max = value > 0 ? value : 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "livelist") == 0) {
    c->fused.knobs.use_live_list = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "prologue") == 0) {
    if (value < 0 || value > 2) return VCY_ERR_INVALID_ARG;
    c->fused.knobs.prologue_mode = value;
    return VCY_OK;
  }
  if (std::strcmp(name, "livesync") == 0) {
    c->fused.knobs.live_sync = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "recordcache") == 0) {
    c->fused.knobs.record_cache = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "coopstore") == 0) {
    c->fused.knobs.coop_store = value < 0 ? -1 : (value != 0 ? 1 : 0);
    return VCY_OK;
  }
  if (std::strcmp(name, "listrecords") == 0) {
    c->fused.knobs.list_records = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "eagerstate") == 0) {
    c->fused.knobs.eager_state = value < 0 ? -1 : (value != 0 ? 1 : 0);
    return VCY_OK;
  }
  if (std::strcmp(name, "oneview") == 0) {
    c->fused.knobs.one_view = value != 0 ? 1 : 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "ntstore") == 0) {
    c->fused.knobs.nt_store = value < 0 ? -1 : (value != 0 ? 1 : 0);
    return VCY_OK;
  }
  if (std::strcmp(name, "rowkernel") == 0) {
    c->fused.knobs.row_kernel = value < 0 ? -1 : value;
    return VCY_OK;
  }
  if (std::strcmp(name, "mcskip") == 0) {
    c->mc_skip = value <= 0 ? 0 : (value >= 2 ? 2 : 1);
    return VCY_OK;
  }
  if (std::strcmp(name, "meshkeys") == 0) {
    c->mesh_keys = value != 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "rayskip") == 0) {
    c->ray_skip = value != 0 ? 1 : 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "smoothpad") == 0) {
    c->smooth_pad = value != 0 ? 1 : 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "chainrows") == 0) {
    c->chain_rows = value != 0 ? 1 : 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "rasterwide") == 0) {  // candidate pixels above which a face is drawn by its whole wave
    c->raster_wide = value < 0 ? 0 : value;
    return VCY_OK;
  }
  if (std::strcmp(name, "mcdirect") == 0) {  // bytes (of the guessed mesh) up to which mc_emit writes host memory directly
    c->mc_direct_bytes = value < 0 ? 0 : (int64_t)value;
    return VCY_OK;
  }
  if (std::strcmp(name, "mctiming") == 0) {
    c->mc_timing = value != 0 ? 1 : 0;
    return VCY_OK;
  }
  if (std::strcmp(name, "lazycount") == 0) {  // 0: counters at their final width from now on (round 4's layout)
    VCY_HIP_CHECK(hipSetDevice(c->device));
    c->lazy_count = value != 0;
    if (!c->lazy_count) return set_count_width(c, c->cnt_bytes_wire);
    return VCY_OK;
  }
  set_error("unknown parameter %s", name);
  return VCY_ERR_INVALID_ARG;
}

int vcy_get_param(vcy_ctx* c, const char* name, int* value) {
  if (!c || !name || !value) return VCY_ERR_INVALID_ARG;
  if (std::strcmp(name, "fused") == 0) *value = c->use_fused ? 1 : 0;
  else if (std::strcmp(name, "cull") == 0) *value = c->fused.knobs.use_cull ? 1 : 0;
  else if (std::strcmp(name, "tile") == 0) *value = c->fused.knobs.tile_mode;
  else if (std::strcmp(name, "defer") == 0) *value = c->defer ? 1 : 0;
  else if (std::strcmp(name, "shortdiv") == 0) *value = c->fused.knobs.use_short_div ? 1 : 0;
  else if (std::strcmp(name, "div_level") == 0) *value = c->fused.last_div_level;
  else if (std::strcmp(name, "mcsweep") == 0) *value = c->mc_sweep ? 1 : 0;
  else if (std::strcmp(name, "mcskip") == 0) *value = c->mc_skip;
  else if (std::strcmp(name, "rowkernel") == 0) *value = c->fused.knobs.row_kernel;
  else if (std::strcmp(name, "ntstore") == 0) *value = c->fused.knobs.nt_store;
  else if (std::strcmp(name, "oneview") == 0) *value = c->fused.knobs.one_view;
  else if (std::strcmp(name, "eagerstate") == 0) *value = c->fused.knobs.eager_state;
  else if (std::strcmp(name, "listrecords") == 0) *value = c->fused.knobs.list_records;
  else if (std::strcmp(name, "mcdirect") == 0) *value = (int)std::min<int64_t>(c->mc_direct_bytes, 0x7fffffff);
  else if (std::strcmp(name, "livelist") == 0) *value = c->fused.knobs.use_live_list ? 1 : 0;
  else if (std::strcmp(name, "prologue") == 0) *value = c->fused.knobs.prologue_mode;
  else if (std::strcmp(name, "coopstore") == 0) *value = c->fused.knobs.coop_store;
  else if (std::strcmp(name, "livesync") == 0) *value = c->fused.knobs.live_sync ? 1 : 0;
  else if (std::strcmp(name, "recordcache") == 0) *value = c->fused.knobs.record_cache ? 1 : 0;
  else if (std::strcmp(name, "recordcache_hits") == 0) *value = c->fused.rec_cache.hits;
  else if (std::strcmp(name, "brick_min_valid") == 0) *value = c->st.brick_min_valid && !c->st.fresh ? 1 : 0;
  else if (std::strcmp(name, "fresh") == 0) *value = c->st.fresh ? 1 : 0;  // the fill has not been written yet
  else if (std::strcmp(name, "meshkeys") == 0) *value = c->mesh_keys ? 1 : 0;
  else if (std::strcmp(name, "rayskip") == 0) *value = c->ray_skip;
  else if (std::strcmp(name, "smoothpad") == 0) *value = c->smooth_pad;
  else if (std::strcmp(name, "chainrows") == 0) *value = c->chain_rows;
  else if (std::strcmp(name, "rasterwide") == 0) *value = c->raster_wide;
  else if (std::strcmp(name, "lazycount") == 0) *value = c->lazy_count ? 1 : 0;
  else if (std::strcmp(name, "carvetimer") == 0) *value = c->time_carve ? 1 : 0;
  else if (std::strcmp(name, "carvelog_dropped") == 0) *value = c->carve_log_dropped;
  else if (std::strcmp(name, "count_bytes") == 0) *value = c->cnt_bytes;
  else if (std::strcmp(name, "count_bytes_final") == 0) *value = c->cnt_bytes_wire;
  else {
    set_error("unknown parameter %s", name);
    return VCY_ERR_INVALID_ARG;
  }
  return VCY_OK;
}

int vcy_get_stream(vcy_ctx* c, void** out) {
  if (!c || !out) return VCY_ERR_INVALID_ARG;
  *out = (void*)(hipStream_t)c->stream;
  return VCY_OK;
}

int vcy_sync(vcy_ctx* c) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  { const int rcf = flush_pending(c); if (rcf != VCY_OK) return rcf; }
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  return VCY_OK;
}

int vcy_timer_begin(vcy_ctx* c) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  VCY_HIP_CHECK(hipEventRecord(c->ev_begin, c->stream));
  return VCY_OK;
}

int vcy_timer_end(vcy_ctx* c, float* ms) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  { const int rcf = flush_pending(c); if (rcf != VCY_OK) return rcf; }  // queued views belong to the interval
  VCY_HIP_CHECK(hipEventRecord(c->ev_end, c->stream));
  VCY_HIP_CHECK(hipEventSynchronize(c->ev_end));
  VCY_HIP_CHECK(hipEventElapsedTime(ms, c->ev_begin, c->ev_end));
  return VCY_OK;
}

int vcy_last_carve_ms(vcy_ctx* c, float* prepass_ms, float* kernel_ms) {
  if (!c || !prepass_ms || !kernel_ms) return VCY_ERR_INVALID_ARG;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  *prepass_ms = *kernel_ms = 0.0f;
  if (c->carve_log_last_dropped) {  // (never an older launch's times in its place)
    set_error("vcy_last_carve_ms: the event log is full (%d records); read it with vcy_carve_log(clear = 1)", kCarveLogMax);
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = c->carve_log_last; i < c->carve_log_n; ++i) {  // the chunks of the last launch
    const vcy_ctx::CarveStamp& st = c->carve_log[(size_t)i];
    float a = 0.0f, b = 0.0f;
    VCY_HIP_CHECK(hipEventSynchronize(st.ev[2]));
    VCY_HIP_CHECK(hipEventElapsedTime(&a, st.ev[0], st.ev[1]));
    VCY_HIP_CHECK(hipEventElapsedTime(&b, st.ev[1], st.ev[2]));
    *prepass_ms += a;
    *kernel_ms += b;
  }
  return VCY_OK;
}

int vcy_carve_log(vcy_ctx* c, int max_records, float* begin_ms, float* prepass_ms, float* kernel_ms,
                  int32_t* first_chunk, int* n_records, int clear) {
  if (!c || !n_records || max_records < 0) return VCY_ERR_INVALID_ARG;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const int n = std::min(max_records, c->carve_log_n);
  for (int i = 0; i < n; ++i) {
    const vcy_ctx::CarveStamp& st = c->carve_log[(size_t)i];
    float t0 = 0.0f, a = 0.0f, b = 0.0f;
    VCY_HIP_CHECK(hipEventSynchronize(st.ev[2]));
    if (i > 0) VCY_HIP_CHECK(hipEventElapsedTime(&t0, c->carve_log[0].ev[0], st.ev[0]));
    VCY_HIP_CHECK(hipEventElapsedTime(&a, st.ev[0], st.ev[1]));
    VCY_HIP_CHECK(hipEventElapsedTime(&b, st.ev[1], st.ev[2]));
    if (begin_ms) begin_ms[i] = t0;
    if (prepass_ms) prepass_ms[i] = a;
    if (kernel_ms) kernel_ms[i] = b;
    if (first_chunk) first_chunk[i] = st.first_chunk ? 1 : 0;
  }
  *n_records = n;
  if (clear) {
    c->carve_log_n = c->carve_log_last = c->carve_log_dropped = 0;
    c->carve_log_last_dropped = false;
  }
  return VCY_OK;
}

int vcy_last_carve_pairs(vcy_ctx* c, int64_t* processed, int64_t* total, int64_t* per_layer, int max_layers, int* n_layers) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  if (!c->fused.knobs.count_pairs || !c->fused.d_pair_count) {
    set_error("vcy_last_carve_pairs: no fused launch since vcy_set_param(\"paircount\", 1)");
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const int nbz = (c->nz_local() + 7) / 8;
  std::vector<unsigned long long> h((size_t)nbz, 0ull);
  VCY_HIP_CHECK(hipMemcpyAsync(h.data(), c->fused.d_pair_count, sizeof(unsigned long long) * (size_t)nbz, hipMemcpyDeviceToHost, c->stream));
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  int64_t sum = 0;
  for (int l = 0; l < nbz; ++l) {
    sum += (int64_t)h[(size_t)l];
    if (per_layer && l < max_layers) per_layer[l] = (int64_t)h[(size_t)l];
  }
  if (processed) *processed = sum;
  if (total) *total = (int64_t)((c->nx + 7) / 8) * ((c->ny + 7) / 8) * nbz * c->fused.pair_count_views;
  if (n_layers) *n_layers = nbz;
  return VCY_OK;
}

int vcy_selftest(vcy_ctx* c) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  return selftest_fused(c->stream);
}

int vcy_sdf_upload(vcy_ctx* c, const float* host, int w, int h, float** dev_out) {
  if (!c || !host || !dev_out || w <= 0 || h <= 0) {
    set_error("invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  float* d = nullptr;
  VCY_HIP_CHECK(hipMalloc(&d, sizeof(float) * (size_t)w * h));
  hipError_t e = hipMemcpy(d, host, sizeof(float) * (size_t)w * h, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    set_error("hipMemcpy H2D failed: %s", hipGetErrorString(e));
    return VCY_ERR_HIP;
  }
  *dev_out = d;
  return VCY_OK;
}

int vcy_device_alloc(vcy_ctx* c, int64_t bytes, void** out) {
  if (!c || !out || bytes <= 0) return VCY_ERR_INVALID_ARG;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  VCY_HIP_CHECK(hipMalloc(out, (size_t)bytes));
  return VCY_OK;
}

int vcy_memcpy_h2d(vcy_ctx* c, void* dst, const void* src, int64_t bytes) {
  if (!c || !dst || !src || bytes < 0) return VCY_ERR_INVALID_ARG;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  VCY_HIP_CHECK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
  return VCY_OK;
}

int vcy_memcpy_d2h(vcy_ctx* c, void* dst, const void* src, int64_t bytes) {
  if (!c || !dst || !src || bytes < 0) return VCY_ERR_INVALID_ARG;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  VCY_HIP_CHECK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
  return VCY_OK;
}

int vcy_device_free(vcy_ctx* c, void* p) {
  if (!c) return VCY_ERR_NOT_INITIALIZED;
  VCY_HIP_CHECK(hipSetDevice(c->device));
  VCY_HIP_CHECK(hipStreamSynchronize(c->stream));
  VCY_HIP_CHECK(hipFree(p));
  return VCY_OK;
}

}  // extern "C"
