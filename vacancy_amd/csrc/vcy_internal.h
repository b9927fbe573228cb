// Internal declarations shared by the HIP translation units of libvacancy_hip.so.
// gfx950 (MI355X) only; built with -ffp-contract=off (bit-exact parity with the
// reference's non-FMA x86 arithmetic).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "vacancy_hip.h"

#include "host_shared.h"  // set_error, axis_positions, dims_from_option, check_view_static

namespace vcy {

#define VCY_HIP_CHECK(expr)                                                        \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) {                                                        \
      ::vcy::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),      \
                       __FILE__, __LINE__);                                        \
      return VCY_ERR_HIP;                                                          \
    }                                                                              \
  } while (0)

// std::numeric_limits<float>::lowest(), InvalidSdf::kVal (reference voxel_carver.cc:100)
constexpr float kInvalidSdf = -3.402823466e+38f;

}  // namespace vcy

#include "vcy_resources.h"  // DeviceBuf, PinnedBuf, Event, Stream: what owns the context's resources
#include "state_flags.h"    // StateFlags: what the context knows about its voxel state, and who may say so
#include "carve_fused_state.h"  // FusedState: what the fused carve keeps between its launches

// The device-resident voxel grid of one z-slab.
//
// Layout (structure of arrays, the reference's 40-byte AoS Voxel is never materialised):
//   sdf   float  [halo_lo + nz_local][ny][nx]   x fastest, one contiguous slab in HBM
//   cnt   u8/u16/u32 same shape                 Voxel::update_num
//   px/py/pz     float[nx]/[ny]/[nz]            Voxel::pos per axis (global index)
// halo_lo = 2 slices below the slab when z_begin > 0 (filled by vcy_halo_unpack before
// extraction), 0 otherwise.  Voxel::index/id are implicit, Voxel::outside is dead in the
// reference, Voxel::on_surface belongs to ExtractVoxel (host).
struct vcy_ctx {
  int device = 0;
  bool counted = false;               // registered in the process-wide context count (vcy_create succeeded)
  // Members are destroyed in reverse order of declaration and a stream must outlive everything that was used on it:
  // the two streams come first, every buffer and event after them.
  vcy::Stream stream;
  vcy::Stream aux_stream;             // producer stream of the streamed batch (uploads + SDF build)
  vcy::Event ev_begin, ev_end;
  vcy::FusedState fused;              // the fused carve's knobs, buffers and view cache (carve_fused_state.h): after the streams, so destroyed before them

  vcy_carver_option opt{};
  int nx = 0, ny = 0, nz = 0;  // global dims
  int z0 = 0, z1 = 0;          // owned slab [z0, z1)
  int halo_lo = 0;             // slices stored below z0
  vcy::StateFlags st;          // fresh, halo_valid, cnt_implied, brick_min_valid, views_carved, epoch: read everywhere, changed only through its functions
  int64_t slice = 0;           // nx*ny
  // Counter width, lazily widened (round 5): update_num of a voxel cannot exceed the number of views applied since the
  // fill, so the array is u8 while at most 255 views have been applied (or uploaded counts are <= 255), u16 up to 65535,
  // u32 beyond -- whatever voxel_max_update_num would allow in the end (cnt_bytes_wire, also the width of the halo
  // packs, whose layout therefore does not depend on how far a slab has got).  The default options (max 255 -> counts up
  // to 256) used to mean 6 B/voxel from the start; now 5 B/voxel until the 256th view.  ensure_count_width() widens
  // (one conversion pass, skipped on a fresh slab); vcy_reset goes back to u8.  vcy_set_param "lazycount" 0 keeps the
  // final width from the start.
  int cnt_bytes = 1;
  int cnt_bytes_wire = 1;
  bool lazy_count = true;

  vcy::DeviceBuf<float> d_sdf;        // includes halo slices
  vcy::DeviceBuf<> d_cnt;
  vcy::DeviceBuf<> d_cnt_spare;       // the counter array of the OTHER width, kept once it exists (set_count_width): a
                                      // reset / carve cycle across the 256th view then allocates and frees nothing
  vcy::DeviceBuf<> d_xv_scratch;      // ExtractVoxel: keep bits, block counts, scan scratch (grow-only)
  vcy::DeviceBuf<> d_xv_ids;          // ExtractVoxel: the kept voxel ids before their copy to the host (grow-only)
  vcy::DeviceBuf<> d_halo_tmp;        // two slices of a neighbour's counters at ITS width (vcy_halo_copy_from)
  vcy::DeviceBuf<float> d_px, d_py, d_pz;

  bool mesh_keys = true;              // vcy_extract_iso also returns the edge key of every vertex (vcy_set_param "meshkeys")
  int mc_skip = 1;                    // marching cubes: bricks whose kept minimum is above the iso level are not read (vcy_set_param "mcskip": 0 never, 1 where it pays -- rows of 1024 voxels and more --, 2 wherever possible)
  bool mc_sweep = false;              // marching cubes: cell search in one sweep with the bit planes in LDS where the row shape allows (vcy_set_param "mcsweep")
  // Views accepted by the per-view entry points (vcy_carve, vcy_carve_device, vcy_carve_silhouette) but
  // not applied yet: they are carved together, in order, by ONE fused launch when the state is next
  // needed (extraction, download, halo, timer, sync ...) or when 32 are waiting -- the reference's
  // `for each view: Carve()` loop then costs one pass over the grid instead of one per view.
  struct PendingView {
    vcy_view view;
    vcy::DeviceBuf<float> d_sdf;  // private device copy of the SDF image
  };
  std::vector<PendingView> pending;
  std::vector<vcy::DeviceBuf<float>> sdf_pool;  // idle image buffers
  vcy::DeviceBuf<> d_sil_scratch;     // staging of vcy_carve_silhouette (mask + transform scratch)
  bool defer = true;                  // vcy_set_param("defer", 0): apply every view at once
  // A queued view that failed to apply inside a call that cannot report it to a Carve() caller (an
  // extraction, a download ...) is remembered: the NEXT carve entry point returns it (then clears it).
  int deferred_rc = 0;
  int inject_fail = 0;                // test hook: the next n applications of views fail (vcy_set_param "inject_carve_failure")
  std::string deferred_msg;
  bool use_fused = true;              // vcy_set_option("fused", 0) forces the per-view kernel
  std::vector<float> h_px;            // host copy of the x axis table (c0 tables of the fused carve)
  float h_px_min = 0, h_px_max = 0, h_py_min = 0, h_py_max = 0;  // extreme voxel centres
  std::vector<float> h_pz;            // host copy of d_pz (per-view z tables of the fused carve)
  vcy::DeviceBuf<float> d_brick_min;  // min(sdf) of every 8x8x8 wave brick of the slab [bz][by][bxw], kept by the fused carve
                                      // (current while st.brick_min_valid)
  bool time_carve = false;            // vcy_set_param("carvetimer", 1): events around pre-pass and carve kernel of every fused launch
  struct CarveStamp {                 // one chunk of one fused launch
    vcy::Event ev[3];                 // before window maxima / pre-pass, before the carve kernel, after it
    bool first_chunk;
  };
  std::vector<CarveStamp> carve_log;  // event triplets, created on demand (vcy_carve_log, vcy_last_carve_ms)
  int carve_log_n = 0;                // triplets recorded since the log was last cleared
  int carve_log_last = 0;             // index of the first chunk of the last launch
  int carve_log_dropped = 0;          // chunks that found the log full since it was cleared (vcy_get_param "carvelog_dropped")
  bool carve_log_last_dropped = false;  // ... the last launch among them: vcy_last_carve_ms has nothing to report
  vcy::DeviceBuf<> d_stream_pool;     // staging of vcy_carve_batch_silhouettes (masks, SDFs, scratch)
  vcy::Event ev_ready[2], ev_consumed[2], ev_uploaded[2];
  std::vector<vcy::Event> stream_events;  // four per chunk of the last streamed batch (vcy_last_stream_ms)
  int stream_timed_chunks = 0;
  float stream_wall_ms = 0.0f;
  vcy::PinnedBuf<> h_pinned;          // page-locked staging of the silhouettes, two sets
  vcy::DeviceBuf<> d_mc_tables;       // marching-cubes case tables (mc_extract.hip)
  vcy::DeviceBuf<> d_mc_scratch;      // bit planes, active words, offsets, per-cell info
  vcy::DeviceBuf<> d_mc_flags;        // publication flags of the chained scans (mc_kernels.hip scan_chained_kernel)
  uint32_t mc_scan_epoch = 0;         // ... and the epoch of the last scan (flags never hold a later one)
  vcy::PinnedBuf<void, hipHostMallocPortable | hipHostMallocMapped> h_mc_report;  // 64 page-locked bytes mc_emit reports an extraction's counts in (extract_iso)
  int64_t mc_direct_bytes = (int64_t)32 << 20;  // "mcdirect": meshes guessed up to this size are written by mc_emit straight into host memory
  int mc_timing = 0;                  // "mctiming" 1 (or VCY_MC_TIMING=1): host-side phases of every extraction on stderr
  uint32_t mc_scan_tickets[2] = {0, 0};  // chunk tickets drawn so far from the two scan slots' counters (scan_chained_kernel)
  vcy::DeviceBuf<> d_mc_cells;        // per-active-cell arrays of the extraction
  vcy::DeviceBuf<> d_mc_out;          // device staging of the extracted mesh
  int64_t mc_hint_cells = 0, mc_hint_verts = 0, mc_hint_faces = 0;  // sizes of the last extraction (extract_iso)
  float last_extract_device_ms = 0.0f;
  float last_extract_wall_ms = 0.0f;  // call entry -> mesh arrays in host memory
  vcy::Event ev_mc_begin, ev_mc_end;  // the extraction's own timer
  vcy::DeviceBuf<> d_mc_normals;      // device staging of the normals of vcy_extract_iso_normals (grow-only)
  vcy::Event ev_nrm_begin, ev_nrm_end;  // around the normals launches (vcy_last_normals_ms)
  float last_normals_device_ms = 0.0f;
  // connected components (components.hip); everything grow-only
  vcy::DeviceBuf<> d_cc_labels;       // int32 per voxel: the label (smallest voxel id of the component) or -1, of the last labelling
  vcy::DeviceBuf<> d_cc_bits;         // the solid bit of every voxel in 64-voxel words along x, and the root counter behind them
  vcy::DeviceBuf<> d_cc_roots;        // [statistics | sorted roots | removal flags] of up to cc_roots_cap components
  int cc_roots_cap = 0;               // (a count of components, not of bytes)
  int cc_n_roots = 0;
  vcy::PinnedBuf<> h_cc_report;       // 64 page-locked bytes the number of roots is read through
  bool cc_labels_valid = false;       // vcy_download_labels has something to return ...
  bool cc_labels_empty = false;       // ... namely -1 everywhere (the slab was fresh: nothing was launched)
  vcy::Event ev_cc_begin, ev_cc_end;
  bool cc_timed = false;
  float last_components_device_ms = 0.0f;
  // ... of a z-slab (vcy_label_components_slab and what follows it): host copies of the last labelling, in the order of
  // the sorted root list the device holds (the slot order of cc_filter_kernel)
  std::vector<int> cc_roots_host;     // slab-local roots, ascending
  std::vector<int64_t> cc_nvox_host;  // voxels of each root's piece
  std::vector<int64_t> cc_global_host;  // the installed map (vcy_resolve_components_slab): global label per slot; empty: none
                                      // (whether the seam calls may follow the last labelling: st.seams_current)
  vcy::DeviceBuf<> d_cc_seam;         // seam pairs: [the lower slab's top plane, int64 per voxel | counter | pairs] (grow-only)

  // distance field of the hull (distance.hip); grow-only
  vcy::DeviceBuf<> d_df_buf;          // [solid bits | row distances, 1 B | y-pass values, 2 B | phi table | counters | the int32 field]
  vcy::Event ev_df_begin, ev_df_end;  // around the launches of the last vcy_distance_field / vcy_redistance
  float last_distance_device_ms = 0.0f;
  // ... of a z-slab (vcy_distance_slab_begin and what follows it): the part of the pool that outlives a call
  vcy::DeviceBuf<> d_df_h;            // [planes of the neighbours below | the slab's y-pass values | planes of those above], 2 B each
  int64_t df_epoch = -1;              // d_df_h's middle describes the state of this epoch (against st.epoch; -1: nothing kept) ...
  double df_iso = 0.0;                // ... at this iso level ...
  int df_radius = 0;                  // ... and radius, which also fixes the planes in front and behind

  // ray-cast of the hull (render.hip); everything grow-only
  vcy::DeviceBuf<> d_rn_bits;         // [solid bit of every voxel, 64-voxel words along x | one bit per 8 x 8 x 8 brick that holds a solid voxel]
  bool rn_bits_valid = false;         // ... describe the state of epoch rn_epoch (against st.epoch) at the iso level rn_iso
  int64_t rn_epoch = -1;
  double rn_iso = 0.0;
  vcy::DeviceBuf<float> d_rn_planes;  // the cell planes of the three axes one behind the other (vcy_cell_planes), nx + ny + nz + 3 floats
  vcy::DeviceBuf<> d_rn_out;          // view records, counters, images and silhouettes of one launch
  vcy::Event ev_rn_begin, ev_rn_end;
  float last_render_device_ms = 0.0f;
  int ray_skip = 1;                   // "rayskip": rays step over bricks without a solid voxel (0: crossing by crossing)

  // colours of vertices (color.hip); grow-only
  vcy::DeviceBuf<> d_cl_buf;          // view records, vertices, normals, results, carried accumulators and the images of one chunk of views
  vcy::Event ev_cl_begin, ev_cl_end;
  float last_color_device_ms = 0.0f;

  // rasteriser of an indexed mesh (raster.hip); grow-only
  vcy::DeviceBuf<> d_rs_buf;          // view records, counters, the mesh, and per view of a chunk: key image, depth, face ids, hit bits, silhouette
  vcy::Event ev_rs[3];                // before the key fill and the raster launch, between raster and resolve, after the resolve
  float last_raster_ms[2] = {0.0f, 0.0f};  // vcy_last_raster_ms: raster (with the key fill), resolve
  int raster_wide = 64;               // "rasterwide": a face whose candidate box holds more pixels than this is drawn by its whole wave
  // ... and the shading pass behind it (raster_shade.hip), in the same pool
  vcy::Event ev_sh[3];                // before the key fill and the raster launch, between raster and shade, after the shade
  float last_shade_ms[2] = {0.0f, 0.0f};   // vcy_last_shade_ms: raster (with the key fill), shade

  // robust carve (carve_robust.hip)
  vcy::Event ev_rb_begin, ev_rb_end;  // around its launch (vcy_last_robust_ms)
  float last_robust_device_ms = 0.0f;

  // depth carve (carve_depth.hip)
  std::vector<vcy::Event> ev_dp;      // a pair around every launch of the last call (vcy_last_depth_ms), created on demand
  float last_depth_device_ms = 0.0f;

  // mesh smoothing (mesh_smooth.hip); grow-only
  vcy::DeviceBuf<> d_sm_buf;          // the mesh, its incidence table and gather rows, both position arrays, the normals
  vcy::Event ev_sm[4];                // around the table's launches, the passes and the normals (vcy_last_smooth_ms)
  float last_smooth_ms[3] = {0.0f, 0.0f, 0.0f};
  int smooth_pad = 0;                 // "smoothpad": positions of the passes padded to 16 bytes (one dwordx4 gather) instead of 12 (three dword gathers)

  // normals of an indexed mesh in device memory (mesh_normals.hip): its incidence table and the normals; grow-only
  vcy::DeviceBuf<> d_mn_buf;

  // mesh decimation (mesh_decimate.hip); grow-only
  vcy::DeviceBuf<> d_dc_buf;          // the mesh, keys, both tables, flags and their scans, member rows, the outputs
  vcy::Event ev_dc[6];                // around the cluster, faces, emit launches, and around the normals (vcy_last_decimate_ms)
  float last_decimate_ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  vcy::Event ev_dq[2];                // around the quadric stage of vcy_decimate_mesh_quadric (vcy_last_quadric_ms)
  float last_quadric_ms = 0.0f;

  // extraction chain (mesh_chain.hip); grow-only
  vcy::DeviceBuf<> d_ch_buf;          // the vertex -> incident-corner table of the extracted mesh, shared by the stages
  vcy::Event ev_ch[2];                // around the table's count, scan and fill
  int chain_rows = 1;                 // "chainrows": 1 the table from the cells (mc_corner_rows, mc_normals.hip), 0 from the faces (mesh_rows.h)
  float last_chain_ms[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // vcy_last_chain_ms, in its order

  float* owned_slab_sdf() const { return d_sdf + (int64_t)halo_lo * slice; }
  void* owned_slab_cnt() const { return (char*)d_cnt + (int64_t)halo_lo * slice * cnt_bytes; }
  int nz_local() const { return z1 - z0; }
  int64_t slab_voxels() const { return slice * (int64_t)(z1 - z0); }
};

namespace vcy {

// carve_kernels.hip
// `queued`: the views are those of vcy_ctx::pending (flush_pending alone says so)
int launch_carve(vcy_ctx* ctx, int n_views, const vcy_view* views, const float* const* sdf_dev, bool queued = false);
// carve_fused.hip (host side and pre-pass of the fused carve step; the kernel: carve_fused_kernel.h)
struct GridParams;
struct ViewParams;
bool fused_eligible(const vcy_ctx* ctx, int n_views, const vcy_view* views);
// `ortho`: the projection model of the views (one per launch); `views_before`: views applied since the fill when this
// launch starts (the caller has declared its whole call already)
int launch_carve_fused(vcy_ctx* ctx, const GridParams& g, int n_views, const ViewParams* vp, bool ortho, int64_t views_before);
int fused_max_views();
int plan_layer_pairs(vcy_ctx* ctx, int n_views, const ViewParams* vp, bool ortho, int stride, std::vector<double>* pairs,
                     int64_t* bricks_per_layer);  // the slab planner's estimate (carve_fused.hip)
void partition_layers(const double* cost, int n_layers, int n_slabs, int nz, int32_t* z_bounds);  // carve_kernels.hip
int plan_z_slabs(vcy_ctx* ctx, int n_views, const vcy_view* views, const float* const* sdf_dev, int n_slabs, int stride,
                 float brick_cost, int32_t* z_bounds, double* layer_cost, int max_layers, int* n_layers);  // carve_kernels.hip
int selftest_fused(hipStream_t stream);
int flush_pending(vcy_ctx* ctx, bool from_carve = false);   // applies vcy_ctx::pending (no-op when empty)
int check_carve_views(vcy_ctx* ctx, int n_views, const vcy_view* views);  // argument checks of the carve entry points (vcy_carve.hip)
// ... the part of them that needs no context, image size and ROI: check_view_static (host_shared.h)
int carve_log_open(vcy_ctx* ctx, bool first_chunk);          // next slot of vcy_ctx::carve_log, or -1 (vcy_api.hip)
// mc_extract.hip: the host driver of the marching-cubes extraction (its kernels and their launches: mc_kernels.hip,
// mc_normals.hip; what the three share: mc_common.h)
// `which` (VCY_NORMALS_*) != 0: the normals of the mesh as well, into `normals_out` (mc_normals.hip)
// `layer_faces` != null (vcy_extract_iso_normals_slab): the faces of the first and of the last own cell layer; a context
// that owns a z-slab then gets the slab instance of the vertex normals (seam vertices left at zero)
int extract_iso(vcy_ctx* ctx, double iso, int linear_interp, vcy_mesh* out, int which = 0,
                vcy_mesh_normals* normals_out = nullptr, int64_t* layer_faces = nullptr);
// ... and with the mesh left in the device staging, for the extraction chain: extract_iso_staged (mc_common.h)
// components.hip: vcy_label_components, vcy_keep_components, vcy_download_labels, vcy_last_components_ms, the _slab
// entries of a z-slab context and the seam merge on the host (vcy_merge_components_host)
// the solid bit of every voxel of the owned slices in 64-voxel words along x, (nx + 63) / 64 words per row (cc_bits_kernel);
// the state must be materialised.  Shared by the labelling and the ray-cast (render.hip).
int launch_solid_bits(vcy_ctx* ctx, double iso, unsigned long long* bits);
// distance.hip: vcy_distance_field, vcy_redistance, vcy_last_distance_ms; distance_host.hip (host code only):
// vcy_distance_field_host; what the two share: distance_field.h.  The z-slab form in both: vcy_distance_slab_begin,
// vcy_distance_slab_planes, vcy_distance_field_slab, vcy_redistance_slab; vcy_distance_slab_planes_host, _finish_host
// render.hip: vcy_render_hull, vcy_hull_agreement, vcy_render_hull_slab, vcy_cell_planes, vcy_last_render_ms
// vcy_render_hull's depth images of up to 64 views (one launch), left in device memory: depth_dev[i] points into
// vcy_ctx::d_rn_out and holds until the context next renders; waits for the launch; vcy_last_render_ms as for the render
int render_depth_device(vcy_ctx* ctx, double iso, int n_views, const vcy_view* views, const float** depth_dev, const char* who);
// color.hip: vcy_color_vertices, vcy_color_vertices_host, vcy_last_color_ms
// raster.hip: vcy_raster_mesh, vcy_mesh_agreement, vcy_last_raster_ms; raster_host.hip (host code only):
// vcy_raster_mesh_host and the argument checks of the three; what device and host share: raster_fragment.h
int raster_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                      int n_views, const vcy_view* views);
// raster_shade.hip: vcy_shade_mesh, vcy_mesh_photo_error, vcy_last_shade_ms (the raster launch they share with raster.hip:
// raster_launch.h); shade_host.hip (host code only): vcy_shade_mesh_host, vcy_mesh_photo_error_host and the argument checks
// of the four; what device and host share: raster_shade.h
int shade_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                     const float* attributes, int n_views, const vcy_view* views, const vcy_shade_option* option);
int photo_error_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                           const float* colors, int n_views, const vcy_view* views, const uint8_t* const* photos,
                           const uint8_t* const* masks, const int64_t* sums);
// mesh_smooth.hip: vcy_smooth_mesh, vcy_last_smooth_ms; mesh_smooth_host.hip (host code only): vcy_smooth_mesh_host and
// the argument checks of the two
int smooth_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                      const vcy_smooth_option* option, const float* vertices_out);
// mesh_normals.hip: Mesh::CalcNormal of a mesh in device memory for the mesh operators, launched, not waited for: the two
// kernels through a vertex -> incident-corner table the caller has built (mesh_rows.h; rows sorted ascending) ...
int launch_mesh_normals(hipStream_t stream, int64_t n_vertices, int64_t n_faces, const float* d_vertices, const int32_t* d_faces,
                        const int* d_row_offsets, const int* d_rows, float* d_face_normals, float* d_vertex_normals);
// ... and with a table built for the purpose in a pool of its own (vcy_ctx::d_mn_buf), on the context's stream; the two
// results are device pointers into that pool
int mesh_normals_device(vcy_ctx* ctx, int64_t n_vertices, int64_t n_faces, const float* d_vertices, const int32_t* d_faces,
                        bool vertex_normals, float** d_face_normals, float** d_vertex_normals);
// mesh_decimate.hip: vcy_decimate_mesh, vcy_last_decimate_ms, vcy_decimate_mesh_quadric, vcy_last_quadric_ms;
// mesh_decimate_host.hip (host code only): vcy_decimate_mesh_host, vcy_decimate_mesh_quadric_host and the argument checks
// of the four (`regularize` non-NULL: those of the quadric entry points); what device and host share: mesh_decimate.h,
// mesh_quadric.h
int decimate_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                        const vcy_decimate_option* option, const float* vertices_out, const int32_t* faces_out,
                        const int64_t* n_vertices_out, const int64_t* n_faces_out, const float* regularize = nullptr);
// the in-place exclusive scan of mc_kernels.hip for the other compactions of the library; `scratch`: the chunk sums of
// every level, scan_scratch_words(n) words
int device_exclusive_scan_u64(unsigned long long* d, int64_t n, unsigned long long* d_total, unsigned long long* scratch,
                              hipStream_t stream);
size_t scan_scratch_words(size_t n);
// carve_robust.hip: vcy_carve_robust_device, vcy_carve_robust_silhouettes, vcy_last_robust_ms
// carve_depth.hip: vcy_carve_depth_device, vcy_carve_depth, vcy_last_depth_ms; carve_depth_host.hip (host code only):
// vcy_carve_depth_host; what the two share: depth_sample.h
// render_merge.hip (host code only): vcy_render_merge_host, vcy_hull_agreement_host, and the view checks of the ray-cast
int check_render_view(const vcy_view* v, int i);
// sdf2d.hip
void host_distance_transform_l1(const uint8_t* mask, int w, int h, const int32_t* rmin,
                                const int32_t* rmax, float* out);
void host_make_sdf(const uint8_t* mask, int w, int h, const int32_t* rmin, const int32_t* rmax,
                   bool normalize, bool truncate, float band, float* out);
int device_make_sdf(hipStream_t stream, const uint8_t* mask_dev, int w, int h, const int32_t* rmin,
                    const int32_t* rmax, bool normalize, bool truncate, float band, void* scratch,
                    float* sdf_dev);
size_t device_make_sdf_scratch_bytes(int w, int h);
int device_make_sdf_batch(hipStream_t stream, int n, const uint8_t* const* masks_dev, const vcy_view* views,
                          bool normalize, bool truncate, float band, char* scratch, size_t scratch_stride,
                          float* const* sdf_dev);
// vcy_api.hip: the error string (set_error above), vcy_version, vcy_create / vcy_destroy, dims and axis positions, the
// stream, vcy_set_param / vcy_get_param, timers, the carve log and pair-count readers, the self test, and the device
// memory handed to callers (vcy_sdf_upload, vcy_device_alloc / _free, vcy_memcpy_*)
// vcy_carve.hip: the per-view carve entry points (vcy_carve*, vcy_make_sdf_device), the queue of pending views, the slab
// planner's wrappers and the two host SDF wrappers
// carve_stream.hip: the streamed silhouette paths (vcy_make_sdf_batch_device, vcy_carve_batch_silhouettes,
// vcy_carve_batch_silhouettes_sharded with its cached producer groups, vcy_last_stream_ms): one layout, one producer
// step and one consume step for the three
// rccl_api.h / rccl_api.hip: the dlopen'd RCCL table, the owner of a communicator, vcy_last_collective
// halo_exchange.hip: vcy_halo_allgather with its cached communicator groups, vcy_comm_create / _destroy,
// vcy_halo_allgather_ranks, vcy_halo_shutdown
// rendezvous.hip (host code only): vcy_rendezvous_exchange, over a file or a TCP port
// vcy_mesh.hip: the vcy_extract_iso* wrappers, vcy_mesh_free / vcy_mesh_normals_free, the extraction's timers, and the
// host arrays of returned meshes (page-locked pool); released by vcy_mesh_free
// mesh_host.hip (host code only): vcy_mesh_normals_host*, vcy_mesh_normals_seam_sum, vcy_merge_meshes_host
void* mesh_host_alloc(size_t bytes, bool* pinned_out = nullptr);
void mesh_host_free(void* p);
void mesh_pool_trim();  // frees the pool's idle buffers (vcy_destroy, when the last context goes)
// vcy_state.hip: counter widths, the lazy fill, vcy_reset, download / upload / positions / voxels, vcy_state_equal and
// the vcy_halo_* functions
int ensure_count_width(vcy_ctx* ctx, int64_t max_count);  // d_cnt wide enough for counts up to max_count
// d_cnt at `bytes` per counter, what it holds converted (vcy_set_param "lazycount") or, `keep_contents` false, dropped
int set_count_width(vcy_ctx* ctx, int bytes, bool keep_contents = true);
int count_width_for(const vcy_ctx* ctx, int64_t max_count);
int convert_counts(hipStream_t stream, const void* src, int src_bytes, void* dst, int dst_bytes, int64_t n);  // saturating
int fill_state(vcy_ctx* ctx);   // marks the slab fresh (lazy)
int materialize(vcy_ctx* ctx);  // writes the fresh state to HBM if it is still pending

}  // namespace vcy
