/*
 * vacancy_hip.h -- C-ABI of the MI355X-native voxel-carving hot path.
 *
 * This is the drop-in boundary.  The reference (unclearness/vacancy) has no FFI
 * layer of its own: its hot path is reached through the C++ class
 * vacancy::VoxelCarver (include/vacancy/voxel_carver.h:95-118).  Every entry
 * point below names the reference member/function it replaces; the C++ facade in
 * include/vacancy/ (this repo) keeps the reference's class API and forwards to
 * these symbols (see INTEGRATION.md for the exact binding).
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary;
 *   - every function returns VCY_OK (0) or a negative vcy_status; the text of the
 *     last error on the calling thread is vcy_last_error();
 *   - inputs are caller-owned and never retained past the call unless the
 *     function name says "_device" (then the pointer is a HIP device pointer that
 *     must stay valid until vcy_sync());
 *   - outputs that the library allocates are released with the matching *_free;
 *   - one context = one GPU = one caller thread.  A context owns a z-slab
 *     [z_begin, z_end) of the global grid (the whole grid when world size is 1).
 *     Every stage runs per slab -- carve, SDF producer, marching cubes, ExtractVoxel,
 *     mesh normals; what spans two slabs (shared-plane vertices, the normals of the
 *     vertices on a seam plane) is stitched on the host by vcy_merge_meshes_host.
 *   - there is NO CPU fallback: if no HIP device is usable, vcy_create fails.
 */
#ifndef VACANCY_HIP_H_
#define VACANCY_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vcy_status {
  VCY_OK = 0,
  VCY_ERR_INVALID_ARG = -1,   /* reference: `return false` + LOGE in Init()/Carve() */
  VCY_ERR_NOT_INITIALIZED = -2,
  VCY_ERR_TOO_MANY_VOXELS = -3,
  VCY_ERR_HIP = -4,           /* a HIP runtime call failed */
  VCY_ERR_NO_DEVICE = -5,
  VCY_ERR_UNSUPPORTED = -6,
  VCY_ERR_INTERNAL = -7       /* vcy_selftest: a device-side identity a fast path relies on does not hold */
} vcy_status;

/* vacancy::VoxelUpdate / SdfInterpolation / UpdateOutsideImage
 * (include/vacancy/voxel_carver.h:20-38) */
enum { VCY_UPDATE_MAX = 0, VCY_UPDATE_WEIGHTED_AVERAGE = 1 };
enum { VCY_INTERP_NN = 0, VCY_INTERP_BILINEAR = 1 };
enum { VCY_OUTSIDE_NONE = 0, VCY_OUTSIDE_MAX = 1 };
/* VCY_OUTSIDE_MAX: a voxel in front of the camera that projects outside the ROI samples max_sdf, which is exactly
 * *std::max_element over the WHOLE image buffer (voxel_carver.cc:436), not only its ROI:
 *   - if pixel 0 is a NaN, max_sdf is that NaN (nothing compares greater than it);
 *   - otherwise a NaN never wins, and of equal maxima the one with the lowest index does; +0 and -0 compare equal, so a
 *     zero maximum carries the sign of the first maximal zero;
 *   - +inf and -inf are values like any other (an image of -inf everywhere gives -inf).
 * Every carve entry point that honours update_outside resolves it this way, per view, on the device. */

/* vacancy::VoxelUpdateOption (voxel_carver.h:43-52), same defaults. */
typedef struct vcy_update_option {
  int32_t voxel_update;          /* VCY_UPDATE_*           default kMax      */
  int32_t sdf_interp;            /* VCY_INTERP_*           default kBilinear */
  int32_t update_outside;        /* VCY_OUTSIDE_*          default kNone     */
  int32_t voxel_max_update_num;  /*                        default 255       */
  float   voxel_update_weight;   /*                        default 1.0f      */
  int32_t use_truncation;        /* bool                   default false     */
  float   truncation_band;       /*                        default 0.1f      */
} vcy_update_option;

/* vacancy::VoxelCarverOption (voxel_carver.h:54-60). */
typedef struct vcy_carver_option {
  float bb_max[3];
  float bb_min[3];
  float resolution;              /* default 0.1f */
  int32_t sdf_minmax_normalize;  /* bool, default true */
  vcy_update_option update_option;
} vcy_carver_option;

/* Everything Carve() reads from `const Camera&` plus the ROI:
 *   w2c      = camera.w2c().cast<float>() (voxel_carver.cc:438), row-major 3x4
 *   fx,fy,cx,cy = PinholeCamera focal_length / principal_point (camera.cc:131-137)
 *   is_ortho = OrthoCamera::Project (camera.cc:201-205)
 *   roi_min/roi_max = the Vector2i arguments of Carve (voxel_carver.cc:415-416)
 *   width,height = sdf.width()/height() (image.h:65-74 layout: data[w*y+x]) */
typedef struct vcy_view {
  float   w2c[12];
  float   fx, fy, cx, cy;
  int32_t is_ortho;
  int32_t roi_min[2];
  int32_t roi_max[2];
  int32_t width, height;
} vcy_view;

/* Output of marching cubes: what MarchingCubes() hands to
 * Mesh::set_vertices / set_vertex_indices (marching_cubes.cc:223-224), plus the
 * dedup key of every vertex (the sorted voxel-id pair, marching_cubes.cc:78). */
typedef struct vcy_mesh {
  int64_t  n_vertices;
  int64_t  n_faces;
  float*   vertices;   /* 3 * n_vertices, xyz                         */
  int32_t* faces;      /* 3 * n_faces, indices into vertices          */
  int64_t* edge_keys;  /* 2 * n_vertices, (lower id, higher id), GLOBAL voxel ids; NULL with "meshkeys" 0 */
  /* Multi-GPU only (0 for a whole grid): the first n_foreign_vertices entries duplicate
   * vertices that the previous z-slab owns (edges on the shared plane z_begin-1); a merge
   * maps them onto that slab's numbering by edge key. */
  int64_t  n_foreign_vertices;
} vcy_mesh;

typedef struct vcy_ctx vcy_ctx;

/* ---- lifetime ----------------------------------------------------------- */

/* Replaces VoxelCarver::set_option + VoxelCarver::Init (voxel_carver.cc:373-392)
 * and VoxelGrid::Init (voxel_carver.cc:276-345): validates the options with the
 * reference's rules, sizes the grid n[i] = (int)((bb_max-bb_min)[i]/resolution),
 * allocates the slab z in [z_begin, z_end) on `device_id` (pass z_begin=0,
 * z_end=-1 for the whole grid) and sets sdf = lowest(), update_num = 0. */
int vcy_create(const vcy_carver_option* option, int device_id, int z_begin,
               int z_end, vcy_ctx** out);
void vcy_destroy(vcy_ctx* ctx);

/* VoxelGrid::voxel_num() (voxel_carver.cc:347): global dims (nx,ny,nz). */
int vcy_grid_dims(const vcy_ctx* ctx, int32_t dims[3]);
/* The z-range this context owns. */
int vcy_slab_range(const vcy_ctx* ctx, int32_t z_range[2]);
/* Grid dims without creating a context (host arithmetic of VoxelGrid::Init, voxel_carver.cc:278-301).  A box thinner
 * than one voxel along an axis gives dims[axis] = 0 and VCY_OK -- the reference builds an empty grid there --; only
 * vcy_create refuses it (there is nothing to put in HBM). */
int vcy_compute_dims(const float bb_min[3], const float bb_max[3],
                     float resolution, int32_t dims[3]);

/* Voxel::pos along one axis (0 = x, 1 = y, 2 = z): out[i], i < dims[axis], as VoxelGrid::Init computes it
 * (voxel_carver.cc:308-326) -- the same host arithmetic the device's axis tables are built with; needs no GPU. */
int vcy_axis_positions(const float bb_min[3], const float bb_max[3], float resolution, int axis, float* out);

/* ---- carving ------------------------------------------------------------ */

/* Replaces bool VoxelCarver::Carve(const Camera&, const Vector2i& roi_min,
 * const Vector2i& roi_max, const Image1f& sdf) (voxel_carver.cc:415-496).
 * `sdf_host` is row-major float[height*width]; it is copied before the call returns.  The view is
 * queued and applied later, in order (see "defer" under vcy_set_param); argument errors are reported
 * here.  A failure while applying queued views is returned by the call that applies them AND, if that
 * call was not a carve entry point (an extraction, a download), once more by the next vcy_carve* call,
 * so a `for each view: if (!Carve()) ...` loop sees it like the reference's bool Carve() would. */
int vcy_carve(vcy_ctx* ctx, const vcy_view* view, const float* sdf_host);
/* Same, SDF image already resident in HBM on the context's device (copied, ordered on the context's
 * stream: do not overwrite it before the stream has passed this call). */
int vcy_carve_device(vcy_ctx* ctx, const vcy_view* view, const float* sdf_device);
/* Replaces the loop of Carve(const std::vector<Camera>&, ...)
 * (voxel_carver.cc:516-528) for pre-built SDFs: fuses `n_views` views in
 * sequence order with the voxel state held in registers across views (up to 64
 * views per kernel launch, more are split).  The result is bit-identical to
 * n_views calls of vcy_carve_device.  The images are read while the launch runs:
 * keep them unchanged until the context's stream has passed this call. */
int vcy_carve_batch_device(vcy_ctx* ctx, int n_views, const vcy_view* views,
                           const float* const* sdf_device);
/* Replaces bool VoxelCarver::Carve(const Camera&, const Image1b& silhouette,
 * const Vector2i& roi_min, const Vector2i& roi_max, Image1f* sdf)
 * (voxel_carver.cc:394-413): MakeSignedDistanceField then the carve.
 * `sdf_out_host` (may be NULL) receives the SDF image like the Image1f* does. */
int vcy_carve_silhouette(vcy_ctx* ctx, const vcy_view* view,
                         const uint8_t* mask_host, float* sdf_out_host);

/* Replaces bool VoxelCarver::Carve(const std::vector<Camera>&, const std::vector<Image1b>&)
 * (voxel_carver.cc:516-528) end to end: every silhouette is uploaded (8 bit), turned into its SDF
 * on the device and fused, in chunks of 32 views; the upload + SDF build of chunk i+1 runs on a
 * second stream while chunk i is carved.  Result identical to n calls of vcy_carve_silhouette. */
int vcy_carve_batch_silhouettes(vcy_ctx* ctx, int n_views, const vcy_view* views,
                                const uint8_t* const* masks_host);

/* The same over the z-slabs of ONE grid held by this process (`slabs`: contexts of the same option set, any order, on
 * one or several devices -- vacancy::ShardedVoxelCarver::Carve): the devices SHARE the producer.  Device r of R uploads
 * and transforms the views r, r + R, ... of every chunk of 32; one ncclAllGather per chunk (librccl, the communicators
 * of vcy_halo_allgather) hands every device all the images of the chunk (width * height * 4 bytes each); every slab
 * carves the chunk from its device's copy while the next chunk is produced and gathered.  Slabs that share a device
 * share its images.  Same result as vcy_carve_batch_silhouettes on every slab -- where every GPU would build every
 * SDF (voxel_carver.cc:516-528 calls MakeSignedDistanceField once per view, :405-408).  One host thread per device
 * inside the call; vcy_last_stream_ms reports per slab.  VCY_ERR_UNSUPPORTED when several devices are involved and
 * librccl cannot be loaded (call vcy_carve_batch_silhouettes per slab then). */
int vcy_carve_batch_silhouettes_sharded(vcy_ctx* const* slabs, int n_slabs, int n_views, const vcy_view* views,
                                        const uint8_t* const* masks_host);

/* MakeSignedDistanceField (voxel_carver.cc:169-237, as Carve calls it at :405-408 with the context's options) for
 * n silhouettes in host memory into CALLER-owned device images (sdf_device_out[i]: width * height floats on the
 * context's device).  Returns when the images are complete.  The producer share of one rank of a one-process-per-GPU
 * job (vacancy_amd.dist.carve_silhouettes_sharded: build views r, r + G, ..., all-gather, carve). */
int vcy_make_sdf_batch_device(vcy_ctx* ctx, int n_views, const vcy_view* views, const uint8_t* const* masks_host,
                              float* const* sdf_device_out);

/* Of the last vcy_carve_batch_silhouettes: milliseconds its producer side took (per chunk of 32 views: the copy of the
 * silhouettes into page-locked staging, their DMA and the SDF build, events on the producer stream), its consumer
 * side (the fused carve launches, events on the context's stream), both summed over the chunks, and the call's wall
 * time.  max(produce, carve) / wall says how much of the shorter side was hidden behind the longer. */
int vcy_last_stream_ms(vcy_ctx* ctx, float* produce_ms, float* carve_ms, float* wall_ms);

/* Replaces void DistanceTransformL1(...) (voxel_carver.cc:102-167). */
int vcy_distance_transform_l1(const uint8_t* mask, int width, int height,
                              const int32_t roi_min[2], const int32_t roi_max[2],
                              float* dist_out);
/* Replaces void MakeSignedDistanceField(...) (voxel_carver.cc:169-237). */
int vcy_make_sdf(const uint8_t* mask, int width, int height,
                 const int32_t roi_min[2], const int32_t roi_max[2],
                 int minmax_normalize, int use_truncation, float truncation_band,
                 float* sdf_out);

/* MakeSignedDistanceField on the device: uploads the 8-bit mask, builds the SDF in HBM and returns
 * the device image (release with vcy_device_free); feed it to vcy_carve_device / _batch_device. */
int vcy_make_sdf_device(vcy_ctx* ctx, const uint8_t* mask_host, int width, int height,
                        const int32_t roi_min[2], const int32_t roi_max[2], int minmax_normalize,
                        int use_truncation, float truncation_band, float** sdf_device_out);

/* ---- robust carve: keep a voxel unless more than m views carve it ---------- */
/* No counterpart in the reference, whose arithmetic it reuses.  A visual hull is the intersection of the silhouettes: ONE
 * wrong mask (a blown segmentation, a blank frame, an object cut off at the image border) removes a real part of the
 * object.  The robust hull takes, per voxel, the (m + 1)-th largest sample over the views instead of the largest
 * (UpdateVoxelMax, voxel_carver.cc:78-86; positive = outside the silhouette): a voxel is carved only when MORE than m
 * views say outside.  An order statistic needs all views at once (the state keeps one number per voxel), so this is one
 * call over all of them, with a kernel of its own (carve_robust.hip).
 *
 * Inputs.  A context whose option has voxel_update == kMax (weighted average: VCY_ERR_INVALID_ARG); n_views in 1 .. 1024;
 * tolerate = m in 0 .. 3; n_views views with one SDF image each in device memory; an iso_level.  The call REPLACES the
 * context's state, as vcy_reset followed by a carve would: it does not combine with what was carved before.
 *
 * Samples.  For every owned voxel the views are visited in the order given.  View i contributes a sample d_i exactly when
 * the reference's loop (voxel_carver.cc:453-480) would reach its update: the voxel is not behind the camera; it is inside
 * the ROI, or update_outside == kMax gives max_sdf; and the truncation test does not drop it.  Projection, ROI test,
 * sampler and float operation order are those of every other carve entry point.  voxel_max_update_num is NOT applied:
 * its effect depends on the order of the views and has no meaning for an order statistic.  Every view's own is_ortho is
 * honoured: a call may mix the two camera models.
 *
 * Top list.  K = m + 1.  The list t[0 .. K-1] starts empty.  For each sample d, in view order:
 *   1. if the list holds fewer than K entries, append d; otherwise, if d > t[K-1], replace the last entry; if not, drop d;
 *   2. while the new entry has a predecessor t[j-1] and d > t[j-1], swap it upwards.
 * Only the comparison `>` is used, so NaN samples behave as in UpdateVoxelMax (a NaN never moves up and is never
 * displaced by the test); for K = 1 the procedure is exactly first touch followed by UpdateVoxelMax.  The view index of
 * every entry is carried beside its value.
 *
 * Result, with n samples:  n == 0: sdf = lowest(), update_num = 0 (the fill state).  n >= 1: sdf = t[min(K, n) - 1] --
 * the (m + 1)-th largest, or the smallest when fewer than m + 1 views see the voxel, which can therefore never be carved
 * -- and update_num = n.  update_num == 0 still implies sdf == lowest().  n can reach n_views: a context whose
 * voxel_max_update_num keeps its counters at one byte (<= 254) refuses more than 255 views.
 *
 * Blame.  overruled[i] (int64 per view; may be NULL) counts the owned voxels whose result satisfies (double)sdf < iso_level
 * and for which view i holds a discarded entry t[j], j < min(K, n) - 1, with (double)t[j] >= iso_level: the voxels kept
 * solid although view i says outside -- a bad mask shows as a count far above the others'.  Integer sums: exact and
 * independent of the schedule.  A z-slab context counts its own slices; the counts of slabs that cover a grid add up.
 *
 * Views queued by earlier per-view calls are applied first (their failure is returned); then the state is the call's:
 * halos, brick minima and component labels are stale, vcy_render_hull builds its bit planes again.  Refusals
 * (VCY_ERR_INVALID_ARG: tolerate outside 0 .. 3, n_views outside 1 .. 1024, weighted-average mode, null images, and what
 * vcy_carve_batch_device refuses in a view) leave the state and `overruled` untouched and set vcy_last_error().  The
 * images are read while the launch runs; the call returns when it has finished. */
int vcy_carve_robust_device(vcy_ctx* ctx, int n_views, const vcy_view* views, const float* const* sdf_device, int tolerate,
                            double iso_level, int64_t* overruled);
/* The same from silhouettes in host memory: MakeSignedDistanceField of all n_views on the device, with the context's
 * options (vcy_make_sdf_batch_device into images the call owns: width * height * 4 bytes per view at once), then
 * vcy_carve_robust_device. */
int vcy_carve_robust_silhouettes(vcy_ctx* ctx, int n_views, const vcy_view* views, const uint8_t* const* masks_host,
                                 int tolerate, double iso_level, int64_t* overruled);
/* Device milliseconds of the last robust carve's launch (events around the kernel; the SDF build is not in it). */
int vcy_last_robust_ms(const vcy_ctx* ctx, float* device_ms);

/* ---- carve from depth images: projective TSDF fusion ----------------------- */
/* No counterpart in the reference, whose projection, ROI test, nearest-neighbour pixel and update rules it reuses.  A
 * visual hull never recovers a concavity; a depth image does.  The sample of a voxel for a depth view is NOT a pixel of
 * a 2-D SDF: it depends on the voxel's own camera depth, depth(pixel) - z_c, truncated to a band -- the projective TSDF of
 * KinectFusion, which voxel_update = kWeightedAverage averages and kMax carves with.
 *
 * Inputs.  A context of either update mode; n_views >= 1 views with any mix of is_ortho; per view a depth image
 * float[height][width], row-major, with vcy_render_hull's meaning (camera depth z_c, +inf = the ray meets nothing); band
 * in world units, finite and > 0 with a finite 1.0f / band.  inv_band = 1.0f / band is computed once on the host, in float.
 *
 * Per owned voxel at (px, py, pz) the views are visited in the order given, and the running (sdf, update_num) is updated
 * exactly as by n_views calls of one view.  For view i:
 *   1. Gate.  Skip if update_num > voxel_max_update_num (voxel_carver.cc:447-450), tested on the running count.
 *   2. Projection.  pc[r] = t[r] + (R[r][0]*px + (R[r][1]*py + R[r][2]*pz)); skip if pc[2] < 0.  Pinhole:
 *      u = fx / pc[2] * pc[0] + cx, w = fy / pc[2] * pc[1] + cy; ortho: u = pc[0], w = pc[1].  The float operations of
 *      every carve kernel, so a voxel lands on the pixel it lands on in vcy_carve.
 *   3. ROI test.  inside = u >= roi_min.x && w >= roi_min.y && u <= roi_max.x && w <= roi_max.y (the ROI as float; a NaN
 *      coordinate is outside).  Skip when outside: update_outside is NOT read -- outside the image there is no measurement.
 *   4. Pixel.  xi = (int)roundf(u), yi = (int)roundf(w), each clamped into the ROI; Z = depth[yi][xi].  sdf_interp is NOT
 *      read: depth is never interpolated across a discontinuity.
 *   5. Validity.  The view contributes only if Z > 0.0f: NaN, 0 and negative values mean "no measurement"; +inf passes.
 *   6. Sample.  e = Z - pc[2]; d = e * inv_band (the product rounded on its own, no FMA); if d > 1.0f then d = 1.0f; the
 *      view contributes only if d >= -1.0f (a NaN is dropped, and so is a voxel more than one band behind the surface:
 *      occluded).  Positive = free space in front of the surface = "outside", the sign convention of the silhouette SDF,
 *      so depth views and silhouette views may be applied to the same state.  The truncation is always on; use_truncation
 *      and truncation_band of the option belong to the silhouette builder and are not read.
 *   7. Update.  First touch (update_num < 1: sdf = d, update_num = 1, voxel_carver.cc:482-486), else UpdateVoxelMax
 *      (:78-86) or UpdateVoxelWeightedAverage (:88-95) with the context's voxel_update_weight.
 *
 * Bookkeeping, as a per-view (non-fused) carve: views queued by earlier per-view calls are applied first (their failure is
 * returned); update counters widen as for any carve of n_views views; brick minima, halos and component labels become
 * stale, vcy_render_hull builds its bit planes again.  More than 64 views run as further launches of 64.  Refusals
 * (VCY_ERR_INVALID_ARG: a bad band, n_views < 1, a NULL image, and what vcy_carve_batch_device refuses in a view) leave
 * the state untouched and set vcy_last_error().
 *
 * The images are in the memory of the context's device and are read while the launches run; the call returns when they
 * have finished. */
int vcy_carve_depth_device(vcy_ctx* ctx, int n_views, const vcy_view* views, const float* const* depth_device, float band);
/* The same from images in host memory: uploads them (width * height * 4 bytes per view, all at once), then runs the
 * device path. */
int vcy_carve_depth(vcy_ctx* ctx, int n_views, const vcy_view* views, const float* const* depth_host, float band);
/* The definition, serial, on the host: no GPU, no context.  Works in place on sdf / update_num in vcy_download's layout
 * for the slices [z_begin, z_end) of the grid of `option` (x fastest, then y, then z - z_begin); the voxel positions are
 * vcy_axis_positions'.  The device path equals it bit for bit.  The same refusals; the arrays are then untouched. */
int vcy_carve_depth_host(const vcy_carver_option* option, int z_begin, int z_end, int n_views, const vcy_view* views,
                         const float* const* depth, float band, float* sdf, int32_t* update_num);
/* Device milliseconds of the last depth carve's launches (events around every kernel, summed; uploads are not in it). */
int vcy_last_depth_ms(const vcy_ctx* ctx, float* device_ms);

/* ---- surface extraction ------------------------------------------------- */

/* Replaces void VoxelCarver::ExtractIsoSurface(Mesh*, double iso_level,
 * bool linear_interp) (voxel_carver.cc:540-543) = MarchingCubes()
 * (marching_cubes.cc:63-228).  Vertex order and face order equal the
 * reference's serial scan (first reference in z,y,x order). */
int vcy_extract_iso(vcy_ctx* ctx, double iso_level, int linear_interp,
                    vcy_mesh* out);
/* Replaces void VoxelCarver::ExtractVoxel(Mesh*, bool inside_empty) (voxel_carver.cc:530-538 ->
 * extract_voxel.cc:258-317): one cube (24 vertices, 12 triangles) per kept voxel.  Runs on the
 * host on the downloaded state (the reference's drifting-cube arithmetic is serial by
 * construction); needs the whole grid in one context.  edge_keys is unused. */
int vcy_extract_voxel(vcy_ctx* ctx, int inside_empty, vcy_mesh* out);
/* The two halves of ExtractVoxel for a grid cut into z-slabs (vacancy::ShardedVoxelCarver::ExtractVoxel).
 * vcy_extract_voxel_ids: the parallel half on the device -- the keep predicate of every voxel of this context's slab
 * (extract_voxel.cc:283-286, or with inside_empty UpdateOnSurface :15-79; a slab above another one reads the slice below
 * its first from its halo: vcy_halo_allgather / _unpack / _install first) and the compaction -- returns the kept voxels'
 * GLOBAL ids in scan order (library-owned, vcy_ids_free; *ids_out = NULL when none is kept).
 * vcy_voxel_cubes: the serial half on the host, no GPU needed -- the reference translates ONE cube mesh to every kept
 * voxel and back (extract_voxel.cc:290-311), so every corner carries the rounding of all earlier kept voxels: the
 * slabs' lists, concatenated in z order, are walked with one drifting cube, and the mesh equals the single-context
 * vcy_extract_voxel array for array. */
int vcy_extract_voxel_ids(vcy_ctx* ctx, int inside_empty, int64_t** ids_out, int64_t* n_out);
void vcy_ids_free(int64_t* ids);
int vcy_voxel_cubes(const vcy_carver_option* option, int64_t n_ids, const int64_t* ids, vcy_mesh* out);
/* The same two calls writing into arrays of the CALLER: once the sizes are known -- 24 vertices and 12 triangles per kept
 * voxel -- `arrays` is called exactly once (not at all for an empty mesh; a non-zero return is passed on as
 * VCY_ERR_INTERNAL) and returns where 3 * n_vertices floats and 3 * n_faces int32 go; the host threads that fill them are
 * the first to touch them.  What a class API whose Mesh owns std::vectors wants (vacancy::VoxelCarver::ExtractVoxel: no
 * library-owned copy of an 800 MB mesh in between).  16-byte aligned arrays are written with streaming stores. */
typedef int (*vcy_mesh_arrays_fn)(void* user, int64_t n_vertices, int64_t n_faces, float** vertices, int32_t** faces);
int vcy_extract_voxel_into(vcy_ctx* ctx, int inside_empty, vcy_mesh_arrays_fn arrays, void* user);
int vcy_voxel_cubes_into(const vcy_carver_option* option, int64_t n_ids, const int64_t* ids, vcy_mesh_arrays_fn arrays,
                         void* user);

void vcy_mesh_free(vcy_mesh* mesh);
/* Milliseconds the device kernels of the last vcy_extract_iso took (hipEvents on the
 * context's stream: classify + owner + scan + emit; the mesh download is not included).
 * This is the region the reference's MarchingCubes timer brackets, minus the copy into Mesh. */
int vcy_last_extract_ms(const vcy_ctx* ctx, float* device_ms);
/* Milliseconds from the entry of the last vcy_extract_iso to its return, i.e. until the mesh arrays are
 * in host memory: the region the reference's MarchingCubes timer brackets (marching_cubes.cc:65-66,
 * 226-227).  The arrays of a vcy_mesh are page-locked host memory from a pool owned by the library. */
int vcy_last_extract_wall_ms(const vcy_ctx* ctx, float* wall_ms);

/* ---- normals of the iso surface ------------------------------------------ */

#define VCY_NORMALS_VERTEX 1
#define VCY_NORMALS_FACE   2
typedef struct vcy_mesh_normals {
  float* vertex_normals;  /* 3 * n_vertices or NULL */
  float* face_normals;    /* 3 * n_faces or NULL    */
} vcy_mesh_normals;
/* vcy_extract_iso plus Mesh::CalcNormal (mesh.cc:197-240) of its result, computed on the device.
 * `which` = bit set of VCY_NORMALS_*.  The mesh (positions, faces, keys, n_foreign_vertices) is bit for bit what
 * vcy_extract_iso returns; the normals' bits equal vcy_mesh_normals_host on that mesh: face normal =
 * ((p1 - p0).normalized() x (p2 - p0).normalized()).normalized(), vertex normal = the face normals of the faces that
 * name the vertex summed in ASCENDING FACE INDEX (once per corner), divided by their number, normalised -- float, with
 * the evaluation order of include/vacancy/linalg.h.  Two launches behind the extraction's last kernel: one thread per
 * face over the emitted arrays, and one thread per surface cell that sums, for every edge the cell owns, over the
 * cells around that edge in raster order (no atomics, no sorting).  The mesh is staged in device memory whatever
 * "mcdirect" says (the face kernel reads it there), so the call waits twice, like an extraction above that threshold.
 * The arrays are page-locked host memory of the library's pool: vcy_mesh_normals_free.  An empty mesh has none.
 * VCY_ERR_UNSUPPORTED for a context that does not own the whole grid (z_begin > 0 or z_end < nz): a vertex on a slab's
 * top or bottom plane has faces in the neighbouring slab -- vcy_extract_iso_normals_slab and the seam finish below, or
 * merge the slabs' meshes and use vcy_mesh_normals_host. */
int vcy_extract_iso_normals(vcy_ctx* ctx, double iso_level, int linear_interp, int which,
                            vcy_mesh* out, vcy_mesh_normals* normals_out);
/* The same for a context that owns a z-slab [z_begin, z_end) (any context: for a whole grid the mesh and the normals
 * are exactly vcy_extract_iso_normals').  The mesh is bit for bit vcy_extract_iso's on that context.  The face normals
 * are final.  The vertex normals are final for every vertex all of whose faces lie in this slab, i.e. all but the SEAM
 * vertices: those on x- or y-axis edges in the plane of slice z_begin - 1 that cells of the slab below own (this slab's
 * first n_foreign_vertices) and, when z_end < nz, those on such edges in the plane of slice z_end - 1 (the foreign
 * vertices of the slab above).  Their faces lie in two slabs and a float sum cannot be continued as a lump, so their
 * entries are zero here and vcy_merge_meshes_host finishes them:
 *   1. the slabs' normals concatenated with the merged numbering (a slab's foreign entries dropped, like its vertices);
 *   2. per seam, vcy_mesh_normals_seam_sum (or vcy_mesh_normals_host_seam) on the MERGED arrays with the face range
 *      [first face of the upper slab - layer_faces[1] of the lower slab, first face of the upper slab + layer_faces[0]
 *      of the upper slab) and the merged ids the upper slab's foreign vertices were mapped to by edge key.
 * layer_faces[0] / [1] = the numbers of faces of the slab's first / last own cell layer (both n_faces for a slab of one
 * cell layer): the last layer's faces are the end of the slab's face array, the next slab's first layer's the start of
 * its own, and together they hold every face that names a vertex of the seam between them.
 * A slab needs "meshkeys" 1 (VCY_ERR_INVALID_ARG otherwise) and its halo installed, as for vcy_extract_iso. */
int vcy_extract_iso_normals_slab(vcy_ctx* ctx, double iso_level, int linear_interp, int which, vcy_mesh* out,
                                 vcy_mesh_normals* normals_out, int64_t layer_faces[2]);
void vcy_mesh_normals_free(vcy_mesh_normals* n);
/* Device milliseconds of the normals launches of the last vcy_extract_iso_normals (0 after vcy_extract_iso);
 * vcy_last_extract_ms stays the mesh kernels alone. */
int vcy_last_normals_ms(const vcy_ctx* ctx, float* device_ms);
/* Mesh::CalcFaceNormal + Mesh::CalcNormal (mesh.cc:197-240) on raw arrays, serial, on the host (no GPU needed).
 * face_normals (3*n_faces) and/or vertex_normals (3*n_vertices) may be NULL.  A vertex no face names gets 0 / 0 = NaN,
 * as in the reference.  VCY_ERR_INVALID_ARG when a face names a vertex outside [0, n_vertices). */
int vcy_mesh_normals_host(int64_t n_vertices, int64_t n_faces, const float* vertices,
                          const int32_t* faces, float* vertex_normals, float* face_normals);
/* The seam finish (host only, no GPU needed): Mesh::CalcFaceNormal of the faces [face_begin, face_end) and Mesh::CalcNormal's
 * sum in ascending face index, division and normalisation for the n_seam listed vertices ONLY, with the arithmetic of
 * vcy_mesh_normals_host; vertex_normals (3 * n_vertices, in-out) changes at the listed vertices and nowhere else.  The
 * range must hold every face that names a listed vertex.  n_seam = 0 is a no-op.  VCY_ERR_INVALID_ARG for a listed id or
 * a vertex named by a face of the range outside [0, n_vertices), or a range that is not 0 <= face_begin <= face_end. */
int vcy_mesh_normals_host_seam(int64_t n_vertices, const float* vertices, const int32_t* faces, int64_t face_begin,
                               int64_t face_end, int64_t n_seam, const int64_t* seam_vertex_ids, float* vertex_normals);
/* The same finish from face normals that exist already: face_normals (3 floats per face of the MERGED mesh, the slabs'
 * device results concatenated) instead of the positions.  For a mesh without NaN the two calls give the same bits.  A
 * mesh over NaN voxels has NaN face normals of either sign; this call takes the devices' own and adds them as the
 * vertex normals kernel does (of two NaNs the later term's), so that the seam vertices equal the whole-grid context's
 * to the bit there as well.  vcy_merge_meshes_host uses this one.  Errors as above. */
int vcy_mesh_normals_seam_sum(int64_t n_vertices, const int32_t* faces, const float* face_normals, int64_t face_begin,
                              int64_t face_end, int64_t n_seam, const int64_t* seam_vertex_ids, float* vertex_normals);
/* The stitch of the meshes of a grid cut into z-slabs (host only, no GPU, no context): `slabs` = the n_slabs meshes in z
 * order as vcy_extract_iso / vcy_extract_iso_normals_slab return them.  Own vertices keep their order and a slab's first
 * n_foreign_vertices are dropped; a face corner that names one is re-pointed, by the vertex's edge key, to the own vertex
 * with that key of the slab directly below.  The result is array for array the mesh of one context holding the grid.
 * The arrays are the caller's, and their sizes follow from the structs alone:
 *   merged vertices V = sum over the slabs of (n_vertices - n_foreign_vertices), merged faces F = sum of n_faces;
 *   vertices 3 * V floats, faces 3 * F int32, edge_keys 2 * V int64 or NULL (not wanted).
 * `normals` (one struct per slab, both arrays of every slab that has vertices / faces) and `layer_faces` (2 * n_slabs,
 * the pair vcy_extract_iso_normals_slab returned per slab) are given together or both NULL.  Given, vertex_normals
 * (3 * V) and face_normals (3 * F) receive steps 1 and 2 above: Mesh::CalcNormal of the merged mesh, to the bit what
 * vcy_extract_iso_normals returns on the whole grid.  Not given, the two must be NULL.  An array of no elements may be NULL.
 * VCY_ERR_INVALID_ARG, with the slab named in vcy_last_error(): a negative count or n_foreign_vertices > n_vertices, a
 * null array, foreign vertices in slab 0 or without edge keys, normals missing for a slab, a layer_faces entry outside
 * [0, n_faces], V > INT32_MAX, a foreign key without an owner in the slab below (the key is named) -- all found before
 * the first write, the output arrays are untouched -- and a face that names a vertex outside its slab's, found while
 * the faces are written: the output arrays are unspecified after that one. */
int vcy_merge_meshes_host(int n_slabs, const vcy_mesh* slabs, const vcy_mesh_normals* normals, const int64_t* layer_faces,
                          float* vertices, int32_t* faces, int64_t* edge_keys, float* vertex_normals, float* face_normals);

/* ---- connected components of the hull ------------------------------------ */

/* 6-connected components of the SOLID voxels, labelled on the device (no reference counterpart: what a
 * shape-from-silhouette user otherwise does on the host with the downloaded grid, to drop the phantom volumes and specks
 * a visual hull of few views has).
 *   solid voxel : update_num >= 1 && (double)sdf < iso_level -- marching cubes' own comparison (marching_cubes.cc:121-128);
 *                 an untouched voxel (sdf = lowest(), update_num = 0) and a NaN are not solid;
 *   adjacency   : the six axis neighbours inside the grid (the adjacency of marching cubes' edges);
 *   label       : the smallest global voxel id (z*nx*ny + y*nx + x) of the component;
 *   order       : n_voxels descending, ties by label ascending; "the k largest" are the first k of it.
 * The results are therefore exact and independent of how the kernels were scheduled. */
typedef struct vcy_component {   /* 40 bytes */
  int64_t label;                 /* smallest global voxel id of the component */
  int64_t n_voxels;
  int32_t bb_min[3], bb_max[3];  /* inclusive voxel-index bounds, x y z */
} vcy_component;

/* Applies queued ("defer") views, labels, and returns the list in the order above (library-owned:
 * vcy_components_free; *out = NULL and *n_out = 0 when no voxel is solid).  The state is not changed; a context
 * nothing has been carved into since vcy_create / vcy_reset returns the empty list without its lazy fill being
 * written.  Labels take 4 bytes per voxel of device memory (kept by the context): VCY_ERR_TOO_MANY_VOXELS above
 * 2^31 - 1 voxels.  VCY_ERR_UNSUPPORTED, with the state untouched, for a context that does not own the whole grid
 * (z_begin > 0 or z_end < nz): a component may continue in the neighbouring slab -- vcy_label_components_slab and the
 * seam merge below are the calls for a grid cut into z-slabs. */
int  vcy_label_components(vcy_ctx* ctx, double iso_level, vcy_component** out, int64_t* n_out);
void vcy_components_free(vcy_component* components);
/* label of every voxel of the LAST vcy_label_components / vcy_keep_components on this context,
 * -1 for a voxel that is not solid; nx*ny*nz entries, reference order (a z-slab: nx*ny*(z_end - z_begin), global ids).
 * For vcy_keep_components these are the labels BEFORE its removal.  VCY_ERR_INVALID_ARG before any labelling. */
int  vcy_download_labels(vcy_ctx* ctx, int64_t* labels);
/* Labels, then keeps a component iff (keep_largest <= 0 or its rank in the order above is below keep_largest) and
 * n_voxels >= min_voxels.  Every voxel of every other component gets sdf = fill_sdf; update_num and every other
 * byte of the state stay.  fill_sdf must be finite with (double)fill_sdf >= iso_level (VCY_ERR_INVALID_ARG
 * otherwise): a removed voxel is then outside for marching cubes and so are all its axis neighbours (outside,
 * removed too, or untouched -- and cells with an untouched corner are skipped), so fill_sdf is never interpolated.
 * The brick minima stay what they were: valid ones are reduced again by the kernel that rewrites a brick, so brick
 * skipping in vcy_extract_iso and the live list of the next carve survive -- which a vcy_download / vcy_upload round
 * trip would lose.  removed_components / removed_voxels (either may be NULL): what went.
 * VCY_ERR_UNSUPPORTED, state untouched, for a context that does not own the whole grid (see above;
 * vcy_keep_components_slab is the filter of a z-slab). */
int  vcy_keep_components(vcy_ctx* ctx, double iso_level, int keep_largest, int64_t min_voxels,
                         float fill_sdf, int64_t* removed_components, int64_t* removed_voxels);
/* Milliseconds between HIP events on the context's stream around the kernels of the last vcy_label_components /
 * vcy_keep_components (solid bits, run labels, merge, flatten, statistics and, for the latter, the filter), the
 * two short host waits for the number of roots and their sorted list included; 0 when nothing was launched. */
int  vcy_last_components_ms(const vcy_ctx* ctx, float* device_ms);

/* ---- connected components of a grid cut into z-slabs ---------------------- */

/* The same definitions for contexts that each own a z-slab [z_begin, z_end) of one grid (any devices, one process or
 * one per GPU).  Every slab labels its own slices on its device; what crosses a seam is ONE plane of labels
 * (nx * ny int64, through host memory) and a list of label pairs, never a slab's label volume; the host joins the
 * pieces.  Per-voxel storage stays 32 bits per SLAB (VCY_ERR_TOO_MANY_VOXELS above 2^31 - 1 voxels in one slab) while
 * everything that leaves a context is a 64-bit global voxel id, so a grid of more than 2^31 voxels can be labelled
 * in slabs.  The merged list and the merged per-voxel labels equal what vcy_label_components returns on one context
 * holding the whole grid, wherever the grid is cut.  Order of calls, slabs in z order s = 0 .. S - 1:
 *   1. vcy_label_components_slab on every slab: the slab's own pieces with PROVISIONAL labels -- z_begin * nx * ny + the
 *      smallest slab-local id of the piece, i.e. its smallest global id -- and boxes in global z;
 *   2. vcy_component_top_plane on slabs 0 .. S - 2, vcy_component_seam_pairs on slabs 1 .. S - 1 with the plane of the
 *      slab below: (label below, label above) for the pieces that touch across the seam;
 *   3. vcy_merge_components_host (no GPU): the merged list and, per slab, the global label of every piece;
 *   4. vcy_resolve_components_slab on every slab installs its map: vcy_download_labels then returns merged labels;
 *   5. for the filter, vcy_select_components_host (no GPU) says which pieces go, and vcy_keep_components_slab on every slab
 *      takes its own.
 * Steps 2, 4 and 5 speak about the state step 1 labelled: after a carve, vcy_upload or vcy_reset they return
 * VCY_ERR_INVALID_ARG until the slab is labelled again.  A slab's halo below an upper slab is stale after step 5, as
 * after a carve, and the library enforces it in the same way: every successful vcy_keep_components_slab on an upper
 * slab marks its halo as not installed -- also when this slab itself removed nothing, because the slab below may have
 * --, and vcy_extract_iso* and the on-surface vcy_extract_voxel_ids then refuse ("halo slices not installed", the
 * error they return after a carve) until the halos are exchanged again (vcy_halo_allgather, ...), which every sharded extractor does
 * anyway. */

/* vcy_label_components on the slices this context owns (any context: on a whole grid the list is exactly
 * vcy_label_components').  Applies queued views; the state is not changed; a context nothing has been carved into
 * since vcy_create / vcy_reset returns the empty list without its lazy fill being written.  Drops a map installed
 * earlier: vcy_download_labels returns the provisional labels until step 4. */
int  vcy_label_components_slab(vcy_ctx* ctx, double iso_level, vcy_component** out, int64_t* n_out);
/* The provisional labels of this slab's last slice z_end - 1 (nx * ny entries, -1 where not solid): what the slab
 * above needs.  VCY_ERR_INVALID_ARG before vcy_label_components_slab. */
int  vcy_component_top_plane(vcy_ctx* ctx, int64_t* plane_labels);
/* On the UPPER slab of a seam: `below_plane_labels` (host memory, nx * ny) is vcy_component_top_plane of the slab that
 * ends at this context's z_begin.  Uploads it and compares it on the device with this slab's own labels of slice
 * z_begin; returns 2 * n int64 -- (label below, label above) per pair, sorted, every pair once -- library-owned
 * (vcy_seam_pairs_free; NULL and 0 when nothing touches).  VCY_ERR_INVALID_ARG for a context with z_begin == 0 (no seam
 * below it) or one that has not been labelled.  vcy_last_components_ms afterwards: this call's device time. */
int  vcy_component_seam_pairs(vcy_ctx* ctx, const int64_t* below_plane_labels, int64_t** pairs_out, int64_t* n_pairs_out);
void vcy_seam_pairs_free(int64_t* pairs);
/* The seam merge, host arithmetic only (no GPU needed).  `lists`: the slabs' lists of step 1 one behind the other in z
 * order, n_lists[s] entries of slab s; `pairs`: the seams' pair lists one behind the other, n_pairs[s] pairs (2 int64
 * each) for the seam between slabs s and s + 1 -- duplicates allowed, either array NULL when empty.  Union-find over the
 * labels: a merged component's label is the smallest provisional label of its set (= its smallest global voxel id),
 * n_voxels are summed, boxes joined.  merged_out: the list in the order of vcy_label_components (library-owned,
 * vcy_components_free; NULL when empty); global_labels[i]: the merged label of entry i of `lists` (caller-allocated, sum
 * of n_lists entries).  VCY_ERR_INVALID_ARG for a pair that names a label its slab did not report (first number: slab
 * s, second: slab s + 1), a label a slab reports twice, or a negative count. */
int  vcy_merge_components_host(int n_slabs, const vcy_component* lists, const int64_t* n_lists, const int64_t* pairs,
                               const int64_t* n_pairs, vcy_component** merged_out, int64_t* n_merged_out,
                               int64_t* global_labels);
/* Installs this slab's part of the merge: n = the number of pieces step 1 reported, every one of them named once in
 * provisional_labels, with its merged label.  VCY_ERR_INVALID_ARG, nothing installed, for another count, a label the
 * slab did not report or names twice, or a merged label that is negative or above the piece's own. */
int  vcy_resolve_components_slab(vcy_ctx* ctx, int64_t n, const int64_t* provisional_labels, const int64_t* global_labels);
/* The filter of vcy_keep_components on a slab: every voxel of the listed pieces (provisional labels of step 1) gets
 * sdf = fill_sdf, in place, over the slab's own 8 x 8 x 8 bricks; update_num and every other byte of the state stay;
 * valid brick minima are reduced again in the bricks that changed and only there.  Which pieces go is the caller's
 * decision on the MERGED list (vcy_select_components_host).  fill_sdf: finite and not below the iso level of step
 * 1, VCY_ERR_INVALID_ARG otherwise, as for a label the slab did not report or a slab that has not been labelled --
 * state untouched in every such case.  vcy_download_labels afterwards: the labels from before the removal; a second
 * filter needs a new labelling.  removed_voxels may be NULL.  vcy_last_components_ms: the filter's device time. */
int  vcy_keep_components_slab(vcy_ctx* ctx, float fill_sdf, int64_t n_remove, const int64_t* remove_provisional_labels,
                              int64_t* removed_voxels);
/* The rule of vcy_keep_components, host arithmetic only (no GPU, no context): of `components`, a list in the order of
 * vcy_label_components, entry i stays iff (keep_largest <= 0 or i < keep_largest) and n_voxels >= min_voxels.
 * removed[i] = 1 where it goes, 0 where it stays (caller-allocated, n_components entries); removed_components /
 * removed_voxels (either may be NULL): what went.  With the global_labels of vcy_merge_components_host as
 * piece_global_labels (n_pieces entries, the slabs' pieces one behind the other), piece_removed[k] = 1 iff piece k belongs
 * to a component that goes: slab s then hands vcy_keep_components_slab the provisional labels of its flagged pieces.
 * Callers without pieces pass NULL, 0, NULL.  fill_sdf is not this call's business: every filter checks it before
 * anything is labelled.  VCY_ERR_INVALID_ARG for a negative count or a NULL array with a positive one. */
int  vcy_select_components_host(const vcy_component* components, int64_t n_components, int keep_largest, int64_t min_voxels,
                                uint8_t* removed, int64_t* removed_components, int64_t* removed_voxels,
                                const int64_t* piece_global_labels, int64_t n_pieces, uint8_t* piece_removed);

/* ---- distance field of the hull ------------------------------------------- */

/* The voxel state after a carve is no distance field: a kMax context holds the maximum over the views of 2-D silhouette
 * distances in image units, a weighted-average context a blend of them.  These calls give every voxel its Euclidean
 * distance to the surface of the hull, exact up to a cap, in integers (no reference counterpart).
 *   solid     update_num >= 1 && (double)sdf < iso_level -- the labelling's predicate; an untouched voxel and a NaN are
 *             not solid;
 *   touched   update_num >= 1;
 *   d2(v)     for a voxel v of class c (solid or not solid): the minimum of dx*dx + dy*dy + dz*dz, in voxel indices, over
 *             all voxels INSIDE THE GRID of the other class.  Untouched voxels count as not solid; nothing outside the grid
 *             counts as anything, so a solid block that touches the grid's border is not "near the outside" on that side;
 *   radius    an integer R, 1 <= R <= 127 (VCY_ERR_INVALID_ARG otherwise, nothing touched).  A d2 <= R*R is exact; a
 *             larger one, and "no voxel of the other class at all", is reported as FAR = R*R + 1;
 *   field     int32 per voxel in reference order (z*nx*ny + y*nx + x): -d2 for a solid voxel, +d2 for any other.  d2 >= 1
 *             always, so the sign is never ambiguous;
 *   phi       the metric value: with d2c = min(d2, R*R) as a float (exact), phi = (sqrtf(d2c) - 0.5f) * resolution, every
 *             operation rounded once, nothing contracted; negated for a solid voxel (inside is negative here).  A solid
 *             voxel next to one that is not gets -0.5 * resolution and its neighbour +0.5 * resolution: marching cubes at
 *             iso 0 with linear interpolation puts the surface half-way between the two.
 * The evaluation is separable and exact under the cap:
 *   x pass  g(x,y,z) = the squared distance along the row to the nearest voxel of the other class, or FAR when there is
 *           none within R;
 *   y pass  h = min over |dy| <= R, y + dy inside the grid, of (class(x,y+dy,z) != c ? 0 : g(x,y+dy,z)) + dy*dy;
 *   z pass  the y pass over h, along z; then every value > R*R becomes FAR.
 * "0 where the neighbour is itself of the other class" makes ONE field and the solid bits enough for both signs.  The
 * device, the host function below and the numpy restatement of the tests give the same integers and the same float bits. */

/* Applies queued views, builds the signed integer field on the device and copies it to d2_host (nx*ny*nz int32).  Reads
 * the state and declares nothing: brick minima, bit planes, labellings and halos stay what they were.  A context nothing
 * has been carved into since vcy_create / vcy_reset returns +FAR everywhere without its lazy fill being written.  Device
 * memory kept by the context: 1 bit + 1 + 2 bytes of scratch and the 4 bytes of the field per voxel.
 * VCY_ERR_UNSUPPORTED, state untouched, for a context that does not own the whole grid (the transform of a z-slab needs
 * R slices of its neighbours per seam). */
int vcy_distance_field(vcy_ctx* ctx, double iso_level, int radius, int32_t* d2_host);
/* A state WRITER: every touched voxel gets sdf = phi (negated where solid) of the field above; update_num, untouched
 * voxels and every other byte of the state stay as they were.  *n_rewritten (may be NULL): the touched voxels.  A context
 * known to hold no touched voxel (nothing carved since vcy_create / vcy_reset, or an upload of zero counts) launches
 * nothing, declares nothing and reports 0.  Afterwards vcy_extract_iso at iso +r is the hull grown by r, at -r the hull
 * shrunk by r, at 0 the hull itself -- valid for |r| < (R - 0.5) * resolution, beyond which the cap shows.  The brick
 * minima are LOST (the final kernel works on columns along z, not on bricks, and does not reduce them again): the next
 * extraction reads every brick and the next fused carve rebuilds them.  Bit planes of the ray-cast, a slab labelling and
 * the halo are stale as after any write.  Views carved afterwards mix image-unit samples into a metric field: that is
 * the caller's business.  VCY_ERR_UNSUPPORTED, state untouched, for a context that does not own the whole grid. */
int vcy_redistance(vcy_ctx* ctx, double iso_level, int radius, int64_t* n_rewritten);
/* The definition, serial, on the host: no GPU, no context.  sdf / update_num in vcy_download's layout for the whole grid
 * of `option`; d2: the signed integer field (may be NULL); sdf_out (may be NULL, may be sdf itself): the state's sdf
 * after vcy_redistance -- phi where touched, the input's bits elsewhere.  The device calls equal it bit for bit. */
int vcy_distance_field_host(const vcy_carver_option* option, const float* sdf, const int32_t* update_num, double iso_level,
                            int radius, int32_t* d2, float* sdf_out);
/* Device milliseconds between HIP events around the launches (solid bits, the three passes) of the last
 * vcy_distance_field (its copy to the host not included) or vcy_redistance on this context; 0 when nothing was launched. */
int vcy_last_distance_ms(const vcy_ctx* ctx, float* device_ms);
/* Closing the hull (VoxelCarver::CloseHull, vacancy_amd.carver.VoxelCarver.CloseHull and their z-slab forms): three
 * steps composed by the front end, on the plan of vcy_close_hull_plan.  With r = radius_voxels * resolution and
 * R = ceil(radius_voxels) + 2,
 *   vcy_redistance(iso_level, R), vcy_redistance(r, R), vcy_redistance(-r, R)
 * -- the metric field, the field of the hull grown by r, the field of that shrunk by r again: the state ends as the
 * metric field of the closed hull with its surface at iso 0.  Tie rule: a voxel is dilated when phi < r, that is
 * sqrt(d2) < radius_voxels + 0.5.  When (radius_voxels + 0.5)^2 is an integer that is a sum of three squares, voxels sit
 * exactly on both thresholds and `<` sends the growing and the shrinking step the same way: the closing is then no
 * longer extensive (with 1.5 voxels, two 5^3 blocks two voxels apart shrink from 250 solid voxels to 90; with 1.3 exactly
 * the 50 gap voxels are filled).  Such radii are refused; pick 1.3, 2.3, ...
 * vcy_close_hull_plan (host arithmetic only: no GPU, no context): *r and *big_r = R for 0 < radius_voxels with R <= 127;
 * VCY_ERR_INVALID_ARG, with the reason and a radius to pick instead in vcy_last_error, outside that range and for a
 * radius that ties ((radius_voxels + 0.5)^2 within 1e-9 of such an integer).  radius_voxels is a double: a float
 * argument is passed widened, and decides as it did as a float. */
int vcy_close_hull_plan(double radius_voxels, float resolution, double* r, int* big_r);

/* The same field for a grid cut into z-slabs.  The x pass and the y pass never leave an xy slice; only the z pass looks
 * across a seam, R slices deep, and what it needs from there is the y pass's output
 *   h(v) = class(v) << 15 | the y pass's value (1 .. FAR, 15 bits), uint16, nx*ny per slice ("a plane").
 * The order of the calls, every slab finishing one step before any slab begins the next:
 *   1. vcy_distance_slab_begin on every slab;
 *   2. vcy_distance_slab_planes: every slab hands out its lowest and its highest min(R, own slices) planes; the host puts
 *      together, for slab [z0, z1), the planes of the global slices [z0 - min(R, z0), z0) and [z1, z1 + min(R, nz - z1)),
 *      from as many neighbours as that takes (vcy_distance_halo_host);
 *   3. vcy_distance_field_slab or vcy_redistance_slab on every slab.
 * With exactly those planes at the ends of the slab's columns the z pass's bounds are the whole grid's own for every
 * step <= R: the results equal vcy_distance_field / vcy_redistance of one context for the slab's slices, bit for bit.
 *
 * Step 1: applies queued views, runs the solid bits, the x pass and the y pass over the slab's OWN slices and keeps h in
 * the context's distance pool (2 bytes per voxel of the slab and of the planes to come), tagged with (iso_level, radius,
 * the state as it is now).  Reads the state and declares nothing; the context's 2 halo slices are not looked at.  A
 * context nothing has been carved into since vcy_create / vcy_reset gets class 0, FAR everywhere without its lazy fill
 * being written.  radius as above.  Works on a context that owns the whole grid too (no planes at either end).  A second
 * call replaces the tag. */
int vcy_distance_slab_begin(vcy_ctx* ctx, double iso_level, int radius);
/* Step 2: the kept planes of the global slices [z_begin, z_end), which must lie among the context's own, to h_host in
 * slice order.  VCY_ERR_INVALID_ARG without a vcy_distance_slab_begin, or when the state has been written (or a view
 * queued) since. */
int vcy_distance_slab_planes(const vcy_ctx* ctx, int z_begin, int z_end, uint16_t* h_host);
/* Step 3.  below: the planes of the global slices [z0 - n_below, z0), above: [z1, z1 + n_above), both in ascending z;
 * n_below == min(R, z0) and n_above == min(R, nz - z1) with the R of step 1, and the tag of step 1 still describes the
 * state -- VCY_ERR_INVALID_ARG with nothing touched otherwise.  A pointer may be NULL where its count is 0.
 * vcy_distance_field_slab: the signed field of the slab's slices (nx*ny*(z1 - z0) int32) to d2_host; reads the state's
 * tag only and declares nothing.
 * vcy_redistance_slab: a state WRITER, exactly vcy_redistance for the slab's slices -- sdf = +-phi where update_num >= 1,
 * *n_rewritten (may be NULL) the touched voxels, brick minima lost, halo stale; a context known to hold no touched voxel
 * launches nothing, declares nothing and reports 0.  The write ends the tag: another step 1 precedes another step 3.
 * vcy_last_distance_ms after any of step 1 and step 3: the launches of that call (step 1: solid bits, x pass, y pass;
 * step 3: the z pass; the copies of planes not included). */
int vcy_distance_field_slab(vcy_ctx* ctx, const uint16_t* below, int n_below, const uint16_t* above, int n_above,
                            int32_t* d2_host);
int vcy_redistance_slab(vcy_ctx* ctx, const uint16_t* below, int n_below, const uint16_t* above, int n_above,
                        int64_t* n_rewritten);
/* The two halves serially on the host: no GPU, no context; they share their arithmetic with vcy_distance_field_host,
 * which is the two over the whole grid.  sdf_slab / update_num_slab: vcy_download's layout for the slices [z_begin, z_end)
 * of the grid of `option`.  planes: h of those slices.  finish: d2 (may be NULL) the signed field of the slab, sdf_out (may
 * be NULL, may be sdf_slab itself) the slab's sdf after vcy_redistance_slab; sdf_slab and update_num_slab may be NULL when
 * sdf_out is.  The counts n_below / n_above are checked as in step 3. */
int vcy_distance_slab_planes_host(const vcy_carver_option* option, int z_begin, int z_end, const float* sdf_slab,
                                  const int32_t* update_num_slab, double iso_level, int radius, uint16_t* h);
int vcy_distance_slab_finish_host(const vcy_carver_option* option, int z_begin, int z_end, const uint16_t* h,
                                  const uint16_t* below, int n_below, const uint16_t* above, int n_above, int radius,
                                  const int32_t* update_num_slab, const float* sdf_slab, int32_t* d2, float* sdf_out);
/* Step 2's assembly, host copies only (no GPU, no context).  The grid's n_slabs slabs are [z_bounds[s], z_bounds[s + 1]),
 * n_slabs + 1 bounds ascending from 0; bottoms[s] / tops[s]: the lowest / highest min(radius, own slices) planes of slab s,
 * plane_voxels = nx*ny uint16 each, in ascending z.  For slab `slab` = [z0, z1): *n_below = min(radius, z0) and
 * *n_above = min(radius, nz - z1), and the planes of the global slices [z0 - *n_below, z0) to `below`, [z1, z1 + *n_above)
 * to `above` (caller-allocated; NULL allowed where the count is 0), from as many neighbours as that takes -- a slab thinner
 * than the radius passes its neighbours' planes on.  Edge planes nobody reads may be NULL: the bottom of slab 0, the top of
 * the last slab, and for one `slab` everything out of its reach.  VCY_ERR_INVALID_ARG for bounds that do not ascend from 0,
 * a slab index out of range, a needed edge pointer that is NULL (the buffers then hold nothing to rely on), a radius outside
 * [1, 127] or plane_voxels < 1. */
int vcy_distance_halo_host(int n_slabs, const int32_t* z_bounds, int radius, int64_t plane_voxels,
                           const uint16_t* const* bottoms, const uint16_t* const* tops, int slab, uint16_t* below,
                           uint16_t* above, int* n_below, int* n_above);

/* ---- ray-cast of the hull into a view ------------------------------------- */

/* What the hull looks like from a camera: per pixel, the first SOLID voxel on the pixel's ray (no reference counterpart:
 * the reference's Camera carries ray_w / org_ray_w, camera.cc:164-261, and nothing uses them).  Every rule below is
 * float arithmetic in a fixed order, so the images are exact and independent of how a kernel walks the grid.
 *   solid voxel : update_num >= 1 && (double)sdf < iso_level, the predicate of vcy_label_components; an untouched voxel
 *                 and a NaN are not solid.
 *   cell        : voxel i of axis a is the interval between the planes P_a[i] and P_a[i + 1] of vcy_cell_planes.
 *   ray         : of pixel (u, v), integer pixel coordinates -- where the carve samples data[w * v + u] --, the
 *                 camera-space points the carve's own projection sends to that pixel, by camera depth t = z_c >= 0:
 *                   pinhole  o_c = (0, 0, 0),  d_c = (((float)u - cx) / fx, ((float)v - cy) / fy, 1);
 *                   ortho    o_c = ((float)u, (float)v, 0),  d_c = (0, 0, 1) -- the inverse of OrthoCamera::Project
 *                            (camera.cc:196-212), which the carve uses, NOT the reference's org_ray_c, which is offset
 *                            by half the image;
 *                 world ray, with R[r][c] = w2c[4 * r + c] taken as orthonormal and t_w2c[r] = w2c[4 * r + 3]:
 *                   q = o_c - t_w2c (q_2 = 0.0f - t_w2c[2]),
 *                   o_a = R[0][a] * q_0 + R[1][a] * q_1 + R[2][a] * q_2,
 *                   d_a = R[0][a] * d_c0 + R[1][a] * d_c1 + R[2][a] * 1.0f     (products summed left to right).
 *                 A ray with a non-finite component of o or d is a miss.
 *   crossing    : axis a has crossings when d_a != 0 and inv_a = 1.0f / d_a is finite; plane k is crossed at
 *                 t_a(k) = (P_a[k] - o_a) * inv_a -- from the integer k, never accumulated; t_a is monotone in k.
 *   start       : crossings with t < 0 lie behind the start (t == 0, of either sign, lies ahead).  On an axis with
 *                 crossings the start cell is i_a = (number of planes behind, i.e. below the ray for d_a > 0) - 1 for
 *                 d_a > 0 and (number of planes ahead) - 1 for d_a < 0; on an axis without, i_a = (number of k with
 *                 P_a[k] <= o_a) - 1.  i_a = -1 and i_a = n_a are the two sides outside the grid.
 *   path        : the crossings ahead, every axis in its direction of travel, merged by (t, axis) ascending; a
 *                 crossing of axis a moves i_a by one.  Crossings with t = +inf are never reached.  The voxel path is
 *                 a pure function of (o, d) and the plane tables.
 *   hit         : the first state of the path (the start included) with all three i_a inside the grid and the voxel
 *                 solid, for a pixel inside the view's ROI.  Pixels outside the ROI, and rays that meet no solid voxel,
 *                 are misses.
 *   outputs     : depth (float)  t of the crossing that entered the voxel (+0.0f for t == 0), 0 when the ray starts
 *                                inside a solid voxel; +inf on a miss;
 *                 voxel (int64)  global id of the hit voxel (z * nx * ny + y * nx + x); -1 on a miss;
 *                 axis  (uint8)  0 / 1 / 2: the axis whose plane was crossed to enter, 3: started inside; 255 on a miss.
 *                                -sign(d_axis) * e_axis is a flat normal for previews. */

/* The planes between the cells of one axis (host arithmetic, no GPU): out[0 .. n], n = dims[axis] of vcy_compute_dims.
 * With p = vcy_axis_positions: out[k] = (float)(((double)p[k - 1] + (double)p[k]) * 0.5) for 0 < k < n, and the outer
 * two extrapolated by half the neighbouring pitch, out[0] = (float)((double)p[0] - ((double)p[1] - (double)p[0]) * 0.5),
 * out[n] = (float)((double)p[n - 1] + ((double)p[n - 1] - (double)p[n - 2]) * 0.5); with n == 1 the half pitch is
 * (double)resolution * 0.5.  The voxel pitch is diff / n, not `resolution` (voxel_carver.cc:315-326).
 * VCY_ERR_INVALID_ARG for an empty axis or a table that is not strictly increasing (a box whose centres collide in float). */
int vcy_cell_planes(const float bb_min[3], const float bb_max[3], float resolution, int axis, float* out);

/* Ray-casts the hull into `n_views` views (one launch for up to 64 of them).  depth_host / voxel_host / axis_host: arrays
 * of n_views pointers to row-major width * height images; any of the three arrays, or single entries, may be NULL.
 * Only roi_min / roi_max, width, height, w2c, the intrinsics and is_ortho of a view are read.  Applies queued ("defer")
 * views first; the state is not changed; a context nothing has been carved into since vcy_create / vcy_reset returns
 * all-miss images without its lazy fill being written.  The solid bits (one per voxel) and the occupancy bits (one per
 * 8 x 8 x 8 brick) are kept between calls and rebuilt when a carve, vcy_upload, vcy_reset or a component filter has come
 * in between, or the iso level differs.  VCY_ERR_UNSUPPORTED, state untouched, for a context that does not own the whole
 * grid (such a context renders through vcy_render_hull_slab, below).  VCY_ERR_INVALID_ARG for a non-finite w2c, fx or fy equal to 0 on a pinhole view, a width or height <= 0, or an
 * ROI outside the image. */
int vcy_render_hull(vcy_ctx* ctx, double iso_level, int n_views, const vcy_view* views, float* const* depth_host,
                    int64_t* const* voxel_host, uint8_t* const* axis_host);
/* Renders and compares with the silhouettes on the device; no image is downloaded.  masks_host[i]: width * height
 * bytes, non-zero = object (the convention of vcy_carve_silhouette's callers).  counts[3 * i + 0 .. 2] = pixels of view
 * i inside its ROI with {mask && hull, mask && !hull, !mask && hull}.  Errors as for vcy_render_hull. */
int vcy_hull_agreement(vcy_ctx* ctx, double iso_level, int n_views, const vcy_view* views,
                       const uint8_t* const* masks_host, int64_t* counts);
/* ---- ... of a grid cut into z-slabs ----
 * Everything refers to the definitions above: the global planes of vcy_cell_planes, the path as the merge by (t, axis) of
 * three monotone crossing sequences, t, the entry axis and the -0 -> 0 rule.
 *   slab image : the image of a context that owns the slices [z0, z1) is the whole-grid image of the state in which every
 *                voxel outside [z0, z1) is not solid.  The ray walks the GLOBAL path: plane tables, integer plane indices
 *                and start cells are global, t_a(k) is computed from the global k by the same float expression; a voxel
 *                can only be a hit where z0 <= i_z < z1; the voxel id is the global id (i_z * ny + i_y) * nx + i_x; depth
 *                and entry axis are those of the global path at that cell.  The halo slices below z0 are never read: no
 *                halo exchange is needed before a render.
 *   merge rule : along a ray i_z is monotone -- it rises when s_z > 0, falls when s_z < 0 and is constant when s_z == 0,
 *                s_z being the sign the walk forms: d_z = R[0][2] * d_c0 + R[1][2] * d_c1 + R[2][2] * 1.0f, and the axis
 *                moves iff d_z != 0 && isfinite(1.0f / d_z).  The ray visits the slabs in that order, and the whole-grid
 *                hit is the hit of the FIRST slab in the ray's direction of travel along z that has one: the lowest slab
 *                with voxel >= 0 for s_z > 0, the highest for s_z < 0; for s_z == 0 at most one slab can hit.  Depth,
 *                voxel id and axis come from that slab, +inf / -1 / 255 when no slab hit.
 *                Depth is NOT the key: two consecutive states of a path can carry the same t -- an x crossing and a z
 *                crossing at equal t sort by axis -- and lie in different slabs.
 *   hit bits   : one bit per pixel, rows of (width + 63) / 64 64-bit words; bit u & 63 of word [v][u >> 6] is set iff
 *                pixel (u, v) lies in the ROI and its ray hits a solid voxel of the slab; every other bit, the padding
 *                of a row included, is 0.  The OR of the slabs' bits is the whole grid's silhouette.
 * Per view and slab, depth (4 B / pixel), or the hit bits alone (1 bit / pixel) for the agreement, cross to the host. */

/* vcy_render_hull for ANY context: the slab image of the slices the context owns (on a context that owns the whole grid
 * the first three images equal vcy_render_hull's).  hits_host: n_views pointers to (width + 63) / 64 * height 64-bit
 * words each, or NULL, single entries too.  Arguments, errors, the 64 views per launch, the kept bit planes (of the
 * owned slices, bricks counted from z0) and vcy_last_render_ms as for vcy_render_hull; a fresh slab renders all misses
 * and all-zero hit bits without its lazy fill being written. */
int vcy_render_hull_slab(vcy_ctx* ctx, double iso_level, int n_views, const vcy_view* views, float* const* depth_host,
                         int64_t* const* voxel_host, uint8_t* const* axis_host, uint64_t* const* hits_host);
/* The merge rule on the host (no GPU, no context).  depth / voxel / axis: n_slabs pointers each to the slabs' images of
 * `view`, slabs in ascending z.  `voxel` is required (it says which slab hit); depth and axis may be NULL as a whole,
 * and then their output is not written; voxel_out may be NULL.  VCY_ERR_INVALID_ARG for n_slabs <= 0, a NULL where an
 * image is required, or a view vcy_render_hull would refuse. */
int vcy_render_merge_host(const vcy_view* view, int n_slabs, const float* const* depth, const int64_t* const* voxel,
                          const uint8_t* const* axis, float* depth_out, int64_t* voxel_out, uint8_t* axis_out);
/* vcy_hull_agreement from the slabs' hit bits (host only): ORs hits[0 .. n_slabs - 1] and counts, inside the view's ROI,
 * {mask && hull, mask && !hull, !mask && hull}; mask as for vcy_hull_agreement.  Errors as above. */
int vcy_hull_agreement_host(const vcy_view* view, int n_slabs, const uint64_t* const* hits, const uint8_t* mask,
                            int64_t counts[3]);
/* Milliseconds between HIP events around the launches (bit planes when rebuilt, the ray-cast) of the last
 * vcy_render_hull / vcy_render_hull_slab / vcy_hull_agreement, summed over its launches; copies of images are not included. */
int vcy_last_render_ms(const vcy_ctx* ctx, float* device_ms);

/* ---- colour of vertices from the input photographs ------------------------ */

/* What colour a point of the surface has in the photographs that see it (no reference counterpart: the reference's Mesh
 * carries vertex_colors_ and nothing fills them).  Inputs: n_vertices points p (float xyz, world; any points, not only an
 * extraction's vertices), optionally one float normal n per point, n_views views, per view a photograph
 * uint8 [height][width][3] (RGB, row-major; the sizes may differ between views) and a depth image float [height][width]
 * with vcy_render_hull's meaning (camera depth, +inf on a miss), and a vcy_color_option.  All arithmetic is float, every
 * product and every sum rounded on its own (no FMA), division and square root correctly rounded.
 * Per vertex the accumulators start at S_c = 0, W = 0, n_used = 0, w_best = -1, best_view = -1; then, for each view i in
 * ascending order, with R[r][c] = w2c[4 * r + c], t[r] = w2c[4 * r + 3]:
 *   1. projection : the carve's own, pc[r] = t[r] + (R[r][0] * px + (R[r][1] * py + R[r][2] * pz)); the view is skipped
 *                   if pc[2] < 0; pinhole u = fx / pc[2] * pc[0] + cx, w = fy / pc[2] * pc[1] + cy; ortho u = pc[0],
 *                   w = pc[1].
 *   2. ROI test   : the carve's in its complement form, inside iff u >= (float)roi_min[0] && w >= (float)roi_min[1] &&
 *                   u <= (float)roi_max[0] && w <= (float)roi_max[1]: NaN coordinates are outside.  Skipped when outside.
 *   3. occlusion  : the depth pixel is the carve's nearest-neighbour pixel, xi = (int)roundf(u), yi = (int)roundf(w)
 *                   (halves away from zero), each clamped into the ROI.  The view sees the vertex iff
 *                   pc[2] <= depth[yi][xi] + depth_tolerance -- one float add, one compare; a depth of +inf always sees
 *                   it, a NaN depth never.  Skipped when it does not.
 *   4. sample     : per channel c, of the texels converted (float)uint8.  VCY_INTERP_NN: the texel (xi, yi).
 *                   VCY_INTERP_BILINEAR: x0 = (int)floorf(u), x1 = x0 + 1, then x0 = max(x0, roi_min[0]),
 *                   x1 = min(x1, roi_max[0]), the same for y; lu = u - (float)x0, lv = w - (float)y0;
 *                   sample_c = (((1 - lu) * (1 - lv) * s00 + lu * (1 - lv) * s10) + (1 - lu) * lv * s01) + lu * lv * s11
 *                   with s00 = texel (x0, y0), s10 = (x1, y0), s01 = (x0, y1), s11 = (x1, y1), products left to right.
 *   5. weight     : VCY_COLOR_MEAN: wt = 1; normals and min_cos are not read.  Otherwise the camera-space normal
 *                   nc[r] = R[r][0] * nx + (R[r][1] * ny + R[r][2] * nz); pinhole
 *                   len = sqrtf((pc0 * pc0 + pc1 * pc1) + pc2 * pc2), cos = ((nc0 * pc0 + nc1 * pc1) + nc2 * pc2) / len;
 *                   ortho cos = nc[2]; wt = fabsf(cos) -- the absolute value is deliberate: marching cubes' winding
 *                   fixes the sign of Mesh::CalcNormal, and faces that point away are removed by the occlusion test, not
 *                   by the sign.  The view contributes iff wt > min_cos; a NaN weight (the normal of a vertex no face
 *                   names) never does.
 *   6. accumulate : S_c += wt * sample_c, W += wt, n_used += 1; if wt > w_best (strict: the lowest index wins a tie)
 *                   w_best = wt, best_view = i, best_c = sample_c.
 * Result: VCY_COLOR_MEAN and VCY_COLOR_WEIGHTED rgb_c = S_c / W, VCY_COLOR_BEST rgb_c = best_c; with n_used == 0
 * rgb = fallback.  rgb is float in 0 .. 255, not rounded -- the convention of Mesh::vertex_colors_. */
enum { VCY_COLOR_MEAN = 0, VCY_COLOR_WEIGHTED = 1, VCY_COLOR_BEST = 2 };
typedef struct vcy_color_option {
  int32_t mode;            /* VCY_COLOR_MEAN, VCY_COLOR_WEIGHTED, VCY_COLOR_BEST */
  int32_t interp;          /* VCY_INTERP_NN / VCY_INTERP_BILINEAR, the carve's two samplers */
  float   depth_tolerance; /* world units, >= 0 and finite */
  float   min_cos;         /* modes 1, 2: a view contributes iff its weight > min_cos; finite, >= 0 */
  float   fallback[3];     /* colour of a vertex no view contributes to */
} vcy_color_option;

/* The definition above, serial, on the host (no GPU, no context).  vertices / normals: 3 floats per vertex (normals may
 * be NULL in VCY_COLOR_MEAN); photos / depth: n_views pointers each, all required.  rgb_out: 3 * n_vertices floats;
 * n_used_out, best_view_out: n_vertices int32 each (best_view -1 when no view contributes), either may be NULL.
 * n_vertices == 0 is VCY_OK and writes nothing.  VCY_ERR_INVALID_ARG, nothing written, for a NULL required pointer,
 * n_views <= 0, a view vcy_render_hull would refuse, an unknown mode or interp, a negative or non-finite depth_tolerance or
 * min_cos, or NULL normals in modes 1 and 2. */
int vcy_color_vertices_host(int64_t n_vertices, const float* vertices, const float* normals, int n_views,
                            const vcy_view* views, const uint8_t* const* photos, const float* const* depth,
                            const vcy_color_option* option, float* rgb_out, int32_t* n_used_out, int32_t* best_view_out);
/* The same on the device, bit for bit (one lane per vertex, the view loop inside the lane; views in chunks of 64 with the
 * accumulators carried between them, so any n_views >= 1).  depth_host != NULL: the depth images are uploaded and used as
 * given, iso_level is ignored and the context only names the device and the stream -- any context will do, a z-slab
 * included: this is how a sharded caller colours (with the merged depth of vcy_render_merge_host), and where a depth
 * sensor's image goes.  depth_host == NULL: the library ray-casts the hull itself at iso_level, every view with its own
 * ROI, and the depth images stay in device memory (none crosses to the host or back); this applies queued ("defer") views
 * first, as the render does, and needs a context that owns the whole grid -- VCY_ERR_UNSUPPORTED otherwise.  The state is
 * never changed; a fresh context renders all misses without its lazy fill being written.  Arguments and errors as for
 * the host function. */
int vcy_color_vertices(vcy_ctx* ctx, double iso_level, int64_t n_vertices, const float* vertices, const float* normals,
                       int n_views, const vcy_view* views, const uint8_t* const* photos_host, const float* const* depth_host,
                       const vcy_color_option* option, float* rgb_out, int32_t* n_used_out, int32_t* best_view_out);
/* Milliseconds between HIP events around the colouring launches (the packing of the photographs to one dword per texel
 * and the colouring kernel) of the last vcy_color_vertices, summed over its chunks of views.  Copies and the ray-cast are
 * not included; the ray-cast of a call without depth images is in vcy_last_render_ms. */
int vcy_last_color_ms(const vcy_ctx* ctx, float* device_ms);

/* ---- rasterising an indexed mesh into views: depth, face id, hit bits, agreement ----- */
/* No reference counterpart: this section is the definition.  vcy_raster_mesh_host is it in serial host code,
 * tests/raster_ref.py restates it in numpy, vcy_raster_mesh runs it on the device; the three agree bit for bit.
 *
 * Inputs: n_vertices points (float xyz, world), n_faces int32 triples (f0, f1, f2), n_views views, of which the fields
 * vcy_render_hull reads are read (roi_min / roi_max, width, height, w2c, the intrinsics, is_ortho) and the views it refuses
 * are refused.  With R[r][c] = w2c[4 * r + c], t[r] = w2c[4 * r + 3], every step is arithmetic in a fixed order, every
 * product and every sum rounded on its own (no FMA), division correctly rounded.  Per view:
 *   1. projection : of a vertex p, the carve's own float arithmetic (step 1 of the colour definition):
 *                   pc[r] = t[r] + (R[r][0] * px + (R[r][1] * py + R[r][2] * pz)); pinhole u = fx / pc[2] * pc[0] + cx,
 *                   w = fy / pc[2] * pc[1] + cy; ortho u = pc[0], w = pc[1]; z = pc[2].  The vertex is UNUSABLE in the
 *                   view when a component of pc, u or w is not finite, on a pinhole view when pc[2] <= 0, on an ortho view
 *                   when pc[2] < 0.  (u, w, z) is a pure function of (vertex, view): every face that names the vertex
 *                   sees the same bits.
 *   2. dropped    : a face is not drawn in the view, class 0, when one of its vertices is unusable -- there is NO
 *                   near-plane clipping: a face that crosses the camera plane disappears whole --; otherwise, class 1,
 *                   when it names a vertex twice or its signed area A (step 4) is 0 or not finite.
 *                   n_dropped[2 * i + c] counts the faces of class c in view i.
 *   3. edge       : in double, from the float coordinates, canonical per edge: for the vertex indices i < j, a = (u_i, w_i)
 *                   and b = (u_j, w_j) converted to double, E_ij(p) = (bx - ax) * (py - ay) - (by - ay) * (px - ax).  The
 *                   face's value for its directed edge f_k -> f_k+1 is E_ij(p) when the face runs from i to j and
 *                   -E_ij(p) when it runs from j to i.  Two faces that share an edge in opposite directions therefore get
 *                   exactly opposite values at every p: the image has no hole and no double cover along an interior edge.
 *   4. area       : A = the face's value for the edge (f0, f1) at p = (u, w) of f2; s = +1 for A > 0, -1 for A < 0.  Both
 *                   windings are drawn: there is no culling.
 *   5. candidates : the integer pixels (x, y) -- the carve's and the ray-cast's pixel, data[width * y + x] -- with
 *                   ceilf(min u) <= x <= floorf(max u), ceilf(min w) <= y <= floorf(max w), inside the ROI
 *                   (roi_min <= (x, y) <= roi_max).  The box is part of the definition.
 *   6. coverage   : closed.  With e_0, e_1, e_2 the face's values at p = ((double)x, (double)y) for the edges (f1, f2),
 *                   (f2, f0), (f0, f1): the pixel is covered iff s * e_k >= 0 for all three.
 *   7. depth      : l_k = e_k / A.  Pinhole z = 1.0 / ((l_0 * (1.0 / z_0) + l_1 * (1.0 / z_1)) + l_2 * (1.0 / z_2)), ortho
 *                   z = (l_0 * z_0 + l_1 * z_1) + l_2 * z_2, with z_k = (double)pc[2] of f_k; depth = (float)z, -0 stored
 *                   as +0.  A fragment whose depth is not finite or < 0 is discarded.
 *   8. winner     : per pixel, the fragment with the smallest (depth bits as uint32, face index), compared
 *                   lexicographically -- a rule without an order, so any traversal gives the same image.
 *   9. outputs    : depth (float)   camera depth of the winner, the quantity of vcy_render_hull's depth; +inf on a miss;
 *                   face  (int32)   the winner's face index; -1 on a miss;
 *                   hits  (uint64)  the hit bits of vcy_render_hull_slab, word for word: (width + 63) / 64 words per
 *                                   row, bit x & 63 of word [y][x >> 6] set iff pixel (x, y) has a winner; every other
 *                                   bit, the padding of a row included, is 0.  Pixels outside the ROI are misses.
 * VCY_ERR_INVALID_ARG, nothing written, for a NULL required pointer, negative counts, n_views <= 0, a view vcy_render_hull
 * would refuse, or a face index outside [0, n_vertices) (the contract of vcy_smooth_mesh); VCY_ERR_UNSUPPORTED beyond
 * vcy_mesh_index_limits.  A mesh without faces gives all-miss images. */

/* The definition above, serial, on the host (no GPU, no context).  depth / face / hits: arrays of n_views pointers to
 * width * height floats, width * height int32 and (width + 63) / 64 * height 64-bit words; any of the three arrays, or
 * single entries, may be NULL.  n_dropped: 2 * n_views counts, or NULL. */
int vcy_raster_mesh_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces, int n_views,
                         const vcy_view* views, float* const* depth, int32_t* const* face, uint64_t* const* hits,
                         int64_t* n_dropped);
/* The same on the device of `ctx`, on its stream, from and into HOST arrays, bit for bit (a 64-bit key image per view,
 * 64-bit integer atomic minima; one lane per face with the view loop inside it, faces with large candidate boxes drawn by
 * their whole wave -- vcy_set_param "rasterwide"; views in chunks of 64, so any n_views >= 1).  The context only names the
 * device and the stream: any context will do, a z-slab included; the voxel state, queued views and every cache stay
 * untouched.  Arguments and errors as for the host function; VCY_ERR_NOT_INITIALIZED for a NULL context, behind the
 * argument checks.  Device memory: the mesh, and per view of a chunk 8 bytes per pixel plus the images asked for, kept by
 * the context (grow-only). */
int vcy_raster_mesh(vcy_ctx* ctx, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces, int n_views,
                    const vcy_view* views, float* const* depth_host, int32_t* const* face_host, uint64_t* const* hits_host,
                    int64_t* n_dropped);
/* Rasterises and compares with the silhouettes on the device; no image is downloaded.  masks_host and counts as for
 * vcy_hull_agreement: counts[3 * i + 0 .. 2] = pixels of view i inside its ROI with {mask && mesh, mask && !mesh,
 * !mask && mesh}; equal to vcy_hull_agreement_host over the hit bits of vcy_raster_mesh_host. */
int vcy_mesh_agreement(vcy_ctx* ctx, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces, int n_views,
                       const vcy_view* views, const uint8_t* const* masks_host, int64_t* counts);
/* Milliseconds between HIP events of the last vcy_raster_mesh / vcy_mesh_agreement, summed over its chunks of views: the
 * fill of the key images with the raster launch, and the resolve launch.  Copies are not included.  Either may be NULL. */
int vcy_last_raster_ms(const vcy_ctx* ctx, float* raster_ms, float* resolve_ms);

/* ---- shading a rasterised mesh: attribute images, photometric error ----- */
/* No reference counterpart: this section is the definition, a continuation of "rasterising an indexed mesh".
 * vcy_shade_mesh_host is it in serial host code, tests/shade_ref.py restates it in numpy, vcy_shade_mesh runs it on the
 * device; the three agree bit for bit.
 *
 * Inputs: the rasteriser's, per vertex `channels` floats (attributes[channels * vertex + c]: colours, normals, anything),
 * channels in 1 .. 4, and a vcy_shade_option.  Steps 1 to 8 of the rasteriser decide the winner of every pixel; the steps
 * below stand in the place of its step 9.  For a pixel (x, y) of view i with the winning face F = (f0, f1, f2):
 *   9. weights    : in double.  e_0, e_1, e_2 and A are exactly those of steps 4 and 6 for F at p = ((double)x, (double)y);
 *                   l_k = e_k / A.  Ortho b_k = l_k.  Pinhole t_k = l_k * (1.0 / z_k), T = (t_0 + t_1) + t_2,
 *                   b_k = t_k / T -- the t_k and the sum of step 7, so that the depth image is (float)(1.0 / T) of the T
 *                   used here.
 *  10. value      : per channel c, with a_k the attribute of f_k,
 *                   v_c = (float)((b_0 * (double)a_0c + b_1 * (double)a_1c) + b_2 * (double)a_2c), every product and sum
 *                   rounded on its own.  On a miss -- every pixel outside the ROI is one -- v_c = background[c].
 *                   Attributes that are not finite go through the same arithmetic; which NaN comes out is not part of
 *                   the contract.
 *  11. outputs    : value  (float [height][width][channels])  v;
 *                   value8 (uint8 [height][width][channels])  q(v) = !(v > 0) ? 0 : v >= 255 ? 255 : (uint8)floorf(v + 0.5f),
 *                                   the v + 0.5f one float addition: NaN gives 0, and the background goes through q too;
 *                   bary   (float [height][width][3])         (float)b_k; 0, 0, 0 on a miss.
 *  12. photometric error (channels == 3): with a photograph uint8 [height][width][3] per view and optionally a silhouette
 *                   per view (vcy_mesh_agreement's: non-zero = object), per view over the pixels that have a winner and,
 *                   where silhouettes are given, a non-zero silhouette: n = their number, sad[c] = sum |q(v_c) - photo_c|,
 *                   ssd[c] = sum (q(v_c) - photo_c)^2, as int64 {n, sad0, sad1, sad2, ssd0, ssd1, ssd2}.  Integer sums
 *                   have no order: any traversal gives the same seven numbers.  Background pixels never count.
 * Errors: the rasteriser's; VCY_ERR_INVALID_ARG, nothing written, also for a NULL option, NULL attributes with
 * n_vertices > 0, channels outside 1 .. 4, and in the error calls NULL photos or sums, a NULL photograph, or a NULL entry
 * of a non-NULL silhouette array. */
typedef struct vcy_shade_option {
  int32_t channels;       /* floats per vertex, 1 .. 4 */
  float   background[4];  /* the value of a pixel without a winner; the first `channels` are read */
} vcy_shade_option;

/* The definition above, serial, on the host (no GPU, no context): vcy_raster_mesh_host, then steps 9 to 11.  value /
 * value8 / bary: arrays of n_views pointers; any of the three arrays, or single entries, may be NULL. */
int vcy_shade_mesh_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                        const float* attributes, int n_views, const vcy_view* views, const vcy_shade_option* option,
                        float* const* value, uint8_t* const* value8, float* const* bary);
/* The same on the device of `ctx`, on its stream, from and into HOST arrays, bit for bit: vcy_raster_mesh's key images
 * and raster launch, then one lane per pixel that re-projects the winner's corners and evaluates steps 9 to 11 (views in
 * chunks of 64).  Any context will do, a z-slab included; the voxel state, queued views and every cache stay untouched.
 * The arguments are checked before the context is looked at; VCY_ERR_NOT_INITIALIZED for a NULL context.  Device memory:
 * the rasteriser's pool, with the attributes and the images asked for. */
int vcy_shade_mesh(vcy_ctx* ctx, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                   const float* attributes, int n_views, const vcy_view* views, const vcy_shade_option* option,
                   float* const* value_host, uint8_t* const* value8_host, float* const* bary_host);
/* Step 12 on the host.  colors: 3 floats per vertex; the background is never counted, so there is no option.  photos:
 * n_views pointers; masks: NULL, or n_views pointers; sums: 7 * n_views int64. */
int vcy_mesh_photo_error_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                              const float* colors, int n_views, const vcy_view* views, const uint8_t* const* photos,
                              const uint8_t* const* masks, int64_t* sums);
/* ... and on the device: photographs and silhouettes are uploaded as given, the seven sums are reduced per wave, then per
 * workgroup, then by one 64-bit integer atomic add per counter; no image is downloaded. */
int vcy_mesh_photo_error(vcy_ctx* ctx, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                         const float* colors, int n_views, const vcy_view* views, const uint8_t* const* photos_host,
                         const uint8_t* const* masks_host, int64_t* sums);
/* Milliseconds between HIP events of the last vcy_shade_mesh / vcy_mesh_photo_error, summed over its chunks of views: the
 * fill of the key images with the raster launch, and the shade launch.  Copies are not included.  Either may be NULL. */
int vcy_last_shade_ms(const vcy_ctx* ctx, float* raster_ms, float* shade_ms);

/* ---- mesh smoothing: Taubin passes over an indexed mesh, fresh normals ----- */
/* No reference counterpart: this section is the definition.  vcy_smooth_mesh_host is it in serial host code,
 * tests/smooth_ref.py restates it in numpy, vcy_smooth_mesh runs it on the device; the three agree bit for bit.
 *
 * All arithmetic is float; every product, sum and division is rounded on its own (no FMA), division and square root
 * are correctly rounded -- the flags the library is built with.
 *
 * Rows.  The row of vertex v lists every corner (f, j) with faces[3f + j] == v in ascending f, then ascending j; a face
 * that names v twice has two corners in the row.  cnt(v) is twice the row's length.
 *
 * One pass with factor s, from positions p to positions q (a Jacobi pass: every q is computed from the same p).
 *   cnt(v) == 0 or v pinned:  q[v] = p[v], an exact copy of the bits.
 *   otherwise, per coordinate c:  S_c = +0; through the row in order, for each corner (f, j), with
 *     a = p[faces[3f + (j+1)%3]],  b = p[faces[3f + (j+2)%3]]:   S_c = S_c + a_c;  S_c = S_c + b_c.
 *   Then  m_c = S_c / (float)cnt,  d_c = m_c - p_c,  q_c = p_c + s * d_c.
 * On a closed manifold this is the uniform umbrella operator with every neighbour counted twice; the order of the sum is
 * Mesh::CalcNormal's.  The passes of a call: lambda, mu, lambda, mu, ... -- 2 * iterations of them; iterations == 0
 * returns the input bits.  (A pass with s == 0 is still a pass: p_c + 0 * d_c.)
 *
 * Pinned vertices.  With pin_boundary, v is pinned iff some vertex u != v occurs exactly once among the cnt(v) ids the
 * pass would gather for v: an edge that one face uses.
 *
 * Normals.  If either normals output is non-NULL, the result is vcy_mesh_normals_host of (vertices_out, faces), to the bit.
 * A vertex that no face names gets NaN, as there; the sign of that NaN is not part of the contract.
 *
 * Non-finite input positions go through the same arithmetic; which NaN comes out (sign, payload) is not part of the
 * contract.  vertices_out may alias vertices.
 *
 * VCY_ERR_INVALID_ARG, nothing written, for a NULL required pointer, negative counts, a face index outside
 * [0, n_vertices), iterations outside 0 .. 10000, a non-finite lambda or mu, pin_boundary not 0 or 1.
 * VCY_ERR_UNSUPPORTED when 3 * n_faces >= 2^31 or n_vertices >= 2^31 (corner ids are int32 on the device).
 * n_vertices == 0 is VCY_OK and writes nothing. */
typedef struct vcy_smooth_option {
  int32_t iterations;    /* >= 0; one iteration = a lambda pass, then a mu pass; at most 10000 */
  float   lambda;        /* finite */
  float   mu;            /* finite; 0 makes it plain Laplacian smoothing */
  int32_t pin_boundary;  /* 0 / 1 */
} vcy_smooth_option;

int vcy_smooth_mesh_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                         const vcy_smooth_option* option, float* vertices_out,
                         float* vertex_normals_out /* may be NULL */, float* face_normals_out /* may be NULL */);
/* The same on the device of `ctx`, on its stream, from and into HOST arrays (as vcy_color_vertices).  The context only
 * names the device and the stream: any context will do, a z-slab included -- a sharded caller smooths the merged mesh on
 * one of its slabs.  The voxel state, queued views and every cache stay untouched.  Device memory: about 175 bytes per
 * vertex of a triangle mesh, kept by the context (grow-only). */
int vcy_smooth_mesh(vcy_ctx* ctx, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                    const vcy_smooth_option* option, float* vertices_out,
                    float* vertex_normals_out /* may be NULL */, float* face_normals_out /* may be NULL */);
/* Device time of the last vcy_smooth_mesh: the incidence table (count, scan, fill, row sort, gather rows), all passes, the
 * normals (0 when none were asked for).  Any output may be NULL. */
int vcy_last_smooth_ms(const vcy_ctx* ctx, float* build_ms, float* passes_ms, float* normals_ms);

/* ---- mesh decimation: vertex clustering over an indexed mesh, fresh normals ----- */
/* No reference counterpart: this section is the definition (vertex clustering after Rossignac and Borrel).
 * vcy_decimate_mesh_host is it in serial host code, tests/decimate_ref.py restates it in numpy, vcy_decimate_mesh runs it on
 * the device; the three agree bit for bit.
 *
 * All arithmetic is float; every difference, product, sum and division is rounded on its own (no FMA), division is
 * correctly rounded -- the flags the library is built with.
 *
 * Cell of a vertex.  Per coordinate c:  t_c = (p_c - origin_c) / cell,  k_c = floor(t_c) as int32 (-0.0 gives 0).  A
 * non-finite p_c, or |t_c| >= 2^30, makes the call fail.
 *
 * Clusters.  Two vertices are in one cluster iff their three k are equal.  Every input vertex is a member, whether or not
 * a face names it.  Clusters are numbered 0, 1, ... by ascending lowest member index.
 *
 * Faces, in ascending input index: every corner is replaced by its cluster number, (a, b, c).  The face is dropped if two
 * of the three are equal.  Otherwise its canonical form is the rotation of (a, b, c) that puts the smallest number first,
 * cyclic order kept: (a, b, c), (b, c, a) and (c, a, b) are the same, (a, c, b) is not.  Of the faces with one canonical
 * form only the lowest input index survives.  Surviving faces keep their input order and their own corner order (they are
 * not rotated).
 *
 * Output vertices: the clusters that at least one surviving face names, in cluster order.  vertex_map[v] is the output
 * index of v's cluster, or -1; face_source[g] is the input index of output face g; faces_out names output vertices.
 *
 * Position of a cluster with members i_0 < i_1 < ... < i_{n-1}:
 *   FIRST    the bits of p[i_0].
 *   MEAN     per coordinate S = +0, then S = S + p[i_j]_c for j = 0 .. n-1, then m_c = S / (float)n.
 *   NEAREST  m as in MEAN;  d(i) = (dx*dx + dy*dy) + dz*dz  with dx = p[i]_x - m_x, likewise dy, dz;  best = i_0; for
 *            j = 1 .. n-1, i_j replaces best iff d(i_j) < d(best) (strict: a NaN never wins, ties go to the lower index);
 *            the output is the bits of p[best].
 *
 * Normals.  If either normals output is non-NULL, the result is vcy_mesh_normals_host of the output mesh, to the bit.
 *
 * Checks, in this order.  VCY_ERR_INVALID_ARG: negative counts; option, n_vertices_out or n_faces_out NULL; with both
 * counts > 0 any of vertices, faces, vertices_out, faces_out NULL; cell not finite or <= 0; a non-finite origin; mode
 * outside 0 .. 2.  VCY_ERR_UNSUPPORTED: n_vertices >= 2^31 or 3 * n_faces >= 2^31.  Then n_vertices == 0 or n_faces == 0 is
 * VCY_OK with both counts 0, no array read and no array written.  Then VCY_ERR_INVALID_ARG for a face index outside
 * [0, n_vertices) and for a vertex that fails the cell rule.  Whatever is refused, nothing is written, not even the
 * counts.  Outputs must not overlap inputs or each other; this is not checked. */
#define VCY_DECIMATE_MEAN 0
#define VCY_DECIMATE_NEAREST 1
#define VCY_DECIMATE_FIRST 2
typedef struct vcy_decimate_option {
  float   cell;       /* finite, > 0: edge of the clustering cells          */
  float   origin[3];  /* finite: a corner of the cell lattice               */
  int32_t mode;       /* 0 MEAN, 1 NEAREST, 2 FIRST                         */
} vcy_decimate_option;   /* 20 bytes */

int vcy_decimate_mesh_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                           const vcy_decimate_option* option,
                           float* vertices_out   /* room for 3 * n_vertices */,
                           int32_t* faces_out    /* room for 3 * n_faces    */,
                           int64_t* n_vertices_out, int64_t* n_faces_out,
                           int32_t* vertex_map   /* [n_vertices], may be NULL */,
                           int32_t* face_source  /* room for n_faces, may be NULL */,
                           float* vertex_normals_out /* room for 3 * n_vertices, may be NULL */,
                           float* face_normals_out   /* room for 3 * n_faces, may be NULL */);
/* The same on the device of `ctx`, on its stream, from and into HOST arrays (as vcy_smooth_mesh).  The context only names
 * the device and the stream: any context will do, a z-slab included -- a sharded caller decimates the merged mesh on one of
 * its slabs.  The voxel state, queued views and every cache stay untouched.  Face indices and the cell rule are checked on
 * the device (flags read at the call's one wait for its launches; the results are copied out behind it, sized by the
 * counts).  A cluster's sum is serial by definition: a cell that holds more than 256 vertices is summed by one lane of a
 * workgroup of its own, so cells far larger than the mesh's spacing are correct but slow.  Device memory: 108 bytes per
 * input vertex and 52 per input face plus the two tables, 8 to 16 bytes per vertex and per face (a closed triangle mesh:
 * about 250 bytes per vertex), kept by the context (grow-only); the normals of the result use vcy_smooth_mesh's pool. */
int vcy_decimate_mesh(vcy_ctx* ctx, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                      const vcy_decimate_option* option, float* vertices_out, int32_t* faces_out,
                      int64_t* n_vertices_out, int64_t* n_faces_out, int32_t* vertex_map /* may be NULL */,
                      int32_t* face_source /* may be NULL */, float* vertex_normals_out /* may be NULL */,
                      float* face_normals_out /* may be NULL */);
/* Device time of the last vcy_decimate_mesh: clusters (keys, table, numbering, member rows), faces (mapping, duplicate
 * table, numbering of survivors and of output vertices), emit (positions, faces, maps), normals (0 when none were asked
 * for).  Any output may be NULL. */
int vcy_last_decimate_ms(const vcy_ctx* ctx, float* cluster_ms, float* faces_ms, float* emit_ms, float* normals_ms);

/* ---- mesh decimation, quadric representatives: the cluster's least-squares point ----- */
/* No reference counterpart: this section is the definition (quadric error after Garland and Heckbert, per cluster after
 * Lindstrom).  The host function below is it in serial host code, tests/quadric_ref.py restates it in numpy, the device
 * function runs it on the device; the three agree bit for bit.
 *
 * Cells, clusters, cluster numbering, face rules, output vertices, vertex_map, face_source, normals and the order of the
 * checks are those of "mesh decimation", word for word.  Only the position of a cluster differs: MEAN pulls the surface
 * inward at every edge and corner; this position minimises the sum of squared (area-weighted) distances to the planes of
 * the input faces around the cluster's members.
 *
 * All arithmetic below is double; every product, sum, difference and division is rounded on its own (no FMA), division
 * is correctly rounded; (double) of a float is exact.
 *
 * Mean.  m is the cluster's MEAN, in float as defined above.
 *
 * Quadric of a face f = (i0, i1, i2), seen from cluster C:  a = (double)p[i0] - (double)m per coordinate, likewise b, c;
 * e = b - a, g = c - a;  nx = e_y*g_z - e_z*g_y,  ny = e_z*g_x - e_x*g_z,  nz = e_x*g_y - e_y*g_x;
 * d = -((nx*a_x + ny*a_y) + nz*a_z);  q(f) = (nx*nx, nx*ny, nx*nz, ny*ny, ny*nz, nz*nz, nx*d, ny*d, nz*d).
 *
 * Quadric of a vertex v in cluster C.  Qv = nine zeros; then through v's corner row -- every corner (f, j) with
 * faces[3f+j] == v, in ascending f, then ascending j -- Qv = Qv + q(f) componentwise.  A face that names v twice is added
 * twice.
 *
 * Quadric of a cluster.  Q = nine zeros; through the members in ascending index, Q = Q + Qv.  Two levels of sums, in this
 * order.
 *
 * Solve.  t = (Q0 + Q3) + Q5;  w = (double)regularize * t;  A00 = Q0 + w, A11 = Q3 + w, A22 = Q5 + w, A01 = Q1, A02 = Q2,
 * A12 = Q4;  r = (-Q6, -Q7, -Q8);  d0 = A00;  l10 = A01/d0, l20 = A02/d0;  d1 = A11 - l10*A01;  u = A12 - l20*A01,
 * l21 = u/d1;  d2 = (A22 - l20*A02) - l21*u;  y0 = r0, y1 = r1 - l10*y0, y2 = (r2 - l20*y0) - l21*y1;  z_i = y_i/d_i;
 * x2 = z2, x1 = z1 - l21*x2, x0 = (z0 - l10*x1) - l20*x2;  P_c = (float)((double)m_c + x_c), rounded to nearest even.
 *
 * Fallback.  The cluster's position is the bits of m instead of P whenever t is not finite or not > 0 (a cluster without
 * faces, or with zero-area faces only); one of d0, d1, d2 is not > 0; a coordinate of P is not finite; the cell rule of
 * "mesh decimation" fails for P; or the cell of P is not the cluster's: a representative never leaves its cell.
 *
 * regularize pulls the optimum towards the mean by a share of the quadric's trace: on a flat part the tangential position
 * stays at the mean.  With regularize == 0 a flat or edge-like cluster falls back.
 *
 * Checks: those of "mesh decimation" in their order; where the mode check stands there, here: option->mode must be
 * VCY_DECIMATE_MEAN, regularize finite and in [0, 1], else VCY_ERR_INVALID_ARG.  *n_fallback (may be NULL) is the number
 * of OUTPUT vertices that carry the mean.  Whatever is refused, nothing is written, not the counts and not *n_fallback;
 * n_vertices == 0 or n_faces == 0 sets all three to 0. */
int vcy_decimate_mesh_quadric_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                                   const vcy_decimate_option* option, float regularize,
                                   float* vertices_out   /* room for 3 * n_vertices */,
                                   int32_t* faces_out    /* room for 3 * n_faces    */,
                                   int64_t* n_vertices_out, int64_t* n_faces_out,
                                   int32_t* vertex_map   /* [n_vertices], may be NULL */,
                                   int32_t* face_source  /* room for n_faces, may be NULL */,
                                   float* vertex_normals_out /* room for 3 * n_vertices, may be NULL */,
                                   float* face_normals_out   /* room for 3 * n_faces, may be NULL */,
                                   int64_t* n_fallback       /* may be NULL */);
/* The same on the device of `ctx`, under the terms of the device function of "mesh decimation".  The quadric stage runs
 * behind the member rows and means: the vertex -> corner table of the input mesh (a corner with a bad index is left out and
 * refuses the call like any bad face index), nine doubles per vertex, one lane per cluster for the sum and the solve; a
 * cell that holds more than 256 vertices is correct but slow here too.  Device memory on top of the MEAN call's: 77 bytes
 * per input vertex (72 of them the vertex quadrics) and 12 per input face (the corner table). */
int vcy_decimate_mesh_quadric(vcy_ctx* ctx, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                              const vcy_decimate_option* option, float regularize, float* vertices_out, int32_t* faces_out,
                              int64_t* n_vertices_out, int64_t* n_faces_out, int32_t* vertex_map /* may be NULL */,
                              int32_t* face_source /* may be NULL */, float* vertex_normals_out /* may be NULL */,
                              float* face_normals_out /* may be NULL */, int64_t* n_fallback /* may be NULL */);
/* Device time of the quadric stage (corner table, vertex quadrics, sums and solves) of the last device call of this section;
 * 0 after one that had nothing to do.  vcy_last_decimate_ms reports that call's four groups, this stage inside "clusters". */
int vcy_last_quadric_ms(const vcy_ctx* ctx, float* device_ms);

/* ---- extraction chain: extract, smooth, decimate and normals in one call, the mesh staying on the device ----- */
/* The result is BY DEFINITION the bits of the separate calls run in this order: vcy_extract_iso; if `smooth`,
 * vcy_smooth_mesh on its output; if `decimate`, vcy_decimate_mesh (1) or vcy_decimate_mesh_quadric (2, with `regularize`)
 * on that; Mesh::CalcNormal (vcy_mesh_normals_host) of the last mesh for the arrays `which` names.  The order is fixed:
 * smoothing first, then decimation.  With both stages off the call is vcy_extract_iso_normals (which = 0: vcy_extract_iso,
 * without edge keys).  Only the final mesh, its normals and -- `maps` = 1 -- the decimation's two maps cross to the host;
 * the extracted mesh is staged in device memory whatever "mcdirect" says, the stages read it there, and the vertex ->
 * incident-corner table of the extracted mesh is built once and serves the smoothing, the quadric stage and the normals
 * of an undecimated result.  The call waits for the extraction's counts, for the decimation's counts, and for the output.
 *
 * An empty extraction yields an empty mesh and VCY_OK.  VCY_ERR_UNSUPPORTED for a context that owns a z-slab (a slab's
 * mesh is a part; the merged mesh exists only on the host) and for one that returns edge keys (vcy_set_param "meshkeys"
 * 1: the chain's mesh has none).  Option errors are the refusals of the separate calls with their codes, reported before
 * any launch and before the context is looked at; a stage that is off is not checked.  An extracted mesh beyond
 * vcy_mesh_index_limits is refused with the separate calls' VCY_ERR_UNSUPPORTED before a stage is launched on it (not with
 * both stages off: the extraction takes it).  `smooth`, `maps` outside 0 / 1, `decimate` outside 0 .. 2 or `which` outside
 * the VCY_NORMALS_* bits: VCY_ERR_INVALID_ARG. */
typedef struct vcy_chain_option {
  int32_t smooth;                       /* 0 / 1 */
  vcy_smooth_option smooth_option;
  int32_t decimate;                     /* 0 none, 1 vertex clustering, 2 quadric representatives */
  vcy_decimate_option decimate_option;
  float   regularize;                   /* decimate = 2 */
  int32_t which;                        /* VCY_NORMALS_* of the final mesh */
  int32_t maps;                         /* 1: the report carries vertex_map and face_source (decimate != 0) */
} vcy_chain_option;   /* 56 bytes */
typedef struct vcy_chain_report {
  int64_t n_extracted_vertices, n_extracted_faces;  /* of the mesh vcy_extract_iso would have returned */
  int64_t n_fallback;                   /* decimate = 2: output vertices that keep the mean; else 0 */
  int32_t* vertex_map;                  /* [n_extracted_vertices] output index or -1; NULL unless maps and decimate */
  int32_t* face_source;                 /* [out->n_faces] index of the extracted face; NULL unless maps and decimate */
} vcy_chain_report;   /* 40 bytes; the arrays are the library's: vcy_chain_report_free */
/* out: as vcy_extract_iso's (vcy_mesh_free), edge_keys NULL and n_foreign_vertices 0.  normals may be NULL when which is 0
 * (vcy_mesh_normals_free); report may be NULL. */
int vcy_extract_iso_chain(vcy_ctx* ctx, double iso_level, int linear_interp, const vcy_chain_option* option, vcy_mesh* out,
                          vcy_mesh_normals* normals, vcy_chain_report* report);
void vcy_chain_report_free(vcy_chain_report* report);
/* The size of a mesh the mesh operators of this header take: VCY_OK, or VCY_ERR_UNSUPPORTED for more than 2^31 - 1 vertices
 * or more than (2^31 - 3) / 3 faces -- vertex ids and corner ids 3 f + j are 32 bits wide in their tables.  It is the check
 * vcy_smooth_mesh[_host] and vcy_decimate_mesh[_quadric][_host] apply to their input and vcy_extract_iso_chain applies to
 * the mesh it has extracted (which may be larger: the extraction counts faces in 32 bits unsigned), before any stage is
 * launched on it.  Negative counts: VCY_ERR_INVALID_ARG.  No context, no GPU. */
int vcy_mesh_index_limits(int64_t n_vertices, int64_t n_faces);
/* Times of the last vcy_extract_iso_chain, device milliseconds but the last: the extraction's kernels; the shared corner
 * table (count, scan, fill, and the smoothing's row sort and gather rows); the smoothing passes; the decimation's cluster
 * group (the quadric stage inside it); the quadric stage alone; its faces and emit groups together; the normals of the
 * final mesh; and the call's wall time on the host.  A stage that did not run reports 0, and so does every stage after a
 * call that was refused for its context; a call refused for its arguments leaves the times of the call before.  Any output
 * may be NULL. */
int vcy_last_chain_ms(const vcy_ctx* ctx, float* extract_ms, float* table_ms, float* passes_ms, float* cluster_ms,
                      float* quadric_ms, float* faces_emit_ms, float* normals_ms, float* wall_ms);

/* ---- state access (tests, ExtractVoxel on the host, checkpoint) ---------- */

/* Copies the slab's voxel state to the host: sdf[nx*ny*nz_local] and
 * update_num[nx*ny*nz_local] in the reference's linear order
 * id = z*nx*ny + y*nx + x (voxel_carver.cc:333,349-355).  Either may be NULL. */
int vcy_download(vcy_ctx* ctx, float* sdf, int32_t* update_num);
int vcy_upload(vcy_ctx* ctx, const float* sdf, const int32_t* update_num);
/* Device-side comparison of two contexts that own the same slab of the same grid (on one device):
 * *n_diff = number of voxels whose (sdf bits, update_num) differ.  Nothing is downloaded -- this is
 * how the tests cross-check two kernel paths over a whole 1024^3 / 2048^3 grid. */
int vcy_state_equal(vcy_ctx* a, vcy_ctx* b, int64_t* n_diff);
/* Point query: state of `n` voxels given by global id (must lie in this context's slab). */
int vcy_download_voxels(vcy_ctx* ctx, int64_t n, const int64_t* voxel_ids, float* sdf, int32_t* update_num);
/* Voxel centres of the slab, 3 floats per voxel (Voxel::pos, voxel_carver.cc:315-337). */
int vcy_download_positions(vcy_ctx* ctx, float* pos);

/* ---- multi-GPU halo (one process per GPU; the exchange itself is one RCCL
 * all-gather issued by the caller on the buffers below) ------------------- */

/* Bytes one rank contributes: the LAST two xy-slices of its slab, (sdf, update_num).
 * Rank r consumes rank r-1's contribution as its slices z_begin-2, z_begin-1. */
int64_t vcy_halo_bytes(const vcy_ctx* ctx);
/* Packs this slab's boundary slices into `send_device` (vcy_halo_bytes bytes). */
int vcy_halo_pack(vcy_ctx* ctx, void* send_device);
/* Installs the neighbours' slices from the all-gathered buffer
 * (world * vcy_halo_bytes bytes, rank-major). */
int vcy_halo_unpack(vcy_ctx* ctx, const void* gathered_device, int rank, int world);
/* Same, given directly the pack (vcy_halo_bytes bytes, device) of the slab that ends at this
 * context's z_begin -- for layouts where slabs are not ordered by rank (several slabs per GPU). */
int vcy_halo_install(vcy_ctx* ctx, const void* prev_slab_pack_device);
/* Single-process multi-GPU: copies the last two slices of `below` (the slab that ends at ctx's
 * z_begin, on any device of this process) straight into ctx's halo (peer-to-peer over xGMI). */
int vcy_halo_copy_from(vcy_ctx* ctx, vcy_ctx* below);
/* Single-process multi-GPU, the north star's "single RCCL all-gather of boundary slabs before mesh
 * extraction" (the exchange step of MarchingCubes(), marching_cubes.cc:93-101 reads z-1): `slabs` are
 * ALL z-slabs of one grid in z order (slab i ends where slab i+1 begins), on any devices of this
 * process.  Every slab's pack goes into its device's send buffer, ONE ncclAllGather (one communicator
 * rank per distinct device, ncclCommInitAll; communicators and staging are cached per device list)
 * hands every device every pack, and each slab installs the pack of the slab below it.  librccl.so is
 * opened on first use; VCY_ERR_UNSUPPORTED if it cannot be loaded -- THIS function never falls back to
 * peer copies.  vcy_halo_copy_from is the explicit alternative, and the host layers above take it on exactly
 * that status only where they say so: Python's vacancy_amd.carver.halo_exchange (used by ShardedVoxelCarver and
 * dist.exchange_halo) then copies slab by slab and returns "backend": "peer copies ..."; the C++
 * ShardedVoxelCarver never does it on its own (set_halo_transport(kPeerCopy) asks for it). */
int vcy_halo_allgather(vcy_ctx* const* slabs, int n_slabs);
/* Releases what vcy_halo_allgather keeps between calls (communicators, streams and staging buffers per
 * device set); the next exchange builds them again.  Call when no exchange is in flight. */
void vcy_halo_shutdown(void);
/* One process per GPU WITHOUT torch -- the same single all-gather for a C++ host that runs one process per device
 * (the north star's host model; vacancy_amd/dist.py is its torch.distributed twin; no reference counterpart: the
 * reference is one OpenMP process).  vcy_comm_create: rank `rank` of `world` on `device_id`; rank 0 draws an
 * ncclUniqueId and every rank receives it through `rendezvous` -- "file:<path>" (a path private to the job on a
 * filesystem all ranks of the node see: rank 0 publishes the id by an atomic rename, the others poll for it) or
 * "tcp:<host>:<port>" (rank 0 listens, the others connect, retrying until it does) -- then ncclCommInitRank.  Blocks
 * until all ranks have joined or `timeout_ms` has passed (<= 0: 120 s).  world == 1 needs no rendezvous (NULL is fine).
 * vcy_halo_allgather_ranks: `my_slabs` = this rank's slab contexts in slab order -- the grid's slab ids rank,
 * rank + world, ... (vacancy_amd.dist.slabs_of_rank), every rank holding the SAME number; each packs its last two
 * slices, ONE ncclAllGather (rank-major), every slab installs the pack of the slab below it.
 * vcy_rendezvous_exchange is the rendezvous by itself (128 bytes from rank 0 to every rank): what the CPU tests run. */
typedef struct vcy_comm vcy_comm;
int vcy_comm_create(int rank, int world, int device_id, const char* rendezvous, int timeout_ms, vcy_comm** out);
void vcy_comm_destroy(vcy_comm* comm);
int vcy_halo_allgather_ranks(vcy_comm* comm, vcy_ctx* const* my_slabs, int n_my_slabs);
int vcy_rendezvous_exchange(int rank, int world, const char* rendezvous, void* payload128, int timeout_ms);
/* What the last vcy_halo_allgather of this process did, as text:
 * "backend=rccl op=ncclAllGather version=V ranks=R bytes_per_rank=B calls=N lib=..." or "none". */
const char* vcy_last_collective(void);

/* ---- device memory / stream / timing helpers ----------------------------- */

int vcy_device_count(int* count);
int vcy_sdf_upload(vcy_ctx* ctx, const float* sdf_host, int width, int height,
                   float** sdf_device_out);
int vcy_device_free(vcy_ctx* ctx, void* device_ptr);
int vcy_device_alloc(vcy_ctx* ctx, int64_t bytes, void** device_ptr_out);
int vcy_memcpy_h2d(vcy_ctx* ctx, void* dst_device, const void* src_host, int64_t bytes);
int vcy_memcpy_d2h(vcy_ctx* ctx, void* dst_host, const void* src_device, int64_t bytes);
/* Back to the state right after vcy_create (VoxelGrid::Init: sdf = lowest(), update_num = 0);
 * asynchronous on the context's stream. */
int vcy_reset(vcy_ctx* ctx);
/* Tuning knobs that never change results.  "fused" (default 1): 0 forces one kernel launch
 * per view (the generic kernel) instead of the fused multi-view kernel.  "cull" (default 1): 0 never
 * drops provably idle (brick, view) pairs.  "tile" (default 0 = chosen from the pixel footprint of a
 * voxel): 1 / 2 force the 16 x 16 pixel tile / the 2048-pixel tile of the fused kernel.  "defer" (default 1): the per-view
 * entry points vcy_carve / vcy_carve_device / vcy_carve_silhouette keep a private device copy of the image
 * and queue the view; queued views are carved together, in call order, by one fused launch when the
 * state is next needed (extraction, download, upload, halo, vcy_sync, vcy_timer_end, a batch call) or
 * when 32 wait, so the reference's `for each view: Carve()` loop costs one pass over the grid instead of
 * one per view.  0 carves every view before its call returns.  vcy_reset drops queued views.
 * "shortdiv" (default 1): fx / z in the fused kernel may use a 4- or 6-instruction sequence instead of
 * the full IEEE expansion, but only after the library has checked on the device, for each focal length
 * in use, that the sequence equals IEEE division for EVERY admissible depth (all 2^23 significands in 121
 * binades, about a millisecond once per focal length per process).
 * "mcsweep" (default 0): 1 makes vcy_extract_iso find the surface cells in one sweep over the state with the bit
 * planes in LDS when a voxel row is a power-of-two number of 64-voxel words (nx = 64 ... 2048): 2 % fewer bytes
 * moved than with the bit planes in memory (the default and the path of every other shape), 2 - 30 % more time.
 * "meshkeys" (default 1): vcy_extract_iso returns vcy_mesh.edge_keys; 0 leaves it NULL (nothing is computed for
 * it or copied: a third of the mesh bytes) -- for callers that do not merge z-slabs, i.e. what the reference's
 * MarchingCubes returns.
 * "mcskip" (default 1): vcy_extract_iso does not read bricks whose minimum -- kept per 8 x 8 x 8 brick by the fused
 * carve kernel -- lies above the iso level (they are outside the surface whatever they hold exactly); 0 reads every
 * brick; 1 skips them where that is the faster pass (voxel rows of 1024 and more: at 512^3 the dense pass wins by 7 - 14 %);
 * 2 skips them on any size (what the parity tests ask for).
 * "mcdirect" (default 33554432): vcy_extract_iso lets its last kernel write a mesh whose GUESSED size (the previous
 * extraction's counts + 25 %) is at most this many bytes straight into the page-locked host arrays it returns -- one
 * enqueue, one wait per call; larger meshes are staged in device memory and copied with their exact sizes.  0: always
 * staged.  Results identical.  "mctiming" 1 (or VCY_MC_TIMING=1 in the environment): the host-side phases of every
 * extraction on stderr.
 * "livelist" (default 1): a carve launch of up to 8 views over an already carved grid first lists the workgroups in
 * which some view can still change a voxel (bounds of the views' samples against the kept brick minima / the
 * truncation limit) and starts only those; 0 starts every workgroup and lets each decide for itself.
 * "livesync" (default 1): with the live list, the host waits for the list's length and launches the carve kernel over the
 * listed workgroups only (a single-view launch at 1024^3: 0.115 ms less than starting all 512 K workgroups to have the
 * others leave); 0 starts every workgroup and never waits.
 * "coopstore" (default -1): how a fused launch writes the state back.  1: the four waves of a workgroup exchange their
 * bricks through LDS and store whole 128-byte row segments; 0: every wave stores its own 16-byte pieces; -1: the first
 * for single-view launches (over a carved grid in the weighted-average modes: up to 8 views), the second otherwise.
 * Results are identical.
 * "rowkernel" (default 0): n > 0 or -1 (= 8) sends fused launches of up to n views through the few-view flavour of the
 * carve kernel -- a WAVE walks the four bricks of a row segment, their state requested up front with LDS-direct loads,
 * whole 128-byte row segments stored, no barrier -- instead of a workgroup of four waves with the cooperative write-back.
 * Results identical; measured slower (3.17 against 2.63 ms per weighted-average view at 1024^3: its staging area leaves
 * 2.7 waves per SIMD), so it is off by default and serves as the second implementation the tests compare with.
 * "oneview" (default 1): a fused launch of exactly ONE view -- what every call of the reference's per-view API becomes
 * when an extraction separates the views, examples.cc:117-149 -- takes a kernel instance compiled for one view (the
 * footprint record unpacked into registers, no view loop, no second tile buffer): 15 % fewer vector and 27 % fewer
 * scalar instructions per wave, 2.72 -> 2.43-2.53 ms per weighted-average view at 1024^3, the first view on a fresh grid
 * 1.73-1.92 -> 1.37-1.58, kMax 0.60 -> 0.53; 0: the general instance.  Results identical.
 * "listrecords" (default 1): the live list of a launch of ONE view holds, per listed workgroup, its id, which of its
 * waves are live and their four footprint records (40 bytes instead of 4): a wave learns its record with its id instead
 * of one memory round trip later, and needs no brick minimum for a test the list pass has made (kMax at 1024^3:
 * 0.506 -> 0.496 ms per view).  0: ids only.  Results identical.
 * "eagerstate" (default -1): launches of ONE view ("oneview" 1) over a carved grid request a brick's state next to its footprint
 * record, before the test that lets a wave leave without it, when nearly every started workgroup will need it: listed
 * launches (only live workgroups are started) and launches that skipped their list because the last one held most
 * workgroups; 0 never, 1 every such launch.  One memory round trip less per wave: 2.51 -> 2.35-2.46 ms per
 * weighted-average view at 1024^3, kMax 0.52 -> 0.49 (profiles/r06/eager_state.txt).  Results identical.
 * "ntstore" (default -1 = 1): the cooperative write-back stores its whole row segments as streaming stores (0: ordinary).
 * "recordbytes" (default 0 = 2 GiB): bytes of footprint records one carve launch may take; a launch whose records would
 * be larger is cut into chunks of whole brick layers (2048^3 x 64 views: 8.6 GB of records, four chunks) -- small values
 * let tests run the chunking on small grids.
 * "prologue" (default 0): where a raw-tile launch gets its footprints: 0 or 2 = from the pre-pass's records; 1 = computed
 * in the carve kernel's prologue, one lane per view (one launch whatever the size, and slower: 92.8 against 81.8 ms per
 * step at 2048^3 x 64 views).  Results identical.
 * "recordcache" (default 1): a context remembers which launch its footprint records describe -- the cameras (everything of
 * the views but the images and max_sdf), the slab, the buffer.  A kMax launch of the general flavour with raw tiles, view
 * dropping on, records from the pre-pass in one chunk, window planes and no live list that finds them there skips the
 * pre-pass: the geometry of a record does not depend on the images, and the carve kernel's prologue looks the bounds up
 * itself, with the lookups of the pre-pass.  The first such launch, and every launch after anything of the key has
 * changed, runs the pre-pass as before.  0: every launch runs it.  Results and dropped pairs identical;
 * vcy_get_param "recordcache_hits" counts the launches that reused their records.
 * "carvetimer" (default 0): 1 records HIP events around what runs before the carve kernel (window maxima, pre-pass)
 * and around the carve kernel of every fused launch (vcy_last_carve_ms, vcy_carve_log); setting it clears the log.
 * "lazycount" (default 1): update_num is stored in one byte until more than 255 views have been applied since the fill
 * (a voxel's count cannot exceed that number), then widened in one pass to what voxel_max_update_num needs; 0 allocates
 * the final width at once.  Results are identical; "count_bytes" / "count_bytes_final" read the widths back.
 * "paircount" (default 0): 1 makes every fused launch count the (brick, view) pairs it processes (vcy_last_carve_pairs).
 * "rayskip" (default 1): the rays of vcy_render_hull / vcy_hull_agreement step over 8 x 8 x 8 bricks without a solid voxel
 * and jump to the plane through which they enter the grid; 0: every ray walks crossing by crossing.  Results identical
 * (readable through vcy_get_param).
 * "smoothpad" (default 0): 1 keeps the positions of vcy_smooth_mesh's passes at 16 bytes per vertex (one 16-byte gather)
 * instead of 12 (three 4-byte gathers); measured slower at every size (profiles/smooth/measure_smooth.txt).  Results
 * identical (readable through vcy_get_param).
 * "chainrows" (default 1): the corner table of vcy_extract_iso_chain comes from the cells of the extraction (the walk of the
 * vertex normals: no atomics; rows ascending as written, though the stages sort them regardless); 0: from the faces, as
 * vcy_smooth_mesh builds it.  1 is the faster one at 512^3 and 1024^3 by more than the run-to-run spread
 * (profiles/chain/measure_chain.txt).  Results identical (readable through vcy_get_param).
 * "rasterwide" (default 64, >= 0): a face of vcy_raster_mesh / vcy_mesh_agreement whose candidate box in a view holds more
 * pixels than this is drawn by the 64 lanes of its wave, not by its own lane; 0 sends every face that way.  Results
 * identical (readable through vcy_get_param).
 * "inject_carve_failure" (test hook, default 0): the next `value` applications of views fail with
 * VCY_ERR_INTERNAL before anything is launched -- how the tests exercise the error contract of vcy_carve. */
int vcy_set_param(vcy_ctx* ctx, const char* name, int value);
/* Reads a knob back ("fused", "cull", "tile", "defer", "shortdiv", "mcsweep", "mcskip", "mcdirect", "rowkernel", "oneview", "eagerstate", "listrecords", "ntstore", "livelist", "livesync", "coopstore", "meshkeys",
 * "lazycount", "carvetimer", "recordcache"), "recordcache_hits", "count_bytes" / "count_bytes_final" / "carvelog_dropped" (see above), "div_level": the
 * division sequence the last fused launch was instantiated with (2: 4 instructions, 1: 6, 0: full IEEE expansion), or
 * "brick_min_valid": 1 while the brick minima describe the state (every write since the fill went through the fused kernel),
 * "fresh": 1 while the fill of vcy_create / vcy_reset is known, not written (nothing has been carved or uploaded since). */
int vcy_get_param(vcy_ctx* ctx, const char* name, int* value);
/* Use an existing hipStream_t (e.g. torch's current stream) for all launches. */
int vcy_set_stream(vcy_ctx* ctx, void* hip_stream);
int vcy_get_stream(vcy_ctx* ctx, void** hip_stream_out);
int vcy_sync(vcy_ctx* ctx);
/* hipEvent pair recorded on the context's stream around whatever is launched
 * between begin and end; vcy_timer_end synchronises and returns milliseconds. */
int vcy_timer_begin(vcy_ctx* ctx);
int vcy_timer_end(vcy_ctx* ctx, float* elapsed_ms);

/* With vcy_set_param(ctx, "carvetimer", 1): milliseconds (HIP events on the context's stream) of the last fused
 * carve launch, split into what runs before the carve kernel (footprint pre-pass, live-workgroup list) and the
 * carve kernel itself -- the kernel the roofline is quoted for.  Synchronises with that launch. */
int vcy_last_carve_ms(vcy_ctx* ctx, float* prepass_ms, float* kernel_ms);
/* The whole log "carvetimer" 1 keeps since it was set (or since the last call with clear != 0): one record per chunk
 * of every fused launch (first_chunk[i] != 0 starts a launch; a launch has one chunk unless its footprint records
 * exceed "recordbytes"), up to 8192 records -- later launches are not recorded, and counted:
 * vcy_get_param "carvelog_dropped" (a reader that divides by a step count must check it; vcy_last_carve_ms fails
 * rather than report an older launch).  begin_ms[i] = start of record i
 * (before its window maxima and pre-pass) since the start of record 0; prepass_ms[i] / kernel_ms[i] as for
 * vcy_last_carve_ms.  Any of the arrays may be NULL.  Nothing synchronises while the launches are issued: a sequence
 * of carve steps can be queued back to back and read here afterwards (this call waits for the recorded launches).
 * No reference counterpart (the reference's Timer brackets the loop, voxel_carver.cc:435,492-493). */
int vcy_carve_log(vcy_ctx* ctx, int max_records, float* begin_ms, float* prepass_ms, float* kernel_ms,
                  int32_t* first_chunk, int* n_records, int clear);

/* With vcy_set_param(ctx, "paircount", 1): how many (8 x 8 x 8 brick, view) pairs the last fused launch really
 * processed -- i.e. did not drop as provably idle -- in total and per brick layer of the slab (per_layer may be NULL;
 * *n_layers = layers of the slab), and how many pairs there are.  Synchronises with that launch.  What the scene
 * leaves of the work is visible here (bench.py: "pairs_processed_frac"), and the slab planner's estimate is checked
 * against it. */
int vcy_last_carve_pairs(vcy_ctx* ctx, int64_t* processed, int64_t* total, int64_t* per_layer, int max_layers,
                         int* n_layers);

/* Multi-GPU: where to cut the grid into `n_slabs` z-slabs so that a fused carve of THESE views costs every slab the
 * same (no reference counterpart: the reference's OpenMP loop balances itself with schedule(dynamic, 1),
 * voxel_carver.cc:439-441; z-slabs on different GPUs cannot).  With view dropping the brick layers through the object
 * cost about 1.6x the outer ones, so slabs of equal thickness leave the slowest of 8 GPUs 1.2x over the mean.  `ctx` is
 * any context of the grid on the device that holds the images (typically a small planning context, vcy_create(option,
 * device, 0, 8, ...), destroyed afterwards: only its axis tables and staging buffers are used, its slab is not touched);
 * the estimate -- per brick layer of the WHOLE grid: brick_cost x bricks + (brick, view) pairs a carve will process,
 * found by playing the kernel's drop decisions on upper and lower bounds of every `sample_stride`-th brick's samples
 * (0: every 2nd in x and y) -- is returned in layer_cost[0 .. *n_layers) if not NULL.  brick_cost <= 0: the library's
 * calibrated value.  z_bounds[0 .. n_slabs] receives the cuts (multiples of 8 slices, z_bounds[0] = 0,
 * z_bounds[n_slabs] = nz): the contiguous partition with the smallest largest part.  The same inputs give the same
 * cuts on every rank. */
int vcy_plan_z_slabs(vcy_ctx* ctx, int n_views, const vcy_view* views, const float* const* sdf_device, int n_slabs,
                     int sample_stride, float brick_cost, int32_t* z_bounds, double* layer_cost, int max_layers,
                     int* n_layers);

/* The cut itself, host arithmetic only (no GPU): the contiguous partition of `n_layers` brick layers with the given costs
 * into `n_slabs` parts -- every part at least one layer -- that minimises the largest part and, among those, the sum of
 * squares.  z_bounds[0 .. n_slabs] in slices (multiples of 8, the last one nz; nz in ((n_layers - 1) * 8, n_layers * 8]).
 * What vcy_plan_z_slabs applies to its estimate; callable with measured costs as well. */
int vcy_partition_layers(const double* layer_cost, int n_layers, int n_slabs, int nz, int32_t* z_bounds);

/* Device-side self test of the identities the fast paths rest on (no reference counterpart): the
 * two-instruction reciprocal used for update_num + 1 in the unit-weight weighted average equals the
 * IEEE quotient for every count a u8 / u16 counter can hold.  VCY_OK, or VCY_ERR_INTERNAL with the
 * mismatch in vcy_last_error(). */
int vcy_selftest(vcy_ctx* ctx);

/* Measured device-memory bandwidth of this GPU, for the roofline next to the vendor peak
 * ("print a measured device-memcpy/triad GB/s on the box"): a streaming read of
 * `bytes` (dword loads, eight in flight per lane, the access shape of the grid sweeps here) and a
 * device-to-device copy of `bytes` (counted as read + write).  Best of `reps`; GB/s = 1e9 B/s. */
int vcy_measure_bandwidth(int device_id, uint64_t bytes, int reps, double* read_gbs, double* copy_gbs);

/* Measurement aid, not on the carve path: the shader clock the device runs at WHILE other work is on it.  _start puts one
 * wave on a stream of its own that samples the shader clock counter against the constant 100 MHz reference every ~30 us
 * (at most max_samples samples, then it ends by itself); _stop ends it, frees everything and returns the clock over the
 * whole span (mean_hz) and over its second half (settled_hz: the device idles for a millisecond while the probe is set
 * up, and its clock takes some milliseconds of load to come back), the slowest / fastest interval, the number of samples
 * and the time they cover.  bench.py runs it
 * during six more steps of its workload queued right behind the timed region (a second active hardware queue costs the
 * carve kernel 1.7 %, so not inside it): the VALU issue fraction of the carve kernel is then priced at the clock of the
 * run that is reported, not at the clock of the box the counters were collected on. */
typedef struct vcy_clock_probe vcy_clock_probe;
int vcy_clock_probe_start(int device_id, int max_samples, vcy_clock_probe** out);
int vcy_clock_probe_stop(vcy_clock_probe* probe, double* mean_hz, double* settled_hz, double* min_hz, double* max_hz,
                         int* n_samples, double* covered_ms);

const char* vcy_last_error(void);
/* "vacancy_amd <version> (gfx950) src:<hash>": the hash covers every source file the library was built from
 * (profiles/counters.json entries are stamped with this string; bench.py drops counters of another build). */
const char* vcy_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VACANCY_HIP_H_ */
