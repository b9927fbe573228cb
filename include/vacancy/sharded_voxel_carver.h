// ShardedVoxelCarver: the VoxelCarver API over several GPUs of one node from ONE process.
//
// The grid is cut into z-slabs (k per device, dealt cyclically; one per device by default).  Where it is cut
// matters: with view dropping the slabs through the object cost 1.6x the outer ones, so PlanPartition() places
// the cuts where a carve of the given views is predicted to cost every slab the same (vcy_plan_z_slabs);
// without it the slabs are of equal thickness.  Carving needs no exchange (a batch of views shares ONE producer of SDF
// images: device r builds views r, r + R, ..., one RCCL all-gather per chunk of 32 hands every device all of them,
// vcy_carve_batch_silhouettes_sharded), extraction needs the two slices below
// each slab -- ONE RCCL all-gather of every slab's boundary slices (vcy_halo_allgather: one
// communicator rank per device, ncclCommInitAll) -- and the per-slab meshes are stitched by edge key
// into exactly the mesh a single VoxelCarver returns.  (The one-process-per-GPU form of the same
// scheme is vacancy_amd/dist.py + bench.py, where the all-gather goes through torch.distributed.)
#pragma once

#include <memory>
#include <vector>

#include "vacancy/voxel_carver.h"

namespace vacancy {

class ShardedVoxelCarver {
 public:
  ShardedVoxelCarver(VoxelCarverOption option, std::vector<int> device_ids, int slabs_per_device = 1);
  ~ShardedVoxelCarver();
  ShardedVoxelCarver(const ShardedVoxelCarver&) = delete;
  ShardedVoxelCarver& operator=(const ShardedVoxelCarver&) = delete;

  // Before Init(): cuts of equal predicted carve cost for these views (a small planning context on the first
  // device builds their SDF images and plays the kernel's drop decisions per brick layer; about a millisecond
  // at 1024^3 x 32 views).  The views carved later need not be these -- a camera rig that stays put is the case it
  // is made for.  false (and equal thickness at Init) if the plan cannot be made.
  bool PlanPartition(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes);
  // ... or cuts from elsewhere: slab_count + 1 increasing z values from 0 to nz, every slab >= 2 slices.
  void set_z_bounds(const std::vector<int>& z_bounds);
  const std::vector<int>& z_bounds() const;  // of the slabs Init() created
  bool Init();
  int slab_count() const;
  // how the halo slices travel before extraction: the RCCL all-gather (default) or explicit
  // peer-to-peer copies slab by slab (vcy_halo_copy_from)
  enum class HaloTransport { kRcclAllGather, kPeerCopy };
  void set_halo_transport(HaloTransport t);
  // one view / a batch of views into every slab (slabs of different devices run concurrently)
  bool Carve(const Camera& camera, const Image1b& silhouette);
  bool Carve(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes);
  void ExtractIsoSurface(Mesh* mesh, double iso_level = 0.0, bool linear_interp = true);
  // with_normals: Mesh::CalcNormal() of the merged mesh.  Every slab's normals come from its own device
  // (vcy_extract_iso_normals_slab); a vertex on a slab's boundary plane has faces in two slabs, so those -- a plane's
  // worth per seam -- are finished on the host (vcy_mesh_normals_host_seam).  The bits equal VoxelCarver's device result
  void ExtractIsoSurface(Mesh* mesh, double iso_level, bool linear_interp, bool with_normals);
  // VoxelCarver::ExtractVoxel over the slabs: the keep predicate and the compaction run on every slab's device, the
  // kept voxels of all slabs are walked in z order by ONE drifting cube on the host -- the reference's arithmetic
  // (extract_voxel.cc:290-311), so the mesh equals a single VoxelCarver's array for array.
  void ExtractVoxel(Mesh* mesh, bool inside_empty = false);
  // VoxelCarver::LabelComponents / KeepLargestComponents over the slabs: every slab labels its own slices on its device
  // (vcy_label_components_slab), one plane of labels per seam and the lists of touching pieces go through the host, which
  // joins the pieces (vcy_merge_components_host); the filter is every slab's own kernel (vcy_keep_components_slab), brick
  // minima kept current per slab.  The list, and the state afterwards, equal a single VoxelCarver's.  The halos are
  // stale after the filter as after a Carve(); the extractions exchange them before they read them.
  bool LabelComponents(std::vector<VoxelComponent>* components, double iso_level = 0.0);
  bool KeepLargestComponents(int largest = 1, std::int64_t min_voxels = 0, double iso_level = 0.0, float fill_sdf = 1.0f);
  // VoxelCarver::DistanceField / Redistance / CloseHull for a grid of ONE slab.  The transform of a z-slab needs `radius`
  // slices of its neighbours per seam, which these three do not exchange (the ...Slabs members below do): with more than
  // one slab the three log that and return false, the state untouched.
  bool DistanceField(std::vector<std::int32_t>* d2, double iso_level = 0.0, int radius = 8);
  bool Redistance(double iso_level = 0.0, int radius = 8);
  bool CloseHull(float radius_voxels, double iso_level = 0.0);
  // The same three for ANY number of slabs, with the results of a single VoxelCarver on the whole grid, bit for bit: every
  // slab runs the x and the y pass over its own slices on its device (vcy_distance_slab_begin), its lowest and highest
  // min(radius, own slices) planes of 16-bit values go through the host -- never a slab's volume; a slab thinner than the
  // radius passes its neighbours' planes on --, and every slab finishes with the z pass over its columns extended by those
  // planes (vcy_distance_field_slab / vcy_redistance_slab).  Every slab finishes one step before any slab begins the next.
  // DistanceFieldSlabs: the slabs' fields one behind the other in z order.  RedistanceSlabs: *n_rewritten (may be null) the
  // touched voxels of the grid; the halos are stale afterwards as after a Carve().  CloseHullSlabs: the three steps and the
  // tie rule of VoxelCarver::CloseHull; a refused radius leaves the state untouched.
  bool DistanceFieldSlabs(std::vector<std::int32_t>* d2, double iso_level = 0.0, int radius = 8);
  bool RedistanceSlabs(double iso_level = 0.0, int radius = 8, std::int64_t* n_rewritten = nullptr);
  bool CloseHullSlabs(float radius_voxels, double iso_level = 0.0);
  // VoxelCarver::SmoothMesh for the merged mesh: the call needs a device and a stream, not the voxels, so the first slab's
  // context runs it (vcy_smooth_mesh).  The same bits as VoxelCarver::SmoothMesh and Mesh::Smooth.
  bool SmoothMesh(Mesh* mesh, int iterations, float lambda = 0.5f, float mu = -0.53f, bool pin_boundary = false,
                  bool with_normals = false);
  // VoxelCarver::DecimateMesh for the merged mesh, on the first slab's context (vcy_decimate_mesh), the lattice at the
  // grid's bb_min.  The same bits as VoxelCarver::DecimateMesh.
  bool DecimateMesh(Mesh* mesh, float cell, int mode = 0, bool with_normals = false);
  // VoxelCarver::DecimateMeshQuadric for the merged mesh, on the first slab's context (vcy_decimate_mesh_quadric): the same bits.
  bool DecimateMeshQuadric(Mesh* mesh, float cell, float regularize = 1e-3f, bool with_normals = false,
                           std::int64_t* n_fallback = nullptr);
  // VoxelCarver::RenderMesh / MeshAgreement for the merged mesh, on the first slab's context (vcy_raster_mesh,
  // vcy_mesh_agreement): the same bits.
  bool RenderMesh(const Mesh& mesh, const Camera& camera, Image1f* depth, Image1b* silhouette = nullptr);
  bool MeshAgreement(const Mesh& mesh, const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes,
                     std::vector<std::array<std::int64_t, 3>>* counts);
  // VoxelCarver::ShadeMesh / MeshPhotoError for the merged mesh, on the first slab's context (vcy_shade_mesh,
  // vcy_mesh_photo_error): the same bits and sums.
  bool ShadeMesh(const Mesh& mesh, const Camera& camera, Image3b* image, bool from_normals = false);
  bool MeshPhotoError(const Mesh& mesh, const std::vector<const Camera*>& cameras, const std::vector<Image3b>& photos,
                      const std::vector<Image1b>& silhouettes, std::vector<std::array<std::int64_t, 7>>* sums);
  std::array<float, 2> last_shade_ms() const;
  // VoxelCarver::RenderHull / HullAgreement over the slabs: RenderHullSlabs / HullAgreementSlabs below.  These two older
  // names keep logging an error and returning false.
  bool RenderHull(const Camera& camera, Image1f* depth, Image1b* silhouette = nullptr);
  bool HullAgreement(const std::vector<Camera>& cameras, const std::vector<Image1b>& silhouettes,
                     std::vector<std::array<std::int64_t, 3>>* counts);
  // Every slab renders the image of its own slices on its device (vcy_render_hull_slab: the global path, hits only in
  // the owned slices; no halo exchange), a host thread per slab; the host merges by the rule of vcy_render_merge_host --
  // per pixel the hit of the first slab in the ray's direction of travel along z, NOT the smallest depth, which two slabs
  // can share.  The images equal VoxelCarver::RenderHull's bit for bit wherever the grid is cut.  HullAgreementSlabs
  // brings one hit bit per pixel and slab to the host and counts there (vcy_hull_agreement_host).
  bool RenderHullSlabs(const Camera& camera, Image1f* depth, Image1b* silhouette = nullptr, double iso_level = 0.0);
  bool HullAgreementSlabs(const std::vector<Camera>& cameras, const std::vector<Image1b>& silhouettes,
                          std::vector<std::array<std::int64_t, 3>>* counts, double iso_level = 0.0);
  bool HullAgreementSlabs(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes,
                          std::vector<std::array<std::int64_t, 3>>* counts, double iso_level = 0.0);

 private:
  bool ExchangeHalo();
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace vacancy
