// vacancy::VoxelCarver on MI355X.  Same public API as the reference's
// include/vacancy/voxel_carver.h (option structs :20-60, class :95-118, free functions :120-128);
// the voxel grid lives in HBM behind the C-ABI of vacancy_hip.h instead of a std::vector<Voxel>.
#pragma once

#include <array>
#include <cstdint>
#include <memory>
#include <vector>

#include "vacancy/camera.h"
#include "vacancy/common.h"
#include "vacancy/image.h"
#include "vacancy/mesh.h"

namespace vacancy {

enum class VoxelUpdate { kMax = 0, kWeightedAverage = 1 };
enum class SdfInterpolation { kNn = 0, kBilinear = 1 };
enum class UpdateOutsideImage { kNone = 0, kMax = 1 };

struct InvalidSdf {
  static const float kVal;  // std::numeric_limits<float>::lowest()
};

struct VoxelUpdateOption {
  VoxelUpdate voxel_update{VoxelUpdate::kMax};
  SdfInterpolation sdf_interp{SdfInterpolation::kBilinear};
  UpdateOutsideImage update_outside{UpdateOutsideImage::kNone};
  int voxel_max_update_num{255};
  float voxel_update_weight{1.0f};
  bool use_truncation{false};
  float truncation_band{0.1f};
};

struct VoxelCarverOption {
  Eigen::Vector3f bb_max = Eigen::Vector3f(0.0f, 0.0f, 0.0f);  // (the reference leaves both uninitialised)
  Eigen::Vector3f bb_min = Eigen::Vector3f(0.0f, 0.0f, 0.0f);
  float resolution{0.1f};
  bool sdf_minmax_normalize{true};
  VoxelUpdateOption update_option;
};

// One voxel as the reference stores it (include/vacancy/voxel_carver.h:62-72).  On the device the grid is
// a structure of arrays (vacancy_hip.h); this is the host-side view a VoxelGrid snapshot hands out.
struct Voxel {
  Eigen::Vector3i index{-1, -1, -1};      // voxel index
  int id{-1};
  Eigen::Vector3f pos{0.0f, 0.0f, 0.0f};  // center of voxel
  float sdf{0.0f};                        // Signed Distance Function (SDF) value
  int update_num{0};
  bool outside{false};
  bool on_surface{false};
  Voxel();
  ~Voxel();
};

// The reference's VoxelGrid (:74-93) as a HOST container: Init() lays out the voxels exactly like
// VoxelGrid::Init (voxel_carver.cc:276-345); VoxelCarver::Download(VoxelGrid*) fills sdf / update_num
// from the device-resident grid.  Carving never touches it.
class VoxelGrid {
 public:
  VoxelGrid();
  ~VoxelGrid();
  bool Init(const Eigen::Vector3f& bb_max, const Eigen::Vector3f& bb_min, float resolution);
  const Eigen::Vector3i& voxel_num() const;
  const Voxel& get(int x, int y, int z) const;
  Voxel* get_ptr(int x, int y, int z);
  float resolution() const;
  void ResetOnSurface();
  bool initialized() const;

 private:
  std::vector<Voxel> voxels_;
  Eigen::Vector3f bb_max_;
  Eigen::Vector3f bb_min_;
  float resolution_{-1.0f};
  Eigen::Vector3i voxel_num_{0, 0, 0};
  int xy_slice_num_{0};
};

// How ColorMesh combines the photographs that see a vertex: vcy_color_option of vacancy_hip.h, where the rule is
// defined.  No counterpart in the reference.
enum class ColorMode { kMean = 0, kWeighted = 1, kBest = 2 };
struct ColorOption {
  ColorMode mode{ColorMode::kWeighted};                 // kWeighted: by |cos| between the normal and the viewing ray
  SdfInterpolation interp{SdfInterpolation::kBilinear};
  float depth_tolerance{-1.0f};                         // world units; < 0: 1.5 * the carver's resolution
  float min_cos{0.0f};                                  // kWeighted, kBest: a view contributes iff its weight > min_cos
  Eigen::Vector3f fallback = Eigen::Vector3f(128.0f, 128.0f, 128.0f);  // colour of a vertex no view sees
  bool occlusion_from_mesh{false};                      // the depth images come from the mesh itself (RenderMesh), not the hull
};

// The stages of VoxelCarver::ExtractIsoSurfaceChain and what it reports beside the mesh.  No counterpart in the reference.
struct ChainOption {
  double iso_level{0.0};
  bool linear_interp{true};
  bool smooth{false};           // SmoothMesh(iterations, lambda, mu, pin_boundary)
  int iterations{10};
  float lambda{0.5f};
  float mu{-0.53f};
  bool pin_boundary{false};
  int decimate{0};              // 0 none, 1 DecimateMesh(cell, mode), 2 DecimateMeshQuadric(cell, regularize)
  float cell{0.0f};
  int mode{0};
  float regularize{1e-3f};
  bool maps{false};             // fill ChainReport::vertex_map / face_source (decimate != 0)
};
struct ChainReport {
  std::int64_t n_extracted_vertices{0}, n_extracted_faces{0};  // of the mesh ExtractIsoSurface would have returned
  std::int64_t n_fallback{0};                                  // decimate == 2: output vertices that kept the mean
  std::vector<std::int32_t> vertex_map;   // per extracted vertex: its output vertex or -1
  std::vector<std::int32_t> face_source;  // per output face: the extracted face it was
};

// One 6-connected component of the solid voxels (update_num >= 1 and sdf < iso_level): vcy_component of vacancy_hip.h.
// No counterpart in the reference.
struct VoxelComponent {
  std::int64_t label{0};     // smallest voxel id (z*nx*ny + y*nx + x) of the component
  std::int64_t n_voxels{0};
  Eigen::Vector3i bb_min{0, 0, 0}, bb_max{0, 0, 0};  // inclusive voxel-index bounds
};

class VoxelCarver {
 public:
  VoxelCarver();
  explicit VoxelCarver(VoxelCarverOption option);
  ~VoxelCarver();
  VoxelCarver(const VoxelCarver&) = delete;
  VoxelCarver& operator=(const VoxelCarver&) = delete;

  void set_option(VoxelCarverOption option);
  void set_device(int device_id);  // default 0
  bool Init();
  bool Carve(const Camera& camera, const Image1b& silhouette, const Eigen::Vector2i& roi_min,
             const Eigen::Vector2i& roi_max, Image1f* sdf);
  bool Carve(const Camera& camera, const Eigen::Vector2i& roi_min, const Eigen::Vector2i& roi_max,
             const Image1f& sdf);
  bool Carve(const Camera& camera, const Image1b& silhouette, Image1f* sdf);
  bool Carve(const Camera& camera, const Image1b& silhouette);
  bool Carve(const Camera& camera, const Image1f& sdf);
  // All views in one fused pass over the grid.  The first form is the reference's signature
  // (voxel_carver.h:113); Camera is abstract there as here, so callers hold cameras by pointer --
  // examples.cc:108-128 keeps std::shared_ptr<Camera> -- and the other two forms take those directly.
  bool Carve(const std::vector<Camera>& cameras, const std::vector<Image1b>& silhouettes);
  bool Carve(const std::vector<std::shared_ptr<Camera>>& cameras, const std::vector<Image1b>& silhouettes);
  bool Carve(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes);
  void ExtractVoxel(Mesh* mesh, bool inside_empty = false);
  void ExtractIsoSurface(Mesh* mesh, double iso_level = 0.0, bool linear_interp = true);
  // with_normals: the mesh's normals(), face_normals() and normal_indices() as well -- Mesh::CalcNormal() of the result,
  // computed on the device behind the extraction (vcy_extract_iso_normals), bit-equal to calling CalcNormal() afterwards
  void ExtractIsoSurface(Mesh* mesh, double iso_level, bool linear_interp, bool with_normals);

  // Connected components of the hull, labelled on the device (vcy_label_components): the list, largest first (ties:
  // the lower label).  KeepLargestComponents (vcy_keep_components) carves away, in place, every component that is not
  // among the `largest` largest (<= 0: any number) or has fewer than `min_voxels` voxels -- their voxels get
  // sdf = fill_sdf (finite, >= iso_level), so the phantom volumes and specks of a hull of few views are gone from
  // every later ExtractIsoSurface / ExtractVoxel, and further Carve() calls go on at full speed.  false + LOGE on
  // an error.  ShardedVoxelCarver has the same two members (the pieces of the z-slabs are merged across the seams).
  bool LabelComponents(std::vector<VoxelComponent>* components, double iso_level = 0.0);
  bool KeepLargestComponents(int largest = 1, std::int64_t min_voxels = 0, double iso_level = 0.0, float fill_sdf = 1.0f);

  // The Euclidean distance field of the hull, on the device (the definitions are in vacancy_hip.h, "distance field of the
  // hull").  DistanceField (vcy_distance_field): per voxel, in reference order, the signed squared distance in voxels to
  // the nearest voxel of the other class -- negative where solid --, exact up to radius * radius, radius * radius + 1
  // beyond; the state is not changed.  Redistance (vcy_redistance) rewrites sdf of every touched voxel to
  // (sqrt(min(d2, radius^2)) - 0.5) * resolution, negated where solid: ExtractIsoSurface(mesh, +r) is then the hull grown
  // by r, (mesh, -r) the hull shrunk by r, for |r| < (radius - 0.5) * resolution.  CloseHull is the morphological closing
  // by a ball of radius_voxels voxels -- Redistance(iso_level, R), Redistance(r, R), Redistance(-r, R) with
  // r = radius_voxels * resolution, R = ceil(radius_voxels) + 2 -- which bridges the gaps and pits of up to about twice
  // that width; it refuses a radius on which the closing ties ((radius_voxels + 0.5)^2 a sum of three squares, such as
  // 1.5: pick 1.3, 2.3, ...).  false + LOGE on an error.  ShardedVoxelCarver has the three members for one slab.
  bool DistanceField(std::vector<std::int32_t>* d2, double iso_level = 0.0, int radius = 8);
  bool Redistance(double iso_level = 0.0, int radius = 8);
  bool CloseHull(float radius_voxels, double iso_level = 0.0);

  // The hull as camera `camera` sees it (vcy_render_hull: the first solid voxel on every pixel's ray, exact -- the
  // definition is in vacancy_hip.h): depth = camera depth of the hit, +inf where the ray meets no solid voxel;
  // silhouette (optional) = 255 where it does.  The images get the camera's width x height, the ROI is the whole image.
  // HullAgreement (vcy_hull_agreement) renders every camera and compares with the input silhouettes (non-zero = object)
  // on the device: per view the pixel counts {mask && hull, mask && !hull, !mask && hull}.  false + LOGE on an error.
  bool RenderHull(const Camera& camera, Image1f* depth, Image1b* silhouette = nullptr, double iso_level = 0.0);
  bool HullAgreement(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes,
                     std::vector<std::array<std::int64_t, 3>>* counts, double iso_level = 0.0);
  bool HullAgreement(const std::vector<Camera>& cameras, const std::vector<Image1b>& silhouettes,
                     std::vector<std::array<std::int64_t, 3>>* counts);

  // An indexed mesh as camera `camera` sees it (vcy_raster_mesh: the nearest face over every pixel centre, exact and
  // watertight -- the definition is in vacancy_hip.h): depth = camera depth, RenderHull's quantity, +inf where no face is
  // seen; silhouette (optional) = 255 where one is.  Any mesh will do -- smoothed, decimated, edited, merged --, the voxel
  // state is not touched, there is no near-plane clipping (a face with a vertex behind the camera is not drawn).
  // MeshAgreement (vcy_mesh_agreement) is HullAgreement for the mesh: per view {mask && mesh, mask && !mesh, !mask && mesh}.
  // false + LOGE on an error.  last_raster_ms(): device milliseconds of the raster and the resolve launches.
  bool RenderMesh(const Mesh& mesh, const Camera& camera, Image1f* depth, Image1b* silhouette = nullptr);
  bool MeshAgreement(const Mesh& mesh, const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes,
                     std::vector<std::array<std::int64_t, 3>>* counts);
  std::array<float, 2> last_raster_ms() const;

  // The mesh as a picture (vcy_shade_mesh: per-vertex attributes interpolated, perspective-correct, at the face RenderMesh
  // sees in every pixel -- the definition is in vacancy_hip.h): image = the rounded vertex colours (ColorVertices fills
  // them), or with from_normals the normal map 127.5 * n + 127.5 of normals(); black where no face is seen.  The call
  // refuses a mesh whose chosen attribute array is empty.  MeshPhotoError (vcy_mesh_photo_error) renders the coloured mesh
  // into every camera and compares it with the photographs on the device, under the silhouettes when there are any (an
  // empty vector: none): per view {n, sad r, g, b, ssd r, g, b} over the n pixels the mesh covers.  false + LOGE on an
  // error.  last_shade_ms(): device milliseconds of the raster and the shade launches.
  bool ShadeMesh(const Mesh& mesh, const Camera& camera, Image3b* image, bool from_normals = false);
  bool MeshPhotoError(const Mesh& mesh, const std::vector<const Camera*>& cameras, const std::vector<Image3b>& photos,
                      const std::vector<Image1b>& silhouettes, std::vector<std::array<std::int64_t, 7>>* sums);
  std::array<float, 2> last_shade_ms() const;

  // The robust visual hull (vcy_carve_robust_silhouettes; the definition is in vacancy_hip.h): REPLACES the state by, per
  // voxel, the (tolerate + 1)-th largest sample over all cameras instead of the largest, so that a voxel is carved only
  // when more than `tolerate` (0 .. 3) views say outside -- up to `tolerate` wrong masks no longer remove a part of the
  // object.  overruled (optional) gets one count per view: the voxels kept solid at iso_level although that view says
  // outside; a bad mask shows as a count far above the others'.  kMax options only, up to 1024 views.  false + LOGE on an
  // error, the state then stays as it was.
  bool CarveRobust(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes, int tolerate,
                   std::vector<std::int64_t>* overruled = nullptr, double iso_level = 0.0);
  bool CarveRobust(const std::vector<std::shared_ptr<Camera>>& cameras, const std::vector<Image1b>& silhouettes, int tolerate,
                   std::vector<std::int64_t>* overruled = nullptr, double iso_level = 0.0);

  // Carve from depth images (vcy_carve_depth; the definition is in vacancy_hip.h): per voxel and view the sample
  // (depth(pixel) - z_c) / band, clamped to 1 and dropped below -1, through the option's update rule -- the projective
  // TSDF, which recovers the concavities a visual hull cannot.  depth has RenderHull's meaning (camera depth, +inf where
  // the ray meets nothing; NaN, 0 and negative values are "no measurement") and gives the view its size; the ROI is the
  // whole image; band is in world units, finite and > 0.  Depth and silhouette views may be applied to the same state.
  // false + LOGE on an error, the state then stays as it was.  last_depth_ms(): device milliseconds of the last call's
  // launches.
  bool CarveDepth(const Camera& camera, const Image1f& depth, float band);
  bool CarveDepth(const std::vector<const Camera*>& cameras, const std::vector<Image1f>& depths, float band);
  bool CarveDepth(const std::vector<std::shared_ptr<Camera>>& cameras, const std::vector<Image1f>& depths, float band);
  float last_depth_ms() const;

  // Fills mesh->vertex_colors() (float RGB in 0 .. 255, what WritePly emits) from the photographs, on the device
  // (vcy_color_vertices): a view colours a vertex it sees -- whose camera depth is at most the hull's depth at its pixel,
  // ray-cast here at iso_level, + depth_tolerance.  photos[i] belongs to cameras[i] and gives the view its size; the ROI
  // is the whole image.  Computes the mesh's normals (CalcNormal) if it has none and the mode needs them.
  // option.occlusion_from_mesh: the depth images are RenderMesh's of the mesh being coloured instead of the hull's -- for
  // a smoothed or decimated mesh, which the voxel staircase no longer describes; iso_level is not used then.
  // false + LOGE on an error, the colours then stay as they were.
  bool ColorMesh(Mesh* mesh, const std::vector<const Camera*>& cameras, const std::vector<Image3b>& photos,
                 const ColorOption& option = ColorOption(), double iso_level = 0.0);

  // Mesh::Smooth on this carver's device (vcy_smooth_mesh), the same bits: the mesh goes up, the incidence table is built
  // there, the passes and -- with_normals -- Mesh::CalcNormal() of the result run there, the vertices (and normals) come
  // back.  Any mesh will do, not only one this carver extracted; the voxel state is not touched.  false + LOGE on an
  // error, the mesh then stays as it was.  last_smooth_ms(): device milliseconds of the table, the passes, the normals.
  bool SmoothMesh(Mesh* mesh, int iterations, float lambda = 0.5f, float mu = -0.53f, bool pin_boundary = false,
                  bool with_normals = false);
  std::array<float, 3> last_smooth_ms() const;

  // Mesh::Decimate on this carver's device (vcy_decimate_mesh), the same bits, with the cell lattice at this carver's
  // bb_min, so that cells of `cell` = k * resolution hold k x k x k voxels: the mesh goes up, clusters, surviving faces
  // and -- with_normals -- Mesh::CalcNormal() of the result are computed there, the decimated mesh comes back.  Any mesh
  // will do, not only one this carver extracted; the voxel state is not touched.  false + LOGE on an error, the mesh
  // then stays as it was.  last_decimate_ms(): device milliseconds of the clusters, the faces, the emit, the normals.
  bool DecimateMesh(Mesh* mesh, float cell, int mode = 0, bool with_normals = false);
  std::array<float, 4> last_decimate_ms() const;
  // Mesh::DecimateQuadric on this carver's device (vcy_decimate_mesh_quadric), the same bits, under DecimateMesh's terms.
  // *n_fallback: the output vertices that kept their cluster's mean.  last_decimate_ms() reports this call's four groups,
  // last_quadric_ms() the quadric stage alone (it is part of the clusters).
  bool DecimateMeshQuadric(Mesh* mesh, float cell, float regularize = 1e-3f, bool with_normals = false,
                           std::int64_t* n_fallback = nullptr);
  float last_quadric_ms() const;

  // ExtractIsoSurface, SmoothMesh, DecimateMesh[Quadric] and Mesh::CalcNormal() in one call (vcy_extract_iso_chain), the
  // mesh staying on the device between the stages: the bits of the separate members in that order, smoothing first.  The
  // mesh gets vertices, faces and normals as ExtractIsoSurface(..., with_normals = true) gives them.  false + LOGE on an
  // error, the mesh is then empty.  last_chain_ms(): device milliseconds of the extraction, the corner table, the passes,
  // the clusters, the quadric stage inside them, faces + emit, the normals, and the call's wall time.
  bool ExtractIsoSurfaceChain(Mesh* mesh, const ChainOption& option, ChainReport* report = nullptr);
  std::array<float, 8> last_chain_ms() const;

  // grid access for host-side consumers: global dims and the voxel state in id order
  Eigen::Vector3i voxel_num() const;
  bool Download(std::vector<float>* sdf, std::vector<int>* update_num) const;
  // host snapshot of the grid in the reference's own types: grid->Init(option) + sdf / update_num of every voxel
  bool Download(VoxelGrid* grid) const;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

void DistanceTransformL1(const Image1b& mask, const Eigen::Vector2i& roi_min, const Eigen::Vector2i& roi_max,
                         Image1f* dist);
void MakeSignedDistanceField(const Image1b& mask, const Eigen::Vector2i& roi_min, const Eigen::Vector2i& roi_max,
                             Image1f* dist, bool minmax_normalize, bool use_truncation, float truncation_band);
void SignedDistance2Color(const Image1f& sdf, Image3b* vis_sdf, float min_negative_d, float max_positive_d);

}  // namespace vacancy
