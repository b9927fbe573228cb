// vacancy::VoxelCarver facade: the reference's class API (src/vacancy/voxel_carver.cc:367-543)
// forwarding to the HIP path through the C-ABI of include/vacancy_hip.h.
#include "vacancy/voxel_carver.h"

#include <chrono>
#include <cstring>
#include <limits>

#include "c_abi_structs.h"
#include "mesh_copy.h"
#include "mesh_decimate.h"
#include "mesh_raster.h"
#include "mesh_smooth.h"

namespace vacancy {

const float InvalidSdf::kVal = std::numeric_limits<float>::lowest();

namespace {
double NowMs() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

using detail::ToView;

// Per-view Carve() calls only queue their view; the loop the reference times as "VoxelCarver::Carve main loop"
// (voxel_carver.cc:435,492-493) runs when the queue is applied -- inside the next call that reads the state.  The
// library keeps HIP-event times of every fused launch ("carvetimer"); they are logged here, one line per launch, in the
// reference's words, by the calls that apply the queue.
// The timer costs three event records per fused launch: it is only on while the log level emits LOGI (checked at every
// call that applies the queue, so a level changed after Init is followed; `*timer_on` is the facade's view of the param).
void LogAppliedCarves(vcy_ctx* ctx, bool* timer_on) {
  const bool want = get_log_level() <= LogLevel::kInfo;
  if (*timer_on) {
    // every record the library holds (its log ends at 8192 launches, vcy_carve_log), not a first screenful of them
    constexpr int kCap = 8192;
    std::vector<float> pre(kCap), ker(kCap);
    std::vector<int32_t> first(kCap);
    int n = 0;
    if (vcy_carve_log(ctx, kCap, nullptr, pre.data(), ker.data(), first.data(), &n, 1) == VCY_OK && want) {
      double ms = 0.0;
      for (int i = 0; i < n; ++i) {
        if (first[i] && i > 0) {
          LOGI("VoxelCarver::Carve main loop %02f\n", ms);
          ms = 0.0;
        }
        ms += static_cast<double>(pre[i]) + ker[i];
      }
      if (n > 0) LOGI("VoxelCarver::Carve main loop %02f\n", ms);
    }
  }
  if (want != *timer_on) {
    vcy_set_param(ctx, "carvetimer", want ? 1 : 0);
    *timer_on = want;
  }
}
}  // namespace

Voxel::Voxel() {}
Voxel::~Voxel() {}

VoxelGrid::VoxelGrid() {}
VoxelGrid::~VoxelGrid() {}

// The container of reference voxel_carver.cc:276-345.  Its sizes and voxel centres come from the library -- the
// arithmetic of VoxelGrid::Init lives in ONE place, next to the device's axis tables (vcy_compute_dims,
// vcy_axis_positions; vcy_download_positions returns the same values bit for bit) -- and are only laid out here.
bool VoxelGrid::Init(const Eigen::Vector3f& bb_max, const Eigen::Vector3f& bb_min, float resolution) {
  const float mn[3] = {bb_min.x(), bb_min.y(), bb_min.z()}, mx[3] = {bb_max.x(), bb_max.y(), bb_max.z()};
  int32_t n[3];
  if (vcy_compute_dims(mn, mx, resolution, n) != VCY_OK) {  // (resolution, bounding box: the reference's checks and texts)
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  if (static_cast<long long>(n[0]) * n[1] * n[2] > std::numeric_limits<int>::max()) {  // 32-bit ids, :298-301
    LOGE("too many voxels\n");
    return false;
  }
  const bool empty = n[0] <= 0 || n[1] <= 0 || n[2] <= 0;  // (the reference returns true with no voxels, :292-345)
  std::vector<float> axis[3];
  for (int a = 0; a < 3 && !empty; ++a) {
    axis[a].resize(static_cast<size_t>(n[a]));
    if (vcy_axis_positions(mn, mx, resolution, a, axis[a].data()) != VCY_OK) return false;
  }
  bb_max_ = bb_max;
  bb_min_ = bb_min;
  resolution_ = resolution;
  voxel_num_ = Eigen::Vector3i(n[0], n[1], n[2]);
  xy_slice_num_ = n[0] * n[1];
  voxels_.clear();
  if (empty) return true;
  voxels_.resize(static_cast<size_t>(n[0]) * n[1] * n[2]);
  size_t id = 0;
  for (int z = 0; z < n[2]; z++)
    for (int y = 0; y < n[1]; y++)
      for (int x = 0; x < n[0]; x++, id++) {
        Voxel& voxel = voxels_[id];
        voxel.index = Eigen::Vector3i(x, y, z);
        voxel.id = static_cast<int>(id);
        voxel.pos = Eigen::Vector3f(axis[0][x], axis[1][y], axis[2][z]);
        voxel.sdf = InvalidSdf::kVal;
      }
  return true;
}
const Eigen::Vector3i& VoxelGrid::voxel_num() const { return voxel_num_; }
const Voxel& VoxelGrid::get(int x, int y, int z) const {
  return voxels_[static_cast<size_t>(z) * xy_slice_num_ + (static_cast<size_t>(y) * voxel_num_.x() + x)];
}
Voxel* VoxelGrid::get_ptr(int x, int y, int z) {
  return &voxels_[static_cast<size_t>(z) * xy_slice_num_ + (static_cast<size_t>(y) * voxel_num_.x() + x)];
}
float VoxelGrid::resolution() const { return resolution_; }
void VoxelGrid::ResetOnSurface() {
  for (Voxel& v : voxels_) v.on_surface = false;
}
bool VoxelGrid::initialized() const { return !voxels_.empty(); }

struct VoxelCarver::Impl {
  VoxelCarverOption option;
  vcy_ctx* ctx = nullptr;
  int device = 0;
  bool carve_timer = false;  // "carvetimer" as last set by this facade (LogAppliedCarves)
  ~Impl() { vcy_destroy(ctx); }
};

VoxelCarver::VoxelCarver() : impl_(new Impl) {}
VoxelCarver::VoxelCarver(VoxelCarverOption option) : impl_(new Impl) { set_option(option); }
VoxelCarver::~VoxelCarver() {}

void VoxelCarver::set_option(VoxelCarverOption option) { impl_->option = option; }
void VoxelCarver::set_device(int device_id) { impl_->device = device_id; }

bool VoxelCarver::Init() {
  vcy_destroy(impl_->ctx);
  impl_->ctx = nullptr;
  const vcy_carver_option c = detail::ToC(impl_->option);
  if (vcy_create(&c, impl_->device, 0, -1, &impl_->ctx) != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  // one context holds the whole grid: no slab merge, so the mesh needs no edge keys (the reference's
  // MarchingCubes returns vertices and faces)
  vcy_set_param(impl_->ctx, "meshkeys", 0);
  impl_->carve_timer = get_log_level() <= LogLevel::kInfo;  // (three events per fused launch: only when they are logged)
  vcy_set_param(impl_->ctx, "carvetimer", impl_->carve_timer ? 1 : 0);
  return true;
}

bool VoxelCarver::Carve(const Camera& camera, const Image1b& silhouette, const Eigen::Vector2i& roi_min,
                        const Eigen::Vector2i& roi_max, Image1f* sdf) {
  if (!impl_->ctx) {
    LOGE("VoxelCarver::Carve voxel grid has not been initialized\n");
    return false;
  }
  sdf->Init(silhouette.width(), silhouette.height(), 0.0f);
  bool known = true;
  const vcy_view v = ToView(camera, roi_min, roi_max, silhouette.width(), silhouette.height(), &known);
  if (!known) return false;
  const double t0 = NowMs();
  // The view is QUEUED by the library (vcy_set_param "defer"): this call returns after the silhouette has
  // been uploaded and its SDF built and downloaded; queued views are carved together by one fused
  // launch when the state is next needed (Extract*, Download).  No vcy_sync here -- it would flush the
  // queue after every view and turn the fused pass into one pass per view.
  const int rc = vcy_carve_silhouette(impl_->ctx, &v, silhouette.data().data(), sdf->data_ptr()->data());
  LOGI("VoxelCarver::Carve make SDF + enqueue %02f\n", NowMs() - t0);
  if (rc != VCY_OK) LOGE("%s\n", vcy_last_error());
  return rc == VCY_OK;
}

bool VoxelCarver::Carve(const Camera& camera, const Eigen::Vector2i& roi_min, const Eigen::Vector2i& roi_max,
                        const Image1f& sdf) {
  if (!impl_->ctx) {
    LOGE("VoxelCarver::Carve voxel grid has not been initialized\n");
    return false;
  }
  bool known = true;
  const vcy_view v = ToView(camera, roi_min, roi_max, sdf.width(), sdf.height(), &known);
  if (!known) return false;
  const double t0 = NowMs();
  const int rc = vcy_carve(impl_->ctx, &v, sdf.data().data());  // copied and queued, see above
  LOGI("VoxelCarver::Carve enqueue %02f\n", NowMs() - t0);
  if (rc != VCY_OK) LOGE("%s\n", vcy_last_error());
  return rc == VCY_OK;
}

bool VoxelCarver::Carve(const Camera& camera, const Image1b& silhouette, Image1f* sdf) {
  return Carve(camera, silhouette, Eigen::Vector2i(0, 0),
               Eigen::Vector2i(silhouette.width() - 1, silhouette.height() - 1), sdf);
}

bool VoxelCarver::Carve(const Camera& camera, const Image1b& silhouette) {
  Image1f sdf(camera.width(), camera.height());
  return Carve(camera, silhouette, &sdf);
}

bool VoxelCarver::Carve(const Camera& camera, const Image1f& sdf) {
  return Carve(camera, Eigen::Vector2i(0, 0), Eigen::Vector2i(sdf.width() - 1, sdf.height() - 1), sdf);
}

bool VoxelCarver::Carve(const std::vector<Camera>& cameras, const std::vector<Image1b>& silhouettes) {
  std::vector<const Camera*> ptrs(cameras.size());
  for (size_t i = 0; i < cameras.size(); ++i) ptrs[i] = &cameras[i];
  return Carve(ptrs, silhouettes);
}

bool VoxelCarver::Carve(const std::vector<std::shared_ptr<Camera>>& cameras, const std::vector<Image1b>& silhouettes) {
  std::vector<const Camera*> ptrs(cameras.size());
  for (size_t i = 0; i < cameras.size(); ++i) ptrs[i] = cameras[i].get();
  return Carve(ptrs, silhouettes);
}

bool VoxelCarver::Carve(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes) {
  if (!impl_->ctx || cameras.size() != silhouettes.size() || cameras.empty()) return false;
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(n);
  std::vector<const uint8_t*> masks(n);
  for (int i = 0; i < n; ++i) {
    const Image1b& s = silhouettes[i];
    bool known = true;
    views[i] = ToView(*cameras[i], s.width(), s.height(), &known);
    if (!known) return false;
    masks[i] = s.data().data();
  }
  // masks are streamed to the device, SDFs built there, views fused in chunks of 32
  const bool ok = vcy_carve_batch_silhouettes(impl_->ctx, n, views.data(), masks.data()) == VCY_OK;
  if (!ok) LOGE("%s\n", vcy_last_error());
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  return ok;
}

void VoxelCarver::ExtractIsoSurface(Mesh* mesh, double iso_level, bool linear_interp) {
  mesh->Clear();
  if (!impl_->ctx) return;
  const double t0 = NowMs();
  vcy_mesh m;
  if (vcy_extract_iso(impl_->ctx, iso_level, linear_interp ? 1 : 0, &m) != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    vcy_mesh_free(&m);
    LogAppliedCarves(impl_->ctx, &impl_->carve_timer);  // (the queue may have been applied before the failure)
    return;
  }
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  static_assert(sizeof(Eigen::Vector3f) == 3 * sizeof(float), "packed vector layout");
  static_assert(sizeof(Eigen::Vector3i) == 3 * sizeof(int), "packed vector layout");
  std::vector<Eigen::Vector3f>* v = mesh->mutable_vertices();
  std::vector<Eigen::Vector3i>* f = mesh->mutable_vertex_indices();
  detail::CopyTriples(v, m.vertices, static_cast<size_t>(m.n_vertices));
  detail::CopyTriples(f, m.faces, static_cast<size_t>(m.n_faces));
  vcy_mesh_free(&m);
  LOGI("MarchingCubes %02f\n", NowMs() - t0);
}

void VoxelCarver::ExtractIsoSurface(Mesh* mesh, double iso_level, bool linear_interp, bool with_normals) {
  if (!with_normals) {
    ExtractIsoSurface(mesh, iso_level, linear_interp);
    return;
  }
  mesh->Clear();
  if (!impl_->ctx) return;
  const double t0 = NowMs();
  vcy_mesh m;
  vcy_mesh_normals n;
  if (vcy_extract_iso_normals(impl_->ctx, iso_level, linear_interp ? 1 : 0, VCY_NORMALS_VERTEX | VCY_NORMALS_FACE, &m, &n) !=
      VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    vcy_mesh_free(&m);
    vcy_mesh_normals_free(&n);
    LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
    return;
  }
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  detail::CopyTriples(mesh->mutable_vertices(), m.vertices, static_cast<size_t>(m.n_vertices));
  detail::CopyTriples(mesh->mutable_vertex_indices(), m.faces, static_cast<size_t>(m.n_faces));
  detail::CopyTriples(mesh->mutable_normals(), n.vertex_normals, static_cast<size_t>(m.n_vertices));
  detail::CopyTriples(mesh->mutable_face_normals(), n.face_normals, static_cast<size_t>(m.n_faces));
  mesh->set_normal_indices(mesh->vertex_indices());
  vcy_mesh_free(&m);
  vcy_mesh_normals_free(&n);
  LOGI("MarchingCubes with normals %02f\n", NowMs() - t0);
}

bool VoxelCarver::LabelComponents(std::vector<VoxelComponent>* components, double iso_level) {
  components->clear();
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  vcy_component* list = nullptr;
  std::int64_t n = 0;
  const int rc = vcy_label_components(impl_->ctx, iso_level, &list, &n);
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  components->resize(static_cast<size_t>(n));
  for (std::int64_t i = 0; i < n; ++i) {
    VoxelComponent& c = (*components)[static_cast<size_t>(i)];
    c.label = list[i].label;
    c.n_voxels = list[i].n_voxels;
    for (int k = 0; k < 3; ++k) c.bb_min[k] = list[i].bb_min[k], c.bb_max[k] = list[i].bb_max[k];
  }
  vcy_components_free(list);
  return true;
}

bool VoxelCarver::RenderHull(const Camera& camera, Image1f* depth, Image1b* silhouette, double iso_level) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  const int w = camera.width(), h = camera.height();
  bool known = true;
  const vcy_view v = ToView(camera, w, h, &known);
  if (!known) return false;  // (ToView has logged the camera type)
  if (!depth || w <= 0 || h <= 0) {
    LOGE("VoxelCarver::RenderHull needs a depth image to fill and a camera with a size (%d x %d)\n", w, h);
    return false;
  }
  depth->Init(w, h);
  float* dp = depth->data_ptr()->data();
  const int rc = vcy_render_hull(impl_->ctx, iso_level, 1, &v, &dp, nullptr, nullptr);
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  if (silhouette) {
    silhouette->Init(w, h);
    std::vector<unsigned char>& s = *silhouette->data_ptr();
    for (size_t i = 0; i < s.size(); ++i) s[i] = dp[i] < std::numeric_limits<float>::infinity() ? 255 : 0;
  }
  return true;
}

bool VoxelCarver::HullAgreement(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes,
                                std::vector<std::array<std::int64_t, 3>>* counts, double iso_level) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  if (!counts || cameras.size() != silhouettes.size() || cameras.empty()) {
    LOGE("VoxelCarver::HullAgreement needs one silhouette per camera, at least one, and a place for the counts (%zu cameras, "
         "%zu silhouettes)\n", cameras.size(), silhouettes.size());
    return false;
  }
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(n);
  std::vector<const uint8_t*> masks(n);
  for (int i = 0; i < n; ++i) {
    const Image1b& s = silhouettes[i];
    bool known = true;
    if (!cameras[i] || s.empty()) {
      LOGE("VoxelCarver::HullAgreement: view %d has no camera or an empty silhouette\n", i);
      return false;
    }
    views[i] = ToView(*cameras[i], s.width(), s.height(), &known);
    if (!known) return false;  // (ToView has logged the camera type)
    masks[i] = s.data().data();
  }
  counts->assign(static_cast<size_t>(n), std::array<std::int64_t, 3>{{0, 0, 0}});
  static_assert(sizeof(std::array<std::int64_t, 3>) == 3 * sizeof(std::int64_t), "packed array layout");
  const int rc = vcy_hull_agreement(impl_->ctx, iso_level, n, views.data(), masks.data(), (*counts)[0].data());
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  return true;
}

bool VoxelCarver::HullAgreement(const std::vector<Camera>& cameras, const std::vector<Image1b>& silhouettes,
                                std::vector<std::array<std::int64_t, 3>>* counts) {
  std::vector<const Camera*> ptrs(cameras.size());
  for (size_t i = 0; i < cameras.size(); ++i) ptrs[i] = &cameras[i];
  return HullAgreement(ptrs, silhouettes, counts);
}

bool VoxelCarver::RenderMesh(const Mesh& mesh, const Camera& camera, Image1f* depth, Image1b* silhouette) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  return detail::RenderMeshWith(impl_->ctx, "VoxelCarver::RenderMesh", mesh, camera, depth, silhouette);
}

bool VoxelCarver::MeshAgreement(const Mesh& mesh, const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes,
                                std::vector<std::array<std::int64_t, 3>>* counts) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  return detail::MeshAgreementWith(impl_->ctx, "VoxelCarver::MeshAgreement", mesh, cameras, silhouettes, counts);
}

bool VoxelCarver::ShadeMesh(const Mesh& mesh, const Camera& camera, Image3b* image, bool from_normals) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  return detail::ShadeMeshWith(impl_->ctx, "VoxelCarver::ShadeMesh", mesh, camera, image, from_normals);
}

bool VoxelCarver::MeshPhotoError(const Mesh& mesh, const std::vector<const Camera*>& cameras, const std::vector<Image3b>& photos,
                                 const std::vector<Image1b>& silhouettes, std::vector<std::array<std::int64_t, 7>>* sums) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  return detail::MeshPhotoErrorWith(impl_->ctx, "VoxelCarver::MeshPhotoError", mesh, cameras, photos, silhouettes, sums);
}

std::array<float, 2> VoxelCarver::last_shade_ms() const {
  std::array<float, 2> ms = {{0.0f, 0.0f}};
  if (impl_->ctx) vcy_last_shade_ms(impl_->ctx, &ms[0], &ms[1]);
  return ms;
}

std::array<float, 2> VoxelCarver::last_raster_ms() const {
  std::array<float, 2> ms = {{0.0f, 0.0f}};
  if (impl_->ctx) vcy_last_raster_ms(impl_->ctx, &ms[0], &ms[1]);
  return ms;
}

bool VoxelCarver::CarveRobust(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes, int tolerate,
                              std::vector<std::int64_t>* overruled, double iso_level) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  if (cameras.size() != silhouettes.size() || cameras.empty()) {
    LOGE("VoxelCarver::CarveRobust needs one silhouette per camera, at least one (%zu cameras, %zu silhouettes)\n",
         cameras.size(), silhouettes.size());
    return false;
  }
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(n);
  std::vector<const uint8_t*> masks(n);
  for (int i = 0; i < n; ++i) {
    const Image1b& s = silhouettes[i];
    bool known = true;
    if (!cameras[i] || s.empty()) {
      LOGE("VoxelCarver::CarveRobust: view %d has no camera or an empty silhouette\n", i);
      return false;
    }
    views[i] = ToView(*cameras[i], s.width(), s.height(), &known);
    if (!known) return false;  // (ToView has logged the camera type)
    masks[i] = s.data().data();
  }
  std::vector<std::int64_t> counts(static_cast<size_t>(n), 0);
  const int rc = vcy_carve_robust_silhouettes(impl_->ctx, n, views.data(), masks.data(), tolerate, iso_level,
                                              overruled ? counts.data() : nullptr);
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  if (overruled) overruled->swap(counts);
  return true;
}

bool VoxelCarver::CarveRobust(const std::vector<std::shared_ptr<Camera>>& cameras, const std::vector<Image1b>& silhouettes,
                              int tolerate, std::vector<std::int64_t>* overruled, double iso_level) {
  std::vector<const Camera*> ptrs(cameras.size());
  for (size_t i = 0; i < cameras.size(); ++i) ptrs[i] = cameras[i].get();
  return CarveRobust(ptrs, silhouettes, tolerate, overruled, iso_level);
}

bool VoxelCarver::CarveDepth(const std::vector<const Camera*>& cameras, const std::vector<Image1f>& depths, float band) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  if (cameras.size() != depths.size() || cameras.empty()) {
    LOGE("VoxelCarver::CarveDepth needs one depth image per camera, at least one (%zu cameras, %zu images)\n", cameras.size(),
         depths.size());
    return false;
  }
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(n);
  std::vector<const float*> images(n);
  for (int i = 0; i < n; ++i) {
    const Image1f& d = depths[i];
    bool known = true;
    if (!cameras[i] || d.empty()) {
      LOGE("VoxelCarver::CarveDepth: view %d has no camera or an empty depth image\n", i);
      return false;
    }
    views[i] = ToView(*cameras[i], d.width(), d.height(), &known);
    if (!known) return false;  // (ToView has logged the camera type)
    images[i] = d.data().data();
  }
  const int rc = vcy_carve_depth(impl_->ctx, n, views.data(), images.data(), band);
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  return true;
}

bool VoxelCarver::CarveDepth(const std::vector<std::shared_ptr<Camera>>& cameras, const std::vector<Image1f>& depths, float band) {
  std::vector<const Camera*> ptrs(cameras.size());
  for (size_t i = 0; i < cameras.size(); ++i) ptrs[i] = cameras[i].get();
  return CarveDepth(ptrs, depths, band);
}

bool VoxelCarver::CarveDepth(const Camera& camera, const Image1f& depth, float band) {
  // (one image: copied once into the vector the batch overload reads)
  return CarveDepth(std::vector<const Camera*>{&camera}, std::vector<Image1f>{depth}, band);
}

float VoxelCarver::last_depth_ms() const {
  float ms = 0.0f;
  if (impl_->ctx) vcy_last_depth_ms(impl_->ctx, &ms);
  return ms;
}

bool VoxelCarver::ColorMesh(Mesh* mesh, const std::vector<const Camera*>& cameras, const std::vector<Image3b>& photos,
                            const ColorOption& option, double iso_level) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  if (!mesh || cameras.size() != photos.size() || cameras.empty()) {
    LOGE("VoxelCarver::ColorMesh needs a mesh and one photograph per camera, at least one (%zu cameras, %zu photographs)\n",
         cameras.size(), photos.size());
    return false;
  }
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(n);
  std::vector<const uint8_t*> data(n);
  for (int i = 0; i < n; ++i) {
    const Image3b& p = photos[i];
    bool known = true;
    if (!cameras[i] || p.empty()) {
      LOGE("VoxelCarver::ColorMesh: view %d has no camera or an empty photograph\n", i);
      return false;
    }
    views[i] = ToView(*cameras[i], p.width(), p.height(), &known);
    if (!known) return false;  // (ToView has logged the camera type)
    data[i] = p.data().data();
  }
  vcy_color_option o;
  o.mode = static_cast<int32_t>(option.mode);
  o.interp = static_cast<int32_t>(option.interp);
  o.depth_tolerance = option.depth_tolerance < 0.0f ? 1.5f * impl_->option.resolution : option.depth_tolerance;
  o.min_cos = option.min_cos;
  for (int k = 0; k < 3; ++k) o.fallback[k] = option.fallback[k];
  const size_t nv = mesh->vertices().size();
  if (option.mode != ColorMode::kMean && mesh->normals().size() != nv) mesh->CalcNormal();
  const float* normals = option.mode != ColorMode::kMean ? reinterpret_cast<const float*>(mesh->normals().data()) : nullptr;
  static_assert(sizeof(Eigen::Vector3f) == 3 * sizeof(float), "packed vector layout");
  std::vector<Eigen::Vector3f> colors(nv);
  // occlusion from the mesh itself: its depth images, rasterised here and handed on as the caller's would be
  std::vector<std::vector<float>> depth;
  std::vector<float*> depth_ptr;
  if (option.occlusion_from_mesh) {
    depth.resize(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
      depth[i].resize(static_cast<size_t>(views[i].width) * static_cast<size_t>(views[i].height));
      depth_ptr.push_back(depth[i].data());
    }
    static_assert(sizeof(Eigen::Vector3i) == 3 * sizeof(int32_t), "packed vector layout");
    const int rcr = vcy_raster_mesh(impl_->ctx, static_cast<int64_t>(nv), static_cast<int64_t>(mesh->vertex_indices().size()),
                                    reinterpret_cast<const float*>(mesh->vertices().data()),
                                    reinterpret_cast<const int32_t*>(mesh->vertex_indices().data()), n, views.data(),
                                    depth_ptr.data(), nullptr, nullptr, nullptr);
    if (rcr != VCY_OK) {
      LOGE("%s\n", vcy_last_error());
      return false;
    }
  }
  const int rc = vcy_color_vertices(impl_->ctx, iso_level, static_cast<int64_t>(nv),
                                    reinterpret_cast<const float*>(mesh->vertices().data()), normals, n, views.data(),
                                    data.data(), option.occlusion_from_mesh ? depth_ptr.data() : nullptr, &o,
                                    reinterpret_cast<float*>(colors.data()), nullptr, nullptr);
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  mesh->set_vertex_colors(colors);
  return true;
}

bool VoxelCarver::SmoothMesh(Mesh* mesh, int iterations, float lambda, float mu, bool pin_boundary, bool with_normals) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  if (!mesh) {
    LOGE("VoxelCarver::SmoothMesh needs a mesh\n");
    return false;
  }
  vcy_ctx* ctx = impl_->ctx;
  return detail::SmoothMeshWith(mesh, iterations, lambda, mu, pin_boundary, with_normals,
                                [ctx](int64_t nv, int64_t nf, const float* v, const int32_t* f, const vcy_smooth_option* o,
                                      float* out, float* vn, float* fn) { return vcy_smooth_mesh(ctx, nv, nf, v, f, o, out, vn, fn); });
}

std::array<float, 3> VoxelCarver::last_smooth_ms() const {
  std::array<float, 3> ms = {{0.0f, 0.0f, 0.0f}};
  if (impl_->ctx) vcy_last_smooth_ms(impl_->ctx, &ms[0], &ms[1], &ms[2]);
  return ms;
}

bool VoxelCarver::DecimateMesh(Mesh* mesh, float cell, int mode, bool with_normals) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  if (!mesh) {
    LOGE("VoxelCarver::DecimateMesh needs a mesh\n");
    return false;
  }
  vcy_ctx* ctx = impl_->ctx;
  return detail::DecimateMeshWith(mesh, cell, impl_->option.bb_min, mode, with_normals,
                                  [ctx](int64_t nv, int64_t nf, const float* v, const int32_t* f, const vcy_decimate_option* o,
                                        float* vo, int32_t* fo, int64_t* nvo, int64_t* nfo, int32_t* map, int32_t* src, float* vn,
                                        float* fn) { return vcy_decimate_mesh(ctx, nv, nf, v, f, o, vo, fo, nvo, nfo, map, src, vn, fn); });
}

bool VoxelCarver::DecimateMeshQuadric(Mesh* mesh, float cell, float regularize, bool with_normals, std::int64_t* n_fallback) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  if (!mesh) {
    LOGE("VoxelCarver::DecimateMeshQuadric needs a mesh\n");
    return false;
  }
  vcy_ctx* ctx = impl_->ctx;
  int64_t fallbacks = 0;
  const bool ok = detail::DecimateMeshWith(
      mesh, cell, impl_->option.bb_min, VCY_DECIMATE_MEAN, with_normals,
      [ctx, regularize, &fallbacks](int64_t nv, int64_t nf, const float* v, const int32_t* f, const vcy_decimate_option* o, float* vo,
                                    int32_t* fo, int64_t* nvo, int64_t* nfo, int32_t* map, int32_t* src, float* vn, float* fn) {
        return vcy_decimate_mesh_quadric(ctx, nv, nf, v, f, o, regularize, vo, fo, nvo, nfo, map, src, vn, fn, &fallbacks);
      });
  if (ok && n_fallback) *n_fallback = fallbacks;
  return ok;
}

std::array<float, 4> VoxelCarver::last_decimate_ms() const {
  std::array<float, 4> ms = {{0.0f, 0.0f, 0.0f, 0.0f}};
  if (impl_->ctx) vcy_last_decimate_ms(impl_->ctx, &ms[0], &ms[1], &ms[2], &ms[3]);
  return ms;
}

float VoxelCarver::last_quadric_ms() const {
  float ms = 0.0f;
  if (impl_->ctx) vcy_last_quadric_ms(impl_->ctx, &ms);
  return ms;
}

bool VoxelCarver::ExtractIsoSurfaceChain(Mesh* mesh, const ChainOption& option, ChainReport* report) {
  if (report) *report = ChainReport();
  if (!mesh) {
    LOGE("VoxelCarver::ExtractIsoSurfaceChain needs a mesh\n");
    return false;
  }
  mesh->Clear();
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  const double t0 = NowMs();
  vcy_chain_option o;
  std::memset(&o, 0, sizeof(o));
  o.smooth = option.smooth ? 1 : 0;
  o.smooth_option.iterations = option.iterations;
  o.smooth_option.lambda = option.lambda;
  o.smooth_option.mu = option.mu;
  o.smooth_option.pin_boundary = option.pin_boundary ? 1 : 0;
  o.decimate = option.decimate;
  o.decimate_option.cell = option.cell;
  for (int k = 0; k < 3; ++k) o.decimate_option.origin[k] = impl_->option.bb_min[k];  // (as DecimateMesh: cells line up with voxels)
  o.decimate_option.mode = option.mode;
  o.regularize = option.regularize;
  o.which = VCY_NORMALS_VERTEX | VCY_NORMALS_FACE;
  o.maps = report && option.maps ? 1 : 0;
  vcy_mesh m;
  vcy_mesh_normals n;
  vcy_chain_report r;
  const int rc = vcy_extract_iso_chain(impl_->ctx, option.iso_level, option.linear_interp ? 1 : 0, &o, &m, &n, &r);
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  detail::CopyTriples(mesh->mutable_vertices(), m.vertices, static_cast<size_t>(m.n_vertices));
  detail::CopyTriples(mesh->mutable_vertex_indices(), m.faces, static_cast<size_t>(m.n_faces));
  detail::CopyTriples(mesh->mutable_normals(), n.vertex_normals, static_cast<size_t>(m.n_vertices));
  detail::CopyTriples(mesh->mutable_face_normals(), n.face_normals, static_cast<size_t>(m.n_faces));
  mesh->set_normal_indices(mesh->vertex_indices());
  if (report) {
    report->n_extracted_vertices = r.n_extracted_vertices;
    report->n_extracted_faces = r.n_extracted_faces;
    report->n_fallback = r.n_fallback;
    if (r.vertex_map) report->vertex_map.assign(r.vertex_map, r.vertex_map + r.n_extracted_vertices);
    if (r.face_source) report->face_source.assign(r.face_source, r.face_source + m.n_faces);
  }
  vcy_mesh_free(&m);
  vcy_mesh_normals_free(&n);
  vcy_chain_report_free(&r);
  LOGI("MarchingCubes, smoothing %d, decimation %d, normals %02f\n", o.smooth, o.decimate, NowMs() - t0);
  return true;
}

std::array<float, 8> VoxelCarver::last_chain_ms() const {
  std::array<float, 8> ms = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};
  if (impl_->ctx) vcy_last_chain_ms(impl_->ctx, &ms[0], &ms[1], &ms[2], &ms[3], &ms[4], &ms[5], &ms[6], &ms[7]);
  return ms;
}

bool VoxelCarver::KeepLargestComponents(int largest, std::int64_t min_voxels, double iso_level, float fill_sdf) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  std::int64_t gone = 0, gone_voxels = 0;
  const int rc = vcy_keep_components(impl_->ctx, iso_level, largest, min_voxels, fill_sdf, &gone, &gone_voxels);
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  float ms = 0.0f;
  vcy_last_components_ms(impl_->ctx, &ms);
  LOGI("KeepLargestComponents removed %lld components, %lld voxels %02f\n", static_cast<long long>(gone),
       static_cast<long long>(gone_voxels), static_cast<double>(ms));
  return true;
}

bool VoxelCarver::DistanceField(std::vector<std::int32_t>* d2, double iso_level, int radius) {
  if (!impl_->ctx || !d2) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  std::int32_t dims[3] = {0, 0, 0};
  vcy_grid_dims(impl_->ctx, dims);
  d2->resize(static_cast<size_t>(dims[0]) * dims[1] * dims[2]);
  const int rc = vcy_distance_field(impl_->ctx, iso_level, radius, d2->data());
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    d2->clear();
    return false;
  }
  return true;
}

bool VoxelCarver::Redistance(double iso_level, int radius) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  std::int64_t n = 0;
  const int rc = vcy_redistance(impl_->ctx, iso_level, radius, &n);
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (rc != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  float ms = 0.0f;
  vcy_last_distance_ms(impl_->ctx, &ms);
  LOGI("Redistance rewrote %lld voxels %02f\n", static_cast<long long>(n), static_cast<double>(ms));
  return true;
}

bool VoxelCarver::CloseHull(float radius_voxels, double iso_level) {
  if (!impl_->ctx) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  std::string error;
  const bool ok = detail::CloseHullOn(impl_->ctx, radius_voxels, iso_level, impl_->option.resolution, &error);
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  if (!ok) LOGE("%s\n", error.c_str());
  return ok;
}

void VoxelCarver::ExtractVoxel(Mesh* mesh, bool inside_empty) {
  mesh->Clear();
  if (!impl_->ctx) return;
  const double t0 = NowMs();
  // (the library's host threads fill the Mesh's own vectors: no library-owned copy of the mesh in between)
  typedef detail::MeshArrays<Eigen::Vector3f, Eigen::Vector3i> Arrays;
  Arrays arrays{mesh->mutable_vertices(), mesh->mutable_vertex_indices()};
  if (vcy_extract_voxel_into(impl_->ctx, inside_empty ? 1 : 0, &Arrays::Provide, &arrays) != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    mesh->Clear();
    LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
    return;
  }
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  LOGI("VoxelCarver::ExtractVoxel %02f\n", NowMs() - t0);
}

Eigen::Vector3i VoxelCarver::voxel_num() const {
  int32_t d[3] = {0, 0, 0};
  if (impl_->ctx) vcy_grid_dims(impl_->ctx, d);
  return Eigen::Vector3i(d[0], d[1], d[2]);
}

bool VoxelCarver::Download(std::vector<float>* sdf, std::vector<int>* update_num) const {
  if (!impl_->ctx) return false;
  const Eigen::Vector3i n = voxel_num();
  const size_t total = static_cast<size_t>(n[0]) * n[1] * n[2];
  if (sdf) sdf->resize(total);
  if (update_num) update_num->resize(total);
  const bool ok = vcy_download(impl_->ctx, sdf ? sdf->data() : nullptr, update_num ? update_num->data() : nullptr) == VCY_OK;
  LogAppliedCarves(impl_->ctx, &impl_->carve_timer);
  return ok;
}

bool VoxelCarver::Download(VoxelGrid* grid) const {
  if (!impl_->ctx || !grid) return false;
  const VoxelCarverOption& o = impl_->option;
  if (!grid->Init(o.bb_max, o.bb_min, o.resolution)) return false;
  const Eigen::Vector3i n = grid->voxel_num();
  if (n[0] != voxel_num()[0] || n[1] != voxel_num()[1] || n[2] != voxel_num()[2]) return false;
  std::vector<float> sdf;
  std::vector<int> update_num;
  if (!Download(&sdf, &update_num)) return false;
  size_t i = 0;
  for (int z = 0; z < n[2]; ++z)
    for (int y = 0; y < n[1]; ++y)
      for (int x = 0; x < n[0]; ++x, ++i) {
        Voxel* v = grid->get_ptr(x, y, z);
        v->sdf = sdf[i];
        v->update_num = update_num[i];
      }
  return true;
}

void DistanceTransformL1(const Image1b& mask, const Eigen::Vector2i& roi_min, const Eigen::Vector2i& roi_max,
                         Image1f* dist) {
  dist->Init(mask.width(), mask.height(), 0.0f);
  const int32_t rmin[2] = {roi_min[0], roi_min[1]}, rmax[2] = {roi_max[0], roi_max[1]};
  if (vcy_distance_transform_l1(mask.data().data(), mask.width(), mask.height(), rmin, rmax,
                                dist->data_ptr()->data()) != VCY_OK)
    LOGE("%s\n", vcy_last_error());
}

void MakeSignedDistanceField(const Image1b& mask, const Eigen::Vector2i& roi_min, const Eigen::Vector2i& roi_max,
                             Image1f* dist, bool minmax_normalize, bool use_truncation, float truncation_band) {
  dist->Init(mask.width(), mask.height(), 0.0f);
  const int32_t rmin[2] = {roi_min[0], roi_min[1]}, rmax[2] = {roi_max[0], roi_max[1]};
  if (vcy_make_sdf(mask.data().data(), mask.width(), mask.height(), rmin, rmax, minmax_normalize, use_truncation,
                   truncation_band, dist->data_ptr()->data()) != VCY_OK)
    LOGE("%s\n", vcy_last_error());
}

// blue inside, red outside, white at the silhouette (reference voxel_carver.cc:239-267)
void SignedDistance2Color(const Image1f& sdf, Image3b* vis, float min_negative_d, float max_positive_d) {
  vis->Init(sdf.width(), sdf.height());
  for (int y = 0; y < sdf.height(); ++y)
    for (int x = 0; x < sdf.width(); ++x) {
      const float d = sdf.at(x, y, 0);
      uint8_t* px = vis->at(x, y);
      if (d > 0) {
        float k = (max_positive_d - d) / max_positive_d;
        k = std::min(std::max(k, 0.0f), 1.0f);
        px[0] = 255;
        px[1] = px[2] = static_cast<uint8_t>(255 * k);
      } else {
        float k = (d - min_negative_d) / (-min_negative_d);
        k = std::min(std::max(k, 0.0f), 1.0f);
        px[0] = px[1] = static_cast<uint8_t>(255 * k);
        px[2] = 255;
      }
    }
}

}  // namespace vacancy
