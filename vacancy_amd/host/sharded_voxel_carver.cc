// ShardedVoxelCarver: z-slab sharding over the C-ABI contexts of include/vacancy_hip.h.
#include "vacancy/sharded_voxel_carver.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <array>
#include <functional>
#include <future>
#include <limits>
#include <string>

#include "c_abi_structs.h"
#include "mesh_copy.h"
#include "mesh_decimate.h"
#include "mesh_raster.h"
#include "mesh_smooth.h"

namespace vacancy {

namespace {

// fn(s) for every slab on a host thread of its own (a context is single-threaded, different contexts are independent;
// vcy_last_error() is per thread, so a failure's text comes back with its status)
template <typename Fn>
bool ForEachSlab(size_t ns, const char* what, Fn fn) {
  std::vector<std::future<std::pair<int, std::string>>> jobs;
  for (size_t s = 0; s < ns; ++s)
    jobs.push_back(std::async(std::launch::async, [s, &fn]() {
      const int rc = fn(s);
      return std::make_pair(rc, rc == VCY_OK ? std::string() : std::string(vcy_last_error()));
    }));
  bool ok = true;
  for (auto& j : jobs) {
    const std::pair<int, std::string> r = j.get();
    if (r.first != VCY_OK) {
      LOGE("sharded %s failed: %s\n", what, r.second.c_str());
      ok = false;
    }
  }
  return ok;
}

}  // namespace

struct ShardedVoxelCarver::Impl {
  VoxelCarverOption option;
  std::vector<int> devices;
  int per_device = 1;
  std::vector<int> wanted_bounds;  // PlanPartition / set_z_bounds; empty: equal thickness
  std::vector<int> bounds;         // of the slabs that exist
  int64_t slice = 0;               // voxels per z slice of the grid (nx * ny)
  std::vector<vcy_ctx*> slabs;  // in z order
  bool peer_copy_halo = false;
  // what LabelComponents and KeepLargestComponents share: every slab labelled, the seams paired, the pieces merged
  struct Labelled {
    std::vector<vcy_component> merged;   // the whole grid's list, in the order of vcy_label_components
    std::vector<vcy_component> pieces;   // the slabs' lists one behind the other
    std::vector<int64_t> counts;         // pieces per slab
    std::vector<int64_t> global;         // merged label of every piece
  };
  bool LabelSlabs(double iso_level, Labelled* out);
  // the distance field over the slabs: vcy_distance_slab_begin on every slab, the seam planes through the host, then
  // finish(slab, below, n_below, above, n_above) -- a C-ABI status -- on every slab
  bool DistanceSlabs(double iso_level, int radius, const char* who,
                     const std::function<int(size_t, const uint16_t*, int, const uint16_t*, int)>& finish);
  ~Impl() {
    for (vcy_ctx* c : slabs) vcy_destroy(c);
  }
};

ShardedVoxelCarver::ShardedVoxelCarver(VoxelCarverOption option, std::vector<int> device_ids, int slabs_per_device)
    : impl_(new Impl) {
  impl_->option = option;
  impl_->devices = device_ids.empty() ? std::vector<int>{0} : device_ids;
  impl_->per_device = slabs_per_device < 1 ? 1 : slabs_per_device;
}
ShardedVoxelCarver::~ShardedVoxelCarver() {}

void ShardedVoxelCarver::set_halo_transport(HaloTransport t) { impl_->peer_copy_halo = t == HaloTransport::kPeerCopy; }

int ShardedVoxelCarver::slab_count() const { return static_cast<int>(impl_->slabs.size()); }

void ShardedVoxelCarver::set_z_bounds(const std::vector<int>& z_bounds) { impl_->wanted_bounds = z_bounds; }
const std::vector<int>& ShardedVoxelCarver::z_bounds() const { return impl_->bounds; }

bool ShardedVoxelCarver::PlanPartition(const std::vector<const Camera*>& cameras,
                                       const std::vector<Image1b>& silhouettes) {
  if (cameras.empty() || cameras.size() != silhouettes.size()) return false;
  const vcy_carver_option c = detail::ToC(impl_->option);
  const int count = static_cast<int>(impl_->devices.size()) * impl_->per_device;
  if (count < 2) return true;  // one slab: nothing to cut
  vcy_ctx* planner = nullptr;
  if (vcy_create(&c, impl_->devices[0], 0, 8, &planner) != VCY_OK) {  // (its 8-slice slab is never touched)
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(n);
  std::vector<float*> imgs(n, nullptr);
  bool ok = true;
  for (int i = 0; i < n && ok; ++i) {
    views[i] = detail::ToView(*cameras[i], silhouettes[i].width(), silhouettes[i].height(), &ok);
    if (!ok) break;
    // MakeSignedDistanceField as Carve() will build it (voxel_carver.cc:405-408), on the device
    ok = vcy_make_sdf_device(planner, silhouettes[i].data().data(), views[i].width, views[i].height, views[i].roi_min,
                             views[i].roi_max, c.sdf_minmax_normalize, c.update_option.use_truncation,
                             c.update_option.truncation_band, &imgs[i]) == VCY_OK;
  }
  std::vector<int32_t> b(static_cast<size_t>(count) + 1, 0);
  if (ok)
    ok = vcy_plan_z_slabs(planner, n, views.data(), imgs.data(), count, 0, 0.0f, b.data(), nullptr, 0, nullptr) == VCY_OK;
  if (!ok) LOGE("PlanPartition: %s\n", vcy_last_error());
  for (float* p : imgs)
    if (p) vcy_device_free(planner, p);
  vcy_destroy(planner);
  if (ok) impl_->wanted_bounds.assign(b.begin(), b.end());
  return ok;
}

bool ShardedVoxelCarver::Init() {
  for (vcy_ctx* c : impl_->slabs) vcy_destroy(c);
  impl_->slabs.clear();
  impl_->bounds.clear();
  const vcy_carver_option c = detail::ToC(impl_->option);
  int32_t dims[3];
  if (vcy_compute_dims(c.bb_min, c.bb_max, c.resolution, dims) != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  const int ndev = static_cast<int>(impl_->devices.size());
  int count = ndev * impl_->per_device;
  while (count > 1 && dims[2] / count < 2) --count;  // every slab needs >= 2 slices
  const int base = dims[2] / count, rem = dims[2] % count;
  std::vector<int> bounds(static_cast<size_t>(count) + 1, dims[2]);
  for (int s = 0; s < count; ++s) bounds[s] = s * base + (s < rem ? s : rem);
  {  // cuts from PlanPartition / set_z_bounds, if they fit this grid and slab count
    const std::vector<int>& w = impl_->wanted_bounds;
    bool fits = static_cast<int>(w.size()) == count + 1 && w.front() == 0 && w.back() == dims[2];
    for (size_t s = 0; fits && s + 1 < w.size(); ++s) fits = w[s + 1] - w[s] >= 2;
    if (fits) bounds = w;
    else if (!w.empty()) LOGW("ShardedVoxelCarver: the given z bounds do not fit %d slabs of this grid; equal thickness\n", count);
  }
  impl_->bounds = bounds;
  impl_->slice = static_cast<int64_t>(dims[0]) * dims[1];
  for (int s = 0; s < count; ++s) {
    const int z0 = bounds[s], z1 = bounds[s + 1];
    vcy_ctx* ctx = nullptr;
    if (vcy_create(&c, impl_->devices[s % ndev], z0, z1, &ctx) != VCY_OK) {  // cyclic deal
      LOGE("%s\n", vcy_last_error());
      return false;
    }
    // Several slabs are driven from one host thread here and in vcy_carve_batch_silhouettes_sharded: a launch of few
    // views over a carved slab must not make that thread wait for the slab's live-workgroup count ("livesync" 1, worth
    // 0.1 ms per launch on a whole 1024^3 grid) before it can enqueue the next slab's work.
    if (count > 1) (void)vcy_set_param(ctx, "livesync", 0);
    impl_->slabs.push_back(ctx);
  }
  return true;
}

bool ShardedVoxelCarver::Carve(const Camera& camera, const Image1b& silhouette) {
  return Carve(std::vector<const Camera*>{&camera}, std::vector<Image1b>{silhouette});
}

bool ShardedVoxelCarver::Carve(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes) {
  if (impl_->slabs.empty() || cameras.size() != silhouettes.size() || cameras.empty()) return false;
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(n);
  std::vector<const uint8_t*> masks(n);
  for (int i = 0; i < n; ++i) {
    bool known = true;
    views[i] = detail::ToView(*cameras[i], silhouettes[i].width(), silhouettes[i].height(), &known);
    if (!known) return false;
    masks[i] = silhouettes[i].data().data();
  }
  // Several views: the devices SHARE the producer (vcy_carve_batch_silhouettes_sharded: device r uploads and transforms
  // the silhouettes r, r + R, ... of every chunk of 32, one RCCL all-gather per chunk hands every device all the SDF
  // images, every slab carves from its device's copy) -- the reference calls MakeSignedDistanceField once per view
  // (voxel_carver.cc:405-408), and so does a node of GPUs.  Without librccl (VCY_ERR_UNSUPPORTED) every slab builds
  // its own, below.
  if (n > 1) {
    const int rc = vcy_carve_batch_silhouettes_sharded(impl_->slabs.data(), static_cast<int>(impl_->slabs.size()), n,
                                                       views.data(), masks.data());
    if (rc == VCY_OK) return true;
    if (rc != VCY_ERR_UNSUPPORTED) {
      LOGE("sharded carve failed: %s\n", vcy_last_error());
      return false;
    }
    LOGW("ShardedVoxelCarver: %s; every slab builds its own SDF images\n", vcy_last_error());
  }
  return ForEachSlab(impl_->slabs.size(), "carve", [&](size_t s) {
    // one view: queued by the library, carved together with the following calls (vcy_set_param "defer")
    return n == 1 ? vcy_carve_silhouette(impl_->slabs[s], &views[0], masks[0], nullptr)
                  : vcy_carve_batch_silhouettes(impl_->slabs[s], n, views.data(), masks.data());
  });
}

// the two slices below every slab: ONE RCCL all-gather over the devices that hold slabs
// (vcy_halo_allgather); peer-to-peer copies only when asked for (set_halo_transport)
bool ShardedVoxelCarver::ExchangeHalo() {
  const size_t ns = impl_->slabs.size();
  if (impl_->peer_copy_halo) {
    for (size_t s = 0; s < ns; ++s)
      if (vcy_halo_copy_from(impl_->slabs[s], s ? impl_->slabs[s - 1] : nullptr) != VCY_OK) {
        LOGE("%s\n", vcy_last_error());
        return false;
      }
  } else if (vcy_halo_allgather(impl_->slabs.data(), static_cast<int>(ns)) != VCY_OK) {
    LOGE("%s\n", vcy_last_error());
    return false;
  }
  return true;
}

// The order of calls of include/vacancy_hip.h ("connected components of a grid cut into z-slabs"): every slab labels its
// own slices on its device; per seam the lower slab's top plane of labels (nx * ny int64) goes through host memory to the
// upper slab's device, which returns the pairs of pieces that touch; the host joins the pieces.  No slab's label volume
// leaves its device.
bool ShardedVoxelCarver::Impl::LabelSlabs(double iso_level, Labelled* out) {
  const size_t ns = slabs.size();
  if (ns == 0) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  std::vector<vcy_component*> lists(ns, nullptr);
  std::vector<int64_t> counts(ns, 0);
  std::vector<std::vector<int64_t>> planes(ns);
  bool ok = ForEachSlab(ns, "LabelComponents", [&](size_t s) {
    int rc = vcy_label_components_slab(slabs[s], iso_level, &lists[s], &counts[s]);
    if (rc == VCY_OK && s + 1 < ns) {
      planes[s].resize(static_cast<size_t>(slice));
      rc = vcy_component_top_plane(slabs[s], planes[s].data());
    }
    return rc;
  });
  std::vector<int64_t*> pairs(ns, nullptr);  // [s]: the seam below slab s
  std::vector<int64_t> n_pairs(ns, 0);
  ok = ok && ForEachSlab(ns, "LabelComponents (seams)", [&](size_t s) {
    return s == 0 ? static_cast<int>(VCY_OK) : vcy_component_seam_pairs(slabs[s], planes[s - 1].data(), &pairs[s], &n_pairs[s]);
  });
  if (ok) {
    out->counts = counts;
    out->pieces.clear();
    std::vector<int64_t> all_pairs;
    for (size_t s = 0; s < ns; ++s) {
      out->pieces.insert(out->pieces.end(), lists[s], lists[s] + counts[s]);
      if (s > 0) all_pairs.insert(all_pairs.end(), pairs[s], pairs[s] + 2 * n_pairs[s]);
    }
    out->global.assign(out->pieces.size(), -1);
    vcy_component* merged = nullptr;
    int64_t n_merged = 0;
    if (vcy_merge_components_host(static_cast<int>(ns), out->pieces.data(), counts.data(), all_pairs.data(), n_pairs.data() + 1,
                                  &merged, &n_merged, out->global.data()) != VCY_OK) {
      LOGE("sharded LabelComponents failed: %s\n", vcy_last_error());
      ok = false;
    } else {
      out->merged.assign(merged, merged + n_merged);
      vcy_components_free(merged);
    }
  }
  if (ok) {
    std::vector<int64_t> first(ns + 1, 0);
    for (size_t s = 0; s < ns; ++s) first[s + 1] = first[s] + counts[s];
    ok = ForEachSlab(ns, "LabelComponents (resolve)", [&](size_t s) {
      std::vector<int64_t> provisional(static_cast<size_t>(counts[s]));
      for (int64_t i = 0; i < counts[s]; ++i) provisional[static_cast<size_t>(i)] = out->pieces[static_cast<size_t>(first[s] + i)].label;
      return vcy_resolve_components_slab(slabs[s], counts[s], provisional.data(), out->global.data() + first[s]);
    });
  }
  for (vcy_component* p : lists) vcy_components_free(p);
  for (int64_t* p : pairs) vcy_seam_pairs_free(p);
  return ok;
}

bool ShardedVoxelCarver::LabelComponents(std::vector<VoxelComponent>* components, double iso_level) {
  components->clear();
  Impl::Labelled l;
  if (!impl_->LabelSlabs(iso_level, &l)) return false;
  components->resize(l.merged.size());
  for (size_t i = 0; i < l.merged.size(); ++i) {
    VoxelComponent& c = (*components)[i];
    c.label = l.merged[i].label;
    c.n_voxels = l.merged[i].n_voxels;
    for (int k = 0; k < 3; ++k) c.bb_min[k] = l.merged[i].bb_min[k], c.bb_max[k] = l.merged[i].bb_max[k];
  }
  return true;
}

bool ShardedVoxelCarver::RenderHull(const Camera&, Image1f*, Image1b*) {
  LOGE("ShardedVoxelCarver::RenderHull: the ray-cast needs the whole grid in one context (VoxelCarver::RenderHull)\n");
  return false;
}

bool ShardedVoxelCarver::HullAgreement(const std::vector<Camera>&, const std::vector<Image1b>&,
                                       std::vector<std::array<std::int64_t, 3>>*) {
  LOGE("ShardedVoxelCarver::HullAgreement: the ray-cast needs the whole grid in one context (VoxelCarver::HullAgreement)\n");
  return false;
}

// The ray-cast over the slabs (include/vacancy_hip.h, "... of a grid cut into z-slabs"): every slab renders the image of
// its own slices on its device -- no halo exchange --, the depth and voxel-id images come to the host, and
// vcy_render_merge_host takes, per pixel, the hit of the first slab in the ray's direction of travel along z.
bool ShardedVoxelCarver::RenderHullSlabs(const Camera& camera, Image1f* depth, Image1b* silhouette, double iso_level) {
  const size_t ns = impl_->slabs.size();
  if (ns == 0) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  const int w = camera.width(), h = camera.height();
  bool known = true;
  const vcy_view v = detail::ToView(camera, w, h, &known);
  if (!known) return false;  // (ToView has logged the camera type)
  if (!depth || w <= 0 || h <= 0) {
    LOGE("ShardedVoxelCarver::RenderHullSlabs needs a depth image to fill and a camera with a size (%d x %d)\n", w, h);
    return false;
  }
  const size_t px = static_cast<size_t>(w) * static_cast<size_t>(h);
  std::vector<std::vector<float>> depths(ns, std::vector<float>(px));
  std::vector<std::vector<int64_t>> voxels(ns, std::vector<int64_t>(px));
  if (!ForEachSlab(ns, "RenderHullSlabs", [&](size_t s) {
        float* dp = depths[s].data();
        int64_t* vp = voxels[s].data();
        return vcy_render_hull_slab(impl_->slabs[s], iso_level, 1, &v, &dp, &vp, nullptr, nullptr);
      }))
    return false;
  std::vector<const float*> dps(ns);
  std::vector<const int64_t*> vps(ns);
  for (size_t s = 0; s < ns; ++s) dps[s] = depths[s].data(), vps[s] = voxels[s].data();
  depth->Init(w, h);
  float* out = depth->data_ptr()->data();
  if (vcy_render_merge_host(&v, static_cast<int>(ns), dps.data(), vps.data(), nullptr, out, nullptr, nullptr) != VCY_OK) {
    LOGE("sharded RenderHullSlabs failed: %s\n", vcy_last_error());
    return false;
  }
  if (silhouette) {
    silhouette->Init(w, h);
    std::vector<unsigned char>& sil = *silhouette->data_ptr();
    for (size_t i = 0; i < sil.size(); ++i) sil[i] = out[i] < std::numeric_limits<float>::infinity() ? 255 : 0;
  }
  return true;
}

// ... and the comparison with the silhouettes: one hit bit per pixel and slab comes to the host, which ORs and counts
// (vcy_hull_agreement_host).
bool ShardedVoxelCarver::HullAgreementSlabs(const std::vector<Camera>& cameras, const std::vector<Image1b>& silhouettes,
                                            std::vector<std::array<std::int64_t, 3>>* counts, double iso_level) {
  std::vector<const Camera*> ptrs(cameras.size());
  for (size_t i = 0; i < cameras.size(); ++i) ptrs[i] = &cameras[i];
  return HullAgreementSlabs(ptrs, silhouettes, counts, iso_level);
}

bool ShardedVoxelCarver::HullAgreementSlabs(const std::vector<const Camera*>& cameras, const std::vector<Image1b>& silhouettes,
                                            std::vector<std::array<std::int64_t, 3>>* counts, double iso_level) {
  const size_t ns = impl_->slabs.size();
  if (ns == 0) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  if (!counts || cameras.size() != silhouettes.size() || cameras.empty()) {
    LOGE("ShardedVoxelCarver::HullAgreementSlabs needs one silhouette per camera, at least one, and a place for the counts "
         "(%zu cameras, %zu silhouettes)\n", cameras.size(), silhouettes.size());
    return false;
  }
  const int n = static_cast<int>(cameras.size());
  std::vector<vcy_view> views(static_cast<size_t>(n));
  std::vector<size_t> words(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    const Image1b& sil = silhouettes[static_cast<size_t>(i)];
    bool known = true;
    if (!cameras[static_cast<size_t>(i)] || sil.empty()) {
      LOGE("ShardedVoxelCarver::HullAgreementSlabs: view %d has no camera or an empty silhouette\n", i);
      return false;
    }
    views[static_cast<size_t>(i)] = detail::ToView(*cameras[static_cast<size_t>(i)], sil.width(), sil.height(), &known);
    if (!known) return false;  // (ToView has logged the camera type)
    words[static_cast<size_t>(i)] = (static_cast<size_t>(sil.width()) + 63) / 64 * static_cast<size_t>(sil.height());
  }
  std::vector<std::vector<std::vector<uint64_t>>> hits(ns);  // [slab][view]
  if (!ForEachSlab(ns, "HullAgreementSlabs", [&](size_t s) {
        hits[s].resize(static_cast<size_t>(n));
        std::vector<uint64_t*> ptrs(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) {
          hits[s][static_cast<size_t>(i)].resize(words[static_cast<size_t>(i)]);
          ptrs[static_cast<size_t>(i)] = hits[s][static_cast<size_t>(i)].data();
        }
        return vcy_render_hull_slab(impl_->slabs[s], iso_level, n, views.data(), nullptr, nullptr, nullptr, ptrs.data());
      }))
    return false;
  counts->assign(static_cast<size_t>(n), std::array<std::int64_t, 3>{{0, 0, 0}});
  for (int i = 0; i < n; ++i) {
    std::vector<const uint64_t*> of_view(ns);
    for (size_t s = 0; s < ns; ++s) of_view[s] = hits[s][static_cast<size_t>(i)].data();
    int64_t c[3] = {0, 0, 0};
    if (vcy_hull_agreement_host(&views[static_cast<size_t>(i)], static_cast<int>(ns), of_view.data(),
                                silhouettes[static_cast<size_t>(i)].data().data(), c) != VCY_OK) {
      LOGE("sharded HullAgreementSlabs failed: %s\n", vcy_last_error());
      return false;
    }
    (*counts)[static_cast<size_t>(i)] = {{c[0], c[1], c[2]}};
  }
  return true;
}

// The keep rule on the merged list (vcy_select_components_host), then every slab's own filter kernel over its pieces of the components
// that go.  The two halo slices below every upper slab are stale afterwards, exactly as after a Carve(): ExtractIsoSurface
// always, and ExtractVoxel whenever it reads the slice below a slab (inside_empty), call ExchangeHalo() before they
// read them, so nothing has to be exchanged here.
bool ShardedVoxelCarver::SmoothMesh(Mesh* mesh, int iterations, float lambda, float mu, bool pin_boundary, bool with_normals) {
  if (impl_->slabs.empty() || !mesh) {
    LOGE("ShardedVoxelCarver::SmoothMesh needs a mesh and an initialized carver\n");
    return false;
  }
  vcy_ctx* ctx = impl_->slabs[0];
  return detail::SmoothMeshWith(mesh, iterations, lambda, mu, pin_boundary, with_normals,
                                [ctx](int64_t nv, int64_t nf, const float* v, const int32_t* f, const vcy_smooth_option* o,
                                      float* out, float* vn, float* fn) { return vcy_smooth_mesh(ctx, nv, nf, v, f, o, out, vn, fn); });
}

bool ShardedVoxelCarver::RenderMesh(const Mesh& mesh, const Camera& camera, Image1f* depth, Image1b* silhouette) {
  if (impl_->slabs.empty()) {
    LOGE("ShardedVoxelCarver::RenderMesh needs an initialized carver\n");
    return false;
  }
  return detail::RenderMeshWith(impl_->slabs[0], "ShardedVoxelCarver::RenderMesh", mesh, camera, depth, silhouette);
}

bool ShardedVoxelCarver::MeshAgreement(const Mesh& mesh, const std::vector<const Camera*>& cameras,
                                       const std::vector<Image1b>& silhouettes, std::vector<std::array<std::int64_t, 3>>* counts) {
  if (impl_->slabs.empty()) {
    LOGE("ShardedVoxelCarver::MeshAgreement needs an initialized carver\n");
    return false;
  }
  return detail::MeshAgreementWith(impl_->slabs[0], "ShardedVoxelCarver::MeshAgreement", mesh, cameras, silhouettes, counts);
}

bool ShardedVoxelCarver::ShadeMesh(const Mesh& mesh, const Camera& camera, Image3b* image, bool from_normals) {
  if (impl_->slabs.empty()) {
    LOGE("ShardedVoxelCarver::ShadeMesh needs an initialized carver\n");
    return false;
  }
  return detail::ShadeMeshWith(impl_->slabs[0], "ShardedVoxelCarver::ShadeMesh", mesh, camera, image, from_normals);
}

bool ShardedVoxelCarver::MeshPhotoError(const Mesh& mesh, const std::vector<const Camera*>& cameras, const std::vector<Image3b>& photos,
                                        const std::vector<Image1b>& silhouettes, std::vector<std::array<std::int64_t, 7>>* sums) {
  if (impl_->slabs.empty()) {
    LOGE("ShardedVoxelCarver::MeshPhotoError needs an initialized carver\n");
    return false;
  }
  return detail::MeshPhotoErrorWith(impl_->slabs[0], "ShardedVoxelCarver::MeshPhotoError", mesh, cameras, photos, silhouettes, sums);
}

std::array<float, 2> ShardedVoxelCarver::last_shade_ms() const {
  std::array<float, 2> ms = {{0.0f, 0.0f}};
  if (!impl_->slabs.empty()) vcy_last_shade_ms(impl_->slabs[0], &ms[0], &ms[1]);
  return ms;
}

bool ShardedVoxelCarver::DecimateMesh(Mesh* mesh, float cell, int mode, bool with_normals) {
  if (impl_->slabs.empty() || !mesh) {
    LOGE("ShardedVoxelCarver::DecimateMesh needs a mesh and an initialized carver\n");
    return false;
  }
  vcy_ctx* ctx = impl_->slabs[0];
  return detail::DecimateMeshWith(mesh, cell, impl_->option.bb_min, mode, with_normals,
                                  [ctx](int64_t nv, int64_t nf, const float* v, const int32_t* f, const vcy_decimate_option* o,
                                        float* vo, int32_t* fo, int64_t* nvo, int64_t* nfo, int32_t* map, int32_t* src, float* vn,
                                        float* fn) { return vcy_decimate_mesh(ctx, nv, nf, v, f, o, vo, fo, nvo, nfo, map, src, vn, fn); });
}

bool ShardedVoxelCarver::DecimateMeshQuadric(Mesh* mesh, float cell, float regularize, bool with_normals, std::int64_t* n_fallback) {
  if (impl_->slabs.empty() || !mesh) {
    LOGE("ShardedVoxelCarver::DecimateMeshQuadric needs a mesh and an initialized carver\n");
    return false;
  }
  vcy_ctx* ctx = impl_->slabs[0];
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

namespace {

// the distance field needs the whole grid in one context
bool OneSlab(const std::vector<vcy_ctx*>& slabs, const char* who) {
  if (slabs.size() == 1) return true;
  if (slabs.empty()) LOGE("voxel grid has not been initialized\n");
  else LOGE("%s: the grid is cut into %d z-slabs; the distance field needs the whole grid in one context\n", who,
            static_cast<int>(slabs.size()));
  return false;
}

}  // namespace

bool ShardedVoxelCarver::DistanceField(std::vector<std::int32_t>* d2, double iso_level, int radius) {
  if (!d2 || !OneSlab(impl_->slabs, "DistanceField")) return false;
  std::int32_t dims[3] = {0, 0, 0};
  vcy_grid_dims(impl_->slabs[0], dims);
  d2->resize(static_cast<size_t>(dims[0]) * dims[1] * dims[2]);
  if (vcy_distance_field(impl_->slabs[0], iso_level, radius, d2->data()) == VCY_OK) return true;
  LOGE("%s\n", vcy_last_error());
  d2->clear();
  return false;
}

bool ShardedVoxelCarver::Redistance(double iso_level, int radius) {
  if (!OneSlab(impl_->slabs, "Redistance")) return false;
  std::int64_t n = 0;
  if (vcy_redistance(impl_->slabs[0], iso_level, radius, &n) == VCY_OK) return true;
  LOGE("%s\n", vcy_last_error());
  return false;
}

bool ShardedVoxelCarver::CloseHull(float radius_voxels, double iso_level) {
  if (!OneSlab(impl_->slabs, "CloseHull")) return false;
  std::string error;
  const bool ok = detail::CloseHullOn(impl_->slabs[0], radius_voxels, iso_level, impl_->option.resolution, &error);
  if (!ok) LOGE("%s\n", error.c_str());
  return ok;
}

// Every slab finishes one step before any slab begins the next.  What a slab hands out: its lowest and its highest
// min(radius, own slices) planes of 16-bit values; what it gets, from as many neighbours as that takes, is put together
// by vcy_distance_halo_host.
bool ShardedVoxelCarver::Impl::DistanceSlabs(double iso_level, int radius, const char* who,
                                             const std::function<int(size_t, const uint16_t*, int, const uint16_t*, int)>& finish) {
  const size_t ns = slabs.size();
  if (ns == 0) {
    LOGE("voxel grid has not been initialized\n");
    return false;
  }
  if (!ForEachSlab(ns, who, [&](size_t s) { return vcy_distance_slab_begin(slabs[s], iso_level, radius); })) return false;
  const size_t plane = static_cast<size_t>(slice);
  std::vector<std::vector<uint16_t>> bottoms(ns), tops(ns);
  if (!ForEachSlab(ns, who, [&](size_t s) {
        const int m = std::min(radius, bounds[s + 1] - bounds[s]);
        if (s > 0) {
          bottoms[s].resize(plane * m);
          const int rc = vcy_distance_slab_planes(slabs[s], bounds[s], bounds[s] + m, bottoms[s].data());
          if (rc != VCY_OK) return rc;
        }
        if (s + 1 < ns) {
          tops[s].resize(plane * m);
          return vcy_distance_slab_planes(slabs[s], bounds[s + 1] - m, bounds[s + 1], tops[s].data());
        }
        return static_cast<int>(VCY_OK);
      }))
    return false;
  std::vector<const uint16_t*> bottom_of(ns), top_of(ns);  // (null where nobody asked for them: an empty vector's data())
  for (size_t s = 0; s < ns; ++s) bottom_of[s] = bottoms[s].data(), top_of[s] = tops[s].data();
  std::vector<std::vector<uint16_t>> below(ns), above(ns);
  std::vector<int> n_below(ns), n_above(ns);
  for (size_t s = 0; s < ns; ++s) {
    below[s].resize(plane * std::min(radius, bounds[s]));
    above[s].resize(plane * std::min(radius, bounds[ns] - bounds[s + 1]));
    if (vcy_distance_halo_host(static_cast<int>(ns), bounds.data(), radius, slice, bottom_of.data(), top_of.data(),
                               static_cast<int>(s), below[s].data(), above[s].data(), &n_below[s], &n_above[s]) != VCY_OK) {
      LOGE("%s: %s\n", who, vcy_last_error());
      return false;
    }
  }
  return ForEachSlab(ns, who, [&](size_t s) {
    return finish(s, n_below[s] ? below[s].data() : nullptr, n_below[s], n_above[s] ? above[s].data() : nullptr, n_above[s]);
  });
}

bool ShardedVoxelCarver::DistanceFieldSlabs(std::vector<std::int32_t>* d2, double iso_level, int radius) {
  if (!d2 || impl_->slabs.empty()) {
    LOGE("ShardedVoxelCarver::DistanceFieldSlabs needs an output and an initialized carver\n");
    return false;
  }
  const std::vector<int>& b = impl_->bounds;
  d2->resize(static_cast<size_t>(impl_->slice) * b.back());
  const bool ok = impl_->DistanceSlabs(iso_level, radius, "DistanceFieldSlabs",
                                       [&](size_t s, const uint16_t* below, int nb, const uint16_t* above, int na) {
                                         return vcy_distance_field_slab(impl_->slabs[s], below, nb, above, na,
                                                                        d2->data() + impl_->slice * b[s]);
                                       });
  if (!ok) d2->clear();
  return ok;
}

bool ShardedVoxelCarver::RedistanceSlabs(double iso_level, int radius, std::int64_t* n_rewritten) {
  std::vector<std::int64_t> n(impl_->slabs.size(), 0);
  const bool ok = impl_->DistanceSlabs(iso_level, radius, "RedistanceSlabs",
                                       [&](size_t s, const uint16_t* below, int nb, const uint16_t* above, int na) {
                                         return vcy_redistance_slab(impl_->slabs[s], below, nb, above, na, &n[s]);
                                       });
  if (ok && n_rewritten) {
    *n_rewritten = 0;
    for (std::int64_t k : n) *n_rewritten += k;
  }
  return ok;
}

bool ShardedVoxelCarver::CloseHullSlabs(float radius_voxels, double iso_level) {
  std::string error;
  const bool ok = detail::CloseHullSteps(radius_voxels, iso_level, impl_->option.resolution, &error, [&](double level, int big_r) {
    if (RedistanceSlabs(level, big_r, nullptr)) return true;
    error = "CloseHullSlabs: a step failed";
    return false;
  });
  if (!ok) LOGE("%s\n", error.c_str());
  return ok;
}

bool ShardedVoxelCarver::KeepLargestComponents(int largest, std::int64_t min_voxels, double iso_level, float fill_sdf) {
  if (!std::isfinite(fill_sdf) || !(static_cast<double>(fill_sdf) >= iso_level)) {
    LOGE("KeepLargestComponents: fill_sdf %g must be finite and not below the iso level %g\n", static_cast<double>(fill_sdf),
         iso_level);
    return false;
  }
  Impl::Labelled l;
  if (!impl_->LabelSlabs(iso_level, &l)) return false;
  std::vector<uint8_t> gone(l.merged.size()), piece_gone(l.global.size());  // per merged component, per piece of a slab
  std::int64_t n_gone = 0, gone_voxels = 0;
  if (vcy_select_components_host(l.merged.data(), static_cast<int64_t>(l.merged.size()), largest, min_voxels, gone.data(),
                                 &n_gone, &gone_voxels, l.global.data(), static_cast<int64_t>(l.global.size()),
                                 piece_gone.data()) != VCY_OK) {
    LOGE("KeepLargestComponents: %s\n", vcy_last_error());
    return false;
  }
  if (n_gone > 0) {
    const size_t ns = impl_->slabs.size();
    std::vector<int64_t> first(ns + 1, 0);
    for (size_t s = 0; s < ns; ++s) first[s + 1] = first[s] + l.counts[s];
    const bool ok = ForEachSlab(ns, "KeepLargestComponents", [&](size_t s) {
      std::vector<int64_t> mine;
      for (int64_t i = first[s]; i < first[s + 1]; ++i)
        if (piece_gone[static_cast<size_t>(i)]) mine.push_back(l.pieces[static_cast<size_t>(i)].label);
      return vcy_keep_components_slab(impl_->slabs[s], fill_sdf, static_cast<int64_t>(mine.size()), mine.data(), nullptr);
    });
    if (!ok) return false;
  }
  LOGI("KeepLargestComponents removed %lld components, %lld voxels\n", static_cast<long long>(n_gone),
       static_cast<long long>(gone_voxels));
  return true;
}

void ShardedVoxelCarver::ExtractVoxel(Mesh* mesh, bool inside_empty) {
  mesh->Clear();
  const size_t ns = impl_->slabs.size();
  if (ns == 0) return;
  // UpdateOnSurface (extract_voxel.cc:15-79) compares a voxel with its -z neighbour: the slice below a slab
  if (inside_empty && !ExchangeHalo()) return;
  std::vector<int64_t*> ids(ns, nullptr);
  std::vector<int64_t> counts(ns, 0);
  const bool ok = ForEachSlab(ns, "ExtractVoxel", [&](size_t s) {
    return vcy_extract_voxel_ids(impl_->slabs[s], inside_empty ? 1 : 0, &ids[s], &counts[s]);
  });
  if (ok) {
    // the kept voxels of the whole grid in scan order = the slabs' lists in z order; ONE cube drifts through them
    std::vector<int64_t> all;
    for (size_t s = 0; s < ns; ++s) all.insert(all.end(), ids[s], ids[s] + counts[s]);
    const vcy_carver_option c = detail::ToC(impl_->option);
    typedef detail::MeshArrays<Eigen::Vector3f, Eigen::Vector3i> Arrays;
    Arrays arrays{mesh->mutable_vertices(), mesh->mutable_vertex_indices()};
    if (vcy_voxel_cubes_into(&c, static_cast<int64_t>(all.size()), all.data(), &Arrays::Provide, &arrays) != VCY_OK) {
      LOGE("%s\n", vcy_last_error());
      mesh->Clear();
    }
  }
  for (int64_t* p : ids) vcy_ids_free(p);
}

void ShardedVoxelCarver::ExtractIsoSurface(Mesh* mesh, double iso_level, bool linear_interp) {
  ExtractIsoSurface(mesh, iso_level, linear_interp, false);
}

// Every slab extracts on its own device -- with_normals: its normals too (vcy_extract_iso_normals_slab) --, and
// vcy_merge_meshes_host stitches the parts by edge key, and finishes the normals of the seam vertices, into the Mesh's
// own vectors.
void ShardedVoxelCarver::ExtractIsoSurface(Mesh* mesh, double iso_level, bool linear_interp, bool with_normals) {
  mesh->Clear();
  const size_t ns = impl_->slabs.size();
  if (ns == 0) return;
  if (!ExchangeHalo()) return;
  std::vector<vcy_mesh> parts(ns);  // (all zero: nothing to free where a slab fails)
  std::vector<vcy_mesh_normals> normals(ns);
  std::vector<std::array<int64_t, 2>> layer_faces(ns);
  bool ok = ForEachSlab(ns, "extraction", [&](size_t s) {
    return with_normals ? vcy_extract_iso_normals_slab(impl_->slabs[s], iso_level, linear_interp ? 1 : 0,
                                                       VCY_NORMALS_VERTEX | VCY_NORMALS_FACE, &parts[s], &normals[s],
                                                       layer_faces[s].data())
                        : vcy_extract_iso(impl_->slabs[s], iso_level, linear_interp ? 1 : 0, &parts[s]);
  });
  if (ok) {
    static_assert(sizeof(Eigen::Vector3f) == 3 * sizeof(float) && sizeof(Eigen::Vector3i) == 3 * sizeof(int32_t), "packed vector layout");
    size_t nv = 0, nf = 0;  // (the sizes of vcy_merge_meshes_host's arrays; resize() initialises nothing, see mesh_copy.h)
    for (const vcy_mesh& m : parts) nv += static_cast<size_t>(m.n_vertices - m.n_foreign_vertices), nf += static_cast<size_t>(m.n_faces);
    mesh->mutable_vertices()->resize(nv);
    mesh->mutable_vertex_indices()->resize(nf);
    if (with_normals) mesh->mutable_normals()->resize(nv), mesh->mutable_face_normals()->resize(nf);
    ok = vcy_merge_meshes_host(static_cast<int>(ns), parts.data(), with_normals ? normals.data() : nullptr,
                               with_normals ? layer_faces[0].data() : nullptr,
                               reinterpret_cast<float*>(mesh->mutable_vertices()->data()),
                               reinterpret_cast<int32_t*>(mesh->mutable_vertex_indices()->data()), nullptr,
                               with_normals ? reinterpret_cast<float*>(mesh->mutable_normals()->data()) : nullptr,
                               with_normals ? reinterpret_cast<float*>(mesh->mutable_face_normals()->data()) : nullptr) == VCY_OK;
    if (!ok) LOGE("sharded merge: %s\n", vcy_last_error());
    if (ok && with_normals) mesh->set_normal_indices(mesh->vertex_indices());
  }
  if (!ok) mesh->Clear();
  for (vcy_mesh& m : parts) vcy_mesh_free(&m);
  for (vcy_mesh_normals& n : normals) vcy_mesh_normals_free(&n);
}

}  // namespace vacancy
