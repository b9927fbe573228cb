// CPU-only check of the facade's host utilities (no GPU calls): PNG decode of the bunny masks,
// TUM pose -> w2c arithmetic.  Prints values that tests/test_host.py compares with fixtures.
#include <algorithm>
#include <array>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "vacancy/camera.h"
#include "vacancy/image.h"
#include "vacancy/mesh.h"
#include "vacancy/sharded_voxel_carver.h"
#include "vacancy/voxel_carver.h"

namespace {
// A user's Camera: only Project() overridden -- all the reference's carve path calls (camera.h:39-40,
// voxel_carver.cc:460).  It must compile against the facade, and Carve() must refuse it loudly (the device
// evaluates PinholeCamera and OrthoCamera only).
class FisheyeCamera : public vacancy::Camera {
 public:
  FisheyeCamera(int w, int h) : vacancy::Camera(w, h) {}
  void Project(const Eigen::Vector3f& p, Eigen::Vector2f* q) const override {
    const float r = std::sqrt(p[0] * p[0] + p[1] * p[1]), th = std::atan2(r, p[2]);
    (*q)[0] = 100.0f * th * (r > 0 ? p[0] / r : 0.0f) + 0.5f * width_;
    (*q)[1] = 100.0f * th * (r > 0 ? p[1] / r : 0.0f) + 0.5f * height_;
  }
};
}  // namespace

int main(int argc, char* argv[]) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  if (argc > 2 && std::string(argv[2]) == "gpu") {
    // needs a device: a carver that works for the two known cameras and says no to a third
    vacancy::VoxelCarverOption opt;
    opt.bb_min = Eigen::Vector3f(-16.f, -16.f, -16.f);
    opt.bb_max = Eigen::Vector3f(16.f, 16.f, 16.f);
    opt.resolution = 1.0f;
    vacancy::VoxelCarver carver(opt);
    if (!carver.Init()) return 3;
    vacancy::Image1f sdf(64, 48);
    for (float& v : *sdf.data_ptr()) v = 0.25f;
    Eigen::Translation3d t;
    t.x() = 0.0; t.y() = 0.0; t.z() = -80.0;
    Eigen::Quaterniond q;
    q.x() = 0.0; q.y() = 0.0; q.z() = 0.0; q.w() = 1.0;
    vacancy::PinholeCamera pin(64, 48, t * q, 60.0f);
    vacancy::OrthoCamera ortho(64, 48, t * q);
    FisheyeCamera fish(64, 48);
    const bool a = carver.Carve(pin, sdf), b = carver.Carve(ortho, sdf), c = carver.Carve(fish, sdf);
    std::vector<vacancy::Image1b> sil(1, vacancy::Image1b(64, 48));
    const bool d = carver.Carve(std::vector<const vacancy::Camera*>{&fish}, sil);
    std::vector<float> s;
    std::vector<int> n;
    const bool e = carver.Download(&s, &n);
    long long touched = 0;
    for (int k : n) touched += k > 0;
    std::printf("CUSTOMCAM %d %d %d %d %d %lld\n", a ? 1 : 0, b ? 1 : 0, c ? 1 : 0, d ? 1 : 0, e ? 1 : 0, touched);
    return 0;
  }
  if (argc > 3 && std::string(argv[2]) == "xvtime") {
    // needs a device: what the class API's extractions cost per call, Mesh included (a fresh Mesh per view, as
    // examples.cc:117-149 has it).   host_selftest <data dir> xvtime <resolution>
    std::vector<Eigen::Affine3d> poses;
    {
      std::FILE* fp = std::fopen((dir + "/tumpose.txt").c_str(), "r");
      if (!fp) return 9;
      int id;
      double t[3], q[4];
      while (std::fscanf(fp, "%d %lf %lf %lf %lf %lf %lf %lf", &id, &t[0], &t[1], &t[2], &q[0], &q[1], &q[2], &q[3]) == 8) {
        Eigen::Translation3d tr;
        tr.x() = t[0]; tr.y() = t[1]; tr.z() = t[2];
        Eigen::Quaterniond qu;
        qu.x() = q[0]; qu.y() = q[1]; qu.z() = q[2]; qu.w() = q[3];
        poses.push_back(tr * qu);
      }
      std::fclose(fp);
    }
    vacancy::VoxelCarverOption option;
    option.bb_min = Eigen::Vector3f(-270.000000f, -364.586151f, -149.982697f);
    option.bb_max = Eigen::Vector3f(270.000000f, 170.542343f, 277.329224f);
    option.resolution = (float)std::atof(argv[3]);
    vacancy::VoxelCarver carver(option);
    if (!carver.Init()) return 3;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const int n_slabs = argc > 4 ? std::atoi(argv[4]) : 0;  // > 0: the same views through ShardedVoxelCarver (z-slabs on device 0)
    for (int rep = 0; rep < 2; ++rep) {
      vacancy::VoxelCarver c2(option);
      if (!c2.Init()) return 3;
      std::unique_ptr<vacancy::ShardedVoxelCarver> sh;
      if (n_slabs > 0) {
        sh.reset(new vacancy::ShardedVoxelCarver(option, {0}, n_slabs));
        if (!sh->Init()) return 6;
      }
      for (size_t i = 0; i < 6 && i < poses.size(); ++i) {
        vacancy::PinholeCamera cam(320, 240, poses[i], Eigen::Vector2f(159.3f, 127.65f), Eigen::Vector2f(258.65f, 258.25f));
        vacancy::Image1b sil;
        if (!sil.Load(dir + "/mask_" + vacancy::zfill(i) + ".png")) return 4;
        vacancy::Image1f sdf;
        double t0 = now();
        if (!c2.Carve(cam, sil, &sdf)) return 5;
        const double t_carve = now() - t0;
        t0 = now();
        vacancy::Mesh voxels;
        c2.ExtractVoxel(&voxels);
        const double t_xv = now() - t0;
        t0 = now();
        vacancy::Mesh surface;
        c2.ExtractIsoSurface(&surface, 0.0);
        const double t_mc = now() - t0;
        {
          // normals: the device overload (call -> Mesh with normals) next to ExtractIsoSurface + CalcNormal() on the host
          t0 = now();
          vacancy::Mesh dn;
          c2.ExtractIsoSurface(&dn, 0.0, true, true);
          const double t_dev = now() - t0;
          t0 = now();
          vacancy::Mesh hn;
          c2.ExtractIsoSurface(&hn, 0.0, true);
          hn.CalcNormal();
          const double t_host = now() - t0;
          const bool same = dn.normals().size() == hn.normals().size() &&
                            (dn.normals().empty() || !std::memcmp(dn.normals().data(), hn.normals().data(), 12 * hn.normals().size())) &&
                            dn.face_normals().size() == hn.face_normals().size() &&
                            (dn.face_normals().empty() || !std::memcmp(dn.face_normals().data(), hn.face_normals().data(), 12 * hn.face_normals().size()));
          std::printf("XVTIME rep %d view %zu: ExtractIsoSurface(with_normals) %.3f ms, ExtractIsoSurface + CalcNormal() on the host %.3f ms (%zu vertices, identical %d)\n",
                      rep, i, t_dev, t_host, dn.normals().size(), same ? 1 : 0);
        }
        if (sh) {
          if (!sh->Carve(cam, sil)) return 7;
          t0 = now();
          vacancy::Mesh sm;
          sh->ExtractIsoSurface(&sm, 0.0);
          const double t_s = now() - t0;
          t0 = now();
          vacancy::Mesh sv;
          sh->ExtractVoxel(&sv);
          std::printf("XVTIME rep %d view %zu: %d slabs: ExtractIsoSurface %.3f ms (%zu vertices, identical %d), ExtractVoxel %.2f ms (%zu vertices)\n", rep, i,
                      sh->slab_count(), t_s, sm.vertices().size(),
                      sm.vertices().size() == surface.vertices().size() && sm.vertex_indices().size() == surface.vertex_indices().size() ? 1 : 0,
                      now() - t0, sv.vertices().size());
        }
        std::printf("XVTIME rep %d view %zu: Carve(silhouette, &sdf) %.3f ms, ExtractVoxel %.2f ms (%zu vertices), ExtractIsoSurface %.3f ms (%zu vertices)\n", rep, i,
                    t_carve, t_xv, voxels.vertices().size(), t_mc, surface.vertices().size());
      }
    }
    return 0;
  }
  if (argc > 5 && std::string(argv[2]) == "shardnormals") {
    // needs a device: ShardedVoxelCarver::ExtractIsoSurface(with_normals) after the six bunny views, written out raw.
    //   host_selftest <data dir> shardnormals <resolution> <slabs on device 0> <out dir> [iso level] [linear interp]
    //   writes <out dir>/vertices.f32, faces.i32, normals.f32, face_normals.f32, prints SHARDNORMALS <slabs> <sizes>
    vacancy::VoxelCarverOption option;
    option.bb_min = Eigen::Vector3f(-250.000000f, -344.586151f, -129.982697f);
    option.bb_max = Eigen::Vector3f(250.000000f, 150.542343f, 257.329224f);
    for (int i = 0; i < 3; ++i) {  // (examples.cc:91-99)
      option.bb_min[i] -= 20.0f;
      option.bb_max[i] += 20.0f;
    }
    option.resolution = (float)std::atof(argv[3]);
    const std::string out = argv[5];
    const double iso = argc > 6 ? std::atof(argv[6]) : 0.0;
    const bool interp = argc > 7 ? std::atoi(argv[7]) != 0 : true;
    vacancy::ShardedVoxelCarver sh(option, {0}, std::atoi(argv[4]));
    if (!sh.Init()) return 6;
    std::FILE* fp = std::fopen((dir + "/tumpose.txt").c_str(), "r");
    if (!fp) return 9;
    int id;
    double t[3], q[4];
    for (size_t i = 0; i < 6 && std::fscanf(fp, "%d %lf %lf %lf %lf %lf %lf %lf", &id, &t[0], &t[1], &t[2], &q[0], &q[1], &q[2], &q[3]) == 8; ++i) {
      Eigen::Translation3d tr;
      tr.x() = t[0]; tr.y() = t[1]; tr.z() = t[2];
      Eigen::Quaterniond qu;
      qu.x() = q[0]; qu.y() = q[1]; qu.z() = q[2]; qu.w() = q[3];
      vacancy::PinholeCamera cam(320, 240, tr * qu, Eigen::Vector2f(159.3f, 127.65f), Eigen::Vector2f(258.65f, 258.25f));
      vacancy::Image1b sil;
      if (!sil.Load(dir + "/mask_" + vacancy::zfill(i) + ".png")) return 4;
      if (!sh.Carve(cam, sil)) return 7;
    }
    std::fclose(fp);
    vacancy::Mesh mesh;
    sh.ExtractIsoSurface(&mesh, iso, interp, true);
    auto dump = [](const std::string& path, const void* p, size_t bytes) {
      std::FILE* f = std::fopen(path.c_str(), "wb");
      if (!f) return false;
      if (bytes) std::fwrite(p, 1, bytes, f);
      std::fclose(f);
      return true;
    };
    bool ok = dump(out + "/vertices.f32", mesh.vertices().data(), 12 * mesh.vertices().size());
    ok = ok && dump(out + "/faces.i32", mesh.vertex_indices().data(), 12 * mesh.vertex_indices().size());
    ok = ok && dump(out + "/normals.f32", mesh.normals().data(), 12 * mesh.normals().size());
    ok = ok && dump(out + "/face_normals.f32", mesh.face_normals().data(), 12 * mesh.face_normals().size());
    std::printf("SHARDNORMALS %d %d %zu %zu %zu %zu %zu\n", ok ? 1 : 0, sh.slab_count(), mesh.vertices().size(),
                mesh.vertex_indices().size(), mesh.normals().size(), mesh.face_normals().size(), mesh.normal_indices().size());
    return ok ? 0 : 8;
  }
  if (argc > 4 && std::string(argv[2]) == "shardcomponents") {
    // needs a device: ShardedVoxelCarver::LabelComponents / KeepLargestComponents after the six bunny views, next to a
    // single VoxelCarver.   host_selftest <data dir> shardcomponents <resolution> <slabs on device 0>
    //   prints SHARDCOMPONENTS <slabs> <components> <lists equal> <components after> <lists after equal> <mesh identical>
    vacancy::VoxelCarverOption option;
    option.bb_min = Eigen::Vector3f(-250.000000f, -344.586151f, -129.982697f);
    option.bb_max = Eigen::Vector3f(250.000000f, 150.542343f, 257.329224f);
    for (int i = 0; i < 3; ++i) {  // (examples.cc:91-99)
      option.bb_min[i] -= 20.0f;
      option.bb_max[i] += 20.0f;
    }
    option.resolution = (float)std::atof(argv[3]);
    vacancy::VoxelCarver one(option);
    vacancy::ShardedVoxelCarver sh(option, {0}, std::atoi(argv[4]));
    if (!one.Init() || !sh.Init()) return 6;
    std::FILE* fp = std::fopen((dir + "/tumpose.txt").c_str(), "r");
    if (!fp) return 9;
    int id;
    double t[3], q[4];
    for (size_t i = 0; i < 6 && std::fscanf(fp, "%d %lf %lf %lf %lf %lf %lf %lf", &id, &t[0], &t[1], &t[2], &q[0], &q[1], &q[2], &q[3]) == 8; ++i) {
      Eigen::Translation3d tr;
      tr.x() = t[0]; tr.y() = t[1]; tr.z() = t[2];
      Eigen::Quaterniond qu;
      qu.x() = q[0]; qu.y() = q[1]; qu.z() = q[2]; qu.w() = q[3];
      vacancy::PinholeCamera cam(320, 240, tr * qu, Eigen::Vector2f(159.3f, 127.65f), Eigen::Vector2f(258.65f, 258.25f));
      vacancy::Image1b sil;
      if (!sil.Load(dir + "/mask_" + vacancy::zfill(i) + ".png")) return 4;
      if (!one.Carve(cam, sil) || !sh.Carve(cam, sil)) return 7;
    }
    std::fclose(fp);
    auto same_lists = [](const std::vector<vacancy::VoxelComponent>& a, const std::vector<vacancy::VoxelComponent>& b) {
      bool same = a.size() == b.size();
      for (size_t i = 0; same && i < a.size(); ++i)
        for (int k = 0; k < 3; ++k)
          same = same && a[i].label == b[i].label && a[i].n_voxels == b[i].n_voxels && a[i].bb_min[k] == b[i].bb_min[k] &&
                 a[i].bb_max[k] == b[i].bb_max[k];
      return same;
    };
    std::vector<vacancy::VoxelComponent> a, b, a2, b2;
    if (!one.LabelComponents(&a) || !sh.LabelComponents(&b)) return 10;
    if (!one.KeepLargestComponents(1) || !sh.KeepLargestComponents(1)) return 11;
    if (!one.LabelComponents(&a2) || !sh.LabelComponents(&b2)) return 12;
    vacancy::Mesh ma, mb;
    one.ExtractIsoSurface(&ma, 0.0);
    sh.ExtractIsoSurface(&mb, 0.0);
    bool same = ma.vertices().size() == mb.vertices().size() && ma.vertex_indices().size() == mb.vertex_indices().size();
    for (size_t k = 0; same && k < ma.vertices().size(); ++k)
      for (int c = 0; c < 3; ++c) same = same && ma.vertices()[k][c] == mb.vertices()[k][c];
    for (size_t k = 0; same && k < ma.vertex_indices().size(); ++k)
      for (int c = 0; c < 3; ++c) same = same && ma.vertex_indices()[k][c] == mb.vertex_indices()[k][c];
    std::printf("SHARDCOMPONENTS %d %zu %d %zu %d %d\n", sh.slab_count(), b.size(), same_lists(a, b) ? 1 : 0, b2.size(),
                same_lists(a2, b2) ? 1 : 0, same ? 1 : 0);
    return 0;
  }
  if (argc > 4 && std::string(argv[2]) == "slabrender") {
    // needs a device: ShardedVoxelCarver::RenderHullSlabs / HullAgreementSlabs after the six bunny views, next to a single
    // VoxelCarver's RenderHull / HullAgreement.   host_selftest <data dir> slabrender <resolution> <slabs on device 0>
    //   prints SLABRENDER <slabs> <depth bytes equal> <silhouette equal> <counts equal>
    vacancy::VoxelCarverOption option;
    option.bb_min = Eigen::Vector3f(-250.000000f, -344.586151f, -129.982697f);
    option.bb_max = Eigen::Vector3f(250.000000f, 150.542343f, 257.329224f);
    for (int i = 0; i < 3; ++i) {  // (examples.cc:91-99)
      option.bb_min[i] -= 20.0f;
      option.bb_max[i] += 20.0f;
    }
    option.resolution = (float)std::atof(argv[3]);
    vacancy::VoxelCarver one(option);
    vacancy::ShardedVoxelCarver sh(option, {0}, std::atoi(argv[4]));
    if (!one.Init() || !sh.Init()) return 6;
    std::FILE* fp = std::fopen((dir + "/tumpose.txt").c_str(), "r");
    if (!fp) return 9;
    int id;
    double t[3], q[4];
    std::vector<vacancy::PinholeCamera> cams;
    std::vector<vacancy::Image1b> sils;
    for (size_t i = 0; i < 6 && std::fscanf(fp, "%d %lf %lf %lf %lf %lf %lf %lf", &id, &t[0], &t[1], &t[2], &q[0], &q[1], &q[2], &q[3]) == 8; ++i) {
      Eigen::Translation3d tr;
      tr.x() = t[0]; tr.y() = t[1]; tr.z() = t[2];
      Eigen::Quaterniond qu;
      qu.x() = q[0]; qu.y() = q[1]; qu.z() = q[2]; qu.w() = q[3];
      cams.emplace_back(320, 240, tr * qu, Eigen::Vector2f(159.3f, 127.65f), Eigen::Vector2f(258.65f, 258.25f));
      vacancy::Image1b sil;
      if (!sil.Load(dir + "/mask_" + vacancy::zfill(i) + ".png")) return 4;
      if (!one.Carve(cams.back(), sil) || !sh.Carve(cams.back(), sil)) return 7;
      sils.push_back(sil);
    }
    std::fclose(fp);
    bool depth_same = !cams.empty(), sil_same = !cams.empty(), counts_same = !cams.empty();
    for (size_t i = 0; i < cams.size(); ++i) {
      vacancy::Image1f da, db;
      vacancy::Image1b ha, hb;
      if (!one.RenderHull(cams[i], &da, &ha) || !sh.RenderHullSlabs(cams[i], &db, &hb)) return 10;
      depth_same = depth_same && da.data().size() == db.data().size() &&
                   std::memcmp(da.data().data(), db.data().data(), sizeof(float) * da.data().size()) == 0;
      sil_same = sil_same && ha.data() == hb.data();
      std::vector<std::array<std::int64_t, 3>> ca, cb;
      const std::vector<const vacancy::Camera*> ptr{&cams[i]};
      const std::vector<vacancy::Image1b> s1{sils[i]};
      if (!one.HullAgreement(ptr, s1, &ca) || !sh.HullAgreementSlabs(ptr, s1, &cb)) return 11;
      counts_same = counts_same && ca == cb && ca.size() == 1 && ca[0][0] > 0;
    }
    std::printf("SLABRENDER %d %d %d %d\n", sh.slab_count(), depth_same ? 1 : 0, sil_same ? 1 : 0, counts_same ? 1 : 0);
    return 0;
  }
  if (argc > 4 && std::string(argv[2]) == "shardrender") {
    // needs a device: the ray-cast of the hull needs the whole grid in one context, so ShardedVoxelCarver::RenderHull /
    // HullAgreement refuse, and VoxelCarver's own refuse bad arguments -- each with false and a logged error.
    //   host_selftest <data dir> shardrender <resolution> <slabs on device 0>
    //   prints SHARDRENDER <slabs> <sharded RenderHull> <sharded HullAgreement> <null depth> <count mismatch> <no list>
    //          <before Init> <good call>
    vacancy::VoxelCarverOption option;
    option.bb_min = Eigen::Vector3f(-250.000000f, -344.586151f, -129.982697f);
    option.bb_max = Eigen::Vector3f(250.000000f, 150.542343f, 257.329224f);
    for (int i = 0; i < 3; ++i) {  // (examples.cc:91-99)
      option.bb_min[i] -= 20.0f;
      option.bb_max[i] += 20.0f;
    }
    option.resolution = (float)std::atof(argv[3]);
    vacancy::VoxelCarver one(option), never(option);
    vacancy::ShardedVoxelCarver sh(option, {0}, std::atoi(argv[4]));
    if (!one.Init() || !sh.Init()) return 6;
    vacancy::PinholeCamera cam(320, 240, Eigen::Affine3d::Identity(), Eigen::Vector2f(159.3f, 127.65f),
                               Eigen::Vector2f(258.65f, 258.25f));
    vacancy::Image1b sil;
    if (!sil.Load(dir + "/mask_" + vacancy::zfill(0) + ".png")) return 4;
    if (!one.Carve(cam, sil) || !sh.Carve(cam, sil)) return 7;
    vacancy::Image1f depth;
    vacancy::Image1b hull;
    std::vector<std::array<std::int64_t, 3>> counts;
    const std::vector<const vacancy::Camera*> cams{&cam};
    const std::vector<vacancy::Image1b> sils{sil}, two{sil, sil};
    const bool r0 = sh.RenderHull(cam, &depth, &hull);
    const bool r1 = sh.HullAgreement(std::vector<vacancy::Camera>(), std::vector<vacancy::Image1b>(), &counts);
    const bool r2 = one.RenderHull(cam, nullptr);
    const bool r3 = one.HullAgreement(cams, two, &counts);
    const bool r4 = one.HullAgreement(cams, sils, nullptr);
    const bool r5 = never.RenderHull(cam, &depth) || never.HullAgreement(cams, sils, &counts);
    const bool r6 = one.RenderHull(cam, &depth, &hull) && one.HullAgreement(cams, sils, &counts) && counts.size() == 1 &&
                    depth.width() == 320 && hull.height() == 240;
    std::printf("SHARDRENDER %d %d %d %d %d %d %d %d\n", sh.slab_count(), r0 ? 1 : 0, r1 ? 1 : 0, r2 ? 1 : 0, r3 ? 1 : 0,
                r4 ? 1 : 0, r5 ? 1 : 0, r6 ? 1 : 0);
    return 0;
  }
  if (argc > 3 && std::string(argv[2]) == "colormesh") {
    // needs a device: VoxelCarver::ColorMesh on the synthetic sphere scene (vacancy_amd/synth.py: an N^3 grid, cameras on a
    // Fibonacci sphere at distance 2 N, a sphere of radius 0.35 N) with a photograph of one constant colour per view.
    //   host_selftest <data dir> colormesh <out dir>
    //   writes <out>/colored.ply (ASCII), prints one VIEWCOLOR <r> <g> <b> per view, FALLBACK <r> <g> <b> and
    //   COLORMESH <ok> <vertices> <colours> <colours of the kBest run that are no view's colour> <bad calls refused>
    const int n = 24, n_views = 8, w = 48, h = 40;
    vacancy::VoxelCarverOption option;
    option.bb_min = Eigen::Vector3f(-0.5f * n, -0.5f * n, -0.5f * n);
    option.bb_max = Eigen::Vector3f(0.5f * n, 0.5f * n, 0.5f * n);
    option.resolution = 1.0f;
    vacancy::VoxelCarver carver(option), never(option);
    if (!carver.Init()) return 3;
    const double radius = 0.35 * n, dist = 2.0 * n, lim = radius * radius / (dist * dist - radius * radius);
    std::vector<std::shared_ptr<vacancy::Camera>> cams;
    std::vector<const vacancy::Camera*> cam_ptrs;
    std::vector<vacancy::Image1b> sils;
    std::vector<vacancy::Image3b> photos;
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n_views; ++i) {
      const double y = 1.0 - 2.0 * (i + 0.5) / n_views, r = std::sqrt(std::max(0.0, 1.0 - y * y));
      const double phi = i * pi * (3.0 - std::sqrt(5.0));
      const Eigen::Vector3d pos(dist * r * std::cos(phi), dist * y, dist * r * std::sin(phi));
      std::shared_ptr<vacancy::PinholeCamera> cam(
          new vacancy::PinholeCamera(w, h, vacancy::c2w(pos, Eigen::Vector3d(0.0, 0.0, 0.0), Eigen::Vector3d(0.0, 1.0, 0.0)), 60.0f));
      vacancy::Image1b sil(w, h);
      vacancy::Image3b photo(w, h);
      for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
          const double du = (u - cam->principal_point()[0]) / cam->focal_length()[0];
          const double dv = (v - cam->principal_point()[1]) / cam->focal_length()[1];
          sil.at(u, v, 0) = du * du + dv * dv <= lim ? 255 : 0;
          photo.at(u, v, 0) = (unsigned char)(30 + 25 * i), photo.at(u, v, 1) = (unsigned char)(220 - 20 * i);
          photo.at(u, v, 2) = (unsigned char)(60 + (i * 37) % 120);
        }
      std::printf("VIEWCOLOR %d %d %d\n", 30 + 25 * i, 220 - 20 * i, 60 + (i * 37) % 120);
      cams.push_back(cam);
      cam_ptrs.push_back(cam.get());
      sils.push_back(sil);
      photos.push_back(photo);
    }
    if (!carver.Carve(cam_ptrs, sils)) return 7;
    vacancy::Mesh mesh;
    carver.ExtractIsoSurface(&mesh);
    vacancy::ColorOption copt;  // kWeighted, bilinear, 1.5 voxels of tolerance
    copt.fallback = Eigen::Vector3f(100.0f, 150.0f, 90.0f);
    std::printf("FALLBACK 100 150 90\n");
    bool ok = carver.ColorMesh(&mesh, cam_ptrs, photos, copt);
    ok = ok && !mesh.normals().empty() && mesh.WritePly(std::string(argv[3]) + "/colored.ply");
    const size_t nv = mesh.vertices().size(), nc = mesh.vertex_colors().size();
    // kBest with the NN sampler: every colour is one view's colour, or the fallback
    vacancy::Mesh best = mesh;
    copt.mode = vacancy::ColorMode::kBest;
    copt.interp = vacancy::SdfInterpolation::kNn;
    ok = ok && carver.ColorMesh(&best, cam_ptrs, photos, copt) && best.vertex_colors().size() == nv;
    size_t foreign = 0;
    for (const Eigen::Vector3f& c : best.vertex_colors()) {
      bool known = c[0] == 100.0f && c[1] == 150.0f && c[2] == 90.0f;
      for (int i = 0; i < n_views; ++i)
        known = known || (c[0] == (float)(30 + 25 * i) && c[1] == (float)(220 - 20 * i) && c[2] == (float)(60 + (i * 37) % 120));
      foreign += known ? 0 : 1;
    }
    // refused, the colours untouched: no photographs, one photograph too few, a null mesh, a carver without a grid
    int refused = 0;
    std::vector<vacancy::Image3b> fewer(photos.begin(), photos.end() - 1);
    refused += carver.ColorMesh(&best, cam_ptrs, fewer, copt) ? 0 : 1;
    refused += carver.ColorMesh(&best, std::vector<const vacancy::Camera*>(), std::vector<vacancy::Image3b>(), copt) ? 0 : 1;
    refused += carver.ColorMesh(nullptr, cam_ptrs, photos, copt) ? 0 : 1;
    refused += never.ColorMesh(&best, cam_ptrs, photos, copt) ? 0 : 1;
    copt.min_cos = -1.0f;
    refused += carver.ColorMesh(&best, cam_ptrs, photos, copt) ? 0 : 1;
    ok = ok && best.vertex_colors().size() == nv;
    std::printf("COLORMESH %d %zu %zu %zu %d\n", ok ? 1 : 0, nv, nc, foreign, refused);
    return 0;
  }
  if (argc > 3 && std::string(argv[2]) == "normals") {
    // CPU only: Mesh::CalcNormal through the facade.   host_selftest <data dir> normals <dir>
    //   reads <dir>/vertices.f32 and <dir>/faces.i32, writes <dir>/normals.f32, face_normals.f32, normal_indices.i32,
    //   with_normals.ply and without_normals.ply (WritePlyBinary), prints NORMALS <ok> <sizes> <sizes after Clear()>
    const std::string d = argv[3];
    auto slurp = [](const std::string& path, std::vector<char>* out) {
      std::FILE* fp = std::fopen(path.c_str(), "rb");
      if (!fp) return false;
      char buf[65536];
      size_t n;
      while ((n = std::fread(buf, 1, sizeof(buf), fp)) > 0) out->insert(out->end(), buf, buf + n);
      std::fclose(fp);
      return true;
    };
    auto dump = [](const std::string& path, const void* p, size_t bytes) {
      std::FILE* fp = std::fopen(path.c_str(), "wb");
      if (!fp) return false;
      if (bytes) std::fwrite(p, 1, bytes, fp);
      std::fclose(fp);
      return true;
    };
    std::vector<char> vb, fb;
    if (!slurp(d + "/vertices.f32", &vb) || !slurp(d + "/faces.i32", &fb)) return 4;
    vacancy::Mesh mesh;
    mesh.mutable_vertices()->resize(vb.size() / 12);
    mesh.mutable_vertex_indices()->resize(fb.size() / 12);
    if (!vb.empty()) std::memcpy(mesh.mutable_vertices()->data(), vb.data(), vb.size());
    if (!fb.empty()) std::memcpy(mesh.mutable_vertex_indices()->data(), fb.data(), fb.size());
    bool ok = mesh.WritePlyBinary(d + "/without_normals.ply");
    mesh.CalcNormal();
    ok = ok && dump(d + "/normals.f32", mesh.normals().data(), 12 * mesh.normals().size());
    ok = ok && dump(d + "/face_normals.f32", mesh.face_normals().data(), 12 * mesh.face_normals().size());
    ok = ok && dump(d + "/normal_indices.i32", mesh.normal_indices().data(), 12 * mesh.normal_indices().size());
    ok = ok && mesh.WritePlyBinary(d + "/with_normals.ply");
    const size_t a = mesh.normals().size(), b = mesh.face_normals().size(), c = mesh.normal_indices().size();
    mesh.Clear();
    std::printf("NORMALS %d %zu %zu %zu %zu %zu %zu\n", ok ? 1 : 0, a, b, c, mesh.normals().size(), mesh.face_normals().size(),
                mesh.normal_indices().size());
    return 0;
  }
  if (argc > 3 && std::string(argv[2]) == "io") {
    // Host outputs nothing else looks at (rows f3 / f4): tests/test_host.py reads every byte of these files back.
    //   <out>/mesh_ascii.ply, mesh_binary.ply, mesh_empty.ply: the same small mesh through both writers
    //   <out>/sdf_<i>.f32 (written by the test) -> SignedDistance2Color -> <out>/vis_<i>.rgb (raw) and vis_<i>.png
    //   PNGRT lines: WritePng -> Load gives the pixels back (1 and 3 channels)
    const std::string out = argv[3];
    vacancy::Mesh mesh;
    std::vector<Eigen::Vector3f> v;
    std::vector<Eigen::Vector3i> f;
    for (int i = 0; i < 5000; ++i)  // (values with short and long %g forms, negative zero, denormal-free)
      v.push_back(Eigen::Vector3f(0.1f * i - 250.0f, 1.0f / (1.0f + i), (i % 7) * -1234.5678f));
    for (int i = 0; i < 9000; ++i) f.push_back(Eigen::Vector3i(i % 5000, (i * 7 + 1) % 5000, (i * 13 + 2) % 5000));
    mesh.set_vertices(v);
    mesh.set_vertex_indices(f);
    bool ok = mesh.WritePly(out + "/mesh_ascii.ply") && mesh.WritePlyBinary(out + "/mesh_binary.ply");
    vacancy::Mesh empty;
    ok = ok && empty.WritePlyBinary(out + "/mesh_empty.ply");
    ok = ok && !mesh.WritePlyBinary(out + "/no/such/dir/x.ply");
    std::printf("PLY %d %zu %zu\n", ok ? 1 : 0, v.size(), f.size());
    for (int i = 0; i < 6; ++i) {
      vacancy::Image1b m;
      if (!m.Load(dir + "/mask_" + vacancy::zfill(i) + ".png")) return 1;
      vacancy::Image1f sdf(m.width(), m.height());
      std::FILE* fp = std::fopen((out + "/sdf_" + std::to_string(i) + ".f32").c_str(), "rb");
      if (!fp) return 4;
      const size_t n = sdf.data().size();
      if (std::fread(sdf.data_ptr()->data(), sizeof(float), n, fp) != n) return 5;
      std::fclose(fp);
      vacancy::Image3b vis;
      // (the ranges examples.cc passes: -1 .. 1 for normalised fields; view 3 with a narrower one so that both clamps fire)
      const float lo = i == 3 ? -0.25f : -1.0f, hi = i == 3 ? 0.125f : 1.0f;
      vacancy::SignedDistance2Color(sdf, &vis, lo, hi);
      fp = std::fopen((out + "/vis_" + std::to_string(i) + ".rgb").c_str(), "wb");
      if (!fp) return 6;
      std::fwrite(vis.data().data(), 1, vis.data().size(), fp);
      std::fclose(fp);
      bool rt = vis.WritePng(out + "/vis_" + std::to_string(i) + ".png");
      vacancy::Image3b back;
      rt = rt && back.Load(out + "/vis_" + std::to_string(i) + ".png") && back.width() == vis.width() &&
           back.height() == vis.height() && back.data() == vis.data();
      bool rt1 = m.WritePng(out + "/mask_" + std::to_string(i) + ".png");
      vacancy::Image1b back1;
      rt1 = rt1 && back1.Load(out + "/mask_" + std::to_string(i) + ".png") && back1.data() == m.data() &&
            back1.width() == m.width();
      vacancy::Image3b wrong;
      const bool refuses = !wrong.Load(out + "/mask_" + std::to_string(i) + ".png");  // 1 channel into a 3-channel image
      std::printf("PNGRT %d %d %d %d\n", i, rt ? 1 : 0, rt1 ? 1 : 0, refuses ? 1 : 0);
    }
    vacancy::Image1b none;
    std::printf("PNGEMPTY %d\n", none.WritePng(out + "/none.png") ? 1 : 0);
    return 0;
  }
  for (int i = 0; i < 6; ++i) {
    vacancy::Image1b m;
    if (!m.Load(dir + "/mask_" + vacancy::zfill(i) + ".png")) return 1;
    unsigned long long sum = 0;
    for (unsigned char p : m.data()) sum += p;
    std::printf("MASK %d %d %d %llu\n", i, m.width(), m.height(), sum);
  }
  // view 2 of tumpose.txt
  Eigen::Translation3d t;
  t.x() = 710.836121; t.y() = -48.510956; t.z() = 31.836634;
  Eigen::Quaterniond q;
  q.x() = 0.0; q.y() = -0.707107; q.z() = 0.0; q.w() = 0.707107;
  vacancy::PinholeCamera cam(320, 240, t * q, Eigen::Vector2f(159.3f, 127.65f), Eigen::Vector2f(258.65f, 258.25f));
  const Eigen::Affine3f w2c = cam.w2c().cast<float>();
  std::printf("W2C");
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) std::printf(" %.9g", w2c.linear()(i, j));
    std::printf(" %.9g", w2c.translation()[i]);
  }
  std::printf("\n");
  // VoxelGrid::Init on the bunny bounding box (examples.cc:91-99) at resolution 10: dims and an FNV-1a-64
  // hash of the voxel centres in id order (res10_pos)
  {
    Eigen::Vector3f bb_min(-250.000000f, -344.586151f, -129.982697f), bb_max(250.000000f, 150.542343f, 257.329224f);
    for (int i = 0; i < 3; ++i) {
      bb_min[i] -= 20.0f;
      bb_max[i] += 20.0f;
    }
    vacancy::VoxelGrid grid;
    if (grid.initialized() || !grid.Init(bb_max, bb_min, 10.0f) || !grid.initialized()) return 2;
    const Eigen::Vector3i n = grid.voxel_num();
    unsigned long long h = 1469598103934665603ull;
    bool ok = true;
    int id = 0;
    for (int z = 0; z < n[2]; ++z)
      for (int y = 0; y < n[1]; ++y)
        for (int x = 0; x < n[0]; ++x, ++id) {
          const vacancy::Voxel& v = grid.get(x, y, z);
          ok = ok && v.id == id && v.index[0] == x && v.index[1] == y && v.index[2] == z && v.update_num == 0 &&
               v.sdf == vacancy::InvalidSdf::kVal && !v.on_surface && !v.outside;
          for (int k = 0; k < 3; ++k) {
            const float f = v.pos[k];
            const unsigned char* b = reinterpret_cast<const unsigned char*>(&f);
            for (int q = 0; q < 4; ++q) h = (h ^ b[q]) * 1099511628211ull;
          }
        }
    grid.get_ptr(1, 2, 3)->on_surface = true;
    grid.ResetOnSurface();
    ok = ok && !grid.get(1, 2, 3).on_surface && grid.resolution() == 10.0f;
    vacancy::VoxelGrid bad;
    ok = ok && !bad.Init(bb_min, bb_max, 10.0f) && !bad.Init(bb_max, bb_min, 0.0f);  // inverted box, zero resolution
    // a box thinner than one voxel: the reference returns true with an empty grid (voxel_carver.cc:292-345)
    vacancy::VoxelGrid thin;
    ok = ok && thin.Init(Eigen::Vector3f(100.f, 100.f, 5.f), Eigen::Vector3f(0.f, 0.f, 0.f), 10.0f) &&
         !thin.initialized() && thin.voxel_num()[2] == 0 && thin.voxel_num()[0] == 10;
    std::printf("GRID %d %d %d %016llx %d\n", n[0], n[1], n[2], h, ok ? 1 : 0);
  }
  // the reference's look-at forms (common.h:51-75) against the Affine one
  {
    const Eigen::Vector3d pos(0.3, -1.2, 2.5), target(0.1, 0.2, -0.4), up(0.0, -1.0, 0.0);
    const Eigen::Affine3d pose = vacancy::c2w(pos, target, up);
    Eigen::Matrix3d R;
    vacancy::c2w(pos, target, up, &R);
    Eigen::Matrix4d T;
    vacancy::c2w(pos, target, up, &T);
    bool same = T(3, 0) == 0.0 && T(3, 1) == 0.0 && T(3, 2) == 0.0 && T(3, 3) == 1.0;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) same = same && R(i, j) == pose.linear()(i, j) && T(i, j) == R(i, j);
      same = same && T(i, 3) == pos[i];
    }
    std::printf("C2W %d\n", same ? 1 : 0);
  }
  vacancy::PinholeCamera fov(1280, 720, 60.0f);
  std::printf("FOCAL %.9g %.9g %.9g\n", fov.focal_length()[0], fov.principal_point()[0], fov.principal_point()[1]);
  return 0;
}
