// The reference's demo (examples.cc:75-152) on the MI355X path: 6 masks + TUM poses of data/
// bunny, 10 mm voxels; per view carve -> marching cubes (interpolated and not), PLY out.
// Usage: bunny <data_dir> <out_dir> [resolution] [n_slabs] [planned] [--keep-largest] [--render DIR] [--fuse-depth]
//        bunny <data_dir> <out_dir> [resolution] [n_slabs] --tolerate M [--blank-view I]
//        bunny <data_dir> <out_dir> [resolution] [n_slabs] --smooth N [--lambda L --mu M]
//        bunny <data_dir> <out_dir> [resolution] [n_slabs] --decimate CELLS [--decimate-mode mean|nearest|first|quadric [--quadric-reg R]]
//        bunny <data_dir> <out_dir> [resolution] --smooth N ... --decimate CELLS ... --chain
//        bunny <data_dir> <out_dir> [resolution] [n_slabs] [--smooth N] [--decimate CELLS] [--chain] --mesh-agreement
//        bunny <data_dir> <out_dir> [resolution] [n_slabs] [--smooth N] [--decimate CELLS] [--chain] --shade DIR
//        bunny <data_dir> <out_dir> [resolution] [n_slabs] --redistance R [--offset MM]
//        bunny <data_dir> <out_dir> [resolution] [n_slabs] --close VOXELS
//   n_slabs > 0 additionally runs the same views through ShardedVoxelCarver (that many z-slabs on
//   device 0) and checks that its stitched mesh is identical to the single-context one.
//   --shade DIR (DIR must exist) writes DIR/normal_<view>.png, the normal map (127.5 * n + 127.5) of the FINAL mesh -- as
//   --mesh-agreement takes it -- as every input camera sees it (VoxelCarver::ShadeMesh), and prints `SHADE view i pixels n`,
//   the pixels the mesh covers, and `SHADE verts .. faces .. views .. raster_ms .. shade_ms ..`.
//   --render DIR (DIR must exist) writes DIR/hull_<view>.png, the silhouette of the carved hull as every input camera
//   sees it, and prints per view how it agrees with the input silhouette: the three pixel counts and the IoU.
//   --tolerate M carves the six views with the robust hull instead (VoxelCarver::CarveRobust: a voxel is carved only when
//   more than M views say outside), prints per view how many solid voxels it was overruled on, writes
//   surface_robust.ply and ends; n_slabs does not apply (the sharded carver has the call in Python only).
//   --blank-view I replaces the silhouette of view I by an all-background image first: the wrong mask the call is for.
//   --fuse-depth (after the ordinary carve) renders the hull's depth from every input camera, fuses those images into a second
//   carver of the same box and resolution (weighted average, band = 3 voxels: VoxelCarver::CarveDepth), writes the
//   iso-surface as <out_dir>/depth_fused.ply and prints its size and the device time of the fusion.
//   --smooth N (after the ordinary carve) smooths the final iso-surface with N Taubin iterations on the device
//   (VoxelCarver::SmoothMesh, factors --lambda / --mu, by default the usual pair 0.5 / -0.53) and recomputes its normals
//   before it writes it as <out_dir>/surface_smooth.ply (binary, with normals); with slabs the merged mesh is smoothed
//   through ShardedVoxelCarver::SmoothMesh as well and compared.
//   --decimate CELLS (after the ordinary carve, and after --smooth if both are given) decimates the final iso-surface by
//   vertex clustering on the device (VoxelCarver::DecimateMesh: cells of CELLS * resolution from the box's corner, the
//   cluster's mean, its member nearest to the mean or its first member) and writes it as <out_dir>/surface_decimated.ply
//   (binary, with normals); with slabs the merged mesh goes through ShardedVoxelCarver::DecimateMesh as well and is compared.
//   --decimate-mode quadric puts every cluster at its quadric-error representative instead (VoxelCarver::DecimateMeshQuadric,
//   regularisation --quadric-reg R in [0, 1], by default 0.001) and prints how many output vertices kept the mean.
//   --chain (with --smooth and / or --decimate, single carver) runs extraction, smoothing and decimation as ONE call
//   (VoxelCarver::ExtractIsoSurfaceChain: the mesh stays on the device between the stages) and again as the separate calls,
//   prints the chain's sizes and timings with `identical 1` when the two agree bit for bit, and writes the chain's mesh as
//   <out_dir>/surface_chain.ply.
//   --mesh-agreement (after the ordinary carve) rasterises the FINAL mesh -- the iso-surface after --smooth / --decimate, or
//   the one --chain returned -- into every input camera on the device (VoxelCarver::MeshAgreement) and prints per view
//   `MESH_AGREEMENT view i both mask_only mesh_only`, the pixel counts against the input silhouette, with the hull's own
//   `HULL_AGREEMENT view i both mask_only hull_only` (VoxelCarver::HullAgreement) beside it: what smoothing and decimation
//   cost in reprojection.  With slabs the merged mesh goes through ShardedVoxelCarver::MeshAgreement as well and is compared.
//   --redistance R (after the ordinary carve and --keep-largest) rewrites the state as the metric distance field of the hull
//   (VoxelCarver::Redistance, exact up to R voxels), extracts the iso-surface at --offset MM (world units, by default 0:
//   the hull itself; positive grows it, negative shrinks it; |MM| < (R - 0.5) * resolution), writes it as
//   <out_dir>/surface_offset.ply and prints its size.
//   --close VOXELS (in the same place, before --redistance if both are given) closes the hull by a ball of VOXELS voxels
//   (VoxelCarver::CloseHull: 1.3, 2.3, ... -- not 1.5, 2.5, on which the closing ties) and prints the solid voxels before
//   and after; the later extractions are those of the closed hull.
//   With n_slabs > 0 both run through the sharded carver as well (CloseHullSlabs, RedistanceSlabs) and its stitched mesh is
//   compared with the single context's: one more line each, SLAB_CLOSE ... / SLAB_REDISTANCE ..., ending in "identical 1".
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "vacancy/sharded_voxel_carver.h"
#include "vacancy/voxel_carver.h"

// TUM trajectory line: id tx ty tz qx qy qz qw -> pose = Translation * Quaternion (examples.cc:36-50)
static bool LoadTumPoses(const std::string& path, std::vector<Eigen::Affine3d>* poses) {
  std::ifstream in(path);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::vector<std::string> tok;
    for (std::string t; std::getline(ss, t, ' ');) tok.push_back(t);
    if (tok.size() != 8) {
      vacancy::LOGE("wrong tum format\n");
      return false;
    }
    Eigen::Translation3d t;
    t.x() = std::atof(tok[1].c_str());
    t.y() = std::atof(tok[2].c_str());
    t.z() = std::atof(tok[3].c_str());
    Eigen::Quaterniond q;
    q.x() = std::atof(tok[4].c_str());
    q.y() = std::atof(tok[5].c_str());
    q.z() = std::atof(tok[6].c_str());
    q.w() = std::atof(tok[7].c_str());
    poses->push_back(t * q);
  }
  return !poses->empty();
}

int main(int argc, char* argv[]) {
  // --keep-largest (anywhere on the command line): before the final extraction, carve away every connected component
  // of the hull but the largest (VoxelCarver::KeepLargestComponents) -- the floaters six views leave; with slabs, the
  // sharded run is filtered too (ShardedVoxelCarver::KeepLargestComponents) and its kept mesh compared
  bool keep_largest = false;
  bool fuse_depth = false;  // --fuse-depth: the hull's rendered depth images fused into a second carver
  int tolerate = -1;       // --tolerate M: the robust hull instead of the per-view demo
  int blank_view = -1;     // --blank-view I: that view's silhouette becomes all background
  int smooth = -1;         // --smooth N: Taubin iterations over the final iso-surface before it is written
  float smooth_lambda = 0.5f, smooth_mu = -0.53f;  // --lambda L, --mu M
  float decimate = 0.0f;   // --decimate CELLS: vertex clustering over cells of CELLS voxels before the surface is written
  int decimate_mode = 0;   // --decimate-mode mean|nearest|first|quadric (3: VoxelCarver::DecimateMeshQuadric)
  float quadric_reg = 1e-3f;  // --quadric-reg R
  bool quadric_reg_given = false;
  bool chain = false;      // --chain: extraction, --smooth and --decimate in one call, against the separate calls
  int redistance = 0;      // --redistance R: the state becomes the metric distance field of the hull, exact up to R voxels
  float offset_mm = 0.0f;  // --offset MM: the iso level of the surface extracted from it
  float close_voxels = 0.0f;  // --close VOXELS: morphological closing of the hull first
  bool mesh_agreement = false;  // --mesh-agreement: the final mesh rasterised into the input views, against their silhouettes
  std::string shade_dir;   // --shade DIR: the final mesh's normal map as every input camera sees it, as PNG
  std::string render_dir;  // --render DIR: the hull's silhouette of every input view as PNG, and how it agrees with the input
  {
    int n = 1;
    for (int i = 1; i < argc; ++i) {
      if (std::string(argv[i]) == "--keep-largest") keep_largest = true;
      else if (std::string(argv[i]) == "--chain") chain = true;
      else if (std::string(argv[i]) == "--mesh-agreement") mesh_agreement = true;
      else if (std::string(argv[i]) == "--fuse-depth") fuse_depth = true;
      else if (std::string(argv[i]) == "--shade") {
        if (i + 1 >= argc) {
          std::fprintf(stderr, "--shade needs a directory\n");
          return 1;
        }
        shade_dir = argv[++i];
      } else if (std::string(argv[i]) == "--render") {
        if (i + 1 >= argc) {
          std::fprintf(stderr, "--render needs a directory\n");
          return 10;
        }
        render_dir = argv[++i];
      } else if (std::string(argv[i]) == "--tolerate" || std::string(argv[i]) == "--blank-view") {
        if (i + 1 >= argc) {
          std::fprintf(stderr, "%s needs a number\n", argv[i]);
          return 10;
        }
        (std::string(argv[i]) == "--tolerate" ? tolerate : blank_view) = std::atoi(argv[i + 1]);
        ++i;
      } else if (std::string(argv[i]) == "--smooth" || std::string(argv[i]) == "--lambda" || std::string(argv[i]) == "--mu") {
        if (i + 1 >= argc) {
          std::fprintf(stderr, "%s needs a number\n", argv[i]);
          return 10;
        }
        if (std::string(argv[i]) == "--smooth") smooth = std::atoi(argv[i + 1]);
        else (std::string(argv[i]) == "--lambda" ? smooth_lambda : smooth_mu) = (float)std::atof(argv[i + 1]);
        ++i;
      } else if (std::string(argv[i]) == "--redistance" || std::string(argv[i]) == "--offset" || std::string(argv[i]) == "--close") {
        if (i + 1 >= argc) {
          std::fprintf(stderr, "%s needs a number\n", argv[i]);
          return 10;
        }
        if (std::string(argv[i]) == "--redistance") redistance = std::atoi(argv[i + 1]);
        else (std::string(argv[i]) == "--offset" ? offset_mm : close_voxels) = (float)std::atof(argv[i + 1]);
        if ((std::string(argv[i]) == "--redistance" && (redistance < 1 || redistance > 127)) ||
            (std::string(argv[i]) == "--close" && !(close_voxels > 0.0f))) {
          std::fprintf(stderr, "%s needs %s\n", argv[i], std::string(argv[i]) == "--close" ? "a positive number" : "a radius in [1, 127]");
          return 10;
        }
        ++i;
      } else if (std::string(argv[i]) == "--decimate") {
        if (i + 1 >= argc) {
          std::fprintf(stderr, "%s needs a number\n", argv[i]);
          return 10;
        }
        decimate = (float)std::atof(argv[i + 1]);
        if (!(decimate > 0.0f)) {
          std::fprintf(stderr, "%s needs a positive number\n", argv[i]);
          return 10;
        }
        ++i;
      } else if (std::string(argv[i]) == "--decimate-mode") {
        const std::string m = i + 1 < argc ? argv[i + 1] : "";
        if (m != "mean" && m != "nearest" && m != "first" && m != "quadric") {
          std::fprintf(stderr, "%s needs mean, nearest, first or quadric\n", argv[i]);
          return 10;
        }
        decimate_mode = m == "mean" ? 0 : m == "nearest" ? 1 : m == "first" ? 2 : 3;
        ++i;
      } else if (std::string(argv[i]) == "--quadric-reg") {
        quadric_reg = i + 1 < argc ? (float)std::atof(argv[i + 1]) : -1.0f;
        if (!(quadric_reg >= 0.0f && quadric_reg <= 1.0f)) {
          std::fprintf(stderr, "%s needs a number in [0, 1]\n", argv[i]);
          return 10;
        }
        quadric_reg_given = true;
        ++i;
      } else argv[n++] = argv[i];
    }
    argc = n;
    if (chain && smooth < 0 && !(decimate > 0.0f)) {
      std::fprintf(stderr, "--chain goes with --smooth and / or --decimate\n");
      return 10;
    }
    if (quadric_reg_given && decimate_mode != 3) {
      std::fprintf(stderr, "--quadric-reg goes with --decimate-mode quadric\n");
      return 10;
    }
  }
  const std::string data_dir = argc > 1 ? argv[1] : "../data/";
  const std::string out_dir = argc > 2 ? argv[2] : data_dir;
  const float resolution = argc > 3 ? (float)std::atof(argv[3]) : 10.0f;
  const int n_slabs = argc > 4 ? std::atoi(argv[4]) : 0;
  const bool planned = argc > 5 && std::string(argv[5]) == "planned";
  std::vector<Eigen::Affine3d> poses;
  if (!LoadTumPoses(data_dir + "/tumpose.txt", &poses)) return 1;

  vacancy::VoxelCarverOption option;
  option.bb_min = Eigen::Vector3f(-250.000000f, -344.586151f, -129.982697f);
  option.bb_max = Eigen::Vector3f(250.000000f, 150.542343f, 257.329224f);
  const float bb_offset = 20.0f;  // keep the boundary clean
  for (int i = 0; i < 3; ++i) {
    option.bb_min[i] -= bb_offset;
    option.bb_max[i] += bb_offset;
  }
  option.resolution = resolution;
  vacancy::VoxelCarver carver(option);
  if (!carver.Init()) return 2;

  if (tolerate >= 0) {  // the robust hull of the six views in one call, and who was overruled where
    std::vector<std::shared_ptr<vacancy::Camera>> cams;
    std::vector<vacancy::Image1b> sils(poses.size() < 6 ? poses.size() : 6);
    for (size_t i = 0; i < sils.size(); ++i) {
      cams.push_back(std::make_shared<vacancy::PinholeCamera>(320, 240, poses[i], Eigen::Vector2f(159.3f, 127.65f),
                                                              Eigen::Vector2f(258.65f, 258.25f)));
      if (!sils[i].Load(data_dir + "/mask_" + vacancy::zfill(i) + ".png")) return 3;
      if (static_cast<int>(i) == blank_view) {
        const int w = sils[i].width(), h = sils[i].height();
        sils[i].Init(w, h, static_cast<unsigned char>(0));
      }
    }
    std::vector<std::int64_t> overruled;
    if (!carver.CarveRobust(cams, sils, tolerate, &overruled)) return 13;
    for (size_t i = 0; i < overruled.size(); ++i)
      std::printf("ROBUST view %zu overruled %lld\n", i, static_cast<long long>(overruled[i]));
    vacancy::Mesh mesh;
    carver.ExtractIsoSurface(&mesh, 0.0);
    mesh.WritePly(out_dir + "/surface_robust.ply");
    std::printf("ROBUST tolerate %d verts %zu faces %zu\n", tolerate, mesh.vertices().size(), mesh.vertex_indices().size());
    return 0;
  }

  std::unique_ptr<vacancy::ShardedVoxelCarver> sharded;
  if (n_slabs > 0) {
    sharded.reset(new vacancy::ShardedVoxelCarver(option, {0}, n_slabs));
    if (planned) {  // cuts of equal predicted cost for the six views about to be carved (vcy_plan_z_slabs)
      std::vector<std::shared_ptr<vacancy::PinholeCamera>> cams;
      std::vector<const vacancy::Camera*> cam_ptrs;
      std::vector<vacancy::Image1b> sils(poses.size() < 6 ? poses.size() : 6);
      for (size_t i = 0; i < sils.size(); ++i) {
        cams.push_back(std::make_shared<vacancy::PinholeCamera>(320, 240, poses[i], Eigen::Vector2f(159.3f, 127.65f),
                                                                Eigen::Vector2f(258.65f, 258.25f)));
        cam_ptrs.push_back(cams.back().get());
        if (!sils[i].Load(data_dir + "/mask_" + vacancy::zfill(i) + ".png")) return 3;
      }
      if (!sharded->PlanPartition(cam_ptrs, sils)) return 8;
    }
    if (!sharded->Init()) return 5;
    std::printf("BOUNDS");
    for (int z : sharded->z_bounds()) std::printf(" %d", z);
    std::printf("\n");
  }

  const int width = 320, height = 240;
  std::shared_ptr<vacancy::Camera> camera = std::make_shared<vacancy::PinholeCamera>(
      width, height, Eigen::Affine3d::Identity(), Eigen::Vector2f(159.3f, 127.65f), Eigen::Vector2f(258.65f, 258.25f));

  for (size_t i = 0; i < 6 && i < poses.size(); ++i) {
    camera->set_c2w(poses[i]);
    const std::string num = vacancy::zfill(i);
    vacancy::Image1b silhouette;
    if (!silhouette.Load(data_dir + "/mask_" + num + ".png")) return 3;
    vacancy::Image1f sdf;
    if (!carver.Carve(*camera, silhouette, &sdf)) return 4;
    vacancy::Image3b vis;
    vacancy::SignedDistance2Color(sdf, &vis, -1.0f, 1.0f);
    vis.WritePng(out_dir + "/sdf_" + num + ".png");

    if (sharded && !sharded->Carve(*camera, silhouette)) return 6;

    vacancy::Mesh mesh;
    carver.ExtractVoxel(&mesh);  // cube per voxel: large and slow to write, like the reference says
    mesh.WritePlyBinary(out_dir + "/voxel_" + num + ".ply");
    const size_t voxel_verts = mesh.vertices().size();
    if (sharded) {  // ExtractVoxel over the slabs (both predicates) == the single context's, array for array
      bool same = true;
      for (int pass = 0; pass < 2 && same; ++pass) {
        vacancy::Mesh a, b;
        sharded->ExtractVoxel(&a, pass == 1);
        carver.ExtractVoxel(&b, pass == 1);
        same = a.vertices().size() == b.vertices().size() && a.vertex_indices().size() == b.vertex_indices().size() &&
               (pass == 1 || b.vertices().size() == voxel_verts);
        for (size_t k = 0; same && k < a.vertices().size(); ++k)
          for (int q = 0; q < 3; ++q) same = same && a.vertices()[k][q] == b.vertices()[k][q];
        for (size_t k = 0; same && k < a.vertex_indices().size(); ++k)
          for (int q = 0; q < 3; ++q) same = same && a.vertex_indices()[k][q] == b.vertex_indices()[k][q];
      }
      std::printf("VOXELSHARDED view %zu identical %d\n", i, same ? 1 : 0);
    }
    carver.ExtractIsoSurface(&mesh, 0.0);
    mesh.WritePly(out_dir + "/surface_" + num + ".ply");
    const size_t nv = mesh.vertices().size(), nf = mesh.vertex_indices().size();
    double sum[3] = {0, 0, 0};
    for (const auto& v : mesh.vertices())
      for (int k = 0; k < 3; ++k) sum[k] += v[k];
    if (sharded) {
      vacancy::Mesh sm;
      sharded->ExtractIsoSurface(&sm, 0.0);
      bool same = sm.vertices().size() == mesh.vertices().size() &&
                  sm.vertex_indices().size() == mesh.vertex_indices().size();
      for (size_t k = 0; same && k < sm.vertices().size(); ++k)
        for (int a = 0; a < 3; ++a) same = same && sm.vertices()[k][a] == mesh.vertices()[k][a];
      for (size_t k = 0; same && k < sm.vertex_indices().size(); ++k)
        for (int a = 0; a < 3; ++a) same = same && sm.vertex_indices()[k][a] == mesh.vertex_indices()[k][a];
      std::printf("SHARDED view %zu slabs %d identical %d\n", i, sharded->slab_count(), same ? 1 : 0);
    }
    carver.ExtractIsoSurface(&mesh, 0.0, false);
    mesh.WritePly(out_dir + "/surface_nointerp_" + num + ".ply");
    std::printf("RESULT view %zu verts %zu faces %zu nointerp_verts %zu nointerp_faces %zu vsum %.6f %.6f %.6f "
                "voxel_verts %zu\n",
                i, nv, nf, mesh.vertices().size(), mesh.vertex_indices().size(), sum[0], sum[1], sum[2], voxel_verts);
  }

  if (fuse_depth) {  // the hull's own depth images, fused as a sensor's would be (vcy_render_hull -> vcy_carve_depth)
    std::vector<std::shared_ptr<vacancy::Camera>> cams;
    std::vector<vacancy::Image1f> depths(poses.size() < 6 ? poses.size() : 6);
    for (size_t i = 0; i < depths.size(); ++i) {
      cams.push_back(std::make_shared<vacancy::PinholeCamera>(width, height, poses[i], Eigen::Vector2f(159.3f, 127.65f),
                                                              Eigen::Vector2f(258.65f, 258.25f)));
      if (!carver.RenderHull(*cams.back(), &depths[i])) return 14;
    }
    vacancy::VoxelCarverOption fused_option = option;
    fused_option.update_option.voxel_update = vacancy::VoxelUpdate::kWeightedAverage;
    vacancy::VoxelCarver fused(fused_option);
    if (!fused.Init() || !fused.CarveDepth(cams, depths, 3.0f * resolution)) return 14;
    vacancy::Mesh mesh;
    fused.ExtractIsoSurface(&mesh, 0.0);
    mesh.WritePly(out_dir + "/depth_fused.ply");
    std::printf("DEPTH fused verts %zu faces %zu device_ms %.4f\n", mesh.vertices().size(), mesh.vertex_indices().size(),
                fused.last_depth_ms());
  }

  if (smooth >= 0) {  // the final surface, smoothed on the device, with the normals of the smoothed positions
    vacancy::Mesh mesh;
    carver.ExtractIsoSurface(&mesh, 0.0);
    const vacancy::Mesh raw = mesh;
    if (!carver.SmoothMesh(&mesh, smooth, smooth_lambda, smooth_mu, false, true)) return 15;
    mesh.WritePlyBinary(out_dir + "/surface_smooth.ply");
    const std::array<float, 3> ms = carver.last_smooth_ms();
    std::printf("SMOOTH iterations %d lambda %g mu %g verts %zu faces %zu build_ms %.4f passes_ms %.4f normals_ms %.4f\n", smooth,
                smooth_lambda, smooth_mu, mesh.vertices().size(), mesh.vertex_indices().size(), ms[0], ms[1], ms[2]);
    if (sharded) {  // the merged mesh through the first slab's context, and Mesh::Smooth on the host: the same bits
      vacancy::Mesh sm, hm = raw;
      sharded->ExtractIsoSurface(&sm, 0.0);
      if (!sharded->SmoothMesh(&sm, smooth, smooth_lambda, smooth_mu, false, true) || !hm.Smooth(smooth, smooth_lambda, smooth_mu)) return 15;
      bool same = sm.vertices().size() == mesh.vertices().size() && sm.normals().size() == mesh.normals().size() &&
                  hm.vertices().size() == mesh.vertices().size();
      for (size_t k = 0; same && k < sm.vertices().size(); ++k)
        same = std::memcmp(&sm.vertices()[k], &mesh.vertices()[k], 12) == 0 && std::memcmp(&hm.vertices()[k], &mesh.vertices()[k], 12) == 0 &&
               std::memcmp(&sm.normals()[k], &mesh.normals()[k], 12) == 0;
      std::printf("SMOOTHSHARDED slabs %d verts %zu identical %d\n", sharded->slab_count(), sm.vertices().size(), same ? 1 : 0);
    }
  }

  if (decimate > 0.0f) {  // the final surface (smoothed first if asked for), clustered on the device, with fresh normals
    const char* mode_names[4] = {"mean", "nearest", "first", "quadric"};
    const bool quadric = decimate_mode == 3;
    std::int64_t n_fallback = 0;
    const float cell = decimate * resolution;
    vacancy::Mesh mesh;
    carver.ExtractIsoSurface(&mesh, 0.0);
    if (smooth >= 0 && !carver.SmoothMesh(&mesh, smooth, smooth_lambda, smooth_mu, false, false)) return 16;
    const vacancy::Mesh before = mesh;
    if (!(quadric ? carver.DecimateMeshQuadric(&mesh, cell, quadric_reg, true, &n_fallback) : carver.DecimateMesh(&mesh, cell, decimate_mode, true)))
      return 16;
    mesh.WritePlyBinary(out_dir + "/surface_decimated.ply");
    const std::array<float, 4> ms = carver.last_decimate_ms();
    std::printf("DECIMATE cell %g mode %s vertices %zu -> %zu faces %zu -> %zu", cell, mode_names[decimate_mode], before.vertices().size(),
                mesh.vertices().size(), before.vertex_indices().size(), mesh.vertex_indices().size());
    if (quadric) std::printf(" fallback %lld regularize %g quadric_ms %.4f", (long long)n_fallback, quadric_reg, carver.last_quadric_ms());
    std::printf(" cluster_ms %.4f faces_ms %.4f emit_ms %.4f normals_ms %.4f\n", ms[0], ms[1], ms[2], ms[3]);
    if (sharded) {  // the merged mesh through the first slab's context: the same bits
      vacancy::Mesh sm;
      sharded->ExtractIsoSurface(&sm, 0.0);
      if (smooth >= 0 && !sharded->SmoothMesh(&sm, smooth, smooth_lambda, smooth_mu, false, false)) return 16;
      if (!(quadric ? sharded->DecimateMeshQuadric(&sm, cell, quadric_reg, true) : sharded->DecimateMesh(&sm, cell, decimate_mode, true)))
        return 16;
      bool same = sm.vertices().size() == mesh.vertices().size() && sm.normals().size() == mesh.normals().size() &&
                  sm.vertex_indices().size() == mesh.vertex_indices().size();
      for (size_t k = 0; same && k < sm.vertices().size(); ++k)
        same = std::memcmp(&sm.vertices()[k], &mesh.vertices()[k], 12) == 0 && std::memcmp(&sm.normals()[k], &mesh.normals()[k], 12) == 0;
      for (size_t k = 0; same && k < sm.vertex_indices().size(); ++k)
        same = std::memcmp(&sm.vertex_indices()[k], &mesh.vertex_indices()[k], 12) == 0;
      std::printf("DECIMATESHARDED slabs %d verts %zu identical %d\n", sharded->slab_count(), sm.vertices().size(), same ? 1 : 0);
    }
  }

  vacancy::Mesh chain_mesh;  // (--chain's result, for --mesh-agreement)
  if (chain) {  // extraction, smoothing and decimation in ONE call, the mesh staying on the device, against the calls above
    const bool quadric = decimate_mode == 3;
    vacancy::ChainOption co;
    co.smooth = smooth >= 0;
    co.iterations = smooth >= 0 ? smooth : 0;
    co.lambda = smooth_lambda;
    co.mu = smooth_mu;
    co.decimate = decimate > 0.0f ? (quadric ? 2 : 1) : 0;
    co.cell = decimate * resolution;
    co.mode = quadric ? 0 : decimate_mode;
    co.regularize = quadric_reg;
    vacancy::Mesh got, want;
    vacancy::ChainReport report;
    if (!carver.ExtractIsoSurfaceChain(&got, co, &report)) return 19;
    const std::array<float, 8> ms = carver.last_chain_ms();
    std::int64_t n_fallback = 0;
    carver.ExtractIsoSurface(&want, 0.0);
    if (smooth >= 0 && !carver.SmoothMesh(&want, smooth, smooth_lambda, smooth_mu, false, co.decimate == 0)) return 19;
    if (co.decimate != 0 && !(quadric ? carver.DecimateMeshQuadric(&want, co.cell, quadric_reg, true, &n_fallback)
                                      : carver.DecimateMesh(&want, co.cell, decimate_mode, true)))
      return 19;
    bool same = got.vertices().size() == want.vertices().size() && got.vertex_indices().size() == want.vertex_indices().size() &&
                got.normals().size() == want.normals().size() && got.face_normals().size() == want.face_normals().size() &&
                report.n_fallback == n_fallback;
    for (size_t k = 0; same && k < got.vertices().size(); ++k)
      same = std::memcmp(&got.vertices()[k], &want.vertices()[k], 12) == 0 && std::memcmp(&got.normals()[k], &want.normals()[k], 12) == 0;
    for (size_t k = 0; same && k < got.vertex_indices().size(); ++k)
      same = std::memcmp(&got.vertex_indices()[k], &want.vertex_indices()[k], 12) == 0 &&
             std::memcmp(&got.face_normals()[k], &want.face_normals()[k], 12) == 0;
    got.WritePlyBinary(out_dir + "/surface_chain.ply");
    chain_mesh = got;
    std::printf("CHAIN smooth %d decimate %d extracted %lld %lld verts %zu faces %zu fallback %lld extract_ms %.4f table_ms %.4f "
                "passes_ms %.4f cluster_ms %.4f quadric_ms %.4f faces_emit_ms %.4f normals_ms %.4f wall_ms %.4f identical %d\n",
                smooth, co.decimate, (long long)report.n_extracted_vertices, (long long)report.n_extracted_faces, got.vertices().size(),
                got.vertex_indices().size(), (long long)report.n_fallback, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6], ms[7],
                same ? 1 : 0);
  }

  if (mesh_agreement) {  // how the final mesh reprojects onto the input silhouettes, beside the hull itself
    const bool quadric = decimate_mode == 3;
    vacancy::Mesh mesh;
    if (chain) {
      mesh = chain_mesh;
    } else {
      carver.ExtractIsoSurface(&mesh, 0.0);
      if (smooth >= 0 && !carver.SmoothMesh(&mesh, smooth, smooth_lambda, smooth_mu, false, false)) return 20;
      if (decimate > 0.0f && !(quadric ? carver.DecimateMeshQuadric(&mesh, decimate * resolution, quadric_reg, false)
                                        : carver.DecimateMesh(&mesh, decimate * resolution, decimate_mode, false)))
        return 20;
    }
    std::vector<std::shared_ptr<vacancy::PinholeCamera>> cams;
    std::vector<const vacancy::Camera*> cam_ptrs;
    std::vector<vacancy::Image1b> sils(poses.size() < 6 ? poses.size() : 6);
    for (size_t i = 0; i < sils.size(); ++i) {
      cams.push_back(std::make_shared<vacancy::PinholeCamera>(width, height, poses[i], Eigen::Vector2f(159.3f, 127.65f),
                                                              Eigen::Vector2f(258.65f, 258.25f)));
      cam_ptrs.push_back(cams.back().get());
      if (!sils[i].Load(data_dir + "/mask_" + vacancy::zfill(i) + ".png")) return 3;
    }
    std::vector<std::array<std::int64_t, 3>> counts, hull_counts;
    if (!carver.MeshAgreement(mesh, cam_ptrs, sils, &counts) || !carver.HullAgreement(cam_ptrs, sils, &hull_counts)) return 20;
    for (size_t i = 0; i < counts.size(); ++i) {
      std::printf("MESH_AGREEMENT view %zu %lld %lld %lld\n", i, (long long)counts[i][0], (long long)counts[i][1], (long long)counts[i][2]);
      std::printf("HULL_AGREEMENT view %zu %lld %lld %lld\n", i, (long long)hull_counts[i][0], (long long)hull_counts[i][1],
                  (long long)hull_counts[i][2]);
    }
    const std::array<float, 2> ms = carver.last_raster_ms();
    std::printf("MESH_AGREEMENT verts %zu faces %zu views %zu raster_ms %.4f resolve_ms %.4f\n", mesh.vertices().size(),
                mesh.vertex_indices().size(), counts.size(), ms[0], ms[1]);
    if (sharded) {  // the same mesh through the first slab's context: the same counts
      std::vector<std::array<std::int64_t, 3>> scounts;
      if (!sharded->MeshAgreement(mesh, cam_ptrs, sils, &scounts)) return 20;
      std::printf("MESH_AGREEMENTSHARDED slabs %d identical %d\n", sharded->slab_count(), scounts == counts ? 1 : 0);
      if (scounts != counts) return 21;
    }
  }

  if (!shade_dir.empty()) {  // the final mesh's normal map from every input camera (vcy_shade_mesh)
    const bool quadric = decimate_mode == 3;
    vacancy::Mesh mesh;
    if (chain) {
      mesh = chain_mesh;
    } else {
      carver.ExtractIsoSurface(&mesh, 0.0);
      if (smooth >= 0 && !carver.SmoothMesh(&mesh, smooth, smooth_lambda, smooth_mu, false, !(decimate > 0.0f))) return 22;
      if (decimate > 0.0f && !(quadric ? carver.DecimateMeshQuadric(&mesh, decimate * resolution, quadric_reg, true)
                                        : carver.DecimateMesh(&mesh, decimate * resolution, decimate_mode, true)))
        return 22;
    }
    if (mesh.normals().size() != mesh.vertices().size()) mesh.CalcNormal();
    float raster_ms = 0.0f, shade_ms = 0.0f;
    const size_t n_shade = poses.size() < 6 ? poses.size() : 6;
    for (size_t i = 0; i < n_shade; ++i) {
      const vacancy::PinholeCamera cam(width, height, poses[i], Eigen::Vector2f(159.3f, 127.65f), Eigen::Vector2f(258.65f, 258.25f));
      vacancy::Image3b image;
      if (!carver.ShadeMesh(mesh, cam, &image, true)) return 22;
      raster_ms += carver.last_shade_ms()[0], shade_ms += carver.last_shade_ms()[1];
      long long n_px = 0;
      for (int y = 0; y < image.height(); ++y)
        for (int x = 0; x < image.width(); ++x) n_px += image.at(x, y, 0) != 0 || image.at(x, y, 1) != 0 || image.at(x, y, 2) != 0;
      const std::string png = shade_dir + "/normal_" + vacancy::zfill(i) + ".png";
      if (!image.WritePng(png)) {
        std::fprintf(stderr, "cannot write %s (--shade does not create its directory)\n", png.c_str());
        return 22;
      }
      std::printf("SHADE view %zu pixels %lld\n", i, n_px);
      if (sharded) {  // the same mesh through the first slab's context: the same bytes
        vacancy::Image3b again;
        if (!sharded->ShadeMesh(mesh, cam, &again, true)) return 22;
        if (again.data() != image.data()) return 23;
      }
    }
    std::printf("SHADE verts %zu faces %zu views %zu raster_ms %.4f shade_ms %.4f\n", mesh.vertices().size(),
                mesh.vertex_indices().size(), n_shade, raster_ms, shade_ms);
    if (sharded) std::printf("SHADESHARDED slabs %d identical 1\n", sharded->slab_count());
  }

  if (!render_dir.empty()) {  // what the hull looks like from every input camera (vcy_render_hull / vcy_hull_agreement)
    std::vector<std::shared_ptr<vacancy::PinholeCamera>> cams;
    std::vector<const vacancy::Camera*> cam_ptrs;
    std::vector<vacancy::Image1b> sils(poses.size() < 6 ? poses.size() : 6);
    for (size_t i = 0; i < sils.size(); ++i) {
      cams.push_back(std::make_shared<vacancy::PinholeCamera>(width, height, poses[i], Eigen::Vector2f(159.3f, 127.65f),
                                                              Eigen::Vector2f(258.65f, 258.25f)));
      cam_ptrs.push_back(cams.back().get());
      if (!sils[i].Load(data_dir + "/mask_" + vacancy::zfill(i) + ".png")) return 3;
      vacancy::Image1f depth;
      vacancy::Image1b hull;
      if (!carver.RenderHull(*cams.back(), &depth, &hull)) return 11;
      const std::string png = render_dir + "/hull_" + vacancy::zfill(i) + ".png";
      if (!hull.WritePng(png)) {
        std::fprintf(stderr, "cannot write %s (--render does not create its directory)\n", png.c_str());
        return 11;
      }
    }
    std::vector<std::array<std::int64_t, 3>> counts;
    if (!carver.HullAgreement(cam_ptrs, sils, &counts)) return 11;
    for (size_t i = 0; i < counts.size(); ++i) {
      const long long both = counts[i][0], only_mask = counts[i][1], only_hull = counts[i][2];
      const long long uni = both + only_mask + only_hull;
      std::printf("RENDER view %zu mask&hull %lld mask-only %lld hull-only %lld IoU %.4f\n", i, both, only_mask, only_hull,
                  uni ? static_cast<double>(both) / static_cast<double>(uni) : 1.0);
    }
    if (sharded) {  // the same through the slabs: every slab renders its own slices, the host merges (RenderHullSlabs)
      bool same = true;
      for (size_t i = 0; i < cams.size(); ++i) {
        vacancy::Image1f one, merged;
        if (!carver.RenderHull(*cams[i], &one) || !sharded->RenderHullSlabs(*cams[i], &merged)) return 11;
        same = same && one.data().size() == merged.data().size() &&
               std::memcmp(one.data().data(), merged.data().data(), sizeof(float) * one.data().size()) == 0;
      }
      std::vector<std::array<std::int64_t, 3>> scounts;
      if (!sharded->HullAgreementSlabs(cam_ptrs, sils, &scounts)) return 11;
      same = same && scounts == counts;
      std::printf("RENDERSHARDED slabs %d views %zu depth and counts identical %d\n", sharded->slab_count(), cams.size(), same ? 1 : 0);
      if (!same) return 12;
    }
  }

  // the last view once more with normals (computed on the device), as a binary PLY a viewer lights correctly
  if (keep_largest) {
    std::vector<vacancy::VoxelComponent> before, after;
    if (!carver.LabelComponents(&before) || !carver.KeepLargestComponents(1) || !carver.LabelComponents(&after)) return 9;
    std::printf("COMPONENTS before %zu after %zu largest %lld voxels\n", before.size(), after.size(),
                before.empty() ? 0LL : static_cast<long long>(before[0].n_voxels));
    if (sharded) {  // the same filter over the slabs: the same lists, and the kept mesh equals the single carver's
      std::vector<vacancy::VoxelComponent> sbefore, safter;
      if (!sharded->LabelComponents(&sbefore) || !sharded->KeepLargestComponents(1) || !sharded->LabelComponents(&safter)) return 9;
      vacancy::Mesh kept, skept;
      carver.ExtractIsoSurface(&kept, 0.0);
      sharded->ExtractIsoSurface(&skept, 0.0);
      bool same = sbefore.size() == before.size() && safter.size() == after.size() &&
                  skept.vertices().size() == kept.vertices().size() && skept.vertex_indices().size() == kept.vertex_indices().size();
      for (size_t k = 0; same && k < sbefore.size(); ++k) same = sbefore[k].label == before[k].label && sbefore[k].n_voxels == before[k].n_voxels;
      for (size_t k = 0; same && k < skept.vertices().size(); ++k)
        for (int a = 0; a < 3; ++a) same = same && skept.vertices()[k][a] == kept.vertices()[k][a];
      for (size_t k = 0; same && k < skept.vertex_indices().size(); ++k)
        for (int a = 0; a < 3; ++a) same = same && skept.vertex_indices()[k][a] == kept.vertex_indices()[k][a];
      std::printf("COMPONENTSSHARDED slabs %d before %zu after %zu kept verts %zu faces %zu single verts %zu faces %zu identical %d\n",
                  sharded->slab_count(), sbefore.size(), safter.size(), skept.vertices().size(), skept.vertex_indices().size(),
                  kept.vertices().size(), kept.vertex_indices().size(), same ? 1 : 0);
    }
  }
  if (close_voxels > 0.0f || redistance > 0) {
    auto count_solid = [&](long long* solid) {
      std::vector<std::int32_t> d2;
      if (!carver.DistanceField(&d2, 0.0, 1)) return false;
      *solid = 0;
      for (std::int32_t v : d2) *solid += v < 0 ? 1 : 0;
      return true;
    };
    // with slabs the sharded carver takes the same steps through its ...Slabs members (the seam planes of the transform go
    // through the host), and its stitched mesh must equal the single context's, vertex for vertex
    auto same_mesh = [](const vacancy::Mesh& a, const vacancy::Mesh& b) {
      bool same = a.vertices().size() == b.vertices().size() && a.vertex_indices().size() == b.vertex_indices().size();
      for (size_t k = 0; same && k < a.vertices().size(); ++k)
        for (int c = 0; c < 3; ++c) same = same && a.vertices()[k][c] == b.vertices()[k][c];
      for (size_t k = 0; same && k < a.vertex_indices().size(); ++k)
        for (int c = 0; c < 3; ++c) same = same && a.vertex_indices()[k][c] == b.vertex_indices()[k][c];
      return same;
    };
    if (close_voxels > 0.0f) {
      long long before = 0, after = 0;
      if (!count_solid(&before) || !carver.CloseHull(close_voxels) || !count_solid(&after)) return 13;
      std::printf("CLOSE voxels %g solid before %lld after %lld\n", static_cast<double>(close_voxels), before, after);
      if (sharded) {
        if (!sharded->CloseHullSlabs(close_voxels)) return 13;
        std::vector<std::int32_t> d2;
        if (!sharded->DistanceFieldSlabs(&d2, 0.0, 1)) return 13;
        long long solid = 0;
        for (std::int32_t v : d2) solid += v < 0 ? 1 : 0;
        vacancy::Mesh closed, sclosed;
        carver.ExtractIsoSurface(&closed, 0.0);
        sharded->ExtractIsoSurface(&sclosed, 0.0);
        const bool same = solid == after && same_mesh(closed, sclosed);
        std::printf("SLAB_CLOSE slabs %d voxels %g solid %lld verts %zu identical %d\n", sharded->slab_count(),
                    static_cast<double>(close_voxels), solid, sclosed.vertices().size(), same ? 1 : 0);
        if (!same) return 14;
      }
    }
    if (redistance > 0) {
      if (std::fabs(offset_mm) >= (static_cast<float>(redistance) - 0.5f) * resolution) {
        std::fprintf(stderr, "--offset %g is beyond the field's cap (%d - 0.5) * %g\n", static_cast<double>(offset_mm), redistance,
                     static_cast<double>(resolution));
        return 10;
      }
      vacancy::Mesh grown;
      if (!carver.Redistance(0.0, redistance)) return 13;
      carver.ExtractIsoSurface(&grown, static_cast<double>(offset_mm));
      grown.WritePly(out_dir + "/surface_offset.ply");
      std::printf("REDISTANCE radius %d offset %g verts %zu faces %zu\n", redistance, static_cast<double>(offset_mm),
                  grown.vertices().size(), grown.vertex_indices().size());
      if (sharded) {
        std::int64_t rewritten = 0;
        vacancy::Mesh sgrown;
        if (!sharded->RedistanceSlabs(0.0, redistance, &rewritten)) return 13;
        sharded->ExtractIsoSurface(&sgrown, static_cast<double>(offset_mm));
        const bool same = same_mesh(grown, sgrown);
        std::printf("SLAB_REDISTANCE slabs %d radius %d offset %g rewritten %lld verts %zu identical %d\n", sharded->slab_count(),
                    redistance, static_cast<double>(offset_mm), static_cast<long long>(rewritten), sgrown.vertices().size(),
                    same ? 1 : 0);
        if (!same) return 14;
      }
    }
  }
  if (!poses.empty()) {
    vacancy::Mesh lit;
    carver.ExtractIsoSurface(&lit, 0.0, true, true);
    const size_t last = std::min<size_t>(6, poses.size()) - 1;
    lit.WritePlyBinary(out_dir + "/surface_normals_" + vacancy::zfill(last) + ".ply");
    std::printf("NORMALS view %zu verts %zu normals %zu face_normals %zu\n", last, lit.vertices().size(), lit.normals().size(),
                lit.face_normals().size());
  }

  // The same six views through the batch overload (cameras held by shared_ptr, as examples.cc does) on a
  // second carver, read back as the reference's VoxelGrid: touched voxels, negative voxels, sum of update_num.
  {
    std::vector<std::shared_ptr<vacancy::Camera>> cameras;
    std::vector<vacancy::Image1b> silhouettes(6);
    for (size_t i = 0; i < 6 && i < poses.size(); ++i) {
      cameras.push_back(std::make_shared<vacancy::PinholeCamera>(width, height, poses[i], Eigen::Vector2f(159.3f, 127.65f),
                                                                 Eigen::Vector2f(258.65f, 258.25f)));
      if (!silhouettes[i].Load(data_dir + "/mask_" + vacancy::zfill(i) + ".png")) return 3;
    }
    silhouettes.resize(cameras.size());
    vacancy::VoxelCarver batch(option);
    vacancy::VoxelGrid grid;
    if (!batch.Init() || !batch.Carve(cameras, silhouettes) || !batch.Download(&grid)) return 7;
    const Eigen::Vector3i n = grid.voxel_num();
    long long touched = 0, negative = 0, updates = 0;
    for (int z = 0; z < n[2]; ++z)
      for (int y = 0; y < n[1]; ++y)
        for (int x = 0; x < n[0]; ++x) {
          const vacancy::Voxel& v = grid.get(x, y, z);
          if (v.update_num < 1) continue;
          ++touched;
          negative += v.sdf < 0 ? 1 : 0;
          updates += v.update_num;
        }
    std::printf("GRID touched %lld negative %lld updates %lld\n", touched, negative, updates);
    // ... and through ShardedVoxelCarver's batch overload: the slabs share ONE producer of SDF images
    // (vcy_carve_batch_silhouettes_sharded) -- same mesh as the single context
    if (n_slabs > 0) {
      vacancy::ShardedVoxelCarver sb(option, {0}, n_slabs);
      std::vector<const vacancy::Camera*> ptrs;
      for (const auto& c : cameras) ptrs.push_back(c.get());
      vacancy::Mesh a, b;
      if (!sb.Init() || !sb.Carve(ptrs, silhouettes)) return 9;
      sb.ExtractIsoSurface(&a, 0.0);
      batch.ExtractIsoSurface(&b, 0.0);
      bool same = a.vertices().size() == b.vertices().size() && a.vertex_indices().size() == b.vertex_indices().size();
      for (size_t k = 0; same && k < a.vertices().size(); ++k)
        for (int q = 0; q < 3; ++q) same = same && a.vertices()[k][q] == b.vertices()[k][q];
      for (size_t k = 0; same && k < a.vertex_indices().size(); ++k)
        for (int q = 0; q < 3; ++q) same = same && a.vertex_indices()[k][q] == b.vertex_indices()[k][q];
      std::printf("BATCHSHARDED slabs %d verts %zu identical %d\n", sb.slab_count(), a.vertices().size(), same ? 1 : 0);
    }
  }
  return 0;
}
