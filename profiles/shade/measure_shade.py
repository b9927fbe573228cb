"""Device time of the shading pass behind the rasteriser (vcy_shade_mesh, three channels, and vcy_mesh_photo_error; 32 views
at 1280 x 720) on the iso-surface of the bunny at resolution 2.5 and of the bench scene at 512^3 and 1024^3 -- the raw
extraction and the chain's output (10 Taubin iterations, quadric decimation at 2 voxels) --, next to vcy_raster_mesh's
resolve launch of the same visit, the whole calls, the single-thread wall time of the host functions and a floor from the
bytes that must move.
Run from the repository root on the GPU:  python profiles/shade/measure_shade.py > profiles/shade/measure_shade.txt
`python profiles/shade/measure_shade.py raster <scenes>` prints only vcy_raster_mesh's own two times (the lines the parent
commit's tree can print as well: parent / branch / parent).
Device figures: median [min..max] of 7 calls after 2 warm-up calls, HIP events around the launches (vcy_last_shade_ms: the
fill of the key images with the raster kernel, and the shade kernel; vcy_last_raster_ms).  "call" is the wall time of the
whole call, the upload of the mesh, attributes, photographs and silhouettes and the download of what is asked for included.
Host: one call, wall time.  Floor of a shade launch: the key image read (8 B per pixel and view), the output written (12 B
float, 3 B uint8), for the error the photograph (3 B) and the silhouette (1 B) read, over the measured device copy rate; the
gathers of the hit pixels (3 indices, 9 coordinates, 9 attributes) are left out of it."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
W, H, NV = 1280, 720, 32
def med(x): x = sorted(x); return "%.3f [%.3f..%.3f]" % (x[len(x)//2], x[0], x[-1])
def scene(name):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5); views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))); masks = B.load_masks()
        s = W / float(B.WIDTH)  # the bunny's cameras at 1280 x 720: intrinsics scaled by 4, rows cropped
        cams = []
        for k in range(NV):
            v = vc.View.from_buffer_copy(views[k % len(views)])
            v.fx, v.fy, v.cx, v.cy = v.fx * s, v.fy * s, v.cx * s, v.cy * s - (B.HEIGHT * s - H) / 2.0
            v.width, v.height = W, H; v.roi_min[0] = v.roi_min[1] = 0; v.roi_max[0], v.roi_max[1] = W - 1, H - 1
            cams.append(v)
    else:
        n = int(name); opt = synth.sphere_option(n); views, masks = synth.sphere_views(n, 16, 640, 480)
        cams, _ = synth.sphere_views(n, NV, W, H)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    assert d.CarveBatchSilhouettes(views, masks), vc.last_error()
    d.sync()
    return d, cams
def timed(call, times):
    """9 calls, the last 7 kept: (result, per device time a list, wall)."""
    dev, wall = ([], []), []
    for rep in range(9):
        t0 = time.perf_counter()
        got = call()
        w_ms = (time.perf_counter() - t0) * 1e3
        if rep >= 2:
            for k, t in enumerate(times()): dev[k].append(t)
            wall.append(w_ms)
    return got, dev, wall
import shutil, subprocess
only_raster = sys.argv[1:2] == ["raster"]
scenes = sys.argv[2:] if only_raster else sys.argv[1:]
info = shutil.which("rocminfo")
names = [l.split(":", 1)[1].strip() for l in subprocess.run([info], capture_output=True, text=True).stdout.splitlines() if "Marketing Name" in l] if info else []
names = [n for n in names if n]
gpus = [n for n in names if "Instinct" in n or "MI3" in n]
print("machine: %s" % ", ".join(gpus or names or ["unknown"]), flush=True)
print(vc.capi.load().vcy_version().decode(), flush=True)
_, copy_gbs = vc.measure_bandwidth(0, 1 << 30, 3)
print("device copy rate %.0f GB/s (vcy_measure_bandwidth, read + write)" % copy_gbs, flush=True)
floor = lambda per_px: NV * W * H * per_px / (copy_gbs * 1e9) * 1e3
for name in (scenes or ("bunny2.5", "512", "1024")):
    d, cams = scene(name)
    print("%s: dims %s, %d views %dx%d" % (name, d.dims, NV, W, H), flush=True)
    raw = d.ExtractIsoSurface(0.0, True)
    res = float(d.option.resolution)
    d.set_param("meshkeys", 0)  # (the chain's mesh has no edge keys)
    chain = d.ExtractIsoChain(0.0, True, dict(iterations=10, lam=0.5, mu=-0.53, pin_boundary=0), dict(cell=2.0 * res, regularize=1e-3))
    for label, m in (("raw extraction", raw), ("chain output", chain)):
        v, f = m["vertices"], m["faces"]
        # what the call replaces: depth and face ids downloaded (and the edge functions redone on the host)
        got, (rs, rv), wall = timed(lambda: d.RenderMesh(v, f, cams, depth=True, face=True), d.last_raster_ms)
        print("  %-14s: %d vertices, %d faces | vcy_raster_mesh (depth + face ids): raster %s ms | resolve %s ms | call %s ms"
              % (label, len(v), len(f), med(rs), med(rv), med(wall)), flush=True)
        if only_raster:
            continue
        hit = sum(int((g["face"] >= 0).sum()) for g in got)
        del got
        rng = np.random.RandomState(1)
        col = rng.uniform(0.0, 255.0, (len(v), 3)).astype(np.float32)
        photos = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(4)]
        photos = [photos[k % 4] for k in range(NV)]
        masks = [(np.indices((H, W))[1] < W // 2 + 16 * (k % 4)).astype(np.uint8) for k in range(4)]
        masks = [masks[k % 4] for k in range(NV)]
        f32, (rs_f, sh_f), wall_f = timed(lambda: d.ShadeMesh(v, f, col, cams, value=True), d.last_shade_ms)
        del f32
        u8, (rs_8, sh_8), wall_8 = timed(lambda: d.ShadeMesh(v, f, col, cams, value=False, value8=True), d.last_shade_ms)
        err, (rs_e, sh_e), wall_e = timed(lambda: d.MeshPhotoError(v, f, col, cams, photos), d.last_shade_ms)
        errm, (rs_m, sh_m), wall_m = timed(lambda: d.MeshPhotoError(v, f, col, cams, photos, masks), d.last_shade_ms)
        t0 = time.perf_counter()
        host8 = vc.shade_mesh_host(v, f, col, cams, value=False, value8=True)
        host8_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        herr = vc.mesh_photo_error_host(v, f, col, cams, photos)
        herr_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(a["value8"], b["value8"]) for a, b in zip(u8, host8)) and np.array_equal(err, herr)
        same = same and np.array_equal(errm, vc.mesh_photo_error_host(v, f, col, cams, photos, masks))
        del u8, host8
        print("    %.1f %% of the pixels hit | raster (shade calls) %s ms" % (100.0 * hit / (NV * W * H), med(rs_f + rs_8 + rs_e + rs_m)), flush=True)
        print("    shade, float out : %s ms, floor %.3f | call %s ms" % (med(sh_f), floor(20), med(wall_f)), flush=True)
        print("    shade, uint8 out : %s ms, floor %.3f | call %s ms | host, 1 thread %.0f ms" % (med(sh_8), floor(11), med(wall_8), host8_ms), flush=True)
        print("    photo error      : %s ms, floor %.3f | call %s ms | host, 1 thread %.0f ms" % (med(sh_e), floor(11), med(wall_e), herr_ms), flush=True)
        print("    ... with masks   : %s ms, floor %.3f | call %s ms" % (med(sh_m), floor(12), med(wall_m)), flush=True)
        print("    device == host %s | MAE of the first view %s" % (same, np.round(vc.photo_error_stats(err)["mae"][0], 2).tolist()), flush=True)
    d.close()
