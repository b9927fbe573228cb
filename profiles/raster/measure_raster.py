"""Device time of vcy_raster_mesh (32 views at 1280 x 720, depth images asked for) on the iso-surface of the bunny at
resolution 2.5 and of the bench scene at 512^3 and 1024^3 -- the raw extraction and the chain's output (10 Taubin
iterations, quadric decimation at 2 voxels) --, next to vcy_render_hull of the same context and views, the single-thread
wall time of vcy_raster_mesh_host on the same input, a floor from the bytes that must move, and the sweep of "rasterwide".
Run from the repository root on the GPU:  python profiles/raster/measure_raster.py > profiles/raster/measure_raster.txt
Device figures: median [min..max] of 7 calls after 2 warm-up calls, HIP events around the launches (vcy_last_raster_ms: the
fill of the key images with the raster kernel, and the resolve kernel; vcy_last_render_ms).  "call" is the wall time of the
whole call, the upload of the mesh and the download of the depth images included.  Host: one call, wall time.  Floor: faces
(12 B) and their three positions (36 B) once per chunk of views, the key image (8 B per pixel and view) written once and
read once, over the measured device copy rate."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
W, H, NV = 1280, 720, 32
SWEEP = (0, 4, 16, 64, 256, 1024, 4096, 1 << 30)
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
def timed(d, v, f, cams, depth=True):
    rs, rv, wall = [], [], []
    for rep in range(9):
        t0 = time.perf_counter()
        got = d.RenderMesh(v, f, cams, depth=depth)
        w_ms = (time.perf_counter() - t0) * 1e3
        if rep >= 2: rs.append(got[0]["raster_ms"]); rv.append(got[0]["resolve_ms"]); wall.append(w_ms)
    return got, rs, rv, wall
import shutil, subprocess
info = shutil.which("rocminfo")
names = [l.split(":", 1)[1].strip() for l in subprocess.run([info], capture_output=True, text=True).stdout.splitlines() if "Marketing Name" in l] if info else []
names = [n for n in names if n]
gpus = [n for n in names if "Instinct" in n or "MI3" in n]
print("machine: %s" % ", ".join(gpus or names or ["unknown"]), flush=True)
print(vc.capi.load().vcy_version().decode(), flush=True)
_, copy_gbs = vc.measure_bandwidth(0, 1 << 30, 3)
print("device copy rate %.0f GB/s (vcy_measure_bandwidth, read + write)" % copy_gbs, flush=True)
for name in (sys.argv[1:] or ("bunny2.5", "512", "1024")):
    d, cams = scene(name)
    rt = []
    for rep in range(9):
        d.RenderHull(cams, 0.0)
        if rep >= 2: rt.append(d.last_render_ms())
    print("%s: dims %s, %d views %dx%d, \"rasterwide\" %d | vcy_render_hull of the same views %s ms"
          % (name, d.dims, NV, W, H, d.get_param("rasterwide"), med(rt)), flush=True)
    raw = d.ExtractIsoSurface(0.0, True)
    res = float(d.option.resolution)
    d.set_param("meshkeys", 0)  # (the chain's mesh has no edge keys)
    chain = d.ExtractIsoChain(0.0, True, dict(iterations=10, lam=0.5, mu=-0.53, pin_boundary=0), dict(cell=2.0 * res, regularize=1e-3))
    for label, m in (("raw extraction", raw), ("chain output", chain)):
        v, f = m["vertices"], m["faces"]
        got, rs, rv, wall = timed(d, v, f, cams)
        t0 = time.perf_counter()
        host = vc.raster_mesh_host(v, f, cams, face=False, hits=False)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(g["depth"].view(np.uint32), h["depth"].view(np.uint32)) and np.array_equal(g["n_dropped"], h["n_dropped"])
                   for g, h in zip(got, host))
        hit = sum(int(np.isfinite(h["depth"]).sum()) for h in host)
        nbytes = len(f) * 48 + NV * W * H * 16
        floor_ms = nbytes / (copy_gbs * 1e9) * 1e3
        print("  %-14s: %d vertices, %d faces, %.1f %% of the pixels hit | raster %s ms | resolve %s ms | call %s ms | host, 1 thread %.0f ms | "
              "floor %.3f ms | device == host %s" % (label, len(v), len(f), 100.0 * hit / (NV * W * H), med(rs), med(rv), med(wall), host_ms,
                                                     floor_ms, same), flush=True)
        line = []
        for wide in SWEEP:
            d.set_param("rasterwide", wide)
            _, rs, _, _ = timed(d, v, f, cams, depth=False)  # (no image comes back: the launches are the same)
            line.append("%d: %s" % (wide, med(rs)))
        d.set_param("rasterwide", 64)
        print("    raster ms by \"rasterwide\"  " + " | ".join(line), flush=True)
    d.close()
