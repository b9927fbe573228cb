"""Device time of vcy_color_vertices (32 views at 1280 x 720, every mode and sampler, the hull ray-cast inside the call) on
the iso-surface of the bunny at resolution 2.5 and of the bench scene at 512^3 and 1024^3, next to the same context's
ray-cast, the single-thread wall time of vcy_color_vertices_host on the same input, and a floor from the bytes that must move.
Run from the repository root on the GPU:  python profiles/color/measure_color.py > profiles/color/measure_color.txt
Device figures: median [min..max] of 7 calls after 2 warm-up calls, HIP events around the launches (vcy_last_color_ms: the
packing of the photographs to RGBX and the colouring kernel; vcy_last_render_ms: the ray-cast of the same call).  "call" is
the wall time of the whole call, uploads of the photographs included.  Host: one call, wall time, with the depth images of
RenderHull.  Floor: vertices (12 B, with normals 24 B) and outputs (20 B) once, plus one depth dword and the sampler's
taps (1 or 4 dwords) per contributing (vertex, view) pair, counted from n_used, over the measured device copy rate."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
W, H, NV = 1280, 720, 32
MODES = (("mean", 0), ("weighted", 1), ("best", 2))
INTERPS = (("nn", 0), ("bilinear", 1))
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
import shutil, subprocess
info = shutil.which("rocminfo")
names = [l.split(":", 1)[1].strip() for l in subprocess.run([info], capture_output=True, text=True).stdout.splitlines() if "Marketing Name" in l] if info else []
names = [n for n in names if n]
gpus = [n for n in names if "Instinct" in n or "MI3" in n]
print("machine: %s" % ", ".join(gpus or names or ["unknown"]), flush=True)
print(vc.capi.load().vcy_version().decode(), flush=True)
_, copy_gbs = vc.measure_bandwidth(0, 1 << 30, 3)
print("device copy rate %.0f GB/s (vcy_measure_bandwidth, read + write)" % copy_gbs, flush=True)
rng = np.random.RandomState(7)
photos = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(NV)]
for name in ("bunny2.5", "512", "1024"):
    d, cams = scene(name)
    mesh = d.ExtractIsoSurface(0.0, True, normals=True)
    v, nr = mesh["vertices"], mesh["normals"]
    rt = []
    for rep in range(9):
        r = d.RenderHull(cams, 0.0)
        if rep >= 2: rt.append(d.last_render_ms())
    depth = [x["depth"] for x in r]
    print("%s: dims %s, %d vertices, %d views %dx%d | ray-cast alone %s ms" % (name, d.dims, len(v), NV, W, H, med(rt)), flush=True)
    for mn, mode in MODES:
        for sn, interp in INTERPS:
            t, rn, wall = [], [], []
            for rep in range(9):
                t0 = time.perf_counter()
                got = d.ColorVertices(v, cams, photos, nr, None, mode, interp)
                w_ms = (time.perf_counter() - t0) * 1e3
                if rep >= 2: t.append(got["device_ms"]); rn.append(d.last_render_ms()); wall.append(w_ms)
            t0 = time.perf_counter()
            host = vc.color_vertices_host(v, cams, photos, depth, nr, mode, interp, 1.5 * d.option.resolution)
            host_ms = (time.perf_counter() - t0) * 1e3
            same = all(np.array_equal(got[k].view(np.uint32) if k == "rgb" else got[k], host[k].view(np.uint32) if k == "rgb" else host[k])
                       for k in ("rgb", "n_used", "best_view"))
            pairs = int(got["n_used"].astype(np.int64).sum())
            nbytes = len(v) * ((24 if mode else 12) + 20) + pairs * 4 * (1 + (4 if interp else 1))
            floor_ms = nbytes / (copy_gbs * 1e9) * 1e3
            print("  %-8s %-8s: colouring launches %s ms | ray-cast in the call %s ms | call %s ms | host, 1 thread %.0f ms | "
                  "%d contributing pairs (%.1f per vertex), floor %.3f ms | device == host %s"
                  % (mn, sn, med(t), med(rn), med(wall), host_ms, pairs, pairs / max(1, len(v)), floor_ms, same), flush=True)
    d.close()
