"""Device time of vcy_render_hull (1 view and 32 views at 1280 x 720, "rayskip" 1 and 0) next to the dense marching-cubes
pass on the same context, on the bunny at resolution 2.5 and on the bench scene at 512^3 and 1024^3.
Run from the repository root on the GPU:  python profiles/render/measure_render.py > profiles/render/measure_render.txt
Every figure: median [min..max] of 7 calls after 2 warm-up calls, HIP events around the launches (vcy_last_render_ms:
the bit planes are rebuilt only after the state or the iso level has changed, so the figures are the ray-cast alone;
"with bit planes rebuilt" alternates between two iso levels, 5 calls)."""
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
W, H = 1280, 720
def med(x): x = sorted(x); return "%.3f [%.3f..%.3f]" % (x[len(x)//2], x[0], x[-1])
def scene(name):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5); views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))); masks = B.load_masks()
        s = W / float(B.WIDTH)  # the bunny's cameras at 1280 x 720: intrinsics scaled by 4, rows cropped
        cams = []
        for k in range(32):
            v = vc.View.from_buffer_copy(views[k % len(views)])
            v.fx, v.fy, v.cx, v.cy = v.fx * s, v.fy * s, v.cx * s, v.cy * s - (B.HEIGHT * s - H) / 2.0
            v.width, v.height = W, H; v.roi_min[0] = v.roi_min[1] = 0; v.roi_max[0], v.roi_max[1] = W - 1, H - 1
            cams.append(v)
    else:
        n = int(name); opt = synth.sphere_option(n); views, masks = synth.sphere_views(n, 16, 640, 480)
        cams, _ = synth.sphere_views(n, 32, W, H)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    assert d.CarveBatchSilhouettes(views, masks), vc.last_error()
    d.sync()
    return d, cams
import shutil, subprocess
info = shutil.which("rocminfo")
names = [l.split(":", 1)[1].strip() for l in subprocess.run([info], capture_output=True, text=True).stdout.splitlines() if "Marketing Name" in l] if info else []
names = [n for n in names if n]  # (agents without a marketing name print an empty field)
gpus = [n for n in names if "Instinct" in n or "MI3" in n]
print("machine: %s (host and agents as rocminfo names them; the library's target is in the next line)" % ", ".join(gpus or names or ["unknown"]), flush=True)
print(vc.capi.load().vcy_version().decode(), flush=True)
for name in ("bunny2.5", "512", "1024"):
    d, cams = scene(name)
    d.set_param("mcskip", 0)  # the dense pass: every brick read
    mc = []
    for rep in range(9):
        ms = d.ExtractIsoSurface(0.0, True)["device_ms"]
        if rep >= 2: mc.append(ms)
    out = {}
    for nv in (1, 32):
        for skip in (1, 0):
            d.set_param("rayskip", skip)
            t, hit = [], 0
            for rep in range(9):
                r = d.RenderHull(cams[:nv], 0.0)
                if rep >= 2: t.append(d.last_render_ms())
                hit = int(sum(np.isfinite(x["depth"]).sum() for x in r))
            out[nv, skip] = (med(t), hit)
    assert out[1, 1][1] == out[1, 0][1] and out[32, 1][1] == out[32, 0][1]
    d.set_param("rayskip", 1)
    first = []
    for rep in range(5):  # another iso level makes the kept bit planes stale: solid bits and occupancy are built again
        d.RenderHull(cams[:1], -1e-30 if rep % 2 == 0 else 0.0); first.append(d.last_render_ms())
    first = med(first)
    print("%s: dims %s | render 1 view %dx%d: rayskip 1 %s ms, rayskip 0 %s ms (%d hull pixels) | 32 views: rayskip 1 %s ms, "
          "rayskip 0 %s ms (%d hull pixels) | 1 view with bit planes rebuilt %s ms | dense marching-cubes kernels %s ms"
          % (name, d.dims, W, H, out[1, 1][0], out[1, 0][0], out[1, 1][1], out[32, 1][0], out[32, 0][0], out[32, 1][1], first,
             med(mc)), flush=True)
    d.close()
