"""Device time of the robust carve's launch (vcy_last_robust_ms: HIP events around the kernel) for m = 0, 1, 3 with 32
views at 1280 x 720, on the bunny at resolution 2.5 (its six cameras taken in turn, intrinsics and silhouettes scaled by 4,
rows cropped) and on the bench scene at 512^3 and 1024^3 -- next to two carves of the SAME views by code this kernel does
not touch, from the same process: (a) the per-view kernel ("fused" 0), which reads and rewrites the state per view, and
(b) the fused launch with "cull" 0 (no view dropping).  (a) and (b): vcy_timer_begin / _end around reset + carve, so (a)
contains the fill of the fresh slab, as the robust launch contains its own write of every voxel.
Run from the repository root on the GPU:  python profiles/robust/measure_robust.py > profiles/robust/measure_robust.txt
Every figure: median [min..max] of 7 calls after 2 warm-up calls, milliseconds."""
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import shutil, subprocess
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
W, H, NV = 1280, 720, 32
def med(x): x = sorted(x); return "%.3f [%.3f..%.3f]" % (x[len(x)//2], x[0], x[-1])
def last_ms(d):
    ms = vc.C.c_float(); d._lib.vcy_last_robust_ms(d.ctx, vc.C.byref(ms)); return ms.value
def scene(name):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5); views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))); small = B.load_masks()
        s = W // B.WIDTH; crop = (B.HEIGHT * s - H) // 2
        cams, masks = [], []
        for k in range(NV):
            v = vc.View.from_buffer_copy(views[k % len(views)])
            v.fx, v.fy, v.cx, v.cy = v.fx * s, v.fy * s, v.cx * s, v.cy * s - crop
            v.width, v.height = W, H; v.roi_min[0] = v.roi_min[1] = 0; v.roi_max[0], v.roi_max[1] = W - 1, H - 1
            cams.append(v)
            masks.append(np.ascontiguousarray(np.kron(small[k % len(small)], np.ones((s, s), np.uint8))[crop:crop + H]))
    else:
        n = int(name); opt = synth.sphere_option(n); cams, masks = synth.sphere_views(n, NV, W, H)
    return opt, cams, masks
info = shutil.which("rocminfo")
lines = subprocess.run([info], capture_output=True, text=True).stdout.splitlines() if info else []
gpus = [l.split(":", 1)[1].strip() for l in lines if l.strip().startswith("Name:") and "gfx" in l]
print("GPU agents as rocminfo names them: %s" % (", ".join(gpus) or "unknown"), flush=True)
print(vc.capi.load().vcy_version().decode(), flush=True)
for name in ("bunny2.5", "512", "1024"):
    opt, cams, masks = scene(name)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    imgs = [d.make_sdf_device(m) for m in masks]
    batch = d.prepare_batch(cams, imgs)
    nvox = d.dims[0] * d.dims[1] * d.dims[2]
    print("%s: %d x %d x %d voxels, %d views at %d x %d" % ((name,) + d.dims + (NV, W, H)), flush=True)
    robust, solid = {}, {}
    for m in (0, 1, 3):
        t = []
        for rep in range(9):
            r = d.CarveRobustDevice(cams, imgs, m)
            if rep >= 2: t.append(r["device_ms"])
        s, u = d.download()
        robust[m], solid[m] = t, int(((u >= 1) & (s < 0)).sum())
        print("  robust m=%d            %s ms   %.2f ps/voxel/view   solid %d   overruled max %d" % (
            m, med(t), sorted(t)[3] * 1e9 / nvox / NV, solid[m], int(r["overruled"].max())), flush=True)
    t_noblame = []
    arr, ptrs = batch[1], batch[2]
    for rep in range(9):  # m = 3 without a place for the counts: the blame is skipped
        assert d._lib.vcy_carve_robust_device(d.ctx, NV, arr, ptrs, 3, 0.0, None) == 0, vc.last_error()
        if rep >= 2: t_noblame.append(last_ms(d))
    print("  robust m=3, no blame   %s ms" % med(t_noblame), flush=True)
    alt = {}
    for label, fused, cull in (("(a) per-view kernel  ", 0, 0), ("(b) fused, cull 0    ", 1, 0), ("    fused, cull 1    ", 1, 1)):
        d.set_param("fused", fused); d.set_param("cull", cull)
        t = []
        for rep in range(9):
            d.reset(); d.sync(); d.timer_begin()
            assert d.CarveBatchDevice(batch), vc.last_error()
            ms = d.timer_end()
            if rep >= 2: t.append(ms)
        alt[label] = t
        s, u = d.download()
        assert int(((u >= 1) & (s < 0)).sum()) == solid[0], "m = 0 and the ordinary carve disagree on the hull"
        print("  %s  %s ms" % (label, med(t)), flush=True)
    m0, m3 = sorted(robust[0])[3], sorted(robust[3])[3]
    a, b = sorted(alt["(a) per-view kernel  "])[3], sorted(alt["(b) fused, cull 0    "])[3]
    print("  m=0 / (a) = %.2f   m=3 / m=0 = %.2f   m=0 / (b) = %.2f" % (m0 / a, m3 / m0, m0 / b), flush=True)
    for p in imgs: d.free_device(p)
    d.close()
