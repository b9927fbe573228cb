"""Device time of the depth carve's launches (vcy_last_depth_ms: HIP events around the kernels) for 32 views at 1280 x 720 in
kMax and weighted-average mode, on the bunny at resolution 2.5 (its six cameras taken in turn, intrinsics and silhouettes
scaled by 4, rows cropped) and on the bench scene at 512^3 and 1024^3.  The depth images are RenderHull's of the scene's own
carved hull, resident on the device.  Next to it, from the same process and on contexts of the same shape, two carves of
the same views by code this kernel does not touch: (a) the per-view kernel on 32 SDF images with sdf_interp = kNn
("fused" 0) -- one tap per pair like the depth kernel, but the state read and written per view --, and (b) the robust
launch with m = 0 -- the state written once, four taps per pair.  (a): vcy_timer_begin / _end around reset + carve, so it
contains the fill of the fresh slab; the depth carve is given both ways (events around its kernels; timer around reset +
call, fill included).  The floor: the state (4-byte sdf + 1-byte counter) read and written once at the device-to-device
copy rate vcy_measure_bandwidth reports on this GPU.
Run from the repository root on the GPU:  python profiles/depth/measure_depth.py > profiles/depth/measure_depth.txt
Every figure: median [min..max] of 7 calls after 2 warm-up calls, milliseconds."""
import os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import shutil, subprocess
import numpy as np
from vacancy_amd import carver as vc, synth
from vacancy_amd.capi import UpdateOption
import bunny_data as B
W, H, NV = 1280, 720, 32
SIZES = sys.argv[1:] or ["bunny2.5", "512", "1024"]
def med(x): x = sorted(x); return "%.3f [%.3f..%.3f]" % (x[len(x)//2], x[0], x[-1])
def mid(x): return sorted(x)[len(x)//2]
def scene(name, uo):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5, uo); views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))); small = B.load_masks()
        s = W // B.WIDTH; crop = (B.HEIGHT * s - H) // 2
        cams, masks = [], []
        for k in range(NV):
            v = vc.View.from_buffer_copy(views[k % len(views)])
            v.fx, v.fy, v.cx, v.cy = v.fx * s, v.fy * s, v.cx * s, v.cy * s - crop
            v.width, v.height = W, H; v.roi_min[0] = v.roi_min[1] = 0; v.roi_max[0], v.roi_max[1] = W - 1, H - 1
            cams.append(v)
            masks.append(np.ascontiguousarray(np.kron(small[k % len(small)], np.ones((s, s), np.uint8))[crop:crop + H]))
    else:
        n = int(name); opt = synth.sphere_option(n, uo); cams, masks = synth.sphere_views(n, NV, W, H)
    return opt, cams, masks
def context(name, **kw):
    opt, cams, masks = scene(name, UpdateOption(**kw))
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    return d, cams, masks
info = shutil.which("rocminfo")
lines = subprocess.run([info], capture_output=True, text=True).stdout.splitlines() if info else []
gpus = [l.split(":", 1)[1].strip() for l in lines if l.strip().startswith("Name:") and "gfx" in l]
print("GPU agents as rocminfo names them: %s" % (", ".join(gpus) or "unknown"), flush=True)
print(vc.capi.load().vcy_version().decode(), flush=True)
read_gbs, copy_gbs = vc.measure_bandwidth()
print("vcy_measure_bandwidth: read %.0f GB/s, device-to-device copy %.0f GB/s" % (read_gbs, copy_gbs), flush=True)
for name in SIZES:
    # the scene's hull and its depth images, left on the device
    d, cams, masks = context(name)
    assert d.CarveBatchSilhouettes(cams, masks), vc.last_error()
    res = d.option.resolution
    nvox = d.dims[0] * d.dims[1] * d.dims[2]
    print("%s: %d x %d x %d voxels, %d views at %d x %d, band = 3 voxels" % ((name,) + d.dims + (NV, W, H)), flush=True)
    depth = [d.upload_sdf(r["depth"]) for r in d.RenderHull(cams, 0.0)]
    sdfs = [d.make_sdf_device(m) for m in masks]
    d.close()
    floor = 2.0 * nvox * 5 / (copy_gbs * 1e9) * 1e3
    got = {}
    for label, kw in (("depth kMax            ", dict()), ("depth weighted average", dict(voxel_update=1))):
        c, _, _ = context(name, **kw)
        t, wall = [], []
        for rep in range(9):
            c.reset(); c.sync(); c.timer_begin()
            r = c.CarveDepthDevice(cams, depth, 3.0 * res)
            ms = c.timer_end()
            if rep >= 2: t.append(r["device_ms"]); wall.append(ms)
        s, u = c.download()
        got[label] = t
        print("  %s  %s ms   with the fill %s ms   %.2f ps/voxel/view   touched %d   sdf > 0: %d   floor %.3f ms, x %.1f" % (
            label, med(t), med(wall), mid(t) * 1e9 / nvox / NV, int((u >= 1).sum()), int(((u >= 1) & (s > 0)).sum()), floor,
            mid(t) / floor), flush=True)
        c.close()
    c, _, _ = context(name, sdf_interp=0)
    c.set_param("fused", 0)
    batch = c.prepare_batch(cams, sdfs)
    a = []
    for rep in range(9):
        c.reset(); c.sync(); c.timer_begin()
        assert c.CarveBatchDevice(batch), vc.last_error()
        ms = c.timer_end()
        if rep >= 2: a.append(ms)
    print("  (a) per-view kernel, NN  %s ms (with the fill)" % med(a), flush=True)
    c.close()
    c, _, _ = context(name)
    b = []
    for rep in range(9):
        r = c.CarveRobustDevice(cams, sdfs, 0)
        if rep >= 2: b.append(r["device_ms"])
    print("  (b) robust launch, m = 0 %s ms" % med(b), flush=True)
    c.close()
    k = mid(got["depth kMax            "]); w = mid(got["depth weighted average"])
    print("  depth kMax / (a) = %.2f   depth average / (a) = %.2f   depth kMax / (b) = %.2f   depth average / (b) = %.2f" % (
        k / mid(a), w / mid(a), k / mid(b), w / mid(b)), flush=True)
    d, _, _ = context(name)
    for p in depth + sdfs: d.free_device(p)
    d.close()
