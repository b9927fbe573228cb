"""The ray-cast of the hull over z-slabs next to the whole-grid ray-cast on the same state: 1 view and 32 views at
1280 x 720 on the bunny at resolution 2.5 and on the bench scene at 512^3 and 1024^3, the grid cut into 2, 4 and 8
equal slabs on ONE device (ShardedVoxelCarver, devices=[0]).
Run from the repository root on the GPU:  python profiles/render/measure_slab_render.py > profiles/render/measure_slab_render.txt
Without an argument the script runs one child per scene, each under `timeout -k 10`, and stops at the first that fails;
with a scene name it measures that scene.  Every figure: median [min..max] of 7 calls after 2 warm-up calls.
  whole        vcy_render_hull on the single context: device ms (vcy_last_render_ms) | wall ms of RenderHull (depth only)
  S slabs      device ms of every slab (vcy_last_render_ms of vcy_render_hull_slab, in z order) and their sum | wall ms of
               ShardedVoxelCarver.RenderHull: the slabs' renders one after the other on the one device, depth and voxel
               ids to the host, the host merge
  agreement    wall ms of HullAgreement: the single context's (counted on the device) | the sharded carver's (hit bits
               to the host, OR and count there); the counts are asserted equal, as the depth images are."""
import os, subprocess, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
W, H = 1280, 720
SCENES = ("bunny2.5", "512", "1024")
def med(x): x = sorted(x); return "%.3f [%.3f..%.3f]" % (x[len(x)//2], x[0], x[-1])
def timed(fn):
    import time
    t0 = time.perf_counter(); r = fn(); return r, (time.perf_counter() - t0) * 1e3
def measure(name):
    import numpy as np
    from vacancy_amd import carver as vc, sharded, synth
    import bunny_data as B
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
    rng = np.random.RandomState(1)
    sil = [(rng.rand(H, W) < 0.5).astype(np.uint8) for _ in range(32)]
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    assert d.CarveBatchSilhouettes(views, masks), vc.last_error()
    d.sync()
    whole, want, counts = {}, {}, {}
    for nv in (1, 32):
        dev, wall, agree = [], [], []
        for rep in range(9):
            r, ms = timed(lambda: d.RenderHull(cams[:nv], 0.0))
            c, ms_a = timed(lambda: d.HullAgreement(cams[:nv], sil[:nv]))
            if rep >= 2: dev.append(d.last_render_ms()); wall.append(ms); agree.append(ms_a)
        want[nv], counts[nv], whole[nv] = r, c, (med(dev), med(wall), med(agree), sorted(dev)[3])
        print("%s: dims %s | whole grid, %d view(s) %dx%d: device %s ms | wall %s ms | agreement wall %s ms (%d hull pixels)"
              % (name, d.dims, nv, W, H, whole[nv][0], whole[nv][1], whole[nv][2], int(sum(np.isfinite(x["depth"]).sum() for x in r))), flush=True)
    for slabs in (2, 4, 8):
        sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=slabs); assert sh.Init(), vc.last_error()
        assert sh.CarveBatchSilhouettes(views, masks), vc.last_error()
        sh.sync()
        for nv in (1, 32):
            per, wall, agree = [[] for _ in sh.slabs], [], []
            for rep in range(9):
                r, ms = timed(lambda: sh.RenderHull(cams[:nv], 0.0))
                each = [c.last_render_ms() for c in sh.slabs]
                c, ms_a = timed(lambda: sh.HullAgreement(cams[:nv], sil[:nv]))
                if rep >= 2:
                    wall.append(ms); agree.append(ms_a)
                    for k, e in enumerate(each): per[k].append(e)
            assert all(np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32)) for a, b in zip(r, want[nv]))
            assert np.array_equal(c, counts[nv])
            mids = [sorted(p)[3] for p in per]
            print("%s: %d slabs %s, %d view(s): device per slab %s ms, sum %.3f ms (whole grid %.3f ms: x %.2f) | wall render + merge %s ms | "
                  "agreement through hit bits wall %s ms | images and counts equal the whole grid's"
                  % (name, slabs, sh.z_ranges, nv, " ".join("%.3f" % m for m in mids), sum(mids), whole[nv][3], sum(mids) / whole[nv][3],
                     med(wall), med(agree)), flush=True)
        sh.close()
    d.close()
if len(sys.argv) > 1:
    measure(sys.argv[1])
else:
    import shutil
    from vacancy_amd import carver as vc
    info = shutil.which("rocminfo")
    names = [l.split(":", 1)[1].strip() for l in subprocess.run([info], capture_output=True, text=True).stdout.splitlines() if "Marketing Name" in l] if info else []
    names = [n for n in names if n]
    gpus = [n for n in names if "Instinct" in n or "MI3" in n]
    print("machine: %s" % ", ".join(gpus[:1] or names[:1] or ["unknown"]), flush=True)
    print(vc.capi.load().vcy_version().decode(), flush=True)
    for name in SCENES:  # one process per scene, each under its own limit; nothing more is started after a failure
        rc = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), name]).returncode
        if rc != 0:
            print("%s: the step ended with status %d; later scenes were not run" % (name, rc), flush=True)
            sys.exit(rc)
