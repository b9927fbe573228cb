"""Device time of vcy_label_components / vcy_keep_components next to the dense marching-cubes pass on the same context,
and the wall time of the host route they replace (vcy_download -> numpy labelling -> vcy_upload).
Run from the repository root on the GPU:  python profiles/components/measure_components.py > profiles/components/measure_components.txt
Slab mode:  python profiles/components/measure_components.py --slabs > profiles/components/measure_components_slabs.txt
the same scenes cut into 2, 4 and 8 z-slabs on ONE device (ShardedVoxelCarver): the summed device time of the sharded
labelling (slab labelling + seam pairs) and of labelling + filter, the host time of the seam merge alone, and beside them
the whole-grid call on the same state as the figure to compare against."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
import components_ref as R
def scene(name):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5); views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))); masks = B.load_masks()
    else:
        n = int(name); opt = synth.sphere_option(n); views, masks = synth.sphere_views(n, 16, 640, 480)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    def carve():
        d.reset()
        assert d.CarveBatchSilhouettes(views, masks), vc.last_error()
        d.sync()
    d._views, d._masks = views, masks
    carve(); return d, carve
def med(x): x = sorted(x); return "%.3f [%.3f..%.3f]" % (x[len(x)//2], x[0], x[-1])
def slab_mode():
    from vacancy_amd import sharded, dist as vdist
    for name in ("bunny2.5", "512", "1024"):
        d, carve = scene(name)
        whole = d.LabelComponents(0.0)
        lab, keep = [], []
        for rep in range(5):
            lab.append(d.LabelComponents(0.0)["device_ms"])
        for rep in range(3):
            carve(); keep.append(d.KeepComponents(0.0, largest=1)["device_ms"])
        print("%s: dims %s, %d components | whole grid: label device ms %s | label + filter(largest=1) %s"
              % (name, d.dims, len(whole["label"]), med(lab), med(keep)), flush=True)
        views, masks = d._views, d._masks
        for count in (2, 4, 8):
            sh = sharded.ShardedVoxelCarver(d.option, devices=[0], slabs_per_device=count)
            assert sh.Init(), vc.last_error()
            def carve_slabs():
                for c in sh.slabs:
                    c.reset(); assert c.CarveBatchSilhouettes(views, masks), vc.last_error(); c.sync()
            carve_slabs()
            got = sh.LabelComponents(0.0)
            assert np.array_equal(got["label"], whole["label"]) and np.array_equal(got["n_voxels"], whole["n_voxels"])
            lab, keep, merge, wall = [], [], [], []
            for rep in range(5):
                t = time.perf_counter(); lab.append(sh.LabelComponents(0.0)["device_ms"]); wall.append((time.perf_counter() - t) * 1e3)
            r = vdist.label_components_slabs(sh.slabs, 0, 1, 0.0)
            prs = [c.component_seam_pairs(b.component_top_plane()) for b, c in zip(sh.slabs[:-1], sh.slabs[1:])]
            for rep in range(5):
                t = time.perf_counter(); vdist.merge_components(r["lists"], prs); merge.append((time.perf_counter() - t) * 1e3)
            for rep in range(3):
                carve_slabs(); keep.append(sh.KeepComponents(0.0, largest=1)["device_ms"])
            print("%s in %d slabs: pieces %s, seam pairs %s | label: summed device ms %s, call wall ms %s | host merge ms %s | "
                  "label + filter(largest=1): summed device ms %s" % (name, count, [len(l["label"]) for l in r["lists"]],
                  [len(p) for p in prs], med(lab), med(wall), med(merge), med(keep)), flush=True)
            sh.close()
        d.close()
if "--slabs" in sys.argv:
    slab_mode(); sys.exit(0)
for name in ("bunny2.5", "512", "1024"):
    d, carve = scene(name)
    d.set_param("mcskip", 0)  # the dense pass: every brick read, the floor a pass over the state shares
    for _ in range(2): d.ExtractIsoSurface(0.0, True); d.LabelComponents(0.0)
    lab, mc, keep = [], [], []
    for rep in range(7):
        c = d.LabelComponents(0.0); lab.append(c["device_ms"])
        mc.append(d.ExtractIsoSurface(0.0, True)["device_ms"])
    for rep in range(5):
        carve()
        r = d.KeepComponents(0.0, largest=1); keep.append(r["device_ms"])
    carve()
    rall = d.KeepComponents(0.0, largest=0, min_voxels=1 << 40)  # every component goes: every solid brick is rewritten
    carve()
    t = time.perf_counter(); s, u = d.download(); t_down = time.perf_counter() - t
    if name != "1024":
        t = time.perf_counter(); comps, labels = R.reference(s, u, d.dims, 0.0); s2 = R.filter_state(s, labels, comps, 1, 0, 1.0)[0]; t_host = time.perf_counter() - t
        assert np.array_equal(comps["n_voxels"], c["n_voxels"]) and np.array_equal(comps["label"], c["label"])
    else:
        s2, t_host = s, float("nan")  # (a 2^30-voxel numpy labelling: not run; download and upload alone are shown)
    t = time.perf_counter(); d.upload(s2, u); d.sync(); t_up = time.perf_counter() - t
    print("%s: dims %s, %d components, largest %d voxels | label device ms %s | label + filter(largest=1: %d voxels removed) %s | "
          "label + filter(everything: %d voxels) %.3f | dense marching-cubes kernels %s | host route: download %.2f s + numpy %.2f s + upload %.2f s"
          % (name, d.dims, len(c["label"]), int(c["n_voxels"][0]), med(lab), r["removed_voxels"], med(keep), rall["removed_voxels"],
             rall["device_ms"], med(mc), t_down, t_host, t_up), flush=True)
    d.close()
