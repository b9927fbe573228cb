"""Device time of the distance field of the hull (vcy_last_distance_ms: HIP events around solid bits, x pass, y pass, z pass)
for vcy_distance_field -- its copy of the field to the host is not in the figure -- and vcy_redistance, with R = 4, 16, 64,
on the bunny at resolution 2.5 (its six views) and on the bench scene at 512^3 and 1024^3 (8 views at 640 x 480).  Next to
it, on the same context, vcy_last_components_ms of a labelling of the same state -- a yardstick of the same class: solid
bits, then a few passes over the voxels -- and the wall time of the serial host function vcy_distance_field_host on the
downloaded state, the route the device call replaces minus its two PCIe copies of the state.  The floor: solid bits
(1/8 B), row distances (1 B) and y-pass values (2 B) written and read once, the state's sdf (4 B) written once, at the
device-to-device copy rate vcy_measure_bandwidth reports on this GPU.
Run from the repository root on the GPU:  python profiles/distance/measure_distance.py > profiles/distance/measure_distance.txt
(arguments: the sizes to run, by default bunny2.5 512 1024; HOST_CALL_LIMIT_S, by default 4: a host call that takes longer
than this many seconds is measured ONCE and marked "(1 call)", and HOST_VOXEL_RADIUS_LIMIT, by default 1e10: the host
function is not run where voxels * R exceeds it, and the line says so.)
Every other figure: median [min..max] of 7 calls after 2 warm-up calls, milliseconds.
With --slabs (python profiles/distance/measure_distance.py --slabs [sizes] > profiles/distance/measure_distance_slabs.txt):
the same scenes cut into 1, 2 and 4 z-slabs on one device (ShardedVoxelCarver.RedistanceSlabs): device ms of the begin
calls (solid bits, x pass, y pass) and of the finishing calls (the z pass over the extended columns), each summed over the
slabs, the bytes of planes that cross the host, the wall time of the whole RedistanceSlabs, and next to them the whole-grid
vcy_redistance of the same visit with the ratio of the two device times and the ratio the 2 R extra slices staged per seam
let one expect, 1 + 2 R (slabs - 1) / nz."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import shutil, subprocess
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
RADII = (4, 16, 64)
SLABS = "--slabs" in sys.argv[1:]
SIZES = [a for a in sys.argv[1:] if a != "--slabs"] or ["bunny2.5", "512", "1024"]
HOST_CALL_LIMIT_S = float(os.environ.get("HOST_CALL_LIMIT_S", "4"))
HOST_VOXEL_RADIUS_LIMIT = float(os.environ.get("HOST_VOXEL_RADIUS_LIMIT", "1e10"))
def med(x): x = sorted(x); return "%.3f [%.3f..%.3f]" % (x[len(x)//2], x[0], x[-1])
def mid(x): return sorted(x)[len(x)//2]
def scene(name):
    if name == "bunny2.5":
        return B.bunny_option(2.5), B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))), B.load_masks()
    n = int(name); cams, masks = synth.sphere_views(n, 8, 640, 480)
    return synth.sphere_option(n), cams, masks
info = shutil.which("rocminfo")
lines = subprocess.run([info], capture_output=True, text=True).stdout.splitlines() if info else []
gpus = [l.split(":", 1)[1].strip() for l in lines if l.strip().startswith("Name:") and "gfx" in l]
print("GPU agents as rocminfo names them: %s" % (", ".join(gpus) or "unknown"), flush=True)
print(vc.capi.load().vcy_version().decode(), flush=True)
read_gbs, copy_gbs = vc.measure_bandwidth()
print("vcy_measure_bandwidth: read %.0f GB/s, device-to-device copy %.0f GB/s" % (read_gbs, copy_gbs), flush=True)
def measure_slabs(name):
    from vacancy_amd import sharded as vs
    opt, cams, masks = scene(name)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    assert d.CarveBatchSilhouettes(cams, masks), vc.last_error()
    nz = d.dims[2]
    print("%s: %d x %d x %d voxels, %d views" % ((name,) + d.dims + (len(cams),)), flush=True)
    whole = {}
    for radius in RADII:  # (the rewrite keeps the solid set: every call does the same work)
        w = [d.Redistance(0.0, radius)["device_ms"] for rep in range(9)][2:]
        whole[radius] = mid(w)
        print("  whole grid  R %2d  redistance %s ms" % (radius, med(w)), flush=True)
    d.close()
    for count in (1, 2, 4):
        sv = vs.ShardedVoxelCarver(opt, [0], count); assert sv.Init(), vc.last_error()
        assert sv.CarveBatchSilhouettes(cams, masks), vc.last_error()
        for radius in RADII:
            begin, finish, wall = [], [], []
            for rep in range(9):
                t0 = time.perf_counter(); r = sv.RedistanceSlabs(0.0, radius); t = time.perf_counter() - t0
                if rep >= 2: begin.append(r["begin_ms"]); finish.append(r["finish_ms"]); wall.append(t * 1e3)
            both = mid(begin) + mid(finish)
            print("  slabs %d  R %2d  begin %s ms  finish %s ms  sum %.3f ms  = %.3f x whole grid (staged slices: %.3f)   "
                  "planes through the host %d bytes   wall %s ms" % (count, radius, med(begin), med(finish), both,
                  both / whole[radius], 1.0 + 2.0 * radius * (count - 1) / nz, r["plane_bytes"], med(wall)), flush=True)
        sv.close()
if SLABS:
    for name in SIZES: measure_slabs(name)
    sys.exit(0)
for name in SIZES:
    opt, cams, masks = scene(name)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    assert d.CarveBatchSilhouettes(cams, masks), vc.last_error()
    nvox = d.dims[0] * d.dims[1] * d.dims[2]
    floor = nvox * (2.0 * (0.125 + 1 + 2) + 4) / (copy_gbs * 1e9) * 1e3
    lab = []
    for rep in range(9):
        r = d.LabelComponents(0.0)
        if rep >= 2: lab.append(r["device_ms"])
    sdf, cnt = d.download()
    print("%s: %d x %d x %d voxels, %d views, touched %d, solid %d, components %d   floor %.3f ms   labelling %s ms" % (
        (name,) + d.dims + (len(cams), int((cnt >= 1).sum()), int(((cnt >= 1) & (sdf < 0)).sum()), len(r["label"]), floor, med(lab))),
        flush=True)
    for radius in RADII:
        f, w = [], []
        for rep in range(9):
            d2 = d.DistanceField(0.0, radius)
            if rep >= 2: f.append(d.last_distance_ms())
        exact = int((np.abs(d2) <= radius * radius).sum())
        # the host function on the downloaded state, before Redistance replaces it on the device (the solid set stays)
        host, note = [], ""
        if nvox * radius > HOST_VOXEL_RADIUS_LIMIT:
            note = "not run (voxels * R above %g)" % HOST_VOXEL_RADIUS_LIMIT
        else:
            t0 = time.perf_counter(); h2, _ = vc.distance_field_host(opt, sdf, cnt, 0.0, radius); first = time.perf_counter() - t0
            assert np.array_equal(h2, d2), "the host function and the device differ"
            if first > HOST_CALL_LIMIT_S:
                host, note = [first * 1e3], "(1 call)"
            else:
                for rep in range(9):
                    t0 = time.perf_counter(); vc.distance_field_host(opt, sdf, cnt, 0.0, radius); t = time.perf_counter() - t0
                    if rep >= 2: host.append(t * 1e3)
            del h2
        del d2
        for rep in range(9):
            r = d.Redistance(0.0, radius)
            if rep >= 2: w.append(r["device_ms"])
        line = "  R %2d  exact %d   field %s ms  x %.1f floor  x %.2f labelling   redistance %s ms  x %.1f floor  x %.2f labelling" % (
            radius, exact, med(f), mid(f) / floor, mid(f) / mid(lab), med(w), mid(w) / floor, mid(w) / mid(lab))
        if host:
            line += "   host %s ms %s  = %.0f x field, %.0f x redistance" % (med(host), note, mid(host) / mid(f), mid(host) / mid(w))
        else:
            line += "   host " + note
        print(line, flush=True)
        d.upload(sdf, cnt)  # the carved state again for the next radius
    d.close()
    del sdf, cnt
