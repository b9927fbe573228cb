"""Which kernel instance the fused carve driver launches, over which grid: a fixed set of small carves for a kernel trace.

Every flavour of the fused carve gives the same voxel state, so the state tests cannot see a driver that picks another
one.  This script carves fixed synthetic scenes -- 64^3 and 60^3 voxels, 1 / 4 / 8 / 32 views, kMax and the weighted
average with and without truncation, fresh and already carved grids, and every knob of the driver at each of its values
-- and is meant to run under a kernel trace with nothing else collected:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o NAME -- python profiles/fused_driver/trace_launches.py
    python profiles/fused_driver/trace_launches.py --summarise OUT/.../NAME_kernel_trace.csv > launches_NAME.txt

The summary lists the distinct (kernel name with its template arguments, grid size in workgroups, workgroup size)
triples, numbered in sorted order, and then the dispatch sequence as those numbers, 32 to a line.  Two builds that
decide alike give identical summaries (`diff` is empty).  The context waits for the device after every launch: the
hint of the last live list, which the next launch reads, is then the same in every run."""
import csv
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H = 160, 120
MODES = {
    "max": dict(),
    "wa": dict(voxel_update=1),
    "wa_trunc": dict(voxel_update=1, use_truncation=True, truncation_band=0.1),
}
KNOBS = [("tile", (0, 1, 2)), ("rowkernel", (0, -1, 4)), ("oneview", (0, 1)), ("coopstore", (-1, 0, 1)),
         ("ntstore", (-1, 0, 1)), ("prologue", (0, 1, 2)), ("recordbytes", (0, 1024, 4096)), ("livelist", (0, 1)),
         ("listrecords", (0, 1)), ("eagerstate", (-1, 0, 1)), ("livesync", (0, 1))]


def images(n, n_views, scale):
    """A cone per view over the silhouette disc of synth.sphere_views, its radius different from view to view: positive
    inside, below the truncation limit -1 far outside."""
    import numpy as np
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    r = np.hypot(xx - (W / 2 - 0.5), yy - (H / 2 - 0.5))
    rad = 0.35 * n / math.sqrt((2.0 * n) ** 2 - (0.35 * n) ** 2) * (H / 2) / math.tan(math.radians(30.0))
    return [((rad * scale * (0.8 + 0.1 * ((7 * i) % 5)) - r) / 8.0).astype(np.float32) for i in range(n_views)]


def run(n, mode, launches, params=()):
    """One context: `launches` is a list of (view count, radius scale); the first finds the grid fresh."""
    from vacancy_amd import carver as vc
    from vacancy_amd import synth
    from vacancy_amd.capi import UpdateOption
    dev = vc.VoxelCarver(synth.sphere_option(n, UpdateOption(**MODES[mode])))
    assert dev.Init(), vc.last_error()
    for k, v in params:
        dev.set_param(k, v)
    print("n=%d mode=%s launches=%s %s" % (n, mode, launches, dict(params)), flush=True)
    for n_views, scale in launches:
        views, _ = synth.sphere_views(n, n_views, W, H)
        ptrs = [dev.upload_sdf(im) for im in images(n, n_views, scale)]
        assert dev.CarveBatchDevice(views, ptrs), vc.last_error()
        dev.sync()
        for p in ptrs:
            dev.free_device(p)
    dev.close()


def carve_all():
    sys.path.insert(0, ROOT)
    for n in (64, 60):
        for mode in MODES:
            for n_views in (1, 4, 8, 32):
                # fresh, then twice over the carved grid: the second of those reads the hint the first left
                run(n, mode, [(n_views, 1.0), (n_views, 0.7), (n_views, 0.9)])
    for knob, values in KNOBS:
        for value in values:
            for mode in ("max", "wa_trunc"):
                run(64, mode, [(1, 1.0), (1, 0.7), (1, 0.9), (4, 0.8)], ((knob, value),))


def summarise(path):
    """The distinct (kernel, grid, workgroup) triples, numbered in sorted order, then the dispatch sequence as numbers."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    seq = []
    for r in rows:
        wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
        grid = [int(r["Grid_Size_" + a]) // max(w, 1) for a, w in zip("XYZ", wg)]
        seq.append("%s | %dx%dx%d | %dx%dx%d" % ((r["Kernel_Name"],) + tuple(grid) + tuple(wg)))
    ids = {t: i for i, t in enumerate(sorted(set(seq)))}
    for t, i in sorted(ids.items(), key=lambda kv: kv[1]):
        print("%d = %s" % (i, t))
    print("%d dispatches, in dispatch order:" % len(seq))
    for k in range(0, len(seq), 32):
        print(" ".join(str(ids[t]) for t in seq[k:k + 32]))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        carve_all()
