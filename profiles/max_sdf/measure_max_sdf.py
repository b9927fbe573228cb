"""Device time of the max_sdf resolution (resolve_views, carve_kernels.hip: two launches of max_reduce_kernel and a
4-byte copy per image, only with update_outside = kMax) on ONE 1280 x 720 image.  vcy_timer_begin / _end (HIP events on
the context's stream) around a single-view carve of an 8^3 grid by the per-view kernel ("fused" 0), whose own launch is
a few microseconds: once with update_outside = kMax, once without -- the difference is the resolution, its allocation and
its wait included.  The library is the one VCY_HIP_LIB names (default: the tree's), so the parent commit's and the
branch's can be measured alternately in one visit; the argument is a label for the output.
Run from the repository root on the GPU:  python profiles/max_sdf/measure_max_sdf.py branch >> profiles/max_sdf/measure_max_sdf.txt
Every figure: median [min..max] of 200 calls after 20 warm-up calls, milliseconds."""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
from vacancy_amd import carver as vc, synth
from vacancy_amd.capi import UpdateOption
W, H, CALLS, WARM = 1280, 720, 200, 20
def med(x): x = sorted(x); return "%.4f [%.4f..%.4f]" % (x[len(x) // 2], x[0], x[-1])
rng = np.random.RandomState(1)
img = rng.uniform(-1.0, 1.0, (H, W)).astype(np.float32)
views, _ = synth.sphere_views(8, 1, W, H)
print("%s  (library: %s)" % (vc.capi.load().vcy_version().decode(), sys.argv[1] if len(sys.argv) > 1 else "the tree's"), flush=True)
mid = {}
for outside in (1, 0, 1, 0):
    d = vc.VoxelCarver(synth.sphere_option(8, UpdateOption(update_outside=outside)))
    assert d.Init(), vc.last_error()
    d.set_param("fused", 0)
    p = d.upload_sdf(img)
    batch = d.prepare_batch(views, [p])
    t = []
    for k in range(WARM + CALLS):
        d.timer_begin()
        assert d.CarveBatchDevice(batch), vc.last_error()
        ms = d.timer_end()
        if k >= WARM:
            t.append(ms)
    mid.setdefault(outside, []).append(sorted(t)[len(t) // 2])
    print("  update_outside = %d: one view, %d x %d image, 8^3 grid: %s ms per call" % (outside, W, H, med(t)), flush=True)
    d.free_device(p)
    d.close()
print("  max_sdf resolution (kMax minus none, medians of both rounds): %.4f ms, %.4f ms" % (mid[1][0] - mid[0][0], mid[1][1] - mid[0][1]), flush=True)
