"""vcy_extract_iso_chain against the separate route (vcy_extract_iso -> vcy_smooth_mesh -> vcy_decimate_mesh[_quadric] with the
normals of the result) on the bunny at resolution 2.5 and on the bench scene at 512^3 and 1024^3, for smooth 10 + MEAN at
2 voxels and smooth 10 + quadric representatives at 2 voxels; and the chain's corner table from the faces ("chainrows" 0)
against from the cells ("chainrows" 1).
Run from the repository root on the GPU:  python profiles/chain/measure_chain.py > profiles/chain/measure_chain.txt
Every figure: median of 7 calls after 2 warm-up calls, all on one context per scene.  "wall" is the wall time of the whole
route on the host (for the separate route: the three calls one after the other, the arrays handed on as they come back).
The chain's stages are vcy_last_chain_ms.  "launches" is the sum of the chain's device stages; "download" the bytes of the
final mesh (vertices, faces, both normals) over the rate at which the Python extraction call delivers its mesh here (the
download and the wrapper's copy; the best of its 7 calls: a call that finds no buffer of its size in the host pool pays
for page-locking as well).  The chain's
calls run with the default "chainrows".  The claim under test is wall ~ launches + download.  The table line gives table_ms
of 7 calls per setting, their median and their spread (max - min), and applies the rule for the default: "chainrows" 1 only
if its median lies below that of 0 by more than the larger of the two spreads, at 512^3 and at 1024^3 both."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
def mid(x): return sorted(x)[len(x)//2]
SMOOTH = dict(iterations=10, lam=0.5, mu=-0.53, pin_boundary=0)
def scene(name):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5); views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))); masks = B.load_masks()
    else:
        n = int(name); opt = synth.sphere_option(n); views, masks = synth.sphere_views(n, 16, 640, 480)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    d.set_param("meshkeys", 0)
    assert d.CarveBatchSilhouettes(views, masks), vc.last_error()
    d.sync()
    return d, opt
def separate(d, dec):
    t0 = time.perf_counter()
    m = d.ExtractIsoSurface(0.0, True)
    t1 = time.perf_counter()
    s = d.SmoothMesh(m["vertices"], m["faces"], SMOOTH["iterations"], SMOOTH["lam"], SMOOTH["mu"], SMOOTH["pin_boundary"])
    t2 = time.perf_counter()
    if "regularize" in dec: r = d.DecimateMeshQuadric(s["vertices"], m["faces"], dec["cell"], None, dec["regularize"], normals=True)
    else: r = d.DecimateMesh(s["vertices"], m["faces"], dec["cell"], None, dec["mode"], normals=True)
    t3 = time.perf_counter()
    return r, [(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t0, t3))]
def chain(d, dec):
    t0 = time.perf_counter()
    r = d.ExtractIsoChain(0.0, True, SMOOTH, dec, normals=True, maps=False)
    return r, (time.perf_counter() - t0) * 1e3
print(vc.capi.load().vcy_version().decode(), flush=True)
rule = {}
for name in ("bunny2.5", "512", "1024"):
    d, opt = scene(name)
    walls = []
    for rep in range(9):
        t0 = time.perf_counter(); mesh = d.ExtractIsoSurface(0.0, True); w = (time.perf_counter() - t0) * 1e3
        if rep >= 2: walls.append((w, mesh["device_ms"]))
    nv, nf = len(mesh["vertices"]), len(mesh["faces"])
    rate = 12.0 * (nv + nf) / (min(w - k for w, k in walls) * 1e-3) / 1e9   # pinned download, GB/s: the best call minus its kernels
    print("%s: dims %s, %d vertices, %d faces; extraction call %.2f ms, kernels %.2f ms: pinned download about %.1f GB/s"
          % (name, d.dims, nv, nf, mid([w for w, _ in walls]), mid([k for _, k in walls]), rate), flush=True)
    for label, dec in (("smooth 10 + MEAN, 2 voxels   ", dict(cell=2 * opt.resolution, mode=0)),
                       ("smooth 10 + quadric, 2 voxels", dict(cell=2 * opt.resolution, regularize=1e-3))):
        sep, ch, st = [], [], {k: [] for k in d.CHAIN_MS}
        for rep in range(9):
            want, ws = separate(d, dec)
            got, wc = chain(d, dec)
            if rep >= 2:
                sep.append(ws); ch.append(wc)
                for k in st: st[k].append(got[k])
        same = all(np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)) for k in ("vertices", "faces", "normals", "face_normals"))
        nvo, nfo = len(got["vertices"]), len(got["faces"])
        launches = sum(mid(st[k]) for k in d.CHAIN_MS[:-1] if k != "quadric_ms")   # (the quadric stage is inside the clusters)
        download = 24.0 * (nvo + nfo) / (rate * 1e9) * 1e3
        s4 = [mid([x[i] for x in sep]) for i in range(4)]
        print("  %s: %d -> %d vertices, %d -> %d faces | separate: extract %.2f + smooth %.2f + decimate %.2f = wall %.2f ms | chain: wall %.2f ms "
              "= %.2f of the separate route (%s) | chain stages: %s | launches %.2f ms + download %.2f ms = %.2f ms: the wall time is %.2f of "
              "that | chain == separate %s"
              % (label, nv, nvo, nf, nfo, s4[0], s4[1], s4[2], s4[3], mid(ch), mid(ch) / s4[3],
                 "the chain beats the separate route" if mid(ch) < s4[3] else "THE CHAIN DOES NOT BEAT THE SEPARATE ROUTE",
                 " ".join("%s %.3f" % (k[:-3], mid(st[k])) for k in d.CHAIN_MS[:-1]), launches, download, launches + download,
                 mid(ch) / (launches + download), same), flush=True)
    # the corner table: from the faces against from the cells, alternating so that neither has the warmer device
    dec = dict(cell=2 * opt.resolution, regularize=1e-3)
    tab = {0: [], 1: []}
    for rep in range(9):
        for rows_ in (0, 1):
            d.set_param("chainrows", rows_)
            got, _ = chain(d, dec)
            if rep >= 2: tab[rows_].append(got["table_ms"])
    d.set_param("chainrows", 1)   # (the default)
    m0, m1 = mid(tab[0]), mid(tab[1])
    spread = max(max(tab[0]) - min(tab[0]), max(tab[1]) - min(tab[1]))
    rule[name] = m0 - m1 > spread
    print("  table (fill, row sort, gather rows): from the faces %s median %.3f ms | from the cells %s median %.3f ms | spread %.3f ms | from "
          "the cells is %s" % (" ".join("%.3f" % x for x in tab[0]), m0, " ".join("%.3f" % x for x in tab[1]), m1, spread,
                               "faster by more than the spread" if rule[name] else "NOT faster by more than the spread"), flush=True)
    d.close()
print('default for "chainrows" by the rule (1 only if faster by more than the spread at 512 and at 1024): %d' % (1 if rule["512"] and rule["1024"] else 0))
