"""Device time of vcy_smooth_mesh (10 Taubin iterations = 20 passes, normals of the result) on the iso-surface of the bunny
at resolution 2.5 and of the bench scene at 512^3 and 1024^3, with the positions of the passes at 12 and at 16 bytes
("smoothpad" 0 / 1), next to the wall time of the whole call with its copies, the single-thread wall time of
vcy_mesh_normals_host (the only general-mesh walk the library had before) and of vcy_smooth_mesh_host on the same mesh, and a
floor of one pass from the bytes that must move.
Run from the repository root on the GPU:  python profiles/smooth/measure_smooth.py > profiles/smooth/measure_smooth.txt
Device figures: median [min..max] of 7 calls after 2 warm-up calls, HIP events around the three groups of launches
(vcy_last_smooth_ms: incidence table, passes, normals).  "call" is the wall time of the whole call: the check of the face
indices on the host, the uploads of vertices and faces, the launches, the downloads of vertices and normals.  Floor of one
pass: positions in and out (12 or 16 B per vertex each), the gather-row ids (4 B each, 6 per face), the row offsets (4 B per
vertex) and the pinned flags (1 B per vertex) once, over the measured device copy rate."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
IT = 10
def med(x): x = sorted(x); return "%.3f [%.3f..%.3f]" % (x[len(x)//2], x[0], x[-1])
def mid(x): return sorted(x)[len(x)//2]
def scene(name):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5); views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))); masks = B.load_masks()
    else:
        n = int(name); opt = synth.sphere_option(n); views, masks = synth.sphere_views(n, 16, 640, 480)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    assert d.CarveBatchSilhouettes(views, masks), vc.last_error()
    d.sync()
    return d
print(vc.capi.load().vcy_version().decode(), flush=True)
_, copy_gbs = vc.measure_bandwidth(0, 1 << 30, 3)
print("device copy rate %.0f GB/s (vcy_measure_bandwidth, read + write)" % copy_gbs, flush=True)
for name in ("bunny2.5", "512", "1024"):
    d = scene(name)
    mesh = d.ExtractIsoSurface(0.0, True)
    v, f = mesh["vertices"], mesh["faces"]
    nv, nf = len(v), len(f)
    hn = []
    for rep in range(3):
        t0 = time.perf_counter(); vc.mesh_normals_host(v, f); hn.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter(); host = vc.smooth_mesh_host(v, f, IT, 0.5, -0.53, False, True); host_ms = (time.perf_counter() - t0) * 1e3
    print("%s: dims %s, %d vertices, %d faces | vcy_mesh_normals_host, 1 thread %s ms | vcy_smooth_mesh_host, %d iterations + normals, 1 thread %.0f ms"
          % (name, d.dims, nv, nf, med(hn), IT, host_ms), flush=True)
    for pad in (0, 1):
        d.set_param("smoothpad", pad)
        b, p, n, wall = [], [], [], []
        for rep in range(9):
            t0 = time.perf_counter()
            got = d.SmoothMesh(v, f, IT, 0.5, -0.53, False, True)
            w_ms = (time.perf_counter() - t0) * 1e3
            if rep >= 2: b.append(got["build_ms"]); p.append(got["passes_ms"]); n.append(got["normals_ms"]); wall.append(w_ms)
        same = all(np.array_equal(got[k].view(np.uint32), host[k].view(np.uint32)) for k in ("vertices", "normals", "face_normals"))
        per_pass = mid(p) / (2 * IT)
        pos = 16 if pad else 12
        floor_ms = (nv * (2 * pos + 4 + 1) + nf * 6 * 4) / (copy_gbs * 1e9) * 1e3
        dev_ms = mid(b) + mid(p) + mid(n)
        print("  positions %2d B: table %s ms | %d passes %s ms = %.4f ms per pass, floor %.4f ms (%.1fx) | normals %s ms | call %s ms, "
              "%.0f %% of it outside the launches | device == host %s"
              % (pos, med(b), 2 * IT, med(p), per_pass, floor_ms, per_pass / floor_ms, med(n), med(wall),
                 100.0 * (1.0 - dev_ms / mid(wall)), same), flush=True)
        print("    expectation 1 (a pass within 3.3x its byte floor): %s" % ("holds" if per_pass <= 3.3 * floor_ms else
              "does not hold, by %.1fx" % (per_pass / (3.3 * floor_ms))), flush=True)
        print("    expectation 2 (the whole call under one vcy_mesh_normals_host walk, %.1f ms): %s" % (mid(hn), "holds" if mid(wall) < mid(hn)
              else "does not hold, by %.1fx" % (mid(wall) / mid(hn))), flush=True)
    d.close()
