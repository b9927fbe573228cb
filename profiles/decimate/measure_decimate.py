"""Device time of vcy_decimate_mesh (vertex clustering over cells of 2 and of 4 voxels, the three representatives, with and
without the normals of the result) on the iso-surface of the bunny at resolution 2.5 and of the bench scene at 512^3 and
1024^3, next to the wall time of the whole call with its copies, the single-thread wall time of vcy_decimate_mesh_host on
the same input, and a floor from the bytes that must move.
Run from the repository root on the GPU:  python profiles/decimate/measure_decimate.py > profiles/decimate/measure_decimate.txt
Device figures: median of 7 calls after 2 warm-up calls, HIP events around the groups of launches (vcy_last_decimate_ms:
clusters, faces, emit, normals).  "call" is the wall time of the whole call: the uploads of vertices and faces, the launches,
the wait for flags and counts, the normals, the downloads.  "host" is one call of the serial function (median of 3).  Floor:
the input read once (12 B per vertex, 12 B per face), the output written once (12 B per output vertex and face, 4 B per
input vertex for vertex_map, 4 B per output face for face_source, and with normals 12 B more per output vertex and face),
over the measured device copy rate.  The two yardsticks of the issue are printed per line: the device call against the
host function, and the cluster group against the smoothing's table build on the same mesh
(profiles/smooth/measure_smooth.txt: 0.07 / 0.23 / 0.84 ms)."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
MODES = ("mean", "nearest", "first")
SMOOTH_TABLE_MS = {"bunny2.5": 0.068, "512": 0.232, "1024": 0.843}
def mid(x): return sorted(x)[len(x)//2]
def scene(name):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5); views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))); masks = B.load_masks()
    else:
        n = int(name); opt = synth.sphere_option(n); views, masks = synth.sphere_views(n, 16, 640, 480)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    assert d.CarveBatchSilhouettes(views, masks), vc.last_error()
    d.sync()
    return d, opt
print(vc.capi.load().vcy_version().decode(), flush=True)
_, copy_gbs = vc.measure_bandwidth(0, 1 << 30, 3)
print("device copy rate %.0f GB/s (vcy_measure_bandwidth, read + write)" % copy_gbs, flush=True)
for name in ("bunny2.5", "512", "1024"):
    d, opt = scene(name)
    mesh = d.ExtractIsoSurface(0.0, True)
    v, f = mesh["vertices"], mesh["faces"]
    nv, nf = len(v), len(f)
    origin = tuple(opt.bb_min)
    print("%s: dims %s, %d vertices, %d faces" % (name, d.dims, nv, nf), flush=True)
    for cells in (2, 4):
        cell = cells * opt.resolution
        for mode in range(3):
            for normals in (True, False):
                hs = []
                for rep in range(3):
                    t0 = time.perf_counter(); host = vc.decimate_mesh_host(v, f, cell, origin, mode, normals); hs.append((time.perf_counter() - t0) * 1e3)
                ms, wall = {k: [] for k in ("cluster_ms", "faces_ms", "emit_ms", "normals_ms")}, []
                for rep in range(9):
                    t0 = time.perf_counter()
                    got = d.DecimateMesh(v, f, cell, origin, mode, normals)
                    w_ms = (time.perf_counter() - t0) * 1e3
                    if rep >= 2:
                        wall.append(w_ms)
                        for k in ms: ms[k].append(got[k])
                keys = ("vertices", "faces", "vertex_map", "face_source") + (("normals", "face_normals") if normals else ())
                same = all(np.array_equal(got[k].view(np.uint32), host[k].view(np.uint32)) for k in keys)
                nvo, nfo = len(got["vertices"]), len(got["faces"])
                floor_ms = (12 * nv + 12 * nf + 4 * nv + (24 if normals else 12) * (nvo + nfo) + 4 * nfo) / (copy_gbs * 1e9) * 1e3
                dev_ms = sum(mid(ms[k]) for k in ms)
                print("  %d voxels %-7s %s: %d -> %d vertices, %d -> %d faces | cluster %.3f faces %.3f emit %.3f normals %.3f ms, sum %.3f ms, "
                      "floor %.4f ms (%.0fx) | call %.2f ms | host, 1 thread %.1f ms: the call takes %.2f of it (%s) | cluster group / smoothing's "
                      "table build %.1f | device == host %s"
                      % (cells, MODES[mode], "+ normals" if normals else "bare     ", nv, nvo, nf, nfo, mid(ms["cluster_ms"]), mid(ms["faces_ms"]),
                         mid(ms["emit_ms"]), mid(ms["normals_ms"]), dev_ms, floor_ms, dev_ms / floor_ms, mid(wall), mid(hs), mid(wall) / mid(hs),
                         "the device call beats the host function" if mid(wall) < mid(hs) else "THE DEVICE CALL DOES NOT BEAT THE HOST FUNCTION",
                         mid(ms["cluster_ms"]) / SMOOTH_TABLE_MS[name], same), flush=True)
    d.close()
