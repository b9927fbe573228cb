"""Device time of vcy_decimate_mesh_quadric (vertex clustering over cells of 2 and of 4 voxels, quadric-error
representatives at regularize 1e-3, with the normals of the result) on the iso-surface of the bunny at resolution 2.5 and of
the bench scene at 512^3 and 1024^3 -- the meshes of profiles/decimate/measure_decimate.py -- next to the MEAN call of
vcy_decimate_mesh on the same input, the wall time of the whole call with its copies, the single-thread wall time of
vcy_decimate_mesh_quadric_host, and a floor for the quadric stage from the bytes that must move.
Run from the repository root on the GPU:  python profiles/quadric/measure_quadric.py > profiles/quadric/measure_quadric.txt
and, for the yardstick, from the root of a checkout of the parent commit with this file's path:  python <this file> --mean-only
(the MEAN lines alone: that tree has no quadric entry points).
Device figures: median of 7 calls after 2 warm-up calls, HIP events around the groups of launches (vcy_last_decimate_ms:
clusters, faces, emit, normals; vcy_last_quadric_ms: the quadric stage, which is part of "clusters").  "call" is the wall time
of the whole call: the uploads, the launches, the wait for flags and counts, the normals, the downloads.  "host" is one call
of the serial function (median of 3).  Floor of the stage: the vertex quadrics written once and read once (2 x 72 B per
vertex), the faces' indices and the positions read once (12 B per face, 12 B per vertex), over the measured device copy
rate."""
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import carver as vc, synth
import bunny_data as B
MEAN_ONLY = "--mean-only" in sys.argv
GROUPS = ("cluster_ms", "faces_ms", "emit_ms", "normals_ms")
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
def timed(call, keys):
    ms, wall, got = {k: [] for k in keys}, [], None
    for rep in range(9):
        t0 = time.perf_counter()
        got = call()
        w_ms = (time.perf_counter() - t0) * 1e3
        if rep >= 2:
            wall.append(w_ms)
            for k in ms: ms[k].append(got[k])
    return {k: mid(ms[k]) for k in ms}, mid(wall), got
print(vc.capi.load().vcy_version().decode(), "(MEAN only: the yardstick)" if MEAN_ONLY else "", flush=True)
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
        m_ms, m_wall, m_got = timed(lambda: d.DecimateMesh(v, f, cell, origin, 0, True), GROUPS)
        m_sum = sum(m_ms.values())
        print("  %d voxels mean    + normals: %d -> %d vertices, %d -> %d faces | cluster %.3f faces %.3f emit %.3f normals %.3f ms, sum %.3f ms | "
              "call %.2f ms" % (cells, nv, len(m_got["vertices"]), nf, len(m_got["faces"]), m_ms["cluster_ms"], m_ms["faces_ms"], m_ms["emit_ms"],
                                m_ms["normals_ms"], m_sum, m_wall), flush=True)
        if MEAN_ONLY:
            continue
        hs = []
        for rep in range(3):
            t0 = time.perf_counter(); host = vc.decimate_mesh_quadric_host(v, f, cell, origin, 1e-3, True); hs.append((time.perf_counter() - t0) * 1e3)
        q_ms, q_wall, got = timed(lambda: d.DecimateMeshQuadric(v, f, cell, origin, 1e-3, True), GROUPS + ("quadric_ms",))
        keys = ("vertices", "faces", "vertex_map", "face_source", "normals", "face_normals")
        same = all(np.array_equal(got[k].view(np.uint32), host[k].view(np.uint32)) for k in keys) and got["n_fallback"] == host["n_fallback"]
        q_sum = sum(q_ms[k] for k in GROUPS)
        floor_ms = (144 * nv + 12 * nf + 12 * nv) / (copy_gbs * 1e9) * 1e3
        print("  %d voxels quadric + normals: %d -> %d vertices, %d kept the mean | quadric stage %.3f ms, floor %.4f ms (%.0fx) | cluster %.3f faces "
              "%.3f emit %.3f normals %.3f ms, sum %.3f ms: %.2f of MEAN's launches | call %.2f ms: %.2f of MEAN's call | host, 1 thread %.1f ms: "
              "the call takes %.2f of it (%s) | device == host %s"
              % (cells, nv, len(got["vertices"]), got["n_fallback"], q_ms["quadric_ms"], floor_ms, q_ms["quadric_ms"] / floor_ms, q_ms["cluster_ms"],
                 q_ms["faces_ms"], q_ms["emit_ms"], q_ms["normals_ms"], q_sum, q_sum / m_sum, q_wall, q_wall / m_wall, mid(hs), q_wall / mid(hs),
                 "the device call beats the host function" if q_wall < mid(hs) else "THE DEVICE CALL DOES NOT BEAT THE HOST FUNCTION", same),
              flush=True)
    d.close()
