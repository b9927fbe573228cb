"""vcy_decimate_mesh_quadric on the GPU: equality with the host function and the numpy restatement over every case, on a
whole-grid and on a z-slab context; reuse of the context's tables and pooled buffers, MEAN calls in between; the error
contract; the voxel state and queued views stay untouched; the device's own extraction, whole and sharded; the timers;
examples/bunny --decimate-mode quadric.  All comparisons are on bits or integers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import color_cases as CC
import decimate_ref as DR
import quadric_cases as QC
import test_decimate_cpu as TD
import test_gpu_render as TR
import test_gpu_smooth as TGS
import test_quadric_cpu as TQ
from vacancy_amd import capi, synth
from vacancy_amd import carver as vc
from vacancy_amd.sharded import ShardedVoxelCarver

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")


def assert_same(got, want, ctx):
    TQ.assert_equals(got, want, ctx, (want["normals"], want["face_normals"]))


def check(dev, case, cell, reg, ctx):
    v, f = QC.mesh(case)
    got = dev.DecimateMeshQuadric(v, f, cell, QC.origin_of(case), reg, normals=True)
    TQ.assert_equals(got, QC.want(case, cell, reg), ctx + " (restatement)")
    assert_same(got, TQ.host(case, cell, reg), ctx + " (host function)")
    return got


# ---- 1. equality over the cases -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("z_range", [None, (5, 11)], ids=["whole", "slab"])
@pytest.mark.parametrize("case", QC.CASE_NAMES)
def test_device_equals_host_and_restatement(case, z_range):
    dev = TR.make_dev(CC.option(), CC.DIMS, z_range=z_range)   # (the context only names the device and the stream)
    for cell, reg in QC.matrix(case):
        check(dev, case, cell, reg, "%s cell %g regularize %g" % (case, cell, reg))
    if case in ("mc_sphere", "box"):
        cell = QC.cells_of(case)[-1] if case in QC.OWN else 2.0
        check(dev, case, cell, 1.0, case + " regularize 1")


def test_calls_in_a_row_on_one_context_agree_with_fresh_calls():
    dev = TR.make_dev(CC.option(), CC.DIMS)
    # a large mesh, a crowded cell, a tiny mesh: tables, pooled buffers, vertex quadrics and fallback flags left over from
    # the call before; a MEAN call of the old entry point between them
    calls = (("mc_sphere_40", 2.0, 1e-3), ("crowd", 2.0, 0.0), ("octahedron", 0.75, 1e-3))
    for k, (case, cell, reg) in enumerate(calls):
        got = check(dev, case, cell, reg, "call %d %s" % (k, case))
        fresh = TR.make_dev(CC.option(), CC.DIMS)
        v, f = QC.mesh(case)
        assert_same(got, fresh.DecimateMeshQuadric(v, f, cell, QC.origin_of(case), reg, normals=True), "call %d %s (fresh context)" % (k, case))
        fresh.close()
        mean = dev.DecimateMesh(v, f, cell, QC.origin_of(case), DR.MEAN, normals=True)
        want = vc.decimate_mesh_host(v, f, cell, QC.origin_of(case), DR.MEAN, normals=True)
        TD.assert_equals(mean, want, "MEAN behind call %d" % k, (want["normals"], want["face_normals"]))


# ---- 2. outputs that are not asked for, refusals, the timers -------------------------------------------------------------

def test_refusals_on_the_device_leave_every_output_untouched_and_the_next_call_is_right():
    lib = capi.load()
    dev = TR.make_dev(CC.option(), CC.DIMS)
    check(dev, "mc_sphere", 2.0, 1e-3, "before the refusals")
    seen = set()
    for name, qargs, keep, out, n_fallback in TQ.refusals():
        assert lib.vcy_decimate_mesh_quadric(dev.ctx, *qargs) == capi.VCY_ERR_INVALID_ARG, name
        assert vc.last_error(), name
        assert TD.untouched(keep, out) and n_fallback.value == -1, name
        seen.add(name)
        if name in ("face index -1", "face index n", "vertex nan", "vertex inf"):     # found on the device
            check(dev, "mc_sphere", 2.0, 1e-3, "behind " + name)
    assert {"face index -1", "face index n", "too few vertices", "vertex nan", "vertex inf"} <= seen
    for i, value in ((1, (1 << 31) // 3 + 1), (0, 1 << 31)):
        keep, args, out = TQ.quadric_args()
        args[i] = value
        qargs, n_fallback = TQ.finish(args)
        assert lib.vcy_decimate_mesh_quadric(dev.ctx, *qargs) == capi.VCY_ERR_UNSUPPORTED
        assert TD.untouched(keep, out) and n_fallback.value == -1
    check(dev, "crowd", 2.0, 1e-3, "after the refusals")


def test_null_outputs_and_the_timers():
    lib = capi.load()
    dev = TR.make_dev(CC.option(), CC.DIMS)
    want = TQ.host("mc_sphere", 2.0, 1e-3)
    nv, nf = len(want["vertices"]), len(want["faces"])
    ms = [C.c_float(-1.0) for _ in range(4)]
    qms = C.c_float(-1.0)
    keep, args, out = TQ.quadric_args()
    qargs, n_fallback = TQ.finish(args)
    assert lib.vcy_decimate_mesh_quadric(dev.ctx, *qargs) == 0, vc.last_error()
    assert lib.vcy_last_decimate_ms(dev.ctx, *[C.byref(m) for m in ms]) == 0 and lib.vcy_last_quadric_ms(dev.ctx, C.byref(qms)) == 0
    assert all(m.value > 0.0 for m in ms), [m.value for m in ms]
    assert 0.0 < qms.value < ms[0].value                 # the stage lies inside "clusters"
    assert (keep[3][0].value, keep[3][1].value, n_fallback.value) == (nv, nf, want["n_fallback"])
    assert np.all(out["vertices"][nv:] == 77) and np.all(out["faces"][nf:] == 77) and np.all(out["normals"][nv:] == 77)
    keep, args, out = TQ.quadric_args()
    args[9] = args[10] = args[11] = args[12] = None
    qargs, n_fallback = TQ.finish(args)
    qargs[-1] = None
    assert lib.vcy_decimate_mesh_quadric(dev.ctx, *qargs) == 0, vc.last_error()
    QC.DC.assert_bits(out["vertices"][:nv], want["vertices"], "bare")
    assert np.array_equal(out["faces"][:nf], want["faces"])
    assert all(np.all(out[k] == 77) for k in ("vertex_map", "face_source", "normals", "face_normals")) and n_fallback.value == -1
    assert lib.vcy_last_decimate_ms(dev.ctx, *[C.byref(m) for m in ms]) == 0 and lib.vcy_last_quadric_ms(dev.ctx, C.byref(qms)) == 0
    assert ms[0].value > 0.0 and ms[1].value > 0.0 and ms[2].value > 0.0 and ms[3].value == 0.0 and qms.value > 0.0
    for key, drop in (("normals", 12), ("face_normals", 11)):           # either kind of normals alone
        keep, args, out = TQ.quadric_args()
        args[drop] = None
        qargs, n_fallback = TQ.finish(args)
        assert lib.vcy_decimate_mesh_quadric(dev.ctx, *qargs) == 0, vc.last_error()
        n = nv if key == "normals" else nf
        QC.DC.assert_normals(out[key][:n], want[key], key + " alone")
        assert np.array_equal(out["vertex_map"], want["vertex_map"]) and n_fallback.value == want["n_fallback"]
    for zero in ([0], [1], [0, 1]):                              # nothing to do: the three counts and the timers 0
        keep, args, out = TQ.quadric_args()
        for i in zero:
            args[i] = 0
        qargs, n_fallback = TQ.finish(args)
        assert lib.vcy_decimate_mesh_quadric(dev.ctx, *qargs) == 0
        assert all(np.all(o == 77) for o in out.values()) and keep[3][0].value == 0 and keep[3][1].value == 0 and n_fallback.value == 0
        assert lib.vcy_last_quadric_ms(dev.ctx, C.byref(qms)) == 0 and qms.value == 0.0
        assert lib.vcy_last_decimate_ms(dev.ctx, *[C.byref(m) for m in ms]) == 0 and all(m.value == 0.0 for m in ms)
    got = dev.DecimateMeshQuadric(*QC.mesh("one_vertex"), 2.0)
    assert len(got["vertices"]) == 0 and got["n_fallback"] == 0 and got["quadric_ms"] == 0.0


# ---- 3. the voxel state, queued views and the extraction stay as they were -----------------------------------------------

def test_state_and_queued_views_stay_untouched():
    n = 32
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, 4, 160, 120)
    dev, twin = TR.make_dev(opt), TR.make_dev(opt)
    for c in (dev, twin):
        for v, m in zip(views[:3], masks[:3]):
            assert c.CarveSilhouette(v, m), vc.last_error()
    before = dev.ExtractIsoSurface(0.0, True)
    assert len(before["vertices"]) > 500
    for c in (dev, twin):
        assert c.CarveSilhouette(views[3], masks[3]), vc.last_error()     # queued, not applied yet
    v, f = QC.mesh("mc_sphere")
    dev.DecimateMeshQuadric(v, f, 2.0, QC.DC.ORIGIN, normals=True)
    got = dev.DecimateMeshQuadric(before["vertices"], before["faces"], 2.0, normals=True)          # the origin: bb_min
    want = vc.decimate_mesh_quadric_host(before["vertices"], before["faces"], 2.0, tuple(opt.bb_min), normals=True)
    assert_same(got, want, "own mesh")
    assert 0 < len(got["vertices"]) < len(before["vertices"]) and got["n_fallback"] < len(got["vertices"])
    assert dev.state_diff(twin) == 0
    a, b = dev.ExtractIsoSurface(0.0, True), twin.ExtractIsoSurface(0.0, True)
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(QC.bits(a["vertices"]), QC.bits(b["vertices"]))
    assert len(a["vertices"]) != len(before["vertices"])                    # the queued view was applied after all
    dev.DecimateMeshQuadric(a["vertices"], a["faces"], 3.0, regularize=0.0)
    c = dev.ExtractIsoSurface(0.0, True)
    assert np.array_equal(a["faces"], c["faces"]) and np.array_equal(QC.bits(a["vertices"]), QC.bits(c["vertices"]))
    assert dev.state_diff(twin) == 0


# ---- 4. the device's own extraction, whole and sharded --------------------------------------------------------------------

def test_smoke_scene_extraction_whole_and_sharded():
    opt, views, masks, mesh, smoothed = TGS.smoke_scene()
    assert len(mesh["vertices"]) > 2000
    dev = TR.make_dev(opt)
    origin = tuple(opt.bb_min)
    cell = 2.0 * opt.resolution
    want = vc.decimate_mesh_quadric_host(mesh["vertices"], mesh["faces"], cell, origin, normals=True)
    got = dev.DecimateMeshQuadric(mesh["vertices"], mesh["faces"], cell, normals=True)
    assert_same(got, want, "smoke scene")
    assert 0 < len(got["vertices"]) < len(mesh["vertices"]) // 2 and 0 < len(got["faces"]) < len(mesh["faces"]) // 2
    assert got["n_fallback"] < len(got["vertices"]) // 2
    assert all(got[k] > 0.0 for k in ("cluster_ms", "faces_ms", "emit_ms", "normals_ms", "quadric_ms"))
    sh = ShardedVoxelCarver(opt, [0], slabs_per_device=2)
    assert sh.Init()
    assert sh.CarveBatchSilhouettes(views, masks), vc.last_error()
    merged = sh.ExtractIsoSurface(0.0, True)
    assert np.array_equal(merged["faces"], mesh["faces"]) and np.array_equal(QC.bits(merged["vertices"]), QC.bits(mesh["vertices"]))
    part = sh.DecimateMeshQuadric(merged["vertices"], merged["faces"], cell, normals=True)
    assert_same(part, want, "sharded")
    assert part["quadric_ms"] > 0.0
    sh.close()
    dev.close()


# ---- 5. the C++ layer ----------------------------------------------------------------------------------------------------

def test_bunny_example_decimates_what_python_decimates(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "2", "--decimate", "2", "--decimate-mode", "quadric",
                          "--quadric-reg", "0.01"], check=True, capture_output=True, text=True)
    row = [l.split() for l in run.stdout.splitlines() if l.startswith("DECIMATE ")]
    assert len(row) == 1 and row[0][1:5] == ["cell", "20", "mode", "quadric"] and row[0][5] == "vertices" and row[0][9] == "faces", run.stdout
    shard = [l.split() for l in run.stdout.splitlines() if l.startswith("DECIMATESHARDED")]
    assert len(shard) == 1 and shard[0][1:3] == ["slabs", "2"] and shard[0][-2:] == ["identical", "1"], run.stdout
    verts, normals, faces = TGS.read_binary_ply(str(tmp_path / "surface_decimated.ply"))

    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    dev = vc.VoxelCarver(B.bunny_option(10.0))
    assert dev.Init(), vc.last_error()
    for v, m in zip(views, B.load_masks()):
        assert dev.CarveSilhouette(v, m), vc.last_error()
    mesh = dev.ExtractIsoSurface(0.0, True)
    got = dev.DecimateMeshQuadric(mesh["vertices"], mesh["faces"], 20.0, regularize=0.01, normals=True)
    assert [int(row[0][k]) for k in (6, 8, 10, 12)] == [len(mesh["vertices"]), len(verts), len(mesh["faces"]), len(faces)]
    assert row[0][13] == "fallback" and int(row[0][14]) == got["n_fallback"] < len(verts), row[0]
    assert 100 < len(verts) == len(got["vertices"]) < len(mesh["vertices"]) and np.array_equal(faces, got["faces"])
    QC.DC.assert_bits(verts, got["vertices"], "the example's vertices")
    QC.DC.assert_normals(normals, got["normals"], "the example's normals")
    mean = dev.DecimateMesh(mesh["vertices"], mesh["faces"], 20.0)
    assert not np.array_equal(QC.bits(mean["vertices"]), QC.bits(got["vertices"]))

    for extra in (["--decimate-mode", "quadratic"], ["--quadric-reg", "2"], ["--quadric-reg"], ["--decimate-mode", "mean", "--quadric-reg", "0.1"]):
        bad = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "--decimate", "2"] + extra, capture_output=True, text=True)
        assert bad.returncode == 10, (extra, bad.returncode, bad.stderr)
