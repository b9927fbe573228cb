"""vcy_decimate_mesh on the GPU: equality with the host function and the numpy restatement over the test matrix, on a
whole-grid and on a z-slab context; reuse of the context's tables and pooled buffers; the error contract; the voxel state
and queued views stay untouched; the device's own extraction, whole and sharded; smoothing then decimation; the timers;
examples/bunny --decimate.  All comparisons are on bits or integers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import color_cases as CC
import decimate_cases as DC
import decimate_ref as DR
import test_decimate_cpu as TD
import test_gpu_render as TR
import test_gpu_smooth as TGS
from vacancy_amd import capi, synth
from vacancy_amd import carver as vc
from vacancy_amd.sharded import ShardedVoxelCarver

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")


def host_result(case, cell, mode):
    """The host function's outputs with normals, computed once per (case, cell, mode)."""
    def make():
        v, f = DC.mesh(case)
        return vc.decimate_mesh_host(v, f, cell, DC.origin_of(case), mode, normals=True)
    return DC.memo(("decimate host", case, cell, mode), make)


def assert_same(got, want, ctx):
    TD.assert_equals(got, want, ctx, (want["normals"], want["face_normals"]))


def check(dev, case, cell, mode, ctx):
    v, f = DC.mesh(case)
    got = dev.DecimateMesh(v, f, cell, DC.origin_of(case), mode, normals=True)
    TD.assert_equals(got, DC.want(case, cell, mode), ctx + " (restatement)")
    assert_same(got, host_result(case, cell, mode), ctx + " (host function)")
    return got


# ---- 1. equality over the matrix ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("z_range", [None, (5, 11)], ids=["whole", "slab"])
@pytest.mark.parametrize("case", DC.CASE_NAMES)
def test_device_equals_host_and_restatement(case, z_range):
    dev = TR.make_dev(CC.option(), CC.DIMS, z_range=z_range)   # (the context only names the device and the stream)
    for cell, mode in DC.matrix():
        check(dev, case, cell, mode, "%s cell %g mode %d" % (case, cell, mode))


def test_calls_in_a_row_on_one_context_agree_with_fresh_calls():
    dev = TR.make_dev(CC.option(), CC.DIMS)
    # a large mesh, a tiny one, a crowded cell, no faces at all, duplicates, the large one again with another cell, a small
    # one: tables and pooled buffers left over from the call before
    calls = (("mc_sphere_40", 2.0), ("octahedron", 0.75), ("crowd", 2.0), ("one_vertex", 2.0), ("two_sheets_same", 2.0),
             ("mc_sphere_40", 3.7), ("257_vertices", 0.75))
    for k, (case, cell) in enumerate(calls):
        mode = DC.MODES[k % 3]
        got = check(dev, case, cell, mode, "call %d %s" % (k, case))
        fresh = TR.make_dev(CC.option(), CC.DIMS)
        v, f = DC.mesh(case)
        assert_same(got, fresh.DecimateMesh(v, f, cell, DC.origin_of(case), mode, normals=True), "call %d %s (fresh context)" % (k, case))
        fresh.close()


# ---- 2. outputs that are not asked for, refusals --------------------------------------------------------------------------

def test_refusals_on_the_device_leave_outputs_and_counts_untouched_and_the_next_call_is_right():
    lib = capi.load()
    dev = TR.make_dev(CC.option(), CC.DIMS)
    check(dev, "mc_sphere", 2.0, DR.NEAREST, "before the refusals")
    for name in sorted(TD.BAD):
        keep, args, out = TD.decimate_args()
        TD.BAD[name](keep, args)
        assert lib.vcy_decimate_mesh(dev.ctx, *args) == capi.VCY_ERR_INVALID_ARG, name
        assert vc.last_error()
        assert TD.untouched(keep, out), name
    for i, value in ((1, (1 << 31) // 3 + 1), (0, 1 << 31)):
        keep, args, out = TD.decimate_args()
        args[i] = value
        assert lib.vcy_decimate_mesh(dev.ctx, *args) == capi.VCY_ERR_UNSUPPORTED
        assert TD.untouched(keep, out)
    for zero in ([0], [1], [0, 1]):
        keep, args, out = TD.decimate_args()
        for i in zero:
            args[i] = 0
        assert lib.vcy_decimate_mesh(dev.ctx, *args) == 0
        assert all(np.all(o == 77) for o in out.values()) and keep[3][0].value == 0 and keep[3][1].value == 0
    check(dev, "mc_sphere", 2.0, DR.NEAREST, "after the refusals")
    check(dev, "crowd", 2.0, DR.MEAN, "after the refusals")


def test_null_outputs_and_the_timers():
    lib = capi.load()
    dev = TR.make_dev(CC.option(), CC.DIMS)
    want = host_result("mc_sphere", 2.0, DR.NEAREST)
    nv, nf = len(want["vertices"]), len(want["faces"])
    ms = [C.c_float(-1.0) for _ in range(4)]
    keep, args, out = TD.decimate_args()
    assert lib.vcy_decimate_mesh(dev.ctx, *args) == 0, vc.last_error()
    assert lib.vcy_last_decimate_ms(dev.ctx, *[C.byref(m) for m in ms]) == 0
    assert all(m.value > 0.0 for m in ms), [m.value for m in ms]
    assert (keep[3][0].value, keep[3][1].value) == (nv, nf)
    assert np.all(out["vertices"][nv:] == 77) and np.all(out["faces"][nf:] == 77) and np.all(out["normals"][nv:] == 77)
    keep, args, out = TD.decimate_args()
    args[9] = args[10] = args[11] = args[12] = None
    assert lib.vcy_decimate_mesh(dev.ctx, *args) == 0, vc.last_error()
    DC.assert_bits(out["vertices"][:nv], want["vertices"], "bare")
    assert np.array_equal(out["faces"][:nf], want["faces"])
    assert all(np.all(out[k] == 77) for k in ("vertex_map", "face_source", "normals", "face_normals"))
    assert lib.vcy_last_decimate_ms(dev.ctx, *[C.byref(m) for m in ms]) == 0
    assert ms[0].value > 0.0 and ms[1].value > 0.0 and ms[2].value > 0.0 and ms[3].value == 0.0
    keep, args, out = TD.decimate_args()
    args[12] = None                                      # vertex normals alone
    assert lib.vcy_decimate_mesh(dev.ctx, *args) == 0, vc.last_error()
    DC.assert_normals(out["normals"][:nv], want["normals"], "vertex normals alone")
    assert np.all(out["face_normals"] == 77) and np.array_equal(out["vertex_map"], want["vertex_map"])
    keep, args, out = TD.decimate_args()
    args[11] = None                                      # face normals alone
    assert lib.vcy_decimate_mesh(dev.ctx, *args) == 0, vc.last_error()
    DC.assert_normals(out["face_normals"][:nf], want["face_normals"], "face normals alone")
    assert np.all(out["normals"] == 77) and np.array_equal(out["face_source"][:nf], want["face_source"])


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
    v, f = DC.mesh("mc_sphere")
    dev.DecimateMesh(v, f, 2.0, DC.ORIGIN, DR.MEAN, normals=True)
    got = dev.DecimateMesh(before["vertices"], before["faces"], 2.0, normals=True)          # the origin: bb_min
    want = vc.decimate_mesh_host(before["vertices"], before["faces"], 2.0, tuple(opt.bb_min), normals=True)
    assert_same(got, want, "own mesh")
    assert 0 < len(got["vertices"]) < len(before["vertices"])
    assert dev.state_diff(twin) == 0
    a, b = dev.ExtractIsoSurface(0.0, True), twin.ExtractIsoSurface(0.0, True)
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(DC.bits(a["vertices"]), DC.bits(b["vertices"]))
    assert len(a["vertices"]) != len(before["vertices"])                    # the queued view was applied after all
    dev.DecimateMesh(a["vertices"], a["faces"], 3.0, mode=DR.FIRST)
    c = dev.ExtractIsoSurface(0.0, True)
    assert np.array_equal(a["faces"], c["faces"]) and np.array_equal(DC.bits(a["vertices"]), DC.bits(c["vertices"]))
    assert dev.state_diff(twin) == 0


# ---- 4. the device's own extraction, whole and sharded; smoothing first --------------------------------------------------

def test_smoke_scene_extraction_whole_and_sharded():
    opt, views, masks, mesh, smoothed = TGS.smoke_scene()
    assert len(mesh["vertices"]) > 2000
    dev = TR.make_dev(opt)
    origin = tuple(opt.bb_min)
    for mode in DC.MODES:
        got = dev.DecimateMesh(mesh["vertices"], mesh["faces"], 2.0 * opt.resolution, mode=mode, normals=True)
        assert_same(got, vc.decimate_mesh_host(mesh["vertices"], mesh["faces"], 2.0 * opt.resolution, origin, mode, normals=True),
                    "smoke scene mode %d" % mode)
        assert 0 < len(got["vertices"]) < len(mesh["vertices"]) // 2 and 0 < len(got["faces"]) < len(mesh["faces"]) // 2
        assert all(got[k] > 0.0 for k in ("cluster_ms", "faces_ms", "emit_ms", "normals_ms"))
    bare = dev.DecimateMesh(mesh["vertices"], mesh["faces"], 2.0 * opt.resolution)
    assert bare["normals_ms"] == 0.0 and bare["cluster_ms"] > 0.0 and "normals" not in bare
    sh = ShardedVoxelCarver(opt, [0], slabs_per_device=2)
    assert sh.Init()
    assert sh.CarveBatchSilhouettes(views, masks), vc.last_error()
    merged = sh.ExtractIsoSurface(0.0, True)
    assert np.array_equal(merged["faces"], mesh["faces"]) and np.array_equal(DC.bits(merged["vertices"]), DC.bits(mesh["vertices"]))
    part = sh.DecimateMesh(merged["vertices"], merged["faces"], 2.0 * opt.resolution, mode=DR.NEAREST, normals=True)
    assert_same(part, dev.DecimateMesh(mesh["vertices"], mesh["faces"], 2.0 * opt.resolution, mode=DR.NEAREST, normals=True), "sharded")
    assert all(part[k] > 0.0 for k in ("cluster_ms", "faces_ms", "emit_ms", "normals_ms"))
    sh.close()
    dev.close()


def test_smooth_then_decimate_equals_the_host_functions_composed():
    opt, views, masks, mesh, smoothed = TGS.smoke_scene()
    dev = TR.make_dev(opt)
    sm = dev.SmoothMesh(mesh["vertices"], mesh["faces"], 3)
    got = dev.DecimateMesh(sm["vertices"], mesh["faces"], 2.5, mode=DR.MEAN, normals=True)
    again = dev.SmoothMesh(mesh["vertices"], mesh["faces"], 3)             # a decimation between two smoothings disturbs neither
    hs = vc.smooth_mesh_host(mesh["vertices"], mesh["faces"], 3, 0.5, -0.53)
    want = vc.decimate_mesh_host(hs["vertices"], mesh["faces"], 2.5, tuple(opt.bb_min), DR.MEAN, normals=True)
    assert_same(got, want, "smooth then decimate")
    DC.assert_bits(again["vertices"], hs["vertices"], "smoothing after a decimation")
    dev.close()


# ---- 5. the C++ layer ----------------------------------------------------------------------------------------------------

def test_bunny_example_decimates_what_python_decimates(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "2", "--decimate", "2"],
                         check=True, capture_output=True, text=True)
    row = [l.split() for l in run.stdout.splitlines() if l.startswith("DECIMATE ")]
    assert len(row) == 1 and row[0][1:5] == ["cell", "20", "mode", "mean"] and row[0][5] == "vertices" and row[0][9] == "faces", run.stdout
    shard = [l.split() for l in run.stdout.splitlines() if l.startswith("DECIMATESHARDED")]
    assert len(shard) == 1 and shard[0][1:3] == ["slabs", "2"] and shard[0][-2:] == ["identical", "1"], run.stdout
    verts, normals, faces = TGS.read_binary_ply(str(tmp_path / "surface_decimated.ply"))

    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    dev = vc.VoxelCarver(B.bunny_option(10.0))
    assert dev.Init(), vc.last_error()
    for v, m in zip(views, B.load_masks()):
        assert dev.CarveSilhouette(v, m), vc.last_error()
    mesh = dev.ExtractIsoSurface(0.0, True)
    got = dev.DecimateMesh(mesh["vertices"], mesh["faces"], 20.0, normals=True)
    assert [int(row[0][k]) for k in (6, 8, 10, 12)] == [len(mesh["vertices"]), len(verts), len(mesh["faces"]), len(faces)]
    assert row[0][7] == "->" and row[0][11] == "->"
    assert 100 < len(verts) == len(got["vertices"]) < len(mesh["vertices"]) and np.array_equal(faces, got["faces"])
    DC.assert_bits(verts, got["vertices"], "the example's vertices")
    DC.assert_normals(normals, got["normals"], "the example's normals")

    for extra in (["--decimate"], ["--decimate", "0"], ["--decimate", "-1"]):
        bad = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10"] + extra, capture_output=True, text=True)
        assert bad.returncode == 10 and "--decimate needs a" in bad.stderr and "number" in bad.stderr, (extra, bad.stderr)
