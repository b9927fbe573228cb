"""vcy_smooth_mesh on the GPU: bit equality with the host function and the numpy restatement over the test matrix, on a
whole-grid and on a z-slab context; reuse of the context's pooled buffers; the error contract; the voxel state and queued
views stay untouched; the device's own extraction, whole and sharded; the timers; examples/bunny --smooth."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import color_cases as CC
import smooth_cases as SC
import test_gpu_render as TR
import test_smooth_cpu as TS
from vacancy_amd import capi, synth
from vacancy_amd import carver as vc
from vacancy_amd.sharded import ShardedVoxelCarver

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")
TAUBIN = (0.5, -0.53)


def check(dev, case, it, factors, pin, ctx):
    v, f = SC.mesh(case)
    got = dev.SmoothMesh(v, f, it, factors[0], factors[1], pin, normals=True)
    SC.assert_bits(got["vertices"], SC.want(case, it, factors, pin), ctx + " (restatement)")
    host = vc.smooth_mesh_host(v, f, it, factors[0], factors[1], pin, normals=True)
    SC.assert_bits(got["vertices"], host["vertices"], ctx + " (host function)")
    SC.assert_normals(got["normals"], host["normals"], ctx + " (vertex normals)")
    SC.assert_normals(got["face_normals"], host["face_normals"], ctx + " (face normals)")
    return got


# ---- 1. bit equality over the matrix -----------------------------------------------------------------------------------

@pytest.mark.parametrize("z_range", [None, (5, 11)], ids=["whole", "slab"])
@pytest.mark.parametrize("case", SC.CASE_NAMES)
def test_device_equals_host_and_restatement(case, z_range):
    dev = TR.make_dev(CC.option(), CC.DIMS, z_range=z_range)   # (the context only names the device and the stream)
    for it, factors, pin in SC.matrix():                        # iterations 0, 1, 2, 7: both ends of the ping-pong
        check(dev, case, it, factors, pin, "%s it %d factors %s pin %d" % (case, it, factors, pin))
    dev.set_param("smoothpad", 1)                               # positions of the passes at 16 bytes: the same bits
    for it in (0, 1, 7):
        for pin in SC.PINS:
            check(dev, case, it, TAUBIN, pin, "%s it %d pin %d padded" % (case, it, pin))


def test_calls_in_a_row_on_one_context_agree_with_fresh_calls():
    dev = TR.make_dev(CC.option(), CC.DIMS)
    # a large mesh, a tiny one, a long row, no faces at all, the large one again: pooled buffers and rows left over
    for k, case in enumerate(("mc_sphere", "octahedron", "fan300", "one_vertex", "degenerate", "mc_sphere", "257_vertices")):
        check(dev, case, 1 + (k % 2), TAUBIN, k % 2, "call %d %s" % (k, case))


# ---- 2. outputs that are not asked for, refusals ----------------------------------------------------------------------------

def test_null_normals_empty_input_and_refusals_on_the_device():
    lib = capi.load()
    dev = TR.make_dev(CC.option(), CC.DIMS)
    want = SC.want("mc_sphere", 2, TAUBIN, 1)
    keep, args, out = TS.smooth_args()
    args[6] = args[7] = None
    assert lib.vcy_smooth_mesh(dev.ctx, *args) == 0, vc.last_error()
    SC.assert_bits(out["vertices"], want, "no normals")
    assert np.all(out["normals"] == 77) and np.all(out["face_normals"] == 77)
    ms = [C.c_float(-1.0) for _ in range(3)]
    assert lib.vcy_last_smooth_ms(dev.ctx, *[C.byref(m) for m in ms]) == 0
    assert ms[0].value > 0.0 and ms[1].value > 0.0 and ms[2].value == 0.0
    keep, args, out = TS.smooth_args()
    args[7] = None                                       # vertex normals alone
    assert lib.vcy_smooth_mesh(dev.ctx, *args) == 0, vc.last_error()
    SC.assert_normals(out["normals"], vc.mesh_normals_host(want, keep[1])[0], "vertex normals alone")
    assert np.all(out["face_normals"] == 77)
    keep, args, out = TS.smooth_args()
    buf = np.array(keep[0], F)                           # in place
    args[2] = args[5] = vc._p(buf)
    assert lib.vcy_smooth_mesh(dev.ctx, *args) == 0, vc.last_error()
    SC.assert_bits(buf, want, "in place")
    keep, args, out = TS.smooth_args()
    args[0] = args[1] = 0
    assert lib.vcy_smooth_mesh(dev.ctx, *args) == 0
    assert all(np.all(o == 77) for o in out.values())
    for name in sorted(TS.BAD):
        keep, args, out = TS.smooth_args()
        TS.BAD[name](keep, args)
        assert lib.vcy_smooth_mesh(dev.ctx, *args) == capi.VCY_ERR_INVALID_ARG, name
        assert all(np.all(o == 77) for o in out.values()), name
    keep, args, out = TS.smooth_args()
    args[1] = (1 << 31) // 3 + 1
    assert lib.vcy_smooth_mesh(dev.ctx, *args) == capi.VCY_ERR_UNSUPPORTED
    assert all(np.all(o == 77) for o in out.values())
    check(dev, "mc_sphere", 1, TAUBIN, 0, "after the refusals")


# ---- 3. the voxel state, queued views and the extraction stay as they were ------------------------------------------------

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
    v, f = SC.mesh("mc_sphere")
    dev.SmoothMesh(v, f, 3, normals=True)
    got = dev.SmoothMesh(before["vertices"], before["faces"], 3, normals=True)
    SC.assert_bits(got["vertices"], vc.smooth_mesh_host(before["vertices"], before["faces"], 3, *TAUBIN)["vertices"], "own mesh")
    assert dev.state_diff(twin) == 0
    a, b = dev.ExtractIsoSurface(0.0, True), twin.ExtractIsoSurface(0.0, True)
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(SC.bits(a["vertices"]), SC.bits(b["vertices"]))
    assert len(a["vertices"]) != len(before["vertices"])                    # the queued view was applied after all
    dev.SmoothMesh(a["vertices"], a["faces"], 1)
    c = dev.ExtractIsoSurface(0.0, True)
    assert np.array_equal(a["faces"], c["faces"]) and np.array_equal(SC.bits(a["vertices"]), SC.bits(c["vertices"]))
    assert dev.state_diff(twin) == 0


# ---- 4. the device's own extraction, whole and sharded ----------------------------------------------------------------------

def smoke_scene():
    """The smoke scene (64^3, 4 views) carved and extracted on a whole-grid context, smoothed there: computed once."""
    def make():
        n = 64
        opt = synth.sphere_option(n)
        views, masks = synth.sphere_views(n, 4, 160, 120)
        dev = TR.make_dev(opt)
        for v, m in zip(views, masks):
            assert dev.CarveSilhouette(v, m), vc.last_error()
        mesh = dev.ExtractIsoSurface(0.0, True)
        got = dev.SmoothMesh(mesh["vertices"], mesh["faces"], 5, normals=True)
        dev.close()
        return opt, views, masks, mesh, got
    return SC.memo("smoke scene", make)


def test_smoke_scene_extraction():
    opt, views, masks, mesh, got = smoke_scene()
    assert len(mesh["vertices"]) > 2000
    host = vc.smooth_mesh_host(mesh["vertices"], mesh["faces"], 5, *TAUBIN, normals=True)
    for key in ("vertices", "normals", "face_normals"):
        SC.assert_normals(got[key], host[key], key)
    assert not np.isnan(got["vertices"]).any() and not np.array_equal(SC.bits(got["vertices"]), SC.bits(mesh["vertices"]))
    assert got["build_ms"] > 0.0 and got["passes_ms"] > 0.0 and got["normals_ms"] > 0.0


def test_smoke_scene_merged_slab_mesh_through_the_sharded_carver():
    opt, views, masks, mesh, got = smoke_scene()
    sh = ShardedVoxelCarver(opt, [0], slabs_per_device=2)
    assert sh.Init()
    assert sh.CarveBatchSilhouettes(views, masks), vc.last_error()
    merged = sh.ExtractIsoSurface(0.0, True)
    assert np.array_equal(merged["faces"], mesh["faces"]) and np.array_equal(SC.bits(merged["vertices"]), SC.bits(mesh["vertices"]))
    part = sh.SmoothMesh(merged["vertices"], merged["faces"], 5, normals=True)
    for key in ("vertices", "normals", "face_normals"):
        SC.assert_normals(part[key], got[key], "sharded " + key)
    assert part["build_ms"] > 0.0 and part["passes_ms"] > 0.0 and part["normals_ms"] > 0.0
    sh.close()


# ---- 5. the C++ layer ------------------------------------------------------------------------------------------------------

def read_binary_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().split("\n")
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[2])
    nf = int([l for l in head if l.startswith("element face")][0].split()[2])
    assert "property float nx" in head
    rows = np.frombuffer(raw, np.float32, 6 * nv, end).reshape(nv, 6)
    faces = np.frombuffer(raw, np.uint8, 13 * nf, end + 24 * nv).reshape(nf, 13)
    assert np.all(faces[:, 0] == 3)
    return rows[:, :3], rows[:, 3:], np.ascontiguousarray(faces[:, 1:]).view(np.int32)


def test_bunny_example_smooths_what_python_smooths(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "2", "--smooth", "3"],
                         check=True, capture_output=True, text=True)
    row = [l.split() for l in run.stdout.splitlines() if l.startswith("SMOOTH ")]
    assert len(row) == 1 and row[0][1:7] == ["iterations", "3", "lambda", "0.5", "mu", "-0.53"], run.stdout
    shard = [l.split() for l in run.stdout.splitlines() if l.startswith("SMOOTHSHARDED")]
    assert len(shard) == 1 and shard[0][1:3] == ["slabs", "2"] and shard[0][-2:] == ["identical", "1"], run.stdout
    verts, normals, faces = read_binary_ply(str(tmp_path / "surface_smooth.ply"))

    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    dev = vc.VoxelCarver(B.bunny_option(10.0))
    assert dev.Init(), vc.last_error()
    for v, m in zip(views, B.load_masks()):
        assert dev.CarveSilhouette(v, m), vc.last_error()
    mesh = dev.ExtractIsoSurface(0.0, True)
    got = dev.SmoothMesh(mesh["vertices"], mesh["faces"], 3, normals=True)
    assert int(row[0][8]) == len(verts) == len(mesh["vertices"]) > 1000 and np.array_equal(faces, mesh["faces"])
    SC.assert_bits(verts, got["vertices"], "the example's vertices")
    SC.assert_normals(normals, got["normals"], "the example's normals")

    bad = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "--smooth"], capture_output=True, text=True)
    assert bad.returncode == 10 and "--smooth needs a number" in bad.stderr
