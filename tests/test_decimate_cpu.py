"""vcy_decimate_mesh_host (the serial statement of the mesh decimation, no GPU) against the numpy restatement
(tests/decimate_ref.py), against the counts the definition was first run to, properties of every output, and its error
contract."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decimate_cases as DC
import decimate_ref as DR
from vacancy_amd import capi, carver

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(name, cell, mode, normals=False):
    v, f = DC.mesh(name)
    return carver.decimate_mesh_host(v, f, cell, DC.origin_of(name), mode, normals)


def assert_equals(got, want, ctx, normals_of=None):
    """Every output of a call against the restatement's (or another call's) outputs."""
    assert got["faces"].shape == want["faces"].shape and got["vertices"].shape == want["vertices"].shape, (
        ctx, got["vertices"].shape, want["vertices"].shape, got["faces"].shape, want["faces"].shape)
    assert np.array_equal(got["faces"], want["faces"]), ctx
    DC.assert_bits(got["vertices"], want["vertices"], ctx)
    if want["vertex_map"] is not None:
        assert np.array_equal(got["vertex_map"], want["vertex_map"]), ctx
        assert np.array_equal(got["face_source"], want["face_source"]), ctx
    if normals_of is not None:
        vn, fn = normals_of
        DC.assert_normals(got["normals"], vn, ctx + " (vertex normals)")
        DC.assert_normals(got["face_normals"], fn, ctx + " (face normals)")


def check_properties(name, got, cell, mode, ctx):
    v, f = DC.mesh(name)
    faces, vmap, src = got["faces"], got["vertex_map"], got["face_source"]
    nv = len(got["vertices"])
    if len(faces):
        assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 2] != faces[:, 0]).all(), ctx
        assert len(set(DC.canonical_rows(faces))) == len(faces), ctx
        assert faces.min() >= 0 and faces.max() < nv, ctx
    assert np.array_equal(np.unique(faces), np.arange(nv)), ctx              # every output vertex is named by a face
    assert (np.diff(src) > 0).all(), ctx
    assert np.array_equal(vmap[f[src]], faces), ctx                          # vertex_map consistent with face_source
    assert np.array_equal(np.unique(vmap[vmap >= 0]), np.arange(nv)), ctx
    if mode != DR.MEAN and nv:
        keys, ok = DR.cell_keys(v, DC.origin_of(name), cell)
        out_keys, ok2 = DR.cell_keys(got["vertices"], DC.origin_of(name), cell)
        assert ok.all() and ok2.all()
        member = vmap >= 0
        assert np.array_equal(out_keys[vmap[member]], keys[member]), ctx     # the representative lies in its cluster's cell


@pytest.mark.parametrize("case", DC.CASE_NAMES)
def test_host_equals_restatement_in_every_output(case):
    v, f = DC.mesh(case)
    for cell, mode in DC.matrix():
        ctx = "%s cell %g mode %d" % (case, cell, mode)
        got = host(case, cell, mode, normals=True)
        want = DC.want(case, cell, mode)
        normals = carver.mesh_normals_host(got["vertices"], got["faces"]) if len(got["faces"]) else (got["normals"], got["face_normals"])
        assert_equals(got, want, ctx, normals)
        if len(v) and len(f):
            check_properties(case, got, cell, mode, ctx)
        if cell == 0.001 and case in DC.CLEAN:
            DC.assert_bits(got["vertices"], v, ctx + " (the input bits)")
            assert np.array_equal(got["faces"], f) and np.array_equal(got["vertex_map"], np.arange(len(v)))
            assert np.array_equal(got["face_source"], np.arange(len(f)))


def test_counts_of_the_definition():
    counts = lambda name, cell: tuple(len(host(name, cell, DR.MEAN)[k]) for k in ("vertices", "faces"))
    v, f = DC.mesh("mc_sphere")
    assert (len(v), len(f)) == (1296, 2588)
    assert counts("mc_sphere", 0.75) == (954, 1904)
    assert counts("mc_sphere", 2.0) == (273, 542)
    assert counts("mc_sphere", 3.7) == (76, 148)
    assert counts("mc_sphere", 1000.0) == (0, 0)
    patch = DC.want("open_patch", 2.0, DR.MEAN)
    assert len(patch["members"]) == 35 and len(patch["vertices"]) == 34 and counts("open_patch", 2.0)[0] == 34
    assert len(DC.mesh("degenerate")[1]) == 9 and counts("degenerate", 0.001)[1] == 5


def test_the_cases_are_not_vacuous():
    for name in DC.OWN:                                  # each asserts its own property when it is built
        DC.mesh(name)
    r = DC.want("crowd", 2.0, DR.NEAREST)
    assert r["members"].max() >= 700 > 256              # longer than a block, and than any in-register row
    v, f = DC.mesh("boundary")
    assert np.signbit(v[v == 0]).any()
    mean = host("boundary", 0.001, DR.MEAN)["vertices"]
    first = host("boundary", 0.001, DR.FIRST)["vertices"]
    assert not np.signbit(mean[mean == 0]).any() and np.signbit(first[first == 0]).any()   # +0 + -0.0 is +0.0; FIRST copies bits
    near = DC.want("mc_sphere", 3.7, DR.NEAREST)
    assert not np.array_equal(DC.bits(near["vertices"]), DC.bits(DC.want("mc_sphere", 3.7, DR.FIRST)["vertices"]))
    members = DC.want("mc_sphere_40", 3.7, DR.MEAN)["members"]
    assert (members <= 16).any() and ((members > 16) & (members <= 48)).any()    # rows for either in-register sort ...
    longest = DC.want("two_sheets_same", 1000.0, DR.MEAN)["members"].max()
    assert 48 < longest <= 256                                                     # ... for the sort in global memory ...
    assert (DC.want("mc_sphere_40", 1000.0, DR.MEAN)["members"] > 256).sum() >= 2  # ... and rows that get a workgroup each


def decimate_args(name="mc_sphere", cell=2.0, mode=DR.NEAREST, normals=True):
    v, f = DC.mesh(name)
    keep, args, out = carver._decimate_args(v, f, cell, DC.origin_of(name), mode, normals)
    for o in out.values():
        o[...] = 77
    return list(keep), list(args), out


def untouched(keep, out):
    return all(np.all(o == 77) for o in out.values()) and keep[3][0].value == -1 and keep[3][1].value == -1


def test_every_optional_output_left_null_leaves_the_others_correct():
    lib = capi.load()
    want = DC.want("mc_sphere", 2.0, DR.NEAREST)
    names = {9: "vertex_map", 10: "face_source", 11: "normals", 12: "face_normals"}
    for drop in ([9], [10], [11], [12], [9, 10], [11, 12], [9, 10, 11, 12]):
        keep, args, out = decimate_args()
        for i in drop:
            args[i] = None
        assert lib.vcy_decimate_mesh_host(*args) == 0, carver.last_error()
        nv, nf = keep[3][0].value, keep[3][1].value
        assert (nv, nf) == (len(want["vertices"]), len(want["faces"]))
        DC.assert_bits(out["vertices"][:nv], want["vertices"], str(drop))
        assert np.array_equal(out["faces"][:nf], want["faces"])
        assert np.all(out["vertices"][nv:] == 77) and np.all(out["faces"][nf:] == 77)
        vn, fn = carver.mesh_normals_host(want["vertices"], want["faces"])
        for i, key in names.items():
            if i in drop:
                assert np.all(out[key] == 77), (drop, key)
        if 9 not in drop:
            assert np.array_equal(out["vertex_map"], want["vertex_map"])
        if 10 not in drop:
            assert np.array_equal(out["face_source"][:nf], want["face_source"])
        if 11 not in drop:
            DC.assert_normals(out["normals"][:nv], vn, str(drop))
        if 12 not in drop:
            DC.assert_normals(out["face_normals"][:nf], fn, str(drop))


def opt_change(**kw):
    def change(keep, a):
        for k, v in kw.items():
            setattr(keep[2], k, v)
    return change


def origin_change(i, value):
    def change(keep, a):
        keep[2].origin[i] = value
    return change


def arg_change(i, value):
    def change(keep, a):
        a[i] = value
    return change


def face_change(value):
    def change(keep, a):
        f = np.array(keep[1], np.int32)
        f[len(f) // 2, 1] = value
        keep[1] = f
        a[3] = carver._p(f)
    return change


def vertex_change(value, at=None):
    def change(keep, a):
        v = np.array(keep[0], F)
        v[len(v) // 3 if at is None else at, 1] = value
        keep[0] = v
        a[2] = carver._p(v)
    return change


BAD = {
    "null vertices": arg_change(2, None), "null faces": arg_change(3, None), "null option": arg_change(4, None),
    "null vertices_out": arg_change(5, None), "null faces_out": arg_change(6, None), "null n_vertices_out": arg_change(7, None),
    "null n_faces_out": arg_change(8, None), "n_vertices -1": arg_change(0, -1), "n_faces -1": arg_change(1, -1),
    "face index -1": face_change(-1), "face index n": face_change(1 << 20), "too few vertices": arg_change(0, 10),
    "cell 0": opt_change(cell=0.0), "cell -1": opt_change(cell=-1.0), "cell nan": opt_change(cell=float("nan")),
    "cell inf": opt_change(cell=float("inf")), "origin nan": origin_change(0, float("nan")), "origin inf": origin_change(2, float("inf")),
    "mode -1": opt_change(mode=-1), "mode 3": opt_change(mode=3),
    "vertex nan": vertex_change(float("nan")), "vertex inf": vertex_change(float("-inf"), at=0),
    "vertex 2^31 cells away": vertex_change(2.0 ** 32),            # |t| = 2^31 at cell 2
    "vertex 2^30 cells away": vertex_change(2.0 ** 31),            # minus the origin it rounds back to 2^31; over cell 2: 2^30
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_host_argument_errors_leave_outputs_and_counts_untouched(name):
    lib = capi.load()
    keep, args, out = decimate_args()
    BAD[name](keep, args)
    assert lib.vcy_decimate_mesh_host(*args) == capi.VCY_ERR_INVALID_ARG, name
    assert carver.last_error()
    assert untouched(keep, out), name


def test_the_cell_rule_sits_at_2_to_the_30():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], F)
    f = np.array([[0, 1, 2], [3, 1, 2]], np.int32)
    below = np.nextafter(F(2.0 ** 30), F(0))
    for x, ok in ((below, True), (-below, True), (F(2.0 ** 30), False), (F(-2.0 ** 30), False)):
        v[3, 2] = x                                          # cell 1, origin 0: t is the coordinate itself
        if ok:
            got = carver.decimate_mesh_host(v, f, 1.0, (0, 0, 0), DR.FIRST)
            assert len(got["faces"]) == 2 and DR.decimate(v, f, 1.0, (0, 0, 0), DR.FIRST) is not None
        else:
            with pytest.raises(RuntimeError) as e:
                carver.decimate_mesh_host(v, f, 1.0, (0, 0, 0), DR.FIRST)
            assert e.value.rc == capi.VCY_ERR_INVALID_ARG and DR.decimate(v, f, 1.0, (0, 0, 0), DR.FIRST) is None


def test_too_many_corners_empty_meshes_and_the_entry_checks_of_the_device_call():
    lib = capi.load()
    for i, value in ((1, (1 << 31) // 3 + 1), (0, 1 << 31)):    # refused before an array is read
        keep, args, out = decimate_args()
        args[i] = value
        assert lib.vcy_decimate_mesh_host(*args) == capi.VCY_ERR_UNSUPPORTED
        assert lib.vcy_decimate_mesh(None, *args) == capi.VCY_ERR_UNSUPPORTED
        assert untouched(keep, out)
    for zero in ([0], [1], [0, 1]):                              # nothing to do: both counts 0, no array written
        keep, args, out = decimate_args()
        for i in zero:
            args[i] = 0
        assert lib.vcy_decimate_mesh_host(*args) == 0
        assert all(np.all(o == 77) for o in out.values()) and keep[3][0].value == 0 and keep[3][1].value == 0
    got = carver.decimate_mesh_host(*DC.mesh("one_vertex"), 2.0)
    assert len(got["vertices"]) == 0 and len(got["faces"]) == 0 and list(got["vertex_map"]) == [-1]
    # the device entry point checks its arguments before it looks at the context
    for name in ("null option", "null n_faces_out", "cell 0", "origin nan", "mode 3", "n_faces -1"):
        keep, args, out = decimate_args()
        BAD[name](keep, args)
        assert lib.vcy_decimate_mesh(None, *args) == capi.VCY_ERR_INVALID_ARG, name
        assert untouched(keep, out)
    keep, args, out = decimate_args()
    assert lib.vcy_decimate_mesh(None, *args) == capi.VCY_ERR_NOT_INITIALIZED
    assert untouched(keep, out)
    ms = C.c_float(-1.0)
    assert lib.vcy_last_decimate_ms(None, C.byref(ms), None, None, None) == capi.VCY_ERR_INVALID_ARG


def test_symbols_and_struct_size():
    lib = capi.load()
    for name in ("vcy_decimate_mesh_host", "vcy_decimate_mesh", "vcy_last_decimate_ms"):
        assert name in lib._vcy_symbols and hasattr(lib, name)
    assert C.sizeof(capi.DecimateOption) == 20
    header = open(os.path.join(ROOT, "include", "vacancy_hip.h")).read()
    assert "} vcy_decimate_option;" in header
    assert (capi.VCY_DECIMATE_MEAN, capi.VCY_DECIMATE_NEAREST, capi.VCY_DECIMATE_FIRST) == (DR.MEAN, DR.NEAREST, DR.FIRST) == (0, 1, 2)


def test_host_function_is_clean_under_host_sanitizers():
    """The stand-alone program of tests/decimate_host_check.cpp: the host function and the normals behind it under
    AddressSanitizer and UBSan, on the CPU."""
    run = subprocess.run(["make", "-C", os.path.join(ROOT, "vacancy_amd", "csrc"), "-s", "decimate_host_check"], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "decimate_host_check: ok" in run.stdout
