"""vcy_smooth_mesh_host (the serial statement of the mesh smoothing, no GPU) against the numpy restatement
(tests/smooth_ref.py), against hand-computed results, and its error contract."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import smooth_cases as SC
import smooth_ref as SR
from vacancy_amd import capi, carver

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(name, it, factors, pin, normals=False):
    v, f = SC.mesh(name)
    return carver.smooth_mesh_host(v, f, it, factors[0], factors[1], pin, normals)


@pytest.mark.parametrize("case", SC.CASE_NAMES)
def test_host_equals_restatement_and_normals_are_those_of_the_result(case):
    v, f = SC.mesh(case)
    for it, factors, pin in SC.matrix():
        ctx = "%s it %d factors %s pin %d" % (case, it, factors, pin)
        got = host(case, it, factors, pin, normals=True)
        SC.assert_bits(got["vertices"], SC.want(case, it, factors, pin), ctx)
        vn, fn = carver.mesh_normals_host(got["vertices"], f)
        SC.assert_normals(got["normals"], vn, ctx + " (vertex normals)")
        SC.assert_normals(got["face_normals"], fn, ctx + " (face normals)")
        if it == 0 or factors == (0.0, 0.0):
            SC.assert_bits(got["vertices"], v, ctx + " (the input bits)")


def test_octahedron_by_hand():
    v, f = SC.mesh("octahedron")
    for it in (1, 2, 3):      # every pass with 0.5 halves every coordinate: all partial sums are sums of +-2^-k and 0
        got = carver.smooth_mesh_host(v, f, it, 0.5, 0.0)["vertices"]
        assert np.array_equal(got, v * F(0.5 ** it)), it
    got = carver.smooth_mesh_host(v, f, 1, 0.5, -0.5)["vertices"]   # 0.5 p, then 0.5 p - 0.5 * (0 - 0.5 p)
    assert np.array_equal(got, v * F(0.75))


def test_open_patch_pins_exactly_its_rim():
    v, f = SC.mesh("open_patch")
    rim = SC.open_patch_rim()
    assert rim.sum() == 32 and np.array_equal(SR.pinned(len(v), f), rim)
    got = host("open_patch", 2, (0.5, -0.53), 1)["vertices"]
    same = (SC.bits(got) == SC.bits(v)).all(axis=1)
    assert np.array_equal(same, rim)
    free = host("open_patch", 2, (0.5, -0.53), 0)["vertices"]
    assert not (SC.bits(free) == SC.bits(v)).all(axis=1).any()


def test_isolated_vertices_never_move():
    v, f = SC.mesh("isolated")
    ids = list(SC.ISOLATED_IDS)
    assert ids[0] == 0 and ids[-1] == len(v) - 1 and not np.isin(ids, f).any()
    for pin in SC.PINS:
        got = host("isolated", 7, (0.5, -0.53), pin, normals=True)
        SC.assert_bits(got["vertices"][ids], v[ids], "isolated")
        assert np.isnan(got["normals"][ids]).all()
        moved = np.setdiff1d(np.arange(len(v)), ids)
        assert not (SC.bits(got["vertices"][moved]) == SC.bits(v[moved])).all(axis=1).any()


def test_the_cases_are_not_vacuous():
    v, f = SC.mesh("fan300")
    off, corners = SR.rows(len(v), f)
    assert 2 * (off[1] - off[0]) == 600
    assert not np.array_equal(np.sort(f[:, 1]), f[:, 1])             # the hub's faces are not in rim order
    v, f = SC.mesh("degenerate")
    off, corners = SR.rows(len(v), f)
    repeated = [v_ for v_ in range(len(v)) if len(set(corners[off[v_]:off[v_ + 1]] // 3)) < off[v_ + 1] - off[v_]]
    assert 0 in repeated and 2 in repeated and 5 in repeated
    assert (f == f[2]).all(axis=1).sum() == 2                        # one face present twice
    edge = sum(1 for t in f if 3 in t and 4 in t)
    assert edge == 3
    v, f = SC.mesh("mc_sphere")
    assert 1000 < len(v) < 10000 and len(v) % 256 != 0 and len(f) == 2 * len(v) - 4   # a closed surface of genus 0
    off, corners = SR.rows(len(v), f)
    assert (off[1:] - off[:-1]).min() >= 4 and (off[1:] - off[:-1]).max() <= 12
    assert len(SC.mesh("257_vertices")[0]) == 257 and len(SC.mesh("one_vertex")[0]) == 1
    assert len(np.unique(SC.mesh("two_components")[1])) == 12


def smooth_args(name="mc_sphere", it=2, normals=True):
    v, f = SC.mesh(name)
    keep, args, out = carver._smooth_args(v, f, it, 0.5, -0.53, 1, normals)
    for o in out.values():
        o[...] = 77
    return list(keep), list(args), out


def test_in_place_gives_the_same_bits():
    lib = capi.load()
    for name in ("mc_sphere", "fan300", "degenerate"):
        keep, args, out = smooth_args(name, 7, normals=False)
        buf = np.array(keep[0], F)                # a writeable copy: input and output in one
        args[2] = args[5] = carver._p(buf)
        assert lib.vcy_smooth_mesh_host(*args) == 0, carver.last_error()
        SC.assert_bits(buf, SC.want(name, 7, (0.5, -0.53), 1), name)


def opt_change(**kw):
    def change(keep, a):
        for k, v in kw.items():
            setattr(keep[2], k, v)
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


BAD = {
    "null vertices": arg_change(2, None), "null faces": arg_change(3, None), "null option": arg_change(4, None),
    "null vertices_out": arg_change(5, None), "n_vertices -1": arg_change(0, -1), "n_faces -1": arg_change(1, -1),
    "face index -1": face_change(-1), "face index n": face_change(1 << 20), "too few vertices": arg_change(0, 10),
    "iterations -1": opt_change(iterations=-1), "iterations 10001": opt_change(iterations=10001),
    "lambda nan": opt_change(lam=float("nan")), "lambda inf": opt_change(lam=float("inf")),
    "mu nan": opt_change(mu=float("nan")), "mu -inf": opt_change(mu=float("-inf")),
    "pin 2": opt_change(pin_boundary=2), "pin -1": opt_change(pin_boundary=-1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_host_argument_errors_leave_the_outputs_untouched(name):
    lib = capi.load()
    keep, args, out = smooth_args()
    BAD[name](keep, args)
    assert lib.vcy_smooth_mesh_host(*args) == capi.VCY_ERR_INVALID_ARG, name
    assert carver.last_error()
    assert all(np.all(o == 77) for o in out.values()), name


def test_too_many_corners_empty_mesh_and_the_entry_checks_of_the_device_call():
    lib = capi.load()
    keep, args, out = smooth_args()
    args[1] = (1 << 31) // 3 + 1                      # 3 * n_faces >= 2^31: refused before a face is read
    assert lib.vcy_smooth_mesh_host(*args) == capi.VCY_ERR_UNSUPPORTED
    assert lib.vcy_smooth_mesh(None, *args) == capi.VCY_ERR_UNSUPPORTED
    keep, args, out = smooth_args()
    args[0] = args[1] = 0                             # no vertices: fine, nothing written
    assert lib.vcy_smooth_mesh_host(*args) == 0
    assert all(np.all(o == 77) for o in out.values())
    # the device entry point checks its arguments before it looks at the context
    for name in ("null option", "face index -1", "iterations 10001", "mu nan", "pin 2"):
        keep, args, out = smooth_args()
        BAD[name](keep, args)
        assert lib.vcy_smooth_mesh(None, *args) == capi.VCY_ERR_INVALID_ARG, name
    keep, args, out = smooth_args()
    assert lib.vcy_smooth_mesh(None, *args) == capi.VCY_ERR_NOT_INITIALIZED
    assert all(np.all(o == 77) for o in out.values())
    ms = C.c_float(-1.0)
    assert lib.vcy_last_smooth_ms(None, C.byref(ms), None, None) == capi.VCY_ERR_INVALID_ARG


def test_null_normals_outputs_are_not_written():
    lib = capi.load()
    keep, args, out = smooth_args()
    args[6] = None
    assert lib.vcy_smooth_mesh_host(*args) == 0
    assert np.all(out["normals"] == 77) and not np.all(out["face_normals"] == 77)
    want = carver.mesh_normals_host(out["vertices"], keep[1])[1]
    SC.assert_normals(out["face_normals"], want, "face normals alone")


def test_host_function_is_clean_under_host_sanitizers():
    """The stand-alone program of tests/smooth_host_check.cpp: the host function and the normals behind it under
    AddressSanitizer and UBSan, on the CPU."""
    run = subprocess.run(["make", "-C", os.path.join(ROOT, "vacancy_amd", "csrc"), "-s", "smooth_host_check"], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "smooth_host_check: ok" in run.stdout
