"""vcy_decimate_mesh_quadric_host (the serial statement of the decimation with quadric representatives, no GPU) against
the numpy restatement (tests/quadric_ref.py), against today's MEAN call in everything but the positions, the property the
representative exists for, and its error contract."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decimate_ref as DR
import quadric_cases as QC
import test_decimate_cpu as TD
from vacancy_amd import capi, carver

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(name, cell, reg, normals=True):
    """The host function's outputs, computed once per (case, cell, regularize)."""
    def make():
        v, f = QC.mesh(name)
        return carver.decimate_mesh_quadric_host(v, f, cell, QC.origin_of(name), reg, normals)
    return QC.memo(("quadric host", name, cell, reg, normals), make)


def assert_equals(got, want, ctx, normals_of=None):
    """TD.assert_equals plus the fallback count."""
    TD.assert_equals(got, want, ctx, normals_of)
    assert got["n_fallback"] == want["n_fallback"], (ctx, got["n_fallback"], want["n_fallback"])


def normals_of(got):
    return carver.mesh_normals_host(got["vertices"], got["faces"]) if len(got["faces"]) else (got["normals"], got["face_normals"])


@pytest.mark.parametrize("case", QC.CASE_NAMES)
def test_host_equals_restatement_in_every_output(case):
    for cell, reg in QC.matrix(case):
        ctx = "%s cell %g regularize %g" % (case, cell, reg)
        got = host(case, cell, reg)
        assert_equals(got, QC.want(case, cell, reg), ctx, normals_of(got))


@pytest.mark.parametrize("case", ("mc_sphere", "box", "row_tiers", "wedge"))
def test_regularize_one_still_equals_the_restatement(case):
    cell = QC.cells_of(case)[-1] if case in QC.OWN else 2.0
    got = host(case, cell, 1.0)
    assert_equals(got, QC.want(case, cell, 1.0), case, normals_of(got))
    assert len(got["vertices"]) > 0


@pytest.mark.parametrize("case", QC.CASE_NAMES)
def test_faces_and_maps_are_those_of_mean(case):
    v, f = QC.mesh(case)
    for cell, reg in QC.matrix(case):
        ctx = "%s cell %g regularize %g" % (case, cell, reg)
        got = host(case, cell, reg)
        mean = carver.decimate_mesh_host(v, f, cell, QC.origin_of(case), DR.MEAN)
        assert np.array_equal(got["faces"], mean["faces"]) and np.array_equal(got["vertex_map"], mean["vertex_map"]), ctx
        assert np.array_equal(got["face_source"], mean["face_source"]) and got["vertices"].shape == mean["vertices"].shape, ctx
        want = QC.want(case, cell, reg)
        if want["vertex_map"] is not None:        # a fallback carries the mean's bits, and nothing else need
            fb = want["fallback"]
            assert np.array_equal(QC.bits(got["vertices"])[fb], QC.bits(mean["vertices"])[fb]), ctx
            keys, ok = DR.cell_keys(got["vertices"][~fb], QC.origin_of(case), cell)
            mkeys, mok = DR.cell_keys(mean["vertices"][~fb], QC.origin_of(case), cell)
            assert ok.all() and mok.all() and np.array_equal(keys, mkeys), ctx     # a representative never leaves its cell


@pytest.mark.parametrize("case,shift", [("box", 0.0), ("box_far", QC.FAR)])
@pytest.mark.parametrize("cell", (2.0, 3.7))
def test_box_stays_on_its_surface(case, shift, cell):
    """The restatement: 0.0015 against the mean's 0.49 at cell 2.0, 0.0027 against 0.91 at 3.7, about 1 / 330."""
    v, f = QC.mesh(case)
    got = host(case, cell, 1e-3)
    mean = carver.decimate_mesh_host(v, f, cell, QC.origin_of(case), DR.MEAN)
    dq, dm = QC.box_distance(got["vertices"], shift).max(), QC.box_distance(mean["vertices"], shift).max()
    print("%s cell %g: quadric %.4g, mean %.4g" % (case, cell, dq, dm))
    assert got["n_fallback"] == 0 == QC.want(case, cell, 1e-3)["n_fallback"]
    assert dq <= dm / 20.0, (dq, dm)               # (at 4096 the floats are 0.0005 apart: still far below a twentieth)


def test_wedge_falls_back_everywhere_and_carries_the_mean():
    v, f = QC.mesh("wedge")
    for reg in QC.REGS:
        got = host("wedge", 3.7, reg)
        mean = carver.decimate_mesh_host(v, f, 3.7, QC.origin_of("wedge"), DR.MEAN)
        assert len(got["vertices"]) == 4 == got["n_fallback"]
        assert np.array_equal(QC.bits(got["vertices"]), QC.bits(mean["vertices"]))


def test_the_cases_are_not_vacuous():
    for name in QC.OWN:                                  # each asserts its own property when it is built
        QC.mesh(name)
    moved = [n for n in QC.CASE_NAMES for c, r in QC.matrix(n)
             if QC.want(n, c, r)["vertex_map"] is not None and 0 < QC.want(n, c, r)["n_fallback"] < len(QC.want(n, c, r)["vertices"])]
    assert {"mc_sphere", "mc_sphere_40", "row_tiers", "boundary", "fan300"} <= set(moved)   # both branches in one call
    tiers = QC.want("row_tiers", 2.0, 1e-3)
    assert not np.array_equal(QC.bits(tiers["vertices"]), QC.bits(tiers["mean"]))
    assert sorted(tiers["members"]) == sorted(QC.DC.TIER_SIZES + (1,) * 16)
    assert QC.want("crowd", 2.0, 1e-3)["members"].max() >= 700


# ---- the error contract ---------------------------------------------------------------------------------------------------

def quadric_args():
    """TD.decimate_args with MEAN, turned into the quadric call's by finish()."""
    return TD.decimate_args("mc_sphere", 2.0, DR.MEAN)


def finish(args, reg=1e-3):
    n_fallback = C.c_int64(-1)
    return args[:5] + [C.c_float(reg)] + args[5:] + [C.byref(n_fallback)], n_fallback


BAD = dict(TD.BAD)
BAD.update({"mode 1": TD.opt_change(mode=1), "mode 2": TD.opt_change(mode=2)})
BAD_REGS = {"regularize nan": float("nan"), "regularize inf": float("inf"), "regularize -inf": float("-inf"),
            "regularize below 0": -1e-6, "regularize above 1": float(np.nextafter(F(1.0), F(2.0)))}


def refusals():
    """(name, arguments, the arrays kept alive, the outputs, the fallback count) of every call that must be refused."""
    for name in sorted(BAD):
        keep, args, out = quadric_args()
        BAD[name](keep, args)
        qargs, n_fallback = finish(args)
        yield name, qargs, keep, out, n_fallback
    for name in sorted(BAD_REGS):
        keep, args, out = quadric_args()
        qargs, n_fallback = finish(args, BAD_REGS[name])
        yield name, qargs, keep, out, n_fallback


def test_host_argument_errors_leave_outputs_counts_and_the_fallback_count_untouched():
    lib = capi.load()
    seen = 0
    for name, qargs, keep, out, n_fallback in refusals():
        assert lib.vcy_decimate_mesh_quadric_host(*qargs) == capi.VCY_ERR_INVALID_ARG, name
        assert carver.last_error(), name
        assert TD.untouched(keep, out) and n_fallback.value == -1, name
        seen += 1
    assert seen == len(TD.BAD) + 2 + 5
    for reg in (0.0, 1.0):                                       # both ends of the interval are accepted
        keep, args, out = quadric_args()
        qargs, n_fallback = finish(args, reg)
        assert lib.vcy_decimate_mesh_quadric_host(*qargs) == 0, carver.last_error()
        assert n_fallback.value >= 0 and keep[3][0].value == 273


def test_too_many_corners_empty_meshes_null_outputs_and_the_entry_checks_of_the_device_call():
    lib = capi.load()
    for i, value in ((1, (1 << 31) // 3 + 1), (0, 1 << 31)):    # refused before an array is read
        for fn, ctx in ((lib.vcy_decimate_mesh_quadric_host, ()), (lib.vcy_decimate_mesh_quadric, (None,))):
            keep, args, out = quadric_args()
            args[i] = value
            qargs, n_fallback = finish(args)
            assert fn(*ctx, *qargs) == capi.VCY_ERR_UNSUPPORTED
            assert TD.untouched(keep, out) and n_fallback.value == -1
    for zero in ([0], [1], [0, 1]):                              # nothing to do: the three counts 0, no array written
        keep, args, out = quadric_args()
        for i in zero:
            args[i] = 0
        qargs, n_fallback = finish(args)
        assert lib.vcy_decimate_mesh_quadric_host(*qargs) == 0
        assert all(np.all(o == 77) for o in out.values()) and keep[3][0].value == 0 and keep[3][1].value == 0
        assert n_fallback.value == 0
    got = carver.decimate_mesh_quadric_host(*QC.mesh("one_vertex"), 2.0)
    assert len(got["vertices"]) == 0 and list(got["vertex_map"]) == [-1] and got["n_fallback"] == 0
    # every optional output may be NULL, the fallback count included
    want = QC.want("mc_sphere", 2.0, 1e-3)
    keep, args, out = quadric_args()
    args[9] = args[10] = args[11] = args[12] = None
    qargs, n_fallback = finish(args)
    qargs[-1] = None
    assert lib.vcy_decimate_mesh_quadric_host(*qargs) == 0, carver.last_error()
    nv = keep[3][0].value
    QC.DC.assert_bits(out["vertices"][:nv], want["vertices"], "bare")
    assert all(np.all(out[k] == 77) for k in ("vertex_map", "face_source", "normals", "face_normals"))
    # the device entry point checks its arguments before it looks at the context
    for name, qargs, keep, out, n_fallback in refusals():
        if "face index" in name or "vertex" in name.split()[0] or name == "too few vertices":
            continue                                             # (found in the arrays: they need the device)
        assert lib.vcy_decimate_mesh_quadric(None, *qargs) == capi.VCY_ERR_INVALID_ARG, name
        assert TD.untouched(keep, out) and n_fallback.value == -1, name
    keep, args, out = quadric_args()
    qargs, n_fallback = finish(args)
    assert lib.vcy_decimate_mesh_quadric(None, *qargs) == capi.VCY_ERR_NOT_INITIALIZED
    assert TD.untouched(keep, out) and n_fallback.value == -1
    ms = C.c_float(-1.0)
    assert lib.vcy_last_quadric_ms(None, C.byref(ms)) == capi.VCY_ERR_INVALID_ARG


def test_symbols():
    lib = capi.load()
    for name in ("vcy_decimate_mesh_quadric_host", "vcy_decimate_mesh_quadric", "vcy_last_quadric_ms"):
        assert name in lib._vcy_symbols and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "vacancy_hip.h")).read()
    assert "mesh decimation, quadric representatives" in header


def test_host_function_is_clean_under_host_sanitizers():
    """The stand-alone program of tests/quadric_host_check.cpp: the host function and the normals behind it under
    AddressSanitizer and UBSan, on the CPU."""
    run = subprocess.run(["make", "-C", os.path.join(ROOT, "vacancy_amd", "csrc"), "-s", "quadric_host_check"], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "quadric_host_check: ok" in run.stdout
