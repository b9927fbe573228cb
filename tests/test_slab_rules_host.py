"""The host rules the front ends of a grid in z-slabs share, stated once in the library (vacancy_amd/csrc/slab_rules.h
behind vcy_close_hull_plan, vcy_select_components_host and vcy_distance_halo_host), checked without a GPU.

tests/slab_rules_host_check.cpp includes the header alone and compares with literals; it is built and run plain and with
the host sanitizers.  The C-ABI entries are then asked through ctypes against the references the tests keep for
themselves: components_ref.kept, slab_distance_cases.halos_np, distance_ref.close_plan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import components_ref as CR
import distance_ref as DR
import slab_distance_cases as S
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path, name, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is part of the image"
    exe = str(tmp_path / name)
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off"] + extra +
                       ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "vacancy_amd", "csrc"),
                        os.path.join(ROOT, "tests", "slab_rules_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_slab_rules_give_the_stated_answers(tmp_path):
    out = build_and_run(tmp_path, "slab_rules_host_check", [])
    m = re.search(r"(\d+) checks, 0 failures", out)
    assert m and int(m.group(1)) > 1000, out[-500:]


def test_slab_rules_under_the_host_sanitizers(tmp_path):
    """The same stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: every edge array there is exactly
    min(R, thickness) planes long, so the offset into "the highest planes of the owner" cannot be off by one unseen, and
    the conversion of a radius to R is asked for a NaN."""
    out = build_and_run(tmp_path, "slab_rules_host_check_san",
                        ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert ", 0 failures" in out


# ---- the keep rule ---------------------------------------------------------------------------------------------------------

def component_lists():
    """the lists of test_components_ref.test_random_volumes_against_flood_fill, and one with ties in n_voxels"""
    rng = np.random.RandomState(5)
    out = []
    for dims, density in (((5, 4, 3), 0.5), ((9, 10, 7), 0.31), ((13, 3, 5), 0.7)):
        s = rng.rand(dims[0] * dims[1] * dims[2]) < density
        out.append(CR.components(CR.label_volume(s, dims), dims))
    n_voxels = np.array([9, 4, 4, 4, 2, 2, 1], np.int64)
    out.append({"label": np.array([40, 3, 17, 90, 5, 60, 8], np.int64), "n_voxels": n_voxels,
                "bb_min": np.zeros((7, 3), np.int32), "bb_max": np.ones((7, 3), np.int32)})
    return out


def test_select_components_against_the_reference_rule():
    lists = component_lists()
    assert len(lists[1]["label"]) > 8 and len(set(lists[3]["n_voxels"].tolist())) < 7
    for comps in lists:
        n = len(comps["label"])
        sizes = sorted(set(comps["n_voxels"].tolist()))
        for largest in (0, 1, 2, n - 1, n, n + 5, -1):
            for min_voxels in [0, 1] + sizes + [v + 1 for v in sizes]:
                keep = CR.kept(comps, largest, min_voxels)
                # pieces: every component in two, the second piece under a provisional label of its own
                maps = [comps["label"].copy(), comps["label"][::-1].copy(), np.zeros(0, np.int64)]
                gone, pieces, nc, nv = vdist.select_components(comps, largest, min_voxels, maps)
                ctx = (n, largest, min_voxels)
                assert np.array_equal(gone, ~keep), ctx
                assert (nc, nv) == (int((~keep).sum()), int(comps["n_voxels"][~keep].sum())), ctx
                assert [len(p) for p in pieces] == [n, n, 0], ctx
                assert np.array_equal(pieces[0], ~keep) and np.array_equal(pieces[1], ~keep[::-1]), ctx
    empty = CR.subset(lists[0], np.zeros(len(lists[0]["label"]), bool))
    gone, pieces, nc, nv = vdist.select_components(empty, 1, 0)
    assert len(gone) == 0 and pieces == [] and (nc, nv) == (0, 0)


def test_select_components_refusals():
    lib = capi.load()
    flags = np.zeros(4, np.uint8)
    for args in ((None, 2, 1, 0, vc._p(flags), None, None, None, 0, None),
                 (None, -1, 1, 0, None, None, None, None, 0, None),
                 (None, 0, 1, 0, None, None, None, None, 3, vc._p(flags))):
        assert lib.vcy_select_components_host(*args) == capi.VCY_ERR_INVALID_ARG
        assert "vcy_select_components_host" in vc.last_error()


# ---- the seam halo assembly ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", (1, 3, 12, 127))
def test_distance_halo_host_against_slicing_the_whole_grid(radius):
    """The raw call, slab by slab, with buffers of exactly the planes to come."""
    lib = capi.load()
    nz, sl = 23, 5
    whole = np.random.RandomState(100 + radius).randint(0, 65536, (nz, sl)).astype(np.uint16)
    for bounds in S.cuts_of(nz):
        zr = list(zip(bounds[:-1], bounds[1:]))
        planes = [whole[z0:z1] for z0, z1 in zr]
        bottoms, tops = [[np.ascontiguousarray(p) for p in side] for side in S.edge_planes(zr, radius, planes)]
        ns = len(zr)
        b = (C.c_void_p * ns)(*[None if s == 0 else p.ctypes.data for s, p in enumerate(bottoms)])
        t = (C.c_void_p * ns)(*[None if s == ns - 1 else p.ctypes.data for s, p in enumerate(tops)])
        zb = np.array(bounds, np.int32)
        for s, ((z0, z1), (wb, wa)) in enumerate(zip(zr, S.halos_np(zr, radius, planes))):
            below = np.zeros((0 if wb is None else len(wb), sl), np.uint16)
            above = np.zeros((0 if wa is None else len(wa), sl), np.uint16)
            nb, na = C.c_int(-1), C.c_int(-1)
            rc = lib.vcy_distance_halo_host(ns, vc._p(zb), radius, sl, b, t, s, vc._p(below) if len(below) else None,
                                            vc._p(above) if len(above) else None, C.byref(nb), C.byref(na))
            assert rc == 0, (bounds, s, vc.last_error())
            assert (nb.value, na.value) == (len(below), len(above)) == (min(radius, z0), min(radius, nz - z1))
            assert wb is None or np.array_equal(below, wb), (bounds, s)
            assert wa is None or np.array_equal(above, wa), (bounds, s)


def test_distance_halo_host_refusals():
    lib = capi.load()
    sl, bounds = 4, [0, 6, 8, 10, 17]
    zr = list(zip(bounds[:-1], bounds[1:]))
    whole = np.arange(17 * sl, dtype=np.uint16).reshape(17, sl)
    bottoms, tops = [[np.ascontiguousarray(p) for p in side]
                     for side in S.edge_planes(zr, 12, [whole[z0:z1] for z0, z1 in zr])]
    buf = np.zeros((2, 12, sl), np.uint16)
    nb, na = C.c_int(0), C.c_int(0)

    def call(zb=bounds, slab=2, radius=12, plane=sl, no_top=(), no_bottom=()):
        zb = np.array(zb, np.int32)
        b = (C.c_void_p * 4)(*[None if s in no_bottom else p.ctypes.data for s, p in enumerate(bottoms)])
        t = (C.c_void_p * 4)(*[None if s in no_top else p.ctypes.data for s, p in enumerate(tops)])
        return lib.vcy_distance_halo_host(len(zb) - 1, vc._p(zb), radius, plane, b, t, slab, vc._p(buf[0]), vc._p(buf[1]),
                                          C.byref(nb), C.byref(na))

    assert call(no_bottom=(0,), no_top=(3,)) == 0 and (nb.value, na.value) == (8, 7)
    assert np.array_equal(buf[0][:8], whole[0:8]) and np.array_equal(buf[1][:7], whole[10:17])
    for kwargs, word in (({"zb": [1, 6, 8, 10, 17]}, "ascend"), ({"zb": [0, 6, 6, 10, 17]}, "ascend"),
                         ({"zb": [0, 8, 6, 10, 17]}, "ascend"), ({"slab": 4}, "slab 4"), ({"slab": -1}, "slab -1"),
                         ({"no_top": (0,)}, "null"), ({"no_bottom": (3,)}, "null"), ({"radius": 0}, "radius"),
                         ({"radius": 128}, "radius"), ({"plane": 0}, "invalid argument")):
        assert call(**kwargs) == capi.VCY_ERR_INVALID_ARG, kwargs
        assert "vcy_distance_halo_host" in vc.last_error() and word in vc.last_error(), (kwargs, vc.last_error())


# ---- the closing plan ------------------------------------------------------------------------------------------------------

def raw_plan(radius_voxels, resolution):
    r, big_r = C.c_double(-1.0), C.c_int(-1)
    rc = capi.load().vcy_close_hull_plan(radius_voxels, resolution, C.byref(r), C.byref(big_r))
    return rc, r.value, big_r.value


def test_close_hull_plan_against_the_reference():
    """The radii of test_distance_cpu.test_closing_ties_at_one_and_a_half: Python's doubles through close_hull_plan, the
    C++ facade's floats -- widened, as it passes them -- through the raw call."""
    for rv in (1.3, 2.3, 2.0, 125.0):
        for resolution in (1.0, 0.375, 0.1):
            assert vc.close_hull_plan(rv, resolution) == DR.close_plan(rv, resolution)
            wide = float(np.float32(rv))
            assert raw_plan(wide, resolution) == (0,) + DR.close_plan(wide, resolution)
    for rv in (0.5, 1.5, 2.5, 0.0, -1.0, 126.0):
        with pytest.raises(ValueError) as e:
            vc.close_hull_plan(rv, 1.0)
        assert str(e.value).startswith("CloseHull: radius_voxels = %g " % rv)
        assert raw_plan(float(np.float32(rv)), 1.0)[0] == capi.VCY_ERR_INVALID_ARG
        assert vc.last_error() == str(e.value)
    with pytest.raises(ValueError) as e:
        vc.close_hull_plan(1.5, 1.0)
    assert "ties: (radius + 0.5)^2 = 4 is a squared voxel distance" in str(e.value) and str(e.value).endswith("pick e.g. 1.3")
    with pytest.raises(ValueError) as e:
        vc.close_hull_plan(126.0, 1.0)
    assert str(e.value) == "CloseHull: radius_voxels = 126 must be positive and at most 125"
