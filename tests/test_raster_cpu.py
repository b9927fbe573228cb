"""The mesh rasteriser's definition on the CPU: vcy_raster_mesh_host (raster_host.hip) against the numpy restatement of the
section "rasterising an indexed mesh" of vacancy_hip.h (tests/raster_ref.py) in depth BITS, face ids, hit words and drop
counts; lattice scenes whose answer is a literal; the edge cases of the rules, each shown from the restatement to be
reached; the named mutants of the restatement, which the cases must tell from the definition; and a convex box whose
silhouette is decided with exact fractions, sharing none of the restatement's arithmetic."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import raster_cases as RC
import raster_ref as RF
from vacancy_amd import capi
from vacancy_amd import carver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = list(RC.cases())


def host(name, **kw):
    v, f, views = RC.cases()[name]
    return carver.raster_mesh_host(v, f, views, **kw)


def stats(name, view=0):
    v, f, views = RC.cases()[name]
    s = {}
    RF.raster_view(v, f, views[view], stats=s)
    return s


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_restatement(name):
    got, want = host(name), RC.want(name)
    for i, (g, w) in enumerate(zip(got, want)):
        ctx = "%s view %d" % (name, i)
        assert np.array_equal(g["depth"].view(np.uint32), w["depth"].view(np.uint32)), ctx
        assert np.array_equal(g["face"], w["face"]), ctx
        assert np.array_equal(g["hits"], w["hits"]), ctx
        assert np.array_equal(g["n_dropped"], w["n_dropped"]), ctx
    assert len(got) == len(want)


def test_lattice_quad_is_the_plane_equation():
    """Identity ortho view, dyadic coordinates, doubled areas 64: every l_k and the depth are exact."""
    for got in (host("lattice_ortho")[0], RC.want("lattice_ortho")[0]):
        y, x = np.mgrid[0:RC.H, 0:RC.W]
        inside = (x >= 2) & (x <= 10) & (y >= 2) & (y <= 10)   # both ends of the box: min u and max u are integers
        plane = (4.0 + (x - 2) / 2.0 + (y - 2) / 4.0).astype(F)
        assert np.array_equal(got["depth"], np.where(inside, plane, F(np.inf)))
        # pixel centres exactly on the shared diagonal x + y == 12: hit, by the lower face
        assert np.array_equal(got["face"], np.where(inside, np.where(x + y <= 12, 0, 1), -1))
        assert got["face"][2, 2] == 0 and got["face"][10, 10] == 1 and got["face"][2, 10] == 0   # pixels exactly on vertices
        assert int(np.unpackbits(got["hits"].view(np.uint8)).sum()) == 81
    assert stats("lattice_ortho")["ties"] == 9   # the nine pixels of the diagonal meet two fragments of equal depth


def test_fronto_parallel_triangle_in_a_pinhole_is_its_depth():
    got = host("lattice_pinhole")[0]
    y, x = np.mgrid[0:RC.H, 0:RC.W]
    inside = (x >= 8) & (y >= 4) & ((x - 8) + (y - 4) <= 32)
    assert np.array_equal(got["depth"], np.where(inside, F(4.0), F(np.inf)))
    assert np.array_equal(got["face"], np.where(inside, 0, -1))


def test_coincident_faces_and_windings():
    got = host("coincident")[0]
    y, x = np.mgrid[0:RC.H, 0:RC.W]
    inside = (x >= 2) & (x <= 10) & (y >= 2) & (y <= 10)
    # faces 2, 3 repeat 0, 1 with the other winding at equal depth, 4, 5 lie 3 behind: the lower index wins, both windings draw
    assert np.array_equal(got["face"], np.where(inside, np.where(x + y <= 12, 0, 1), -1))
    assert stats("coincident")["ties"] >= 81
    v, f, views = RC.cases()["coincident"]
    flipped = carver.raster_mesh_host(v, f[[2, 3]], views)[0]
    assert np.array_equal(flipped["depth"], got["depth"])


def test_roi_edges_and_the_one_pixel_roi():
    got = host("roi_edges")
    y, x = np.mgrid[0:RC.H, 0:RC.W]
    plane = (4.0 + (x - 2) / 2.0 + (y - 2) / 4.0).astype(F)
    for g, (x0, y0, x1, y1) in zip(got, ((2, 2, 10, 10), (3, 4, 8, 6), (6, 6, 6, 6), (11, 2, 11, 2), (10, 10, 10, 10))):
        inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & (x >= 2) & (x <= 10) & (y >= 2) & (y <= 10)
        assert np.array_equal(g["depth"], np.where(inside, plane, F(np.inf)))
    assert got[3]["face"].max() == -1   # a ROI beside the quad
    assert got[2]["face"][6, 6] == 0 and (got[2]["face"] >= 0).sum() == 1   # one pixel, on the diagonal


def test_needles():
    got = host("needles")[0]
    s = stats("needles")
    assert s["boxes"][0] == 0 and s["boxes"][1] == 0   # boxes without a pixel centre: ceil(min) > floor(max)
    assert s["boxes"][2] > 0 and not (got["face"] == 0).any() and not (got["face"] == 1).any()
    assert (got["face"] == 2).any() and (got["face"] == 3).any()
    assert np.array_equal(got["n_dropped"], [0, 0])   # a face without candidates is drawn, not dropped


def test_drop_classes():
    got = host("degenerate")
    for g in got:   # collinear, a repeated index twice | a NaN vertex named twice, and again: the vertex comes first
        assert np.array_equal(g["n_dropped"], [2, 3])
        assert set(np.unique(g["face"])) == {-1, 3}
    pin, ortho = host("unusable")
    # pinhole: behind the camera, depth 0 (two vertices), NaN, inf, -inf, and both faces of the depth-0 edge
    assert np.array_equal(pin["n_dropped"], [7, 0]) and pin["face"].max() == -1
    # ortho: camera depth 0 is kept -- the faces 1 and 5 are drawn --, a negative depth is not
    assert np.array_equal(ortho["n_dropped"], [5, 0])
    assert set(np.unique(ortho["face"])) == {-1, 5} or set(np.unique(ortho["face"])) == {-1, 1, 5}
    assert ortho["depth"][2, 2] == 0.0 and not np.signbit(ortho["depth"][2, 2])


def test_the_box_is_part_of_the_definition():
    """A far vertex makes the two edges anchored at it vanish at every pixel in double: only the box keeps the column
    left of min u = 5.5 out.  The restatement shows it: with the box's ceil and floor swapped that column is hit."""
    got = host("far_vertex")[0]
    swapped = RC.want("far_vertex", {"boxswap"})[0]
    assert not (got["face"][:, 5] == 0).any() and (swapped["face"][:, 5] == 0).any()
    assert (got["face"][:, 6] == 0).any()
    assert np.array_equal(got["n_dropped"], [0, 1])   # the face that starts at the far vertex has A == 0


@pytest.mark.parametrize("mutant", [m for m in RF.MUTANTS if m != "zlt"])
def test_cases_tell_the_mutant_from_the_definition(mutant):
    small = [n for n in NAMES if n not in ("views_65", "box_192")]
    told = [n for n in small if not RF.same(RC.want(n, {mutant}), RC.want(n))]
    assert told, mutant
    for n in told:   # ... and the host function sides with the definition
        assert RF.same(host(n), RC.want(n)) and not RF.same(host(n), RC.want(n, {mutant}))


def test_camera_depth_zero_on_a_pinhole_is_dropped_by_either_reading():
    """The mutant "zlt" (pc[2] < 0 instead of <= 0) cannot be told from the definition by any mesh: at pc[2] == 0 a
    pinhole's u = fx / pc[2] * pc[0] + cx is infinite or NaN for every fx a view may have, so the vertex is unusable by
    the finiteness rule as well.  What can be checked is checked: the case reaches pc[2] == 0 on both camera kinds, the
    pinhole drops the face in class 0 under both readings, the ortho view keeps it."""
    v, f, views = RC.cases()["unusable"]
    pin, ortho = views
    assert RF.project(pin, v[3])[2] == 0 and not RF.project(pin, v[3])[3] and not RF.project(pin, v[3], {"zlt"})[3]
    assert not np.isfinite(RF.project(pin, v[3], {"zlt"})[0])
    assert RF.project(ortho, v[3])[2] == 0 and RF.project(ortho, v[3])[3]
    for n in NAMES:
        if n not in ("views_65", "box_192"):
            assert RF.same(RC.want(n, {"zlt"}), RC.want(n)), n


def hull(points):
    """Convex hull (counter-clockwise, exact) of points given as pairs of Fractions."""
    pts = sorted(set(points))
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])  # noqa: E731
    lower, upper = [], []
    for chain, seq in ((lower, pts), (upper, pts[::-1])):
        for p in seq:
            while len(chain) >= 2 and cross(chain[-2], chain[-1], p) <= 0:
                chain.pop()
            chain.append(p)
    return lower[:-1] + upper[:-1]


@pytest.mark.parametrize("name", ["box_12", "box_192"])
def test_convex_box_has_no_hole_and_no_pixel_outside(name):
    """The silhouette of a convex solid is the convex hull of its projected corners: decided per pixel centre with exact
    fractions from the projected float coordinates of the 8 corners (the midpoints of the fine box lie on its faces)."""
    v, f, views = RC.cases()[name]
    got = host(name)
    for i, view in enumerate(views):
        corners = [RF.project(view, p) for p in v[:8]]
        assert all(c[3] for c in corners)
        poly = hull([(Fraction(float(c[0])), Fraction(float(c[1]))) for c in corners])
        n = len(poly)
        want = np.zeros((view.height, view.width), bool)
        margin = None
        for y in range(view.height):
            for x in range(view.width):
                e = [(poly[(k + 1) % n][0] - poly[k][0]) * (y - poly[k][1]) - (poly[(k + 1) % n][1] - poly[k][1]) * (x - poly[k][0])
                     for k in range(n)]
                want[y, x] = all(t >= 0 for t in e)
                m = min(abs(t) for t in e)
                margin = m if margin is None or m < margin else margin
        # the fine box's midpoints project a rounding error away from the hull's edges: no pixel centre is that close
        assert margin > Fraction(1, 1000), (name, i, float(margin))
        bits = np.unpackbits(got[i]["hits"].view(np.uint8), bitorder="little").reshape(view.height, -1)[:, :view.width]
        assert np.array_equal(bits.astype(bool), want), (name, i)
        assert np.array_equal(got[i]["face"] >= 0, want) and np.array_equal(np.isfinite(got[i]["depth"]), want)
        assert want.sum() > 500


def test_the_cases_are_not_vacuous():
    """What the GPU tests rely on, from the restatement alone."""
    wide = 64   # the default of "rasterwide"
    boxes = [b for i in range(3) for b in stats("mixed", i)["boxes"]]
    assert any(b > wide for b in boxes) and any(0 < b <= wide for b in boxes) and any(b == 0 for b in boxes)
    assert max(stats("whole_image")["boxes"]) == RC.W * RC.H
    drops = np.sum([w["n_dropped"] for n in NAMES for w in RC.want(n)], axis=0)
    assert drops[0] > 0 and drops[1] > 0
    assert stats("lattice_ortho")["ties"] > 0 and sum(stats("mixed", i)["ties"] for i in range(3)) > 0
    assert all((w["face"] >= 0).any() for w in RC.want("views_65")[64:]) and len(RC.want("views_65")) == 65
    assert RC.cases()["box_12"][2][2].width == 130   # rows of three hit words, two of them crossed
    assert (RC.want("box_12")[2]["hits"][:, 1] != 0).any() and (RC.want("box_12")[2]["hits"][:, 0] != 0).any()


def raw_args(name="lattice_ortho"):
    v, f, views = RC.cases()[name]
    n = len(views)
    out = {"depth": [np.full((w.height, w.width), 77.0, F) for w in views],
           "face": [np.full((w.height, w.width), 77, np.int32) for w in views],
           "hits": [np.full((w.height, (w.width + 63) // 64), 77, np.uint64) for w in views],
           "n_dropped": np.full((n, 2), 77, np.int64)}
    arr = (capi.View * n)(*views)
    ptr = {k: (C.c_void_p * n)(*[a.ctypes.data for a in out[k]]) for k in ("depth", "face", "hits")}
    args = [len(v), len(f), v.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), n, arr, ptr["depth"], ptr["face"],
            ptr["hits"], out["n_dropped"].ctypes.data_as(C.c_void_p)]
    return (v, f, arr, ptr), args, out


def untouched(out):
    return all((a == 77).all() for k in ("depth", "face", "hits") for a in out[k]) and (out["n_dropped"] == 77).all()


def bad_face(keep, args, value):
    f = keep[1].copy()
    f[1, 1] = value
    args[3] = f.ctypes.data_as(C.c_void_p)
    return f


def bad_view(args, **fields):
    v = capi.View.from_buffer_copy(args[5][0])
    for k, x in fields.items():
        if k == "w2c0":
            v.w2c[0] = x
        elif k == "roi_max0":
            v.roi_max[0] = x
        else:
            setattr(v, k, x)
    args[5] = (capi.View * 1)(v)


BAD = {
    "face index too large": (lambda keep, args: bad_face(keep, args, 4), capi.VCY_ERR_INVALID_ARG),
    "face index negative": (lambda keep, args: bad_face(keep, args, -1), capi.VCY_ERR_INVALID_ARG),
    "no views": (lambda keep, args: args.__setitem__(4, 0), capi.VCY_ERR_INVALID_ARG),
    "null views": (lambda keep, args: args.__setitem__(5, None), capi.VCY_ERR_INVALID_ARG),
    "null vertices": (lambda keep, args: args.__setitem__(2, None), capi.VCY_ERR_INVALID_ARG),
    "null faces": (lambda keep, args: args.__setitem__(3, None), capi.VCY_ERR_INVALID_ARG),
    "negative vertex count": (lambda keep, args: args.__setitem__(0, -1), capi.VCY_ERR_INVALID_ARG),
    "negative face count": (lambda keep, args: args.__setitem__(1, -1), capi.VCY_ERR_INVALID_ARG),
    "roi outside": (lambda keep, args: bad_view(args, roi_max0=RC.W), capi.VCY_ERR_INVALID_ARG),
    "w2c not finite": (lambda keep, args: bad_view(args, w2c0=float("nan")), capi.VCY_ERR_INVALID_ARG),
    "pinhole fx 0": (lambda keep, args: bad_view(args, is_ortho=0, fx=0.0), capi.VCY_ERR_INVALID_ARG),
    "empty image": (lambda keep, args: bad_view(args, width=0), capi.VCY_ERR_INVALID_ARG),
    "too many faces": (lambda keep, args: args.__setitem__(1, (1 << 31) // 3 + 1), capi.VCY_ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("name", list(BAD))
def test_host_argument_errors_leave_the_outputs_untouched(name):
    lib = capi.load()
    keep, args, out = raw_args()
    change, status = BAD[name]
    held = change(keep, args)  # noqa: F841  (a replaced array lives until the call is over)
    assert lib.vcy_raster_mesh_host(*args) == status, name
    assert untouched(out), name
    assert carver.last_error()


def test_entry_checks_of_the_device_calls_need_no_context():
    """vcy_raster_mesh and vcy_mesh_agreement refuse their arguments before they look at the context."""
    lib = capi.load()
    for name, (change, status) in BAD.items():
        keep, args, out = raw_args()
        held = change(keep, args)  # noqa: F841
        assert lib.vcy_raster_mesh(None, *args) == status, name
        assert untouched(out), name
    keep, args, out = raw_args()
    assert lib.vcy_raster_mesh(None, *args) == capi.VCY_ERR_NOT_INITIALIZED and untouched(out)
    counts = np.full(3, 77, np.int64)
    mask = np.zeros((RC.H, RC.W), np.uint8)
    masks = (C.c_void_p * 1)(mask.ctypes.data)
    cp = counts.ctypes.data_as(C.c_void_p)
    assert lib.vcy_mesh_agreement(None, *args[:6], None, cp) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_mesh_agreement(None, *args[:6], masks, None) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_mesh_agreement(None, *args[:6], (C.c_void_p * 1)(None), cp) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_mesh_agreement(None, *args[:6], masks, cp) == capi.VCY_ERR_NOT_INITIALIZED
    assert (counts == 77).all()
    ms = C.c_float(5.0)
    assert lib.vcy_last_raster_ms(None, C.byref(ms), None) == capi.VCY_ERR_INVALID_ARG and ms.value == 5.0


def test_null_outputs_and_a_mesh_without_faces():
    lib = capi.load()
    for skip in (6, 7, 8, 9):
        keep, args, out = raw_args("roi_edges")
        args[skip] = None
        assert lib.vcy_raster_mesh_host(*args) == 0
        want = RC.want("roi_edges")
        for i, w in enumerate(want):
            assert skip == 6 or np.array_equal(out["depth"][i].view(np.uint32), w["depth"].view(np.uint32))
            assert skip == 7 or np.array_equal(out["face"][i], w["face"])
            assert skip == 8 or np.array_equal(out["hits"][i], w["hits"])
        assert (out["n_dropped"] == 77).all() if skip == 9 else (out["n_dropped"] == 0).all()
    # single entries
    keep, args, out = raw_args("roi_edges")
    args[6][1] = None
    args[8][0] = None
    assert lib.vcy_raster_mesh_host(*args) == 0
    assert (out["depth"][1] == 77).all() and (out["hits"][0] == 77).all() and np.isinf(out["depth"][0]).any()
    v, f, views = RC.cases()["lattice_ortho"]
    got = carver.raster_mesh_host(v, np.zeros((0, 3), np.int32), views)[0]
    assert np.isinf(got["depth"]).all() and (got["face"] == -1).all() and not got["hits"].any()
    got = carver.raster_mesh_host(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), views[0])
    assert (got["face"] == -1).all() and np.array_equal(got["n_dropped"], [0, 0])


def test_host_function_is_clean_under_host_sanitizers():
    """The stand-alone program of tests/raster_host_check.cpp: the host function and the agreement over its hit bits under
    AddressSanitizer and UBSan, on the CPU."""
    run = subprocess.run(["make", "-C", os.path.join(ROOT, "vacancy_amd", "csrc"), "-s", "raster_host_check"], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "raster_host_check: ok" in run.stdout
