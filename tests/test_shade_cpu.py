"""The shading pass's definition on the CPU: vcy_shade_mesh_host and vcy_mesh_photo_error_host (shade_host.hip) against the
numpy restatement of the section "shading a rasterised mesh" of vacancy_hip.h (tests/shade_ref.py) in float BITS of value
and bary, bytes of value8 and the seven sums; lattice scenes whose answer is a literal; the depth image as (float)(1 / T);
a slanted quad evaluated with exact fractions, sharing none of the restatement's arithmetic; the named mutants of the
restatement, which the cases must tell from the definition; and the argument contract."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import raster_cases as RC
import raster_ref as RF
import shade_cases as SC
import shade_ref as SF
from vacancy_amd import capi
from vacancy_amd import carver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = list(SC.cases())
SMALL = [n for n in NAMES if not n.startswith("views_65")]
PHOTO = list(SC.photo_cases())


def host(name, **kw):
    v, f, a, views, bg = SC.cases()[name]
    kw = dict(dict(value=True, value8=True, bary=True), **kw)
    return carver.shade_mesh_host(v, f, a, views, background=bg, **kw)


def host_error(name, masked=True):
    v, f, col, views, photos, masks = SC.photo_cases()[name]
    return carver.mesh_photo_error_host(v, f, col, views, photos, masks if masked and masks is not None else None)


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_restatement(name):
    got, want = host(name), SC.want(name)
    assert len(got) == len(want)
    same = SF.same_but_nan if name == "odd_values" else SF.same   # (only there may a NaN come out)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("value", "value8", "bary"):
            assert same([g], [w], (k,)), "%s view %d %s" % (name, i, k)
    if name != "odd_values":
        assert all(np.isfinite(w["value"]).all() for w in want)


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("name", PHOTO)
def test_host_error_equals_restatement(name, masked):
    got, want = host_error(name, masked), SC.photo_want(name, masked and SC.photo_cases()[name][5] is not None)
    assert got.dtype == np.int64 and np.array_equal(got, want), (name, masked)


def test_largest_term_against_literals():
    """Every hit pixel differs by 255 in red: n * 255 and n * 65025."""
    got = host_error("photo_255")[0]
    n = int((SC.photo_faces("photo_255")[0] >= 0).sum())
    assert n > 500 and got[0] == n and got[1] == n * 255 and got[4] == n * 65025


def test_lattice_quad_reproduces_a_linear_attribute_exactly():
    """Identity ortho view, dyadic coordinates, doubled areas 64: the weights are multiples of 1 / 64 and exact, and an
    attribute linear in (x, y) comes back as itself at every covered pixel."""
    v, f, views = RC.cases()["lattice_ortho"]
    lin = lambda x, y: np.stack([70.0 + 4.0 * x + 2.5 * y, 250.0 - 8.0 * x - 0.25 * y], axis=-1)  # noqa: E731
    a = lin(v[:, 0].astype(np.float64), v[:, 1].astype(np.float64)).astype(F)
    got = carver.shade_mesh_host(v, f, a, views, background=(1.0, 2.0), value=True, value8=True, bary=True)[0]
    y, x = np.mgrid[0:RC.H, 0:RC.W]
    inside = (x >= 2) & (x <= 10) & (y >= 2) & (y <= 10)
    want = np.where(inside[..., None], lin(x, y), np.array([1.0, 2.0])).astype(F)
    assert np.array_equal(got["value"], want)
    assert np.array_equal(got["value8"], np.floor(want + F(0.5)).astype(np.uint8))
    # face 0 = (0, 1, 2) below the diagonal: b = (1 - (x - 2) / 8 - (y - 2) / 8, (x - 2) / 8, (y - 2) / 8)
    lower = inside & (x + y <= 12)
    b = np.stack([1.0 - (x - 2) / 8.0 - (y - 2) / 8.0, (x - 2) / 8.0, (y - 2) / 8.0], axis=-1).astype(F)
    assert np.array_equal(got["bary"][lower], b[lower])
    assert not got["bary"][~inside].any()
    assert np.array_equal(got["bary"][2, 2], [1, 0, 0]) and np.array_equal(got["bary"][2, 10], [0, 1, 0])   # pixels on vertices


def test_fronto_parallel_triangle_in_a_pinhole_has_screen_space_weights():
    """All z_k equal: t_k = l_k / 4 exactly, T = 1 / 4, b_k == l_k."""
    got = host("lattice_pinhole")[0]
    y, x = np.mgrid[0:RC.H, 0:RC.W]
    inside = (x >= 8) & (y >= 4) & ((x - 8) + (y - 4) <= 32)
    l = np.stack([1.0 - (x - 8) / 32.0 - (y - 4) / 32.0, (x - 8) / 32.0, (y - 4) / 32.0], axis=-1).astype(F)
    assert np.array_equal(got["bary"][inside], l[inside]) and not got["bary"][~inside].any()
    assert SF.same(SC.want("lattice_pinhole", {"affine"}), SC.want("lattice_pinhole"))


@pytest.mark.parametrize("name", SMALL)
def test_depth_is_the_reciprocal_of_the_weights_T(name):
    """(float)(1.0 / T) of the T the weights are divided by is vcy_raster_mesh_host's depth, to the bit."""
    v, f, a, views, bg = SC.cases()[name]
    depth = [r["depth"] for r in carver.raster_mesh_host(v, f, views, face=False, hits=False)]
    seen = 0
    for view, d, w in zip(views, depth, SC.want(name)):
        hit = w["face"] >= 0
        assert np.array_equal(hit, np.isfinite(d))
        if not view.is_ortho and hit.any():
            z = (1.0 / w["T"][hit]).astype(F)
            assert np.array_equal(z.view(np.uint32), d[hit].view(np.uint32)), name
            seen += int(hit.sum())
    assert seen > 0 or all(view.is_ortho or not (w["face"] >= 0).any() for view, w in zip(views, SC.want(name)))


def correctly_rounded(x):
    """The float32 nearest to the Fraction x (ties to even cannot occur off a float's midpoint grid by accident: checked)."""
    r = F(float(x))
    best = r
    for c in (np.nextafter(r, F(-np.inf)), np.nextafter(r, F(np.inf))):
        if abs(Fraction(float(c)) - x) < abs(Fraction(float(best)) - x):
            best = c
    return best


def test_slanted_quad_against_exact_fractions():
    """The perspective-correct value from the float (u, w, z) of the corners and the float attributes in exact rational
    arithmetic, correctly rounded to float.  The bound is derived, not measured: with attributes in [64, 255] every term
    of the sum is non-negative, so nothing cancels behind the edge functions, whose differences of float coordinates are
    exact in double; the double evaluation is then below 2^-40 of the value away from the exact one, far under half a float
    ulp (2^-24), and only the final rounding can differ.  Hence 1 ulp.  The mutant "affine" is off by more than that at
    more than half of the covered pixels: the depth ratio across the quad is 3.5."""
    v, f, a, views, bg = SC.cases()["slanted_quad"]
    view = views[0]
    face = SC.faces_of("slanted_quad")[0]
    got = host("slanted_quad")[0]["value"]
    mutant = SC.want("slanted_quad", {"affine"})[0]["value"]
    proj = [RF.project(view, p) for p in v]
    zs = [float(p[2]) for p in proj]
    assert max(zs) / min(zs) >= 3.0 and a.min() >= 64.0 and a.max() <= 255.0
    U = [(Fraction(float(p[0])), Fraction(float(p[1])), Fraction(float(p[2]))) for p in proj]
    edge = lambda p, q, x, y: (q[0] - p[0]) * (y - p[1]) - (q[1] - p[1]) * (x - p[0])  # noqa: E731
    ys, xs = np.nonzero(face >= 0)
    assert len(xs) > 200
    off = 0
    for x, y in zip(xs.tolist(), ys.tolist()):
        i0, i1, i2 = (int(k) for k in f[face[y, x]])
        p0, p1, p2 = U[i0], U[i1], U[i2]
        area = edge(p0, p1, p2[0], p2[1])
        l = [edge(p1, p2, x, y) / area, edge(p2, p0, x, y) / area, edge(p0, p1, x, y) / area]
        t = [l[0] / p0[2], l[1] / p1[2], l[2] / p2[2]]
        T = sum(t)
        for c in range(3):
            exact = sum(t[k] / T * Fraction(float(a[i][c])) for k, i in enumerate((i0, i1, i2)))
            want = correctly_rounded(exact)
            ulps = abs(int(got[y, x, c].view(np.uint32)) - int(want.view(np.uint32)))
            assert ulps <= 1, (x, y, c, got[y, x, c], want)
            off += c == 0 and abs(int(mutant[y, x, 0].view(np.uint32)) - int(want.view(np.uint32))) > 1
    assert off > len(xs) / 2, (off, len(xs))


@pytest.mark.parametrize("mutant", ["affine", "perm", "sumorder", "floatacc", "trunc", "roi"])
def test_cases_tell_the_mutant_from_the_definition(mutant):
    told = [n for n in SMALL if n != "odd_values" and not SF.same(SC.want(n, {mutant}), SC.want(n))]
    assert told, mutant
    for n in told:   # ... and the host function sides with the definition
        assert SF.same(host(n), SC.want(n)) and not SF.same(host(n), SC.want(n, {mutant}))
    if mutant == "affine":
        assert "slanted_quad" in told
    if mutant == "roi":
        assert "roi_edges" in told and "roi_c1" in told


@pytest.mark.parametrize("mutant", ["bgcount", "nomask", "trunc", "perm"])
def test_photo_cases_tell_the_mutant_from_the_definition(mutant):
    told = [n for n in PHOTO if SC.photo_cases()[n][5] is not None
            and not np.array_equal(SC.photo_want(n, True, {mutant}), SC.photo_want(n, True))]
    assert told, mutant
    for n in told:
        assert np.array_equal(host_error(n), SC.photo_want(n)) and not np.array_equal(host_error(n), SC.photo_want(n, True, {mutant}))


def test_ties_take_the_lower_face():
    """coincident_split: face 1 repeats face 0 with vertex ids of its own and other attributes, face 2 is the other half of
    the quad with its own ids: every pixel of face 0 is a tie, and so is the diagonal."""
    v, f, a, views, bg = SC.cases()["coincident_split"]
    s = {}
    RF.raster_view(v, f, views[0], stats=s)
    assert s["ties"] >= 45 + 9
    got = host("coincident_split")[0]
    y, x = np.mgrid[0:RC.H, 0:RC.W]
    lower = (x >= 2) & (y >= 2) & (x + y <= 12)
    upper = (x <= 10) & (y <= 10) & (x + y > 12)
    assert np.array_equal(SC.faces_of("coincident_split")[0], np.where(lower, 0, np.where(upper, 2, -1)))
    red = got["value"][..., 0]
    assert (red[lower] >= 100).all() and (red[lower] <= 106).all()     # face 0's attributes (100 .. 106), not face 1's (200 .. 206)
    assert (red[upper] >= 150).all() and (red[upper] <= 156).all()     # face 2's, off the diagonal


def test_pixel_centres_on_a_shared_vertex_and_edge_take_the_winner():
    v, f, a, views, bg = SC.cases()["on_vertex"]
    proj = [RF.project(views[0], p) for p in v]
    assert [(float(p[0]), float(p[1])) for p in proj] == [(float(x), float(y)) for x, y in SC.ONVERTEX_PX]
    face = SC.faces_of("on_vertex")[0]
    got = host("on_vertex")[0]
    for k, (x, y) in enumerate(SC.ONVERTEX_PX):   # on the vertex: its weight is 1, its attribute comes back
        corner = list(f[face[y, x]]).index(k)
        assert face[y, x] == (1 if k == 3 else 0)
        assert got["bary"][y, x, corner] == 1.0 and np.array_equal(got["value"][y, x], a[k])
    for x, y in SC.ONEDGE_PX:   # on the shared edge (1, 2): face 0 wins, the weight of its corner 0 is 0
        assert face[y, x] == 0 and got["bary"][y, x, 0] == 0.0 and got["bary"][y, x, 1] > 0.0
        # ... and face 1 alone answers with a value that differs at most by rounding
        other = carver.shade_mesh_host(v, f[1:], a, views)[0]["value"][y, x]
        assert np.allclose(other, got["value"][y, x], rtol=1e-6, atol=0.0)


def test_the_cases_are_not_vacuous():
    """What the GPU tests rely on, from the restatement alone."""
    v, f, a, views, bg = SC.cases()["on_vertex"]
    face = SC.faces_of("on_vertex")[0]
    assert all(face[y, x] >= 0 for x, y in SC.ONVERTEX_PX)   # some pixel centre lies on a vertex, and is covered
    masked, plain = SC.photo_want("photo_sizes", True), SC.photo_want("photo_sizes", False)
    assert (masked[:, 0] == 0).any() and (plain[:, 0] > 0).all()   # a view with n == 0 under its silhouette
    assert (masked[:, 1:4] != plain[:, 1:4]).any() and (0 < masked[0, 0] < plain[0, 0])
    m65 = SC.photo_want("photo_65", True)
    assert len(m65) == 65 and m65[64, 0] > 0
    sizes = [(w.width, w.height) for w in SC.sized_views()]
    assert sizes == [(48, 40), (64, 33), (130, 37)]
    third = SC.faces_of("sizes_c1")[2]
    assert (third[:, :64] >= 0).any() and (third[:, 64:128] >= 0).any()   # hits in more than one word of a row
    assert all((w["face"] >= 0).sum() == 1 for w in [SC.want("roi_c2")[2]])   # the one-pixel ROI
    odd = SC.want("odd_values")
    assert any(np.isnan(w["value"]).any() for w in odd) and any(np.isinf(w["value"]).any() for w in odd)
    q = np.concatenate([w["value8"].reshape(-1) for w in odd])
    assert (q == 0).any() and (q == 255).any()
    assert np.array_equal(SF.quantize(np.array([np.nan, -1.0, 0.0, 0.49999997, 0.5, 1.5, 254.49998, 254.5, 255.0, 1e30, np.inf, -np.inf], F)),
                          [0, 0, 0, 1, 1, 2, 254, 255, 255, 255, 255, 0])   # (0.49999997f + 0.5f is one float add: it rounds to 1)
    assert np.array_equal(SC.want("roi_c4")[3]["value8"][0, 0], [7, 255, 0, 0])   # the background through q


def raw_args(name="lattice_ortho"):
    v, f, a, views, bg = SC.cases()[name]
    n, ch = len(views), a.shape[1]
    out = {"value": [np.full((w.height, w.width, ch), 77.0, F) for w in views],
           "value8": [np.full((w.height, w.width, ch), 77, np.uint8) for w in views],
           "bary": [np.full((w.height, w.width, 3), 77.0, F) for w in views]}
    arr = (capi.View * n)(*views)
    opt = capi.ShadeOption(ch, bg)
    ptr = {k: (C.c_void_p * n)(*[x.ctypes.data for x in out[k]]) for k in out}
    args = [len(v), len(f), v.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), n, arr,
            C.byref(opt), ptr["value"], ptr["value8"], ptr["bary"]]
    return (v, f, a, arr, opt, ptr), args, out


def untouched(out):
    return all((x == 77).all() for k in out for x in out[k])


def bad_face(keep, args, value):
    f = keep[1].copy()
    f[1, 1] = value
    args[3] = f.ctypes.data_as(C.c_void_p)
    return f


def bad_view(args, **fields):
    v = capi.View.from_buffer_copy(args[6][0])
    for k, x in fields.items():
        if k == "roi_max0":
            v.roi_max[0] = x
        else:
            setattr(v, k, x)
    args[6] = (capi.View * 1)(v)


def bad_channels(keep, args, ch):
    opt = capi.ShadeOption(ch, SC.BG)
    args[7] = C.byref(opt)
    return opt


BAD = {
    "null option": (lambda keep, args: args.__setitem__(7, None), capi.VCY_ERR_INVALID_ARG),
    "null attributes": (lambda keep, args: args.__setitem__(4, None), capi.VCY_ERR_INVALID_ARG),
    "no channels": (lambda keep, args: bad_channels(keep, args, 0), capi.VCY_ERR_INVALID_ARG),
    "five channels": (lambda keep, args: bad_channels(keep, args, 5), capi.VCY_ERR_INVALID_ARG),
    "face index too large": (lambda keep, args: bad_face(keep, args, 4), capi.VCY_ERR_INVALID_ARG),
    "face index negative": (lambda keep, args: bad_face(keep, args, -1), capi.VCY_ERR_INVALID_ARG),
    "no views": (lambda keep, args: args.__setitem__(5, 0), capi.VCY_ERR_INVALID_ARG),
    "null views": (lambda keep, args: args.__setitem__(6, None), capi.VCY_ERR_INVALID_ARG),
    "null vertices": (lambda keep, args: args.__setitem__(2, None), capi.VCY_ERR_INVALID_ARG),
    "null faces": (lambda keep, args: args.__setitem__(3, None), capi.VCY_ERR_INVALID_ARG),
    "negative vertex count": (lambda keep, args: args.__setitem__(0, -1), capi.VCY_ERR_INVALID_ARG),
    "roi outside": (lambda keep, args: bad_view(args, roi_max0=RC.W), capi.VCY_ERR_INVALID_ARG),
    "pinhole fx 0": (lambda keep, args: bad_view(args, is_ortho=0, fx=0.0), capi.VCY_ERR_INVALID_ARG),
    "too many faces": (lambda keep, args: args.__setitem__(1, (1 << 31) // 3 + 1), capi.VCY_ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("name", list(BAD))
def test_argument_errors_leave_the_outputs_untouched(name):
    """... of the host function, and of the device entry point, which refuses before it looks at its (NULL) context."""
    lib = capi.load()
    change, status = BAD[name]
    for call in (lib.vcy_shade_mesh_host, lambda *a: lib.vcy_shade_mesh(None, *a)):
        keep, args, out = raw_args()
        held = change(keep, args)  # noqa: F841  (a replaced array lives until the call is over)
        assert call(*args) == status, name
        assert untouched(out), name
        assert carver.last_error()


def test_error_calls_refuse_their_arguments_before_the_context():
    lib = capi.load()
    keep, args, out = raw_args()
    assert lib.vcy_shade_mesh(None, *args) == capi.VCY_ERR_NOT_INITIALIZED and untouched(out)
    v, f, a, arr, opt, ptr = keep
    sums = np.full(7, 77, np.int64)
    photo = np.zeros((RC.H, RC.W, 3), np.uint8)
    mask = np.ones((RC.H, RC.W), np.uint8)
    pp, mp, none = (C.c_void_p * 1)(photo.ctypes.data), (C.c_void_p * 1)(mask.ctypes.data), (C.c_void_p * 1)(None)
    sp = sums.ctypes.data_as(C.c_void_p)
    head = args[:7]
    for call in (lib.vcy_mesh_photo_error_host, lambda *x: lib.vcy_mesh_photo_error(None, *x)):
        assert call(*head, None, mp, sp) == capi.VCY_ERR_INVALID_ARG
        assert call(*head, pp, mp, None) == capi.VCY_ERR_INVALID_ARG
        assert call(*head, none, mp, sp) == capi.VCY_ERR_INVALID_ARG
        assert call(*head, pp, none, sp) == capi.VCY_ERR_INVALID_ARG
        assert call(*(head[:4] + [None] + head[5:]), pp, mp, sp) == capi.VCY_ERR_INVALID_ARG
        assert call(*(head[:5] + [0] + head[6:]), pp, mp, sp) == capi.VCY_ERR_INVALID_ARG
        assert (sums == 77).all()
    assert lib.vcy_mesh_photo_error(None, *head, pp, mp, sp) == capi.VCY_ERR_NOT_INITIALIZED
    assert lib.vcy_mesh_photo_error(None, *head, pp, None, sp) == capi.VCY_ERR_NOT_INITIALIZED and (sums == 77).all()
    assert lib.vcy_mesh_photo_error_host(*head, pp, None, sp) == 0 and sums[0] == 81
    ms = C.c_float(5.0)
    assert lib.vcy_last_shade_ms(None, C.byref(ms), None) == capi.VCY_ERR_INVALID_ARG and ms.value == 5.0


def test_null_outputs_and_single_null_entries():
    lib = capi.load()
    want = SC.want("roi_edges")
    for skip in (8, 9, 10):
        keep, args, out = raw_args("roi_edges")
        args[skip] = None
        assert lib.vcy_shade_mesh_host(*args) == 0
        for k, at in (("value", 8), ("value8", 9), ("bary", 10)):
            if at == skip:
                assert all((x == 77).all() for x in out[k])
            else:
                assert SF.same([{k: x} for x in out[k]], want, (k,))
    keep, args, out = raw_args("roi_edges")
    args[8][1] = None
    args[10][0] = None
    assert lib.vcy_shade_mesh_host(*args) == 0
    assert (out["value"][1] == 77).all() and (out["bary"][0] == 77).all()
    assert SF.same([{"value": out["value"][0]}], want[:1]) and SF.same([{"bary": out["bary"][1]}], want[1:2])
    # no vertices at all: the attributes may be NULL, every pixel is background
    view = RC.ortho_identity()
    got = carver.shade_mesh_host(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), np.zeros((0, 2), F), view, background=(3.0, 4.0),
                                 value8=True, bary=True)
    assert (got["value"] == [3.0, 4.0]).all() and (got["value8"] == [3, 4]).all() and not got["bary"].any()


def test_host_functions_are_clean_under_host_sanitizers():
    """The stand-alone program of tests/shade_host_check.cpp: both host functions under AddressSanitizer and UBSan, on the
    CPU."""
    run = subprocess.run(["make", "-C", os.path.join(ROOT, "vacancy_amd", "csrc"), "-s", "shade_host_check"], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "shade_host_check: ok" in run.stdout


def test_error_statistics_against_literals():
    s = carver.photo_error_stats(np.array([[4, 8, 0, 4, 16, 0, 4 * 65025], [0, 0, 0, 0, 0, 0, 0]], np.int64))
    assert s["n"].tolist() == [4, 0]
    assert s["mae"][0].tolist() == [2.0, 0.0, 1.0] and s["mse"][0].tolist() == [4.0, 0.0, 65025.0]
    assert s["psnr"][0, 0] == 10.0 * np.log10(65025.0 / 4.0) and np.isposinf(s["psnr"][0, 1]) and s["psnr"][0, 2] == 0.0
    assert s["mae_all"][0] == 1.0 and s["psnr_all"][0] == 10.0 * np.log10(65025.0 / ((16 + 4 * 65025) / 12.0))
    assert np.isnan(s["mae"][1]).all() and np.isnan(s["psnr"][1]).all() and np.isnan(s["psnr_all"][1])
    one = carver.photo_error_stats([10, 10, 20, 30, 10, 40, 90])
    assert one["mae"].tolist() == [1.0, 2.0, 3.0] and one["mse"].tolist() == [1.0, 4.0, 9.0] and one["mae_all"] == 2.0
