"""vcy_color_vertices_host (color.hip's serial host function; needs no GPU) against the numpy restatement of its definition
(tests/color_ref.py): rgb BITS, n_used and best_view are compared for equality, every case in the three modes and with
both samplers; then the properties the cases were built for, and every argument error with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import color_cases as CC
import color_ref as CR
from vacancy_amd import capi, carver

F = np.float32


def host(case, mode, interp, vertices=None, normals=None):
    c = CC.cases()[case]
    return carver.color_vertices_host(CC.points() if vertices is None else vertices, c["views"], c["photos"], c["depth"],
                                      CC.normals() if normals is None else normals, mode, interp, c["tol"], c["min_cos"],
                                      c["fallback"])


@pytest.mark.parametrize("interp", CC.INTERPS, ids=["nn", "bilinear"])
@pytest.mark.parametrize("mode", CC.MODES, ids=["mean", "weighted", "best"])
@pytest.mark.parametrize("case", CC.CASE_NAMES)
def test_host_equals_restatement(case, mode, interp):
    got = host(case, mode, interp)
    CC.assert_equal(got, CC.want(case, mode, interp), "%s mode %d interp %d" % (case, mode, interp))
    if case == "two_identical_views":   # ties go to the lower index
        assert set(np.unique(got["best_view"]).tolist()) == {-1, 0}
        assert set(np.unique(got["n_used"]).tolist()) == {0, 2}
    if case == "single_view":
        assert set(np.unique(got["n_used"]).tolist()) == {0, 1}


def test_the_cases_are_not_vacuous():
    """What the constructed points and images are there for does occur."""
    rgb, n_used, best = CC.want("render_depth", CR.WEIGHTED, CR.BILINEAR)
    _, n_inf, _ = CC.want("inf_depth_mincos", CR.MEAN, CR.NN)
    _, n_mc, _ = CC.want("inf_depth_mincos", CR.WEIGHTED, CR.NN)
    _, n_tol0, _ = CC.want("const_depth_tol0", CR.MEAN, CR.NN)
    _, n_chk, _ = CC.want("checker_depth", CR.MEAN, CR.NN)
    fb = np.array(CC.cases()["render_depth"]["fallback"], F)
    assert (n_used == 0).sum() > 50 and np.all(rgb[n_used == 0] == fb) and np.all(best[n_used == 0] == -1)
    assert (n_used >= 3).sum() > 200 and len(np.unique(best)) > 6
    assert n_inf.max() >= 8                      # nothing is occluded under all-miss depth
    assert np.all(n_mc <= n_inf) and (n_mc < n_inf).sum() > 300      # min_cos and the NaN / zero normals drop views
    assert np.all(n_tol0 <= n_inf) and (n_tol0 < n_inf).sum() > 100 and n_tol0.max() > 0   # the depth test bites both ways
    assert np.all(n_chk <= n_inf) and (n_chk < n_inf).sum() > 100 and n_chk.max() > 0
    p = CC.points()
    assert np.all(n_inf[~np.isfinite(p).all(axis=1)] == 0)       # NaN and inf points project nowhere
    _, n70, b70 = CC.want("70_views_8x8", CR.BEST, CR.BILINEAR)
    assert b70.max() >= 64 and n70.max() > 3                    # views of the second chunk contribute


def test_rounding_rule_and_roi_edges_by_hand():
    """One identity ortho view, NN, all-miss depth: u = x + 24, w = y + 20 exactly; the texel is the one at the
    half-away-from-zero rounding, clamped into the ROI; coordinates outside the ROI, by however little, do not count."""
    vs = CC.views()
    v = vs["ortho_axis_roi"]                     # ROI (5, 4) - (40, 33)
    photo = CC.photos([v], 21)[0]
    depth = [np.full((CC.H, CC.W), np.inf, F)]
    cases = [((12.5, 7.5), (13, 8)), ((13.5, 8.5), (14, 9)), ((5.0, 4.0), (5, 4)), ((40.0, 33.0), (40, 33)),
             ((4.5, 10.0), None), ((40.5, 10.0), None), ((5.0 - 2.0 ** -10, 10.0), None), ((40.25, 33.0), None),
             ((39.5, 32.5), (40, 33)), ((5.25, 4.49), (5, 4))]
    pts = np.array([(u - 24.0, w - 20.0, 1.0) for (u, w), _ in cases], F)
    got = carver.color_vertices_host(pts, [v], [photo], depth, None, CR.MEAN, CR.NN, 0.0, 0.0, (1.0, 2.0, 3.0))
    for k, (_, texel) in enumerate(cases):
        if texel is None:
            assert got["n_used"][k] == 0 and got["best_view"][k] == -1 and got["rgb"][k].tolist() == [1.0, 2.0, 3.0], k
        else:
            assert got["n_used"][k] == 1 and got["best_view"][k] == 0, k
            assert got["rgb"][k].tolist() == photo[texel[1], texel[0]].astype(F).tolist(), k
    # camera depth exactly 0 is kept (only pc[2] < 0 is skipped), just behind the plane is not
    z0 = F(-(CC.E + 3.0))
    pts = np.array([(0.0, 0.0, z0), (0.0, 0.0, np.nextafter(z0, F(-100.0)))], F)
    got = carver.color_vertices_host(pts, [vs["ortho_axis"]], [photo], depth, None, CR.MEAN, CR.NN, 0.0, 0.0, (1.0, 2.0, 3.0))
    assert got["n_used"].tolist() == [1, 0]
    # ... and on the pinhole 0 / 0 is NaN: outside
    got = carver.color_vertices_host(pts[:1], [vs["pinhole_axis"]], [photo], depth, None, CR.MEAN, CR.NN, 0.0, 0.0, (1.0, 2.0, 3.0))
    assert got["n_used"].tolist() == [0]
    # a weight of exactly 0 does not pass min_cos = 0; the sign of the normal does not matter
    nrm = np.array([(1.0, 0.0, 0.0), (0.0, 0.6, 0.8), (0.0, -0.6, -0.8)], F)
    pts = np.array([(0.0, 0.0, 1.0)] * 3, F)
    got = carver.color_vertices_host(pts, [vs["ortho_axis"]], [photo], depth, nrm, CR.WEIGHTED, CR.NN, 0.0, 0.0, (1.0, 2.0, 3.0))
    assert got["n_used"].tolist() == [0, 1, 1] and np.array_equal(got["rgb"][1], got["rgb"][2])


def test_empty_input_and_null_outputs():
    lib = capi.load()
    c = CC.cases()["single_view"]
    keep, args, out = carver._color_args(CC.points(), c["views"], c["photos"], None, c["depth"], CR.MEAN, CR.NN, 0.5, 0.0,
                                         (1.0, 2.0, 3.0))
    full = carver.color_vertices_host(CC.points(), c["views"], c["photos"], c["depth"], None, CR.MEAN, CR.NN, 0.5, 0.0, (1.0, 2.0, 3.0))
    a = list(args)
    a[9] = a[10] = None   # n_used_out, best_view_out
    assert lib.vcy_color_vertices_host(*a) == 0, carver.last_error()
    assert np.array_equal(CC.bits(out["rgb"]), CC.bits(full["rgb"]))
    a = list(args)
    a[0] = 0
    out["rgb"][:] = -7.0
    assert lib.vcy_color_vertices_host(*a) == 0
    assert np.all(out["rgb"] == F(-7.0))


def bad_calls():
    """name -> (positional-argument index -> replacement) | a function changing option / views of a fresh argument set"""
    def opt(**kw):
        def change(keep, a):
            o = keep[4]
            for k, v in kw.items():
                setattr(o, k, v)
        return change

    def view(field, value, index=None):
        def change(keep, a):
            v = keep[5][0]
            if index is None:
                setattr(v, field, value)
            else:
                getattr(v, field)[index] = value
        return change

    def null(i):
        def change(keep, a):
            a[i] = None
        return change

    def null_entry(which):
        def change(keep, a):
            keep[which][0] = None
        return change

    def n_views(n):
        def change(keep, a):
            a[3] = n
        return change

    return {
        "null vertices": null(1), "null views": null(4), "null photos": null(5), "null option": null(7), "null rgb": null(8),
        "null photo entry": null_entry(6), "null depth entry": null_entry(7),
        "n_views 0": n_views(0), "n_views -1": n_views(-1),
        "mode 3": opt(mode=3), "mode -1": opt(mode=-1), "interp 2": opt(interp=2),
        "tolerance < 0": opt(depth_tolerance=-0.5), "tolerance nan": opt(depth_tolerance=float("nan")),
        "tolerance inf": opt(depth_tolerance=float("inf")), "min_cos < 0": opt(min_cos=-0.1),
        "min_cos nan": opt(min_cos=float("nan")), "min_cos inf": opt(min_cos=float("inf")),
        "null normals weighted": lambda keep, a: (setattr(keep[4], "mode", 1), a.__setitem__(2, None)),
        "null normals best": lambda keep, a: (setattr(keep[4], "mode", 2), a.__setitem__(2, None)),
        "view nan": view("w2c", float("nan"), 3), "view fx 0": view("fx", 0.0), "view fy 0": view("fy", 0.0),
        "view width 0": view("width", 0), "view height -1": view("height", -1), "view roi": view("roi_max", CC.H, 1),
    }


BAD = bad_calls()


def fresh_args(with_depth=True):
    c = CC.cases()["render_depth"]
    vs = [capi.View.from_buffer_copy(v) for v in c["views"][:2]]      # pinhole views: fx and fy matter
    keep, args, out = carver._color_args(CC.points()[:50], vs, c["photos"][:2], CC.normals()[:50],
                                         c["depth"][:2] if with_depth else None, CR.MEAN, CR.NN, 0.5, 0.0, (1.0, 2.0, 3.0))
    for o in out.values():
        o[...] = 77
    return list(keep), list(args), out


@pytest.mark.parametrize("name", sorted(BAD))
def test_host_argument_errors_leave_the_outputs_untouched(name):
    lib = capi.load()
    keep, args, out = fresh_args()
    assert lib.vcy_color_vertices_host(*args) == 0, carver.last_error()   # the arguments are fine before the change
    for o in out.values():
        o[...] = 77
    BAD[name](keep, args)
    assert lib.vcy_color_vertices_host(*args) == capi.VCY_ERR_INVALID_ARG, name
    assert carver.last_error()
    assert all(np.all(o == 77) for o in out.values()), name


def test_host_needs_depth_and_device_entry_checks_before_the_context():
    lib = capi.load()
    keep, args, out = fresh_args(with_depth=False)
    assert lib.vcy_color_vertices_host(*args) == capi.VCY_ERR_INVALID_ARG
    # the device entry point checks its arguments before it looks at the context
    for name in ("mode 3", "n_views 0", "null photos", "view fx 0", "null normals best"):
        keep, args, out = fresh_args()
        BAD[name](keep, args)
        assert lib.vcy_color_vertices(None, 0.0, *args) == capi.VCY_ERR_INVALID_ARG, name
    keep, args, out = fresh_args()
    assert lib.vcy_color_vertices(None, 0.0, *args) == capi.VCY_ERR_NOT_INITIALIZED
    assert all(np.all(o == 77) for o in out.values())
    ms = C.c_float(-1.0)
    assert lib.vcy_last_color_ms(None, C.byref(ms)) == capi.VCY_ERR_INVALID_ARG


def test_python_wrapper_refuses_mismatched_arrays():
    c = CC.cases()["single_view"]
    with pytest.raises(ValueError):
        carver.color_vertices_host(CC.points(), c["views"], [c["photos"][0][:, :, :2]], c["depth"])
    with pytest.raises(ValueError):
        carver.color_vertices_host(CC.points(), c["views"], c["photos"], [c["depth"][0][:-1]])
    with pytest.raises(ValueError):
        carver.color_vertices_host(CC.points(), c["views"], c["photos"], c["depth"], CC.normals()[:-1])
