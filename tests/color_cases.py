"""The cases the CPU and the GPU tests of the vertex colouring share (tests/test_color_cpu.py, tests/test_gpu_color.py):
the grid and the view families of tests/test_gpu_render.py, 2 000 points, random photographs, depth images and normals,
and the numpy restatement's answer for every (case, mode, sampler), computed once."""
import numpy as np

import color_ref as CR
import render_ref as RR
import test_gpu_render as TR
from vacancy_amd.capi import make_view

F = np.float32
DIMS = (24, 20, 17)
W, H = TR.W, TR.H
MODES = (CR.MEAN, CR.WEIGHTED, CR.BEST)
INTERPS = (CR.NN, CR.BILINEAR)
E = float(max(DIMS))

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def option():
    return TR.grid_option(DIMS)


def views():
    """The families of test_gpu_render, one view of 31 x 17, and three views whose rotation is the identity, so that
    points can be placed on exact pixel coordinates: ortho with the whole image and with a shrunk ROI, and a pinhole."""
    def make():
        vs = dict(TR.views_for(DIMS))
        vs["small_31x17"] = TR.look(np.array([-1.1, 0.8, 1.5]) * E, (0.0, 0.0, 0.0), 22.0, w=31, h=17)
        ident = np.zeros((3, 4), F)
        ident[:, :3] = np.eye(3)
        ident[:, 3] = (W // 2, H // 2, E + 3.0)
        vs["ortho_axis_roi"] = make_view(ident, 1.0, 1.0, 0.0, 0.0, W, H, (5, 4), (40, 33), True)
        pin = ident.copy()
        pin[:, 3] = (0.0, 0.0, E + 3.0)
        vs["pinhole_axis"] = make_view(pin, F(32.0), F(32.0), F(24.0), F(20.0), W, H)
        return vs
    return memo("views", make)


def points():
    """1 600 uniform in the box enlarged by 20 %, 400 constructed: on the ROIs' edges and corners and on x.5 pixel
    coordinates of the identity views, at camera depth 0, and with NaN and inf components."""
    def make():
        rng = np.random.RandomState(11)
        half = np.array(TR.BOX[DIMS]) / 2.0 * 1.2
        p = ((rng.rand(2000, 3) * 2.0 - 1.0) * half).astype(F)
        k = 1600
        # the identity ortho views: u = x + 24, w = y + 20, depth = z + 27, all exact for these values
        edge_u = [0.0, 47.0, 5.0, 40.0, 4.5, 40.5, 12.5, 13.5, -0.5, 47.5, 47.25, 5.0 - 2.0 ** -10, 23.0]
        edge_w = [0.0, 39.0, 4.0, 33.0, 3.5, 33.5, 7.5, 8.5, -0.5, 39.5, 39.25, 4.0 - 2.0 ** -10, 19.0]
        for u in edge_u:
            for w in edge_w:
                p[k] = (u - 24.0, w - 20.0, float(rng.randint(-8, 9)))
                k += 1
        # camera depth exactly 0 of the identity views, on and off the axis
        for x, y in ((0.0, 0.0), (1.0, 0.0), (0.0, -2.0), (3.0, 4.0), (-24.0, -20.0)):
            p[k] = (x, y, -(E + 3.0))
            k += 1
        # just behind and just in front of that plane
        p[k], p[k + 1] = (0.0, 0.0, np.nextafter(F(-(E + 3.0)), F(-100.0))), (0.0, 0.0, np.nextafter(F(-(E + 3.0)), F(0.0)))
        k += 2
        for bad in (np.nan, np.inf, -np.inf):
            for axis in range(3):
                p[k] = (1.0, 2.0, 3.0)
                p[k, axis] = bad
                k += 1
            p[k] = (bad, bad, bad)
            k += 1
        # pixel centres of the identity ortho views at the depth of the box' middle: x.0 coordinates
        while k < 2000:
            p[k] = (float(rng.randint(-24, 24)), float(rng.randint(-20, 20)), float(rng.randint(-8, 9)) + 0.25)
            k += 1
        return p
    return memo("points", make)


def normals():
    """Random unit vectors, with exact zeros, NaNs and normals orthogonal to the z axis (the viewing axis of the identity
    views: their weight there is exactly 0) among them."""
    def make():
        rng = np.random.RandomState(12)
        n = rng.randn(2000, 3)
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
        n[5::40] = 0.0
        n[7::40] = np.nan
        n[9::40, 0] = np.nan
        n[11::20, 2] = 0.0          # nc[2] == 0 for R = identity
        n[1600:1700:3] = (1.0, 0.0, 0.0)
        n[1601:1700:3] = (0.0, 0.0, -1.0)
        return n
    return memo("normals", make)


def photos(vs, seed=13):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (v.height, v.width, 3)).astype(np.uint8) for v in vs]


def random_state():
    """The random 30 % state of test_gpu_render at DIMS: (sdf, cnt, iso)."""
    return memo("state", lambda: TR.states_for(DIMS)["random"])


def depth_images(vs, kind):
    if kind == "render":
        sdf, cnt, iso = random_state()
        solid = RR.solid_mask(sdf, cnt, iso)
        planes = RR.option_planes(option())
        return [RR.render(v, planes, DIMS, solid)[0] for v in vs]
    out = []
    for v in vs:
        if kind == "const":
            d = np.full((v.height, v.width), 30.0, F)
        elif kind == "inf":
            d = np.full((v.height, v.width), np.inf, F)
        else:  # a checkerboard of 0 and +inf
            yy, xx = np.meshgrid(np.arange(v.height), np.arange(v.width), indexing="ij")
            d = np.where((xx + yy) % 2 == 0, F(0.0), F(np.inf)).astype(F)
        out.append(d)
    return out


def tiny_views(n=70):
    """n views of 8 x 8 pixels around the grid, pinhole and ortho in turn: more than one chunk of 64."""
    rng = np.random.RandomState(14)
    out = []
    for i in range(n):
        pos = rng.randn(3)
        pos = pos / np.linalg.norm(pos) * E * (1.2 + rng.rand())
        if i % 3 == 2:
            v = TR.look(pos, rng.randn(3) * 4.0, ortho=True, w=8, h=8)   # (a pixel is a world unit: a beam of 8 x 8)
        else:
            v = TR.look(pos, rng.randn(3) * 2.0, 4.0 + 4.0 * rng.rand(), w=8, h=8)
        out.append(v)
    return out


def tiny_depths(vs):
    rng = np.random.RandomState(15)
    out = []
    for v in vs:
        d = (E * (0.5 + 2.5 * rng.rand(v.height, v.width))).astype(F)
        d[rng.rand(v.height, v.width) < 0.3] = np.inf
        out.append(d)
    return out


def cases():
    """name -> dict(views, photos, depth, tol, min_cos, fallback); vertices and normals are points() and normals()."""
    def make():
        vs = list(views().values())
        ph = photos(vs)
        fb = (128.0, 64.5, 3.0)
        out = {
            "render_depth": dict(views=vs, photos=ph, depth=depth_images(vs, "render"), tol=0.75, min_cos=0.0, fallback=fb),
            "const_depth_tol0": dict(views=vs, photos=ph, depth=depth_images(vs, "const"), tol=0.0, min_cos=0.0, fallback=fb),
            "inf_depth_mincos": dict(views=vs, photos=ph, depth=depth_images(vs, "inf"), tol=1000.0, min_cos=0.5, fallback=fb),
            "checker_depth": dict(views=vs, photos=ph, depth=depth_images(vs, "checker"), tol=0.0, min_cos=0.0, fallback=fb),
        }
        tv = tiny_views()
        out["70_views_8x8"] = dict(views=tv, photos=photos(tv, 16), depth=tiny_depths(tv), tol=1.0, min_cos=0.1, fallback=fb)
        out["single_view"] = dict(views=vs[:1], photos=ph[:1], depth=depth_images(vs[:1], "render"), tol=0.75, min_cos=0.0,
                                  fallback=fb)
        two = [vs[0], vs[0]]
        out["two_identical_views"] = dict(views=two, photos=[ph[0], ph[0]], depth=depth_images(two, "inf"), tol=0.0,
                                          min_cos=0.0, fallback=fb)
        return out
    return memo("cases", make)


CASE_NAMES = ["render_depth", "const_depth_tol0", "inf_depth_mincos", "checker_depth", "70_views_8x8", "single_view",
              "two_identical_views"]


def want(name, mode, interp):
    """The restatement's (rgb, n_used, best_view) of a case."""
    def make():
        c = cases()[name]
        return CR.color_vertices(points(), normals(), c["views"], c["photos"], c["depth"], mode, interp, c["tol"],
                                 c["min_cos"], c["fallback"])
    return memo(("want", name, mode, interp), make)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_equal(got, ref, ctx):
    rgb, n_used, best = ref
    assert np.array_equal(got["n_used"], n_used), "%s: %d n_used differ" % (ctx, int((got["n_used"] != n_used).sum()))
    assert np.array_equal(got["best_view"], best), "%s: %d best_view differ" % (ctx, int((got["best_view"] != best).sum()))
    bad = np.nonzero((bits(got["rgb"]) != bits(rgb)).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d colours differ, first at vertex %d: %r != %r" % (ctx, len(bad), bad[0], got["rgb"][bad[0]],
                                                                               rgb[bad[0]])
