"""Scenes of the depth-carve tests, shared by the CPU tests of the host function and the GPU tests of the kernel: the grids
and view sets of robust_cases.py (pinhole and orthographic views, a shrunk and a one-pixel ROI, a camera that looks away),
four update modes, and depth images built around the grid's own camera depths so that a sample is clamped to 1, dropped
below -1, dropped as invalid and kept in between in every mode."""
import numpy as np

import depth_ref as DR
import oracle_lib as O
import robust_cases as RC
import test_gpu_render as TR
from vacancy_amd.capi import UpdateOption

F = np.float32
LOWEST = np.finfo(np.float32).min
W, H = RC.W, RC.H

DIMS = RC.DIMS
VIEW_SETS = RC.VIEW_SETS

# kwargs of UpdateOption.  "max_gate2": voxel_max_update_num = 2 stops a voxel after its third change, inside one call
MODES = {
    "max": dict(),
    "average_w1": dict(voxel_update=1, voxel_update_weight=1.0),
    "average_w07": dict(voxel_update=1, voxel_update_weight=0.7),
    "max_gate2": dict(voxel_max_update_num=2),
}

# (set, n_views, band): 70 views cross the 64-view launch.  A band of 2 has an exact reciprocal, so a plateau image can
# place samples at exactly 1 and -1; the other bands make the product e * inv_band round.
CALLS = [("mixed", 1, 2.0), ("pinhole", 5, 2.3), ("ortho", 5, 2.0), ("mixed", 70, 1.7)]


def option_for(dims, mode="max"):
    opt = RC.option_for(dims)
    opt.update_option = UpdateOption(**MODES[mode])
    return opt


def depth_image(kind, seed, opt, view, band):
    """kind 0: smooth, a tilted plane plus a paraboloid through the grid's range of camera depths; 1: white noise over that
    range and a band and a half beyond it; 2: plateaus -- every pixel a voxel lands on holds that voxel's camera depth
    plus band, minus band or unchanged, so that d is exactly 1 or -1 where the sum is exact; 3: the smooth image poisoned at
    2 % each with NaN, +inf, -inf, 0, -1 and lowest()."""
    rng = np.random.RandomState(2000 + seed)
    w, h = view.width, view.height
    px, py, pz = DR.positions(opt)
    ok, xi, yi, pc2 = DR.project(view, px, py, pz)
    lo, hi = (float(pc2[ok].min()), float(pc2[ok].max())) if ok.any() else (4.0, 8.0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) + 0.25 * band
    yy, xx = np.mgrid[0:h, 0:w]
    sx, sy = (xx - 0.5 * w) / w, (yy - 0.5 * h) / h
    a, b, c = rng.uniform(-1.0, 1.0, 3)
    smooth = (mid + half * (a * sx + b * sy) + 2.0 * half * c * (sx * sx + sy * sy)).astype(F)
    if kind == 0:
        img = smooth
    elif kind == 1:
        img = rng.uniform(lo - 1.5 * band, hi + 1.5 * band, (h, w)).astype(F)
    elif kind == 2:
        img = (np.round(smooth * 4) / 4).astype(F)
        rows = np.nonzero(ok)[0]
        rows = rows[rng.permutation(len(rows))]  # (of the voxels of a pixel a random one wins)
        step = rng.randint(0, 3, len(rows)) - 1
        with np.errstate(all="ignore"):
            img[yi[rows], xi[rows]] = pc2[rows] + (step * band).astype(F)
    else:
        img = smooth.copy()
        for value in (np.nan, np.inf, -np.inf, 0.0, -1.0, LOWEST):
            img[rng.rand(h, w) < 0.02] = value
    return np.ascontiguousarray(img, F)


_scenes = {}


def scene(dims, set_name, n_views, band):
    """(views, depth images): the views of the set taken in turn, every index with an image of its own."""
    key = (tuple(dims), set_name, n_views, band)
    if key not in _scenes:
        table = TR.views_for(tuple(dims))
        names = VIEW_SETS[set_name]
        views = [table[names[i % len(names)]] for i in range(n_views)]
        opt = option_for(dims)
        depths = [depth_image((i + 2) % 4, 11 * i + len(names), opt, v, band) for i, v in enumerate(views)]
        _scenes[key] = (views, depths)
    return _scenes[key]


_bases = {}


def base_state(dims, mode):
    """(sdf, update_num) the oracle carved from two silhouette views of robust_cases: a state to carve depth on top of."""
    key = (tuple(dims), mode)
    if key not in _bases:
        views, sdfs = RC.scene(dims, "mixed", 2)
        prev = O.set_num_threads(1)
        try:
            g = O.OracleGrid(option_for(dims, mode))
            for v, s in zip(views, sdfs):
                g.carve(v, s)
            _bases[key] = g.download()
            g.close()
        finally:
            O.set_num_threads(prev)
    s, u = _bases[key]
    return s.copy(), u.copy()


_wants = {}


def want(dims, mode, call, on_base):
    """The restatement's (sdf, update_num, stats) of a case, computed once and handed out unchanged."""
    key = (tuple(dims), mode, call, bool(on_base))
    if key not in _wants:
        set_name, nv, band = call
        views, depths = scene(dims, set_name, nv, band)
        stats = {}
        s0, u0 = base_state(dims, mode) if on_base else (None, None)
        sdf, cnt = DR.carve_depth(option_for(dims, mode), views, depths, band, s0, u0, stats=stats)
        sdf.setflags(write=False)
        cnt.setflags(write=False)
        _wants[key] = (sdf, cnt, stats)
    return _wants[key]


# ---- the concavity scene: a ball with a dent no silhouette can see -------------------------------------------------------

DENT_C = np.array([0.0, 0.0, 14.0])


def implicit(p):
    """s(p) = max(|p| - 14, 8 - |p - (0, 0, 14)|) in float64: a ball of radius 14 minus a ball of radius 8; p [..., 3]."""
    return np.maximum(np.linalg.norm(p, axis=-1) - 14.0, 8.0 - np.linalg.norm(p - DENT_C, axis=-1))


_concavity = {}


def concavity_scene():
    """dict: opt(mode), the six orthographic 64 x 64 views along +-x, +-y, +-z from distance 30 (image centre on the axis),
    their analytic depth images (the implicit function marched along every pixel's ray at a step of 0.02), the voxel
    centres (float64 [n, 3]), s at them, the voxels of the dent and those of them hidden from every silhouette."""
    if not _concavity:
        from vacancy_amd.capi import CarverOption
        import render_ref as RR

        def opt(mode="max"):
            return CarverOption(bb_min=[-20.0] * 3, bb_max=[20.0] * 3, resolution=1.0, update_option=UpdateOption(**MODES[mode]))

        views = []
        for axis in range(3):
            for sign in (1.0, -1.0):
                pos = [0.0, 0.0, 0.0]
                pos[axis] = 30.0 * sign
                views.append(TR.look(pos, (0.0, 0.0, 0.0), ortho=True, up=(0.0, 0.0, 1.0) if axis == 1 else (0.0, 1.0, 0.0), w=64, h=64))
        step = 0.02
        t = np.arange(0.0, 60.0, step)
        depths = []
        for v in views:
            o, d, _ = RR.rays(v)  # (point = o + t d, t the camera depth)
            o, d = o.astype(np.float64).T, d.astype(np.float64).T
            first = np.full(len(o), np.inf)
            for t0 in range(0, len(t), 250):
                tt = t[t0:t0 + 250]
                inside = implicit(o[:, None, :] + tt[None, :, None] * d[:, None, :]) <= 0.0
                hit = inside.any(axis=1) & np.isinf(first)
                first[hit] = tt[inside[hit].argmax(axis=1)]
            depths.append(first.reshape(64, 64).astype(F))
        px, py, pz = DR.positions(opt())
        p = np.stack([px, py, pz], axis=1).astype(np.float64)
        dent = (np.linalg.norm(p - DENT_C, axis=1) <= 6.5) & (np.linalg.norm(p, axis=1) <= 14.0)
        # the dent voxels no silhouette of the six views can reach: along each of the three axes the line through the voxel
        # passes through the object at least one pixel (= one world unit) deep, so every view's nearest pixel and its
        # bilinear neighbours lie inside the silhouette.  The rest of the dent IS seen from the side -- the rays along x and y
        # just below the pole pass through the dent alone -- and a visual hull carves it.
        hidden = dent.copy()
        tt = np.arange(-40.0, 40.0, 0.05)
        for axis in range(3):
            e = np.zeros(3)
            e[axis] = 1.0
            through = (implicit(p[dent][:, None, :] + tt[None, :, None] * e) <= -1.0).any(axis=1)
            hidden[np.nonzero(dent)[0][~through]] = False
        _concavity.update(opt=opt, views=views, depths=depths, p=p, s=implicit(p), dent=dent, hidden=hidden)
    return _concavity


def assert_concavity(sdf, cnt, touched_only=False):
    """The property: outside the object by 1.5 -> sdf > 0; inside by 1.5 -> sdf < 0 (an untouched voxel is at lowest());
    every voxel of the dent is carved.  touched_only: the first two only where update_num >= 1."""
    c = concavity_scene()
    sel = (cnt >= 1) if touched_only else np.ones(len(cnt), bool)
    out, ins = sel & (c["s"] >= 1.5), sel & (c["s"] <= -1.5)
    assert out.sum() > 1000 and ins.sum() > 1000 and c["dent"].sum() > 100
    assert (sdf[out] > 0).all(), "%d voxels outside the object are not carved" % int((~(sdf[out] > 0)).sum())
    assert (sdf[ins] < 0).all(), "%d voxels inside the object are carved" % int((~(sdf[ins] < 0)).sum())
    assert (sdf[c["dent"]] > 0).all(), "%d of %d dent voxels are still solid" % (int((~(sdf[c["dent"]] > 0)).sum()), int(c["dent"].sum()))
