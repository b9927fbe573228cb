"""Needle scenes: grid states and SDF images on which the carve kernels' drop bounds decide the result by one pixel.

The state is uploaded with every count >= 1 and sdf = c plus a small non-negative per-voxel jitter, one voxel per 8^3
brick exactly at c, so a brick's minimum is a single voxel.  Every image is a background that changes nothing (below
every state value for kMax, below the truncation limit for the truncation drop, above it for the truncation test of
the weighted average) with sparse needles (or pits) that do change something: on a lattice whose spacing exceeds a
brick's footprint, its phase swept over the whole spacing and the principal point shifted by eighths of a pixel from
view to view, plus needles on the image borders and on / one pixel beyond the ROI edges.  Almost every (brick, view)
pair is dropped by a correct bound; the pairs that must not be depend on whether a needle on the outer ring of their
tap rectangle is seen.  `margin_pairs` counts them in float64, against the CPU oracle."""
import math

import numpy as np

import oracle_lib as O
from vacancy_amd import synth
from vacancy_amd.capi import UpdateOption, make_view

# brick footprints: ~2.4 px (the benchmark's voxels of 0.3 px: raw tiles, k = 4 windows), ~12 px (k = 8, 3 x 3 lookups),
# ~30 px (big tiles, the loop over windows); "ortho": one pixel per voxel
FAMILIES = {
    "raw": dict(n=48, ppv=0.3, w=23, h=19, spacing=8, nv=32, shift=5),
    "k8": dict(n=48, ppv=1.5, w=83, h=61, spacing=17, nv=24, shift=8),
    "big": dict(n=40, ppv=4.0, w=171, h=149, spacing=41, nv=32, shift=12),
    "ortho": dict(n=48, ppv=1.0, w=57, h=55, spacing=13, nv=24, shift=6),
}

C_STATE = np.float32(0.7)   # kMax state (not a dyadic fraction: bilinear sums of it round either way)
C_TRUNC = np.float32(-1.25)  # kMax + truncation: the state lies below every valid (>= -1) sample

# mode: update option, image kind, extras
MODES = {
    "max": dict(uo=dict(), kind="needles"),
    "outside": dict(uo=dict(update_outside=1), kind="needles", roi=True),
    "roi": dict(uo=dict(), kind="needles", roi=True),
    "trunc": dict(uo=dict(use_truncation=True, truncation_band=0.1), kind="trunc_needles"),
    "tsdf_pits": dict(uo=dict(voxel_update=1, voxel_update_weight=0.37, use_truncation=True, truncation_band=0.1),
                      kind="pits"),
    "wa_unit_pits": dict(uo=dict(voxel_update=1, use_truncation=True, truncation_band=0.1), kind="pits"),
    "tsdf_drop": dict(uo=dict(voxel_update=1, voxel_update_weight=0.37, use_truncation=True, truncation_band=0.1),
                      kind="trunc_needles"),
    "nn": dict(uo=dict(sdf_interp=0), kind="needles"),
    "fxfy": dict(uo=dict(), kind="needles", fy_scale=0.2),
}


def _background(kind):
    if kind == "needles":
        return np.float32(C_STATE - np.float32(2.0 ** -8))
    if kind == "trunc_needles":
        return np.float32(-1.5)
    return np.float32(-0.5)  # pits


def _needle_value(kind, i):
    if kind == "needles":
        return np.float32(C_STATE + np.float32(0.25 * (i + 1)))
    if kind == "trunc_needles":
        return np.float32(2.0 + 0.25 * i)
    return np.float32(-100.0 - i)


def _roi(i, w, h, spacing):
    """An interior ROI on every other view (None: the whole image)."""
    if i % 2 == 0:
        return None
    a = 1 + (i // 2) % max(1, spacing // 2)
    return (a, a + 1), (w - 2 - a, h - 1 - a)


def make_scene(family, mode, seed=0, z_axis_view=False):
    """dict(opt, views, images, state=(sdf, cnt) or None, kind, bg, needle_masks, n).  z_axis_view: cameras look
    along +y with image rows following z (each z slab of the grid is a narrow band of rows)."""
    f_ = FAMILIES[family]
    m_ = MODES[mode]
    n, ppv, w, h, spacing, nv, shift = (f_[k] for k in ("n", "ppv", "w", "h", "spacing", "nv", "shift"))
    ortho = family == "ortho"
    kind = m_["kind"]
    uo = UpdateOption(**m_["uo"])
    opt = synth.sphere_option(n, uo)
    rng = np.random.RandomState(seed + 1000 * n + len(mode))
    bg = _background(kind)
    dist = 3.0 * n
    views, images, masks = [], [], []
    for i in range(nv):
        if z_axis_view:
            pos = (0.05 * math.sin(1.3 * i) * dist, -dist, 0.05 * math.cos(0.7 * i) * dist)
            c2w = synth.lookat_c2w(pos, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
        else:
            pos = (0.12 * math.sin(1.7 * i) * dist, 0.12 * math.cos(1.1 * i) * dist, -dist)
            c2w = synth.lookat_c2w(pos, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        w2c = synth.affine_inverse(c2w)
        # principal point: integer offsets up to `shift` px (the grid reaches the borders) plus k/8 of a pixel
        ox = (i * 5) % (2 * shift + 1) - shift + (i % 8) / 8.0
        oy = (i * 3) % (2 * shift + 1) - shift + ((3 * i) % 8) / 8.0
        if ortho:
            w2c = w2c.copy()
            w2c[0, 3] += (w - 1) / 2.0 + ox
            w2c[1, 3] += (h - 1) / 2.0 + oy
            fx = fy = np.float32(1.0)
            cx = cy = np.float32(0.0)
        else:
            fx = np.float32(ppv * dist)
            fy = np.float32(fx * m_.get("fy_scale", 1.0)) if i % 2 else fx
            cx = np.float32((w - 1) / 2.0 + ox)
            cy = np.float32((h - 1) / 2.0 + oy)
        roi = _roi(i, w, h, spacing) if m_.get("roi") else None
        v = make_view(w2c.astype(np.float32), fx, fy, cx, cy, w, h, roi_min=roi[0] if roi else None,
                      roi_max=roi[1] if roi else None, is_ortho=ortho)
        img = np.full((h, w), bg, np.float32)
        nm = np.zeros((h, w), bool)
        px, py = (i * 7) % spacing, (i * 11 + i // spacing) % spacing  # the phase sweeps the whole spacing
        xs = np.arange(px, w, spacing)
        ys = np.arange(py, h, spacing)
        nm[np.ix_(ys, xs)] = True
        nm[ys, 0] = nm[ys, w - 1] = True
        nm[0, xs] = nm[h - 1, xs] = True
        if roi:
            (x0, y0), (x1, y1) = roi
            for x in (x0 - 1, x0, x1, x1 + 1):
                nm[ys, x] = True
            for y in (y0 - 1, y0, y1, y1 + 1):
                nm[y, xs] = True
        img[nm] = _needle_value(kind, i)
        if mode == "outside" and roi:  # the image's maximum lies outside the ROI: max_sdf of the voxels beyond it
            img[0, 0] = np.float32(_needle_value(kind, i) + np.float32(1.0))
            nm[0, 0] = True
        if kind == "needles" and i == 2:  # rounding ties: the image is the state's minimum exactly
            img[:] = C_STATE
            nm[:] = False
        views.append(v)
        images.append(np.ascontiguousarray(img))
        masks.append(nm)
    sc = dict(opt=opt, views=views, images=images, kind=kind, bg=bg, needle_masks=masks, n=n)
    # pits: a carved state (init_view), whose counts agree within every brick and are implied by the state -- what the
    # loops that compile the truncation test out require; the others: uploaded
    sc["state"] = None if kind == "pits" else _state(opt, kind, rng)
    return sc


def brick_ids(dims):
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    nbx, nby = (nx + 7) // 8, (ny + 7) // 8
    return (((z // 8) * nby + (y // 8)) * nbx + (x // 8)).reshape(-1)


def _state(opt, kind, rng):
    """sdf = c + jitter in (0, 2^-10], one voxel of every brick exactly c; counts 1 .. 3."""
    orc = O.OracleGrid(opt)
    n = orc.n
    c = C_TRUNC if kind == "trunc_needles" else C_STATE
    jitter = (rng.randint(1, 1025, n) * 2.0 ** -20).astype(np.float32)
    sdf = (c + jitter).astype(np.float32)
    bid = brick_ids(orc.dims)
    order = rng.permutation(n)
    first = np.zeros(bid.max() + 1, np.int64) - 1
    first[bid[order][::-1]] = order[::-1]  # a random voxel of every brick
    sdf[first] = c
    cnt = rng.randint(1, 4, n).astype(np.int32)
    orc.close()
    return sdf, cnt


def oracle_run(scene, batches, effects=False):
    """States of the oracle after every batch (lists of view indices); with `effects`, per view the voxels whose
    outcome the needles decided: those that changed differently than under the background image alone."""
    orc = O.OracleGrid(scene["opt"])
    if scene["state"] is None:
        orc.carve(*init_view(scene))
    else:
        orc.upload(*scene["state"])
    alt = O.OracleGrid(scene["opt"]) if effects else None
    prev_s, prev_u = orc.download()
    after, effect = [], {}
    for b in batches:
        for i in b:
            orc.carve(scene["views"][i], scene["images"][i])
            s, u = orc.download()
            if effects:
                alt.upload(prev_s, prev_u)
                alt.carve(scene["views"][i], np.full_like(scene["images"][i], scene["bg"]))
                s0, u0 = alt.download()
                effect[i] = (u != u0) | (s.view(np.uint32) != s0.view(np.uint32))
            prev_s, prev_u = s, u
        after.append((prev_s, prev_u))
    orc.close()
    if alt is not None:
        alt.close()
    return (after, effect) if effects else after


def tap_rectangles(scene, i, positions):
    """[x0, x1] x [y0, y1] per brick: the pixels the bilinear samples of its voxels can read (float64 projections)."""
    v = scene["views"][i]
    M = np.array(list(v.w2c), np.float64).reshape(3, 4)
    pc = positions.astype(np.float64) @ M[:, :3].T + M[:, 3]
    if v.is_ortho:
        u, w = pc[:, 0], pc[:, 1]
    else:
        u = float(v.fx) / pc[:, 2] * pc[:, 0] + float(v.cx)
        w = float(v.fy) / pc[:, 2] * pc[:, 1] + float(v.cy)
    bid = scene["bid"]
    nb = bid.max() + 1
    umin = np.full(nb, np.inf)
    umax = np.full(nb, -np.inf)
    wmin = np.full(nb, np.inf)
    wmax = np.full(nb, -np.inf)
    np.minimum.at(umin, bid, u)
    np.maximum.at(umax, bid, u)
    np.minimum.at(wmin, bid, w)
    np.maximum.at(wmax, bid, w)
    return (np.floor(umin).astype(np.int64), np.floor(umax).astype(np.int64) + 1,
            np.floor(wmin).astype(np.int64), np.floor(wmax).astype(np.int64) + 1)


def _rect_count(S, x0, x1, y0, y1):
    """Needles in [x0, x1] x [y0, y1] (clipped to the image) from the summed-area table S ((h + 1) x (w + 1))."""
    h, w = S.shape[0] - 1, S.shape[1] - 1
    a, b = np.clip(x0, 0, w), np.clip(x1 + 1, 0, w)
    c, d = np.clip(y0, 0, h), np.clip(y1 + 1, 0, h)
    ok = (b > a) & (d > c)
    r = S[d, b] - S[c, b] - S[d, a] + S[c, a]
    return np.where(ok, r, 0)


def margin_pairs(scene, effect):
    """(brick, view) pairs whose tap rectangle holds needles on its outer ring and none inside, and in which the oracle
    shows the needles' effect (oracle_run(..., effects=True)).  Returns (margin pairs with an effect, margin pairs)."""
    if "bid" not in scene:
        orc = O.OracleGrid(scene["opt"])
        scene["positions"] = orc.positions()
        scene["bid"] = brick_ids(orc.dims)
        orc.close()
    bid = scene["bid"]
    nb = bid.max() + 1
    hit = total = 0
    for i, nm in enumerate(scene["needle_masks"]):
        if not nm.any():
            continue
        x0, x1, y0, y1 = tap_rectangles(scene, i, scene["positions"])
        S = np.zeros((nm.shape[0] + 1, nm.shape[1] + 1), np.int64)
        S[1:, 1:] = nm.astype(np.int64).cumsum(0).cumsum(1)
        outer = _rect_count(S, x0, x1, y0, y1)
        inner = _rect_count(S, x0 + 1, x1 - 1, y0 + 1, y1 - 1)
        margin = (outer > inner) & (inner == 0)
        per_brick = np.bincount(bid, weights=effect[i].astype(np.float64), minlength=nb) > 0
        hit += int((margin & per_brick).sum())
        total += int(margin.sum())
    return hit, total


def init_view(scene, seed=0):
    """A view that sees the whole grid, and its image: c + jitter in [0, 2^-10] (an eighth of the pixels exactly c; -1
    instead of c for the truncation kinds, whose state must be a valid sample).  A fresh grid carved with it holds the
    scene's kind of state with brick minima that a fused launch kept (a vcy_upload turns those off for good)."""
    v0 = scene["views"][0]
    w, h, n = v0.width, v0.height, scene["n"]
    dist = 3.0 * n
    w2c = synth.affine_inverse(synth.lookat_c2w((0.0, 0.0, -dist), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    f = np.float32(2.0 * min(w, h))
    v = make_view(w2c.astype(np.float32), f, f, np.float32((w - 1) / 2.0), np.float32((h - 1) / 2.0), w, h)
    c = np.float32(-1.0) if scene["kind"] == "trunc_needles" else C_STATE
    rng = np.random.RandomState(seed + 7)
    img = (c + (rng.randint(0, 1025, (h, w)) * 2.0 ** -20)).astype(np.float32)
    img[rng.rand(h, w) < 0.125] = c
    return v, img
