"""Numpy restatement of the section "shading a rasterised mesh" of include/vacancy_hip.h, steps 9 to 12, and its named
mutants.  It sits on the face image of tests/raster_ref.py (steps 1 to 8) and recomputes the weights of every pixel in
float64 in the stated order -- numpy arrays over the pixels, every operation an elementwise IEEE operation rounded on its
own.

`rules`: a set of mutant names, each turning ONE rule of the definition (tests/test_shade_cpu.py shows that the cases
tell every one of them from the definition):
  "affine"    screen-space weights b_k = l_k on a pinhole
  "perm"      weight k paired with the attribute of vertex k + 1
  "sumorder"  b_0 a_0 + (b_1 a_1 + b_2 a_2)
  "floatacc"  the value accumulated in float
  "trunc"     q truncates instead of rounding half up
  "bgcount"   background pixels counted in the photometric error
  "nomask"    the silhouette ignored
  "roi"       pixels outside the ROI shaded from a raster without ROI
"""
import numpy as np

import raster_ref as RF
from vacancy_amd.capi import View

F = np.float32
D = np.float64
MUTANTS = ("affine", "perm", "sumorder", "floatacc", "trunc", "bgcount", "nomask", "roi")


def full_roi(view):
    """The view with its ROI opened to the whole image (the mutant "roi")."""
    v = View.from_buffer_copy(view)
    v.roi_min[0], v.roi_min[1] = 0, 0
    v.roi_max[0], v.roi_max[1] = view.width - 1, view.height - 1
    return v


def has_full_roi(view):
    return tuple(view.roi_min) == (0, 0) and tuple(view.roi_max) == (view.width - 1, view.height - 1)


def face_image(vertices, faces, view, rules=frozenset()):
    """Steps 1 to 8: the winner of every pixel, -1 on a miss (tests/raster_ref.py)."""
    return RF.raster_view(vertices, faces, full_roi(view) if "roi" in rules else view)[1]


def edge_values(i, j, a, b, px, py):
    """Step 3 over arrays: the faces' values at (px, py) for their directed edges from vertex i (at a = (u, w)) to j (at b)."""
    forward = i < j
    ax, ay = np.where(forward, a[0], b[0]), np.where(forward, a[1], b[1])
    bx, by = np.where(forward, b[0], a[0]), np.where(forward, b[1], a[1])
    e = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    return np.where(forward, e, -e)


def weights(vertices, faces, view, face, rules=frozenset()):
    """Step 9 at the pixels with a winner: (ys, xs, ids int [n, 3], b float64 [n, 3], T float64 [n] -- ones on an ortho
    view)."""
    ys, xs = np.nonzero(face >= 0)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    ids = f[face[ys, xs]].astype(np.int64).reshape(-1, 3)
    proj = [RF.project(view, p) for p in np.asarray(vertices, np.float32).reshape(-1, 3)]
    u = np.array([p[0] for p in proj], F).astype(D)
    w = np.array([p[1] for p in proj], F).astype(D)
    z = np.array([p[2] for p in proj], F).astype(D)
    P = [(u[ids[:, k]], w[ids[:, k]]) for k in range(3)]
    px, py = xs.astype(D), ys.astype(D)
    with np.errstate(all="ignore"):
        A = edge_values(ids[:, 0], ids[:, 1], P[0], P[1], P[2][0], P[2][1])
        e = [edge_values(ids[:, 1], ids[:, 2], P[1], P[2], px, py), edge_values(ids[:, 2], ids[:, 0], P[2], P[0], px, py),
             edge_values(ids[:, 0], ids[:, 1], P[0], P[1], px, py)]
        l = [ek / A for ek in e]
        if view.is_ortho or "affine" in rules:
            b, T = l, np.ones(len(xs), D)
        else:
            t = [l[k] * (D(1.0) / z[ids[:, k]]) for k in range(3)]
            T = (t[0] + t[1]) + t[2]
            b = [tk / T for tk in t]
    return ys, xs, ids, np.stack(b, axis=1).reshape(-1, 3), T


def values(ids, b, attributes, rules=frozenset()):
    """Step 10: float32 [n, channels] at the pixels of `weights`."""
    a = np.asarray(attributes, F)
    a = a[:, None] if a.ndim == 1 else a
    pair = [1, 2, 0] if "perm" in rules else [0, 1, 2]
    with np.errstate(all="ignore"):
        if "floatacc" in rules:
            m = [b[:, k].astype(F)[:, None] * a[ids[:, pair[k]]] for k in range(3)]
            return ((m[0] + m[1]) + m[2]).astype(F)
        m = [b[:, k][:, None] * a[ids[:, pair[k]]].astype(D) for k in range(3)]
        if "sumorder" in rules:
            return (m[0] + (m[1] + m[2])).astype(F)
        return ((m[0] + m[1]) + m[2]).astype(F)


def quantize(v, rules=frozenset()):
    """q of step 11 over a float32 array."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        r = np.floor(v) if "trunc" in rules else np.floor(v + F(0.5))
        out = np.where(v >= F(255.0), F(255.0), r)
        out = np.where(v > F(0.0), out, F(0.0))   # (NaN: not > 0)
    return out.astype(np.uint8)


def shade_view(vertices, faces, attributes, view, background=None, rules=frozenset(), face=None):
    """One view: {"value", "value8", "bary", and what the tests look at: "face" (the winners) and "T" (float64, NaN on a
    miss)}.  `face`: the definition's face image, when the caller has it already."""
    rules = frozenset(rules)
    a = np.asarray(attributes, F)
    a = a[:, None] if a.ndim == 1 else a
    ch = a.shape[1]
    bg = np.zeros(4, F) if background is None else np.asarray(list(background) + [0.0] * 4, F)[:4]
    if face is None or ("roi" in rules and not has_full_roi(view)):
        face = face_image(vertices, faces, view, rules)
    h, w = view.height, view.width
    value = np.empty((h, w, ch), F)
    value[:] = bg[:ch]
    bary = np.zeros((h, w, 3), F)
    T = np.full((h, w), np.nan, D)
    if (face >= 0).any():
        ys, xs, ids, b, t = weights(vertices, faces, view, face, rules)
        value[ys, xs] = values(ids, b, a, rules)
        bary[ys, xs] = b.astype(F)
        T[ys, xs] = t
    return {"value": value, "value8": quantize(value, rules), "bary": bary, "face": face, "T": T}


def shade(vertices, faces, attributes, views, background=None, rules=frozenset(), face=None):
    """All views: a list of dicts shaped like carver.shade_mesh_host's (with "face" and "T" beside)."""
    return [shade_view(vertices, faces, attributes, view, background, rules, None if face is None else face[i])
            for i, view in enumerate(views)]


def photo_error(vertices, faces, colors, views, photos, masks=None, rules=frozenset(), face=None):
    """Step 12: int64 [n_views, 7]."""
    rules = frozenset(rules)
    out = np.zeros((len(views), 7), np.int64)
    for i, view in enumerate(views):
        r = shade_view(vertices, faces, colors, view, None, rules, None if face is None else face[i])
        count = np.ones_like(r["face"], bool) if "bgcount" in rules else r["face"] >= 0
        if masks is not None and "nomask" not in rules:
            count &= np.asarray(masks[i]) != 0
        d = r["value8"].astype(np.int64) - np.asarray(photos[i], np.uint8).astype(np.int64)
        d = d[count]
        out[i, 0] = count.sum()
        out[i, 1:4] = np.abs(d).sum(axis=0)
        out[i, 4:7] = (d * d).sum(axis=0)
    return out


def same(a, b, keys=("value", "value8", "bary")):
    """Two lists of result dicts agree: float BITS of value and bary, bytes of value8."""
    def eq(x, y):
        return x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)
    return len(a) == len(b) and all(eq(x[k], y[k]) for x, y in zip(a, b) for k in keys if k in x and k in y)


def same_but_nan(a, b, keys=("value", "value8", "bary")):
    """... where NaNs only have to sit in the same places (which NaN comes out is not part of the contract)."""
    def eq(x, y):
        if x.dtype != F:
            return np.array_equal(x, y)
        nx, ny = np.isnan(x), np.isnan(y)
        return np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.uint32), y[~ny].view(np.uint32))
    return len(a) == len(b) and all(eq(x[k], y[k]) for x, y in zip(a, b) for k in keys if k in x and k in y)
