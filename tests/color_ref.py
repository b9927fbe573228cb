"""numpy restatement of the colouring of vertices (the section "colour of vertices from the input photographs" of
include/vacancy_hip.h), float32 operation for float32 operation: every product and every sum is an array operation of its
own (numpy fuses nothing), the rounding to the nearest pixel is written out (halves away from zero; np.round rounds them to
even), and the sums over the views run in a Python loop in ascending view index.  The vertices advance together through
a view, which is only a way of running the per-vertex rule in numpy."""
import numpy as np

F = np.float32
MEAN, WEIGHTED, BEST = 0, 1, 2
NN, BILINEAR = 0, 1


def round_half_away(x):
    """roundf: floor(|x| + 0.5) with the sign of x; exact in float32 for |x| < 2^23 (|x| + 0.5 is then representable or
    ties correctly: for |x| < 2^22 the sum is exact, and this restatement is only fed pixel coordinates)."""
    a = np.abs(x)
    r = np.floor(a)
    r = np.where(a - r >= F(0.5), r + F(1.0), r)     # (a - r is exact)
    return np.copysign(r, x).astype(F)


def color_vertices(vertices, normals, views, photos, depths, mode, interp, depth_tolerance, min_cos, fallback):
    """rgb float32 [n, 3], n_used int32 [n], best_view int32 [n]."""
    p = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    n = len(p)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    if mode != MEAN:
        nr = np.ascontiguousarray(normals, F).reshape(-1, 3)
        nx, ny, nz = nr[:, 0], nr[:, 1], nr[:, 2]
    tol, mc = F(depth_tolerance), F(min_cos)
    S = np.zeros((3, n), F)
    W = np.zeros(n, F)
    n_used = np.zeros(n, np.int32)
    w_best = np.full(n, -1.0, F)
    best_view = np.full(n, -1, np.int32)
    best = np.zeros((3, n), F)
    with np.errstate(all="ignore"):
        for i, (v, photo, depth) in enumerate(zip(views, photos, depths)):
            m = np.array(list(v.w2c), F).reshape(3, 4)
            photo = np.asarray(photo, np.uint8).reshape(v.height, v.width, 3)
            depth = np.asarray(depth, F).reshape(v.height, v.width)
            pc = [m[r, 3] + (m[r, 0] * px + (m[r, 1] * py + m[r, 2] * pz)) for r in range(3)]
            assert all(c.dtype == F for c in pc)
            ok = ~(pc[2] < 0)
            if v.is_ortho:
                u, w = pc[0], pc[1]
            else:
                u = F(v.fx) / pc[2] * pc[0] + F(v.cx)
                w = F(v.fy) / pc[2] * pc[1] + F(v.cy)
            rx0, ry0, rx1, ry1 = v.roi_min[0], v.roi_min[1], v.roi_max[0], v.roi_max[1]
            ok &= (u >= F(rx0)) & (w >= F(ry0)) & (u <= F(rx1)) & (w <= F(ry1))
            us, ws = np.where(ok, u, F(rx0)), np.where(ok, w, F(ry0))      # (the others take no further part)
            xi = np.clip(round_half_away(us).astype(np.int64), rx0, rx1)
            yi = np.clip(round_half_away(ws).astype(np.int64), ry0, ry1)
            limit = depth[yi, xi] + tol
            ok &= pc[2] <= limit
            if interp == NN:
                sample = [photo[yi, xi, c].astype(F) for c in range(3)]
            else:
                x0, y0 = np.floor(us).astype(np.int64), np.floor(ws).astype(np.int64)
                x1, y1 = x0 + 1, y0 + 1
                x0, y0 = np.maximum(x0, rx0), np.maximum(y0, ry0)
                x1, y1 = np.minimum(x1, rx1), np.minimum(y1, ry1)
                lu, lv = us - x0.astype(F), ws - y0.astype(F)
                one = F(1.0)
                k00, k10, k01, k11 = (one - lu) * (one - lv), lu * (one - lv), (one - lu) * lv, lu * lv
                sample = []
                for c in range(3):
                    a = k00 * photo[y0, x0, c].astype(F)
                    b = k10 * photo[y0, x1, c].astype(F)
                    cc = k01 * photo[y1, x0, c].astype(F)
                    d = k11 * photo[y1, x1, c].astype(F)
                    sample.append(((a + b) + cc) + d)
            if mode == MEAN:
                wt = np.ones(n, F)
            else:
                nc = [m[r, 0] * nx + (m[r, 1] * ny + m[r, 2] * nz) for r in range(3)]
                if v.is_ortho:
                    cos = nc[2]
                else:
                    length = np.sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2])
                    cos = ((nc[0] * pc[0] + nc[1] * pc[1]) + nc[2] * pc[2]) / length
                wt = np.abs(cos)
                ok &= wt > mc
            assert wt.dtype == F and all(s.dtype == F for s in sample)
            for c in range(3):
                S[c] = np.where(ok, S[c] + wt * sample[c], S[c])
            W = np.where(ok, W + wt, W)
            n_used += ok
            better = ok & (wt > w_best)
            w_best = np.where(better, wt, w_best)
            best_view = np.where(better, np.int32(i), best_view)
            for c in range(3):
                best[c] = np.where(better, sample[c], best[c])
        none = n_used == 0
        rgb = np.empty((n, 3), F)
        for c in range(3):
            val = best[c] if mode == BEST else S[c] / W
            rgb[:, c] = np.where(none, F(fallback[c]), val)
    assert W.dtype == F and S.dtype == F
    return rgb, n_used.astype(np.int32), best_view.astype(np.int32)
