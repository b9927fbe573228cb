"""numpy restatement of the depth carve (the section "carve from depth images" of include/vacancy_hip.h), float32 operation
for float32 operation: every product and every sum is an array operation of its own (numpy fuses nothing), the rounding to
the nearest pixel is written out (color_ref.round_half_away), inv_band is one np.float32 division, and the views run in a
Python loop in the order given.  The voxels advance together through a view, which is only a way of running the per-voxel
rule in numpy."""
import numpy as np

import render_ref as RR
from color_ref import round_half_away

F = np.float32
LOWEST = np.finfo(np.float32).min
MAX, WEIGHTED_AVERAGE = 0, 1


def positions(option, z_range=None):
    """(px, py, pz) per voxel of the slices z_range of the grid of `option`, x fastest: vcy_axis_positions' arithmetic."""
    bb_min, bb_max, res = list(option.bb_min), list(option.bb_max), option.resolution
    dims = RR.grid_dims(bb_min, bb_max, res)
    ax = [np.asarray(RR.axis_positions(bb_min, bb_max, res, a, dims[a]), F) for a in range(3)]
    z0, z1 = z_range if z_range is not None else (0, dims[2])
    zz, yy, xx = np.meshgrid(ax[2][z0:z1], ax[1], ax[0], indexing="ij")
    return xx.reshape(-1).astype(F), yy.reshape(-1).astype(F), zz.reshape(-1).astype(F)


def project(v, px, py, pz, ok=None):
    """Steps 2 - 4 for every voxel: (ok, xi, yi, pc2) -- in front of the camera and inside the ROI, the nearest pixel
    clamped into the ROI (the first pixel of the ROI where not ok), the camera depth."""
    m = np.array(list(v.w2c), F).reshape(3, 4)
    ok = np.ones(len(px), bool) if ok is None else ok.copy()
    with np.errstate(all="ignore"):
        pc = [m[r, 3] + (m[r, 0] * px + (m[r, 1] * py + m[r, 2] * pz)) for r in range(3)]  # 2.
        assert all(c.dtype == F for c in pc)
        ok &= ~(pc[2] < 0)
        if v.is_ortho:
            u, w = pc[0], pc[1]
        else:
            u = F(v.fx) / pc[2] * pc[0] + F(v.cx)
            w = F(v.fy) / pc[2] * pc[1] + F(v.cy)
        rx0, ry0, rx1, ry1 = v.roi_min[0], v.roi_min[1], v.roi_max[0], v.roi_max[1]
        ok &= (u >= F(rx0)) & (w >= F(ry0)) & (u <= F(rx1)) & (w <= F(ry1))             # 3.
        us, ws = np.where(ok, u, F(rx0)), np.where(ok, w, F(ry0))  # (the others take no further part)
        xi = np.clip(round_half_away(us).astype(np.int64), rx0, rx1)                    # 4.
        yi = np.clip(round_half_away(ws).astype(np.int64), ry0, ry1)
    return ok, xi, yi, pc[2]


def carve_depth(option, views, depths, band, sdf=None, update_num=None, z_range=None, stats=None):
    """(sdf float32 [n], update_num int32 [n]) after the views, from the given state (default: the fill state).  `stats`
    (a dict) is added to: the (voxel, view) pairs that reach step 5 and are "invalid", "clamped" to 1, "dropped" below -1
    (or NaN), or "between"; and the unclamped samples that are "exactly_plus_one" / "exactly_minus_one"."""
    px, py, pz = positions(option, z_range)
    n = len(px)
    u_opt = option.update_option
    sdf = np.full(n, LOWEST, F) if sdf is None else np.array(sdf, F).reshape(-1)
    cnt = np.zeros(n, np.int32) if update_num is None else np.array(update_num, np.int32).reshape(-1)
    assert len(sdf) == n and len(cnt) == n
    inv_band = F(1.0) / F(band)
    assert inv_band.dtype == F
    weight, max_num = F(u_opt.voxel_update_weight), int(u_opt.voxel_max_update_num)
    with np.errstate(all="ignore"):
        for v, depth in zip(views, depths):
            depth = np.asarray(depth, F).reshape(v.height, v.width)
            ok, xi, yi, pc2 = project(v, px, py, pz, ~(cnt > max_num))                      # 1. - 4.
            z = depth[yi, xi]
            valid = z > F(0.0)                                                              # 5.
            e = z - pc2                                                                     # 6.
            d = e * inv_band
            clamped = d > F(1.0)
            d = np.where(clamped, F(1.0), d).astype(F)
            kept = d >= F(-1.0)
            if stats is not None:
                for key, sel in (("invalid", ok & ~valid), ("clamped", ok & valid & clamped), ("dropped", ok & valid & ~kept),
                                 ("between", ok & valid & kept & ~clamped), ("exactly_plus_one", ok & valid & ~clamped & (d == F(1.0))),
                                 ("exactly_minus_one", ok & valid & (d == F(-1.0)))):
                    stats[key] = stats.get(key, 0) + int(sel.sum())
            ok &= valid & kept
            first = ok & (cnt < 1)                                                          # 7.
            rest = ok & ~first
            if u_opt.voxel_update == MAX:
                rest &= d > sdf
                new = d
            else:
                nf = cnt.astype(F)
                inv_denom = F(1.0) / (weight * (nf + F(1.0)))   # (float)(n + 1): exact for the counts of a test
                new = ((weight * nf * sdf + weight * d) * inv_denom).astype(F)
            sdf = np.where(first, d, np.where(rest, new, sdf)).astype(F)
            cnt = np.where(first, 1, np.where(rest, cnt + 1, cnt)).astype(np.int32)
    return sdf, cnt
