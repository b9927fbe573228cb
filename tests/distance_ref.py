"""numpy restatement of the section "distance field of the hull" of include/vacancy_hip.h: the definition by brute force
over all pairs of voxels, the separable evaluation (x pass, y pass, z pass) the library runs, the metric value phi in
float32, and the closing as its three calls.  Arrays are flat, reference order (z*nx*ny + y*nx + x); dims = (nx, ny, nz)."""
import numpy as np


def solid_mask(sdf, cnt, iso):
    with np.errstate(invalid="ignore"):
        return (np.asarray(cnt) >= 1) & (np.asarray(sdf, np.float32).astype(np.float64) < iso)


def far_of(radius):
    return radius * radius + 1


def brute_d2(solid, dims, radius):
    """d2 of every voxel by the definition: the minimum over ALL voxels of the other class inside the grid."""
    nx, ny, nz = dims
    s = np.asarray(solid, bool).reshape(-1)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).astype(np.int64)
    out = np.full(s.size, far_of(radius), np.int64)
    for c in (False, True):
        mine, other = np.nonzero(s == c)[0], np.nonzero(s != c)[0]
        if len(mine) == 0 or len(other) == 0:
            continue
        for lo in range(0, len(mine), 512):
            m = mine[lo:lo + 512]
            d = ((p[m, None, :] - p[None, other, :]) ** 2).sum(2).min(1)
            out[m] = np.where(d <= radius * radius, d, far_of(radius))
    return out


def _axis_pass(f, s, axis, radius):
    """min over |d| <= radius, inside the grid, of (class differs ? 0 : f) + d*d along `axis` of the [z, y, x] arrays"""
    out = f.copy()
    n = f.shape[axis]

    def cut(a, lo, hi):
        idx = [slice(None)] * 3
        idx[axis] = slice(lo, hi)
        return a[tuple(idx)]

    for d in range(1, min(radius, n - 1) + 1):
        for centre, nb in (((0, n - d), (d, n)), ((d, n), (0, n - d))):
            cand = np.where(cut(s, *nb) != cut(s, *centre), 0, cut(f, *nb)) + d * d
            view = cut(out, *centre)
            np.minimum(view, cand, out=view)
    return out


def separable_d2(solid, dims, radius):
    nx, ny, nz = dims
    s = np.asarray(solid, bool).reshape(nz, ny, nx)
    far = far_of(radius)
    g = np.full(s.shape, far, np.int64)
    for d in range(1, min(radius, nx - 1) + 1):  # x pass: the nearest voxel of the other class along the row
        differs = s[:, :, d:] != s[:, :, :-d]
        for view in (g[:, :, d:], g[:, :, :-d]):
            np.minimum(view, np.where(differs, d * d, far), out=view)
    h = _axis_pass(g, s, 1, radius)
    k = _axis_pass(h, s, 0, radius)
    return np.where(k > radius * radius, far, k).reshape(-1)


def phi_of(d2, radius, resolution):
    """float32, one rounding per operation"""
    d2c = np.minimum(d2, radius * radius).astype(np.float32)
    return (np.sqrt(d2c) - np.float32(0.5)) * np.float32(resolution)


def reference(sdf, cnt, dims, iso, radius, resolution=1.0, brute=False):
    """(signed int32 field, sdf after Redistance) of the state (sdf, cnt)"""
    sdf = np.asarray(sdf, np.float32).reshape(-1)
    cnt = np.asarray(cnt).reshape(-1)
    s = solid_mask(sdf, cnt, iso)
    d2 = (brute_d2 if brute else separable_d2)(s, dims, radius)
    phi = phi_of(d2, radius, resolution)
    out = sdf.copy()
    touched = cnt >= 1
    out[touched] = np.where(s, -phi, phi)[touched]
    return np.where(s, -d2, d2).astype(np.int32), out


def close_plan(radius_voxels, resolution):
    """(r, R) of CloseHull"""
    return float(radius_voxels) * float(np.float32(resolution)), int(np.ceil(radius_voxels)) + 2


def close_hull(sdf, cnt, dims, radius_voxels, iso=0.0, resolution=1.0):
    """the sdf after CloseHull: Redistance(iso, R), Redistance(r, R), Redistance(-r, R)"""
    r, big_r = close_plan(radius_voxels, resolution)
    for level in (iso, r, -r):
        sdf = reference(sdf, cnt, dims, level, big_r, resolution)[1]
    return sdf


def two_blocks():
    """Two 5^3 solid blocks two voxels apart along x, four voxels clear of the border of a (20, 13, 13) grid, every voxel
    touched: (sdf, cnt, dims, the gap's mask)."""
    dims = (20, 13, 13)
    s = np.zeros((13, 13, 20), bool)
    s[4:9, 4:9, 4:9] = True
    s[4:9, 4:9, 11:16] = True
    gap = np.zeros_like(s)
    gap[4:9, 4:9, 9:11] = True
    sdf = np.where(s, np.float32(-0.5), np.float32(0.5)).astype(np.float32).reshape(-1)
    return sdf, np.ones(sdf.size, np.int32), dims, gap.reshape(-1)
