"""What the tests of the distance field across z-slabs share (tests/test_slab_distance_cpu.py: the host halves against the
whole-grid reference; tests/test_gpu_slab_distance.py: the device against both): the cases -- those of distance_cases --,
the cuts of z every case is run under, and a numpy restatement of the slab flow of include/vacancy_hip.h ("distance field
of the hull", the z-slab form): planes per slab, the neighbours' planes at either end, the z pass over the longer column.
The reference of every case stays distance_cases.reference_of: the WHOLE grid's field, computed once."""
import numpy as np

import distance_cases as K
import distance_ref as R

SLAB_RANDOM_DIMS = [(9, 10, 17), (70, 23, 19), (5, 7, 130)]


def all_cases():
    out = list(K.named_cases())
    for dims in SLAB_RANDOM_DIMS:
        out += list(K.random_cases(dims))
    return out


def cuts_of(nz):
    """The bounds lists a grid of nz slices is cut by; every slab has at least 2 slices (vcy_halo_allgather demands it).
    Among them: a slab of exactly 2 slices; a cut at z = 2 and one at z = nz - 2; slabs of 2 slices side by side, so that
    with a radius above 2 a slab's planes come from three slabs and a thin slab passes its neighbours' planes on."""
    out = []
    if nz - 4 >= 2 or nz == 4:
        out.append(sorted({0, 2, nz - 2, nz}))
    else:  # (the two cuts cannot be made at once)
        out += [[0, 2, nz], [0, nz - 2, nz]]
    mid = max(2, nz // 2 - 2)
    if mid + 4 <= nz - 2:
        out.append([0, mid, mid + 2, mid + 4, nz])
    if nz >= 8:
        out.append([0, nz // 2, nz])
    return out


def slab_of(a, dims, z0, z1):
    sl = dims[0] * dims[1]
    return np.asarray(a).reshape(-1)[z0 * sl:z1 * sl]


# ---- the slab flow in numpy ------------------------------------------------------------------------------------------------

def planes_np(sdf, cnt, dims_slab, iso, radius):
    """uint16 [slices, nx * ny] of a slab's own slices: class << 15 | the y pass's value"""
    nx, ny, nzl = dims_slab
    s = R.solid_mask(sdf, cnt, iso).reshape(nzl, ny, nx)
    far = R.far_of(radius)
    g = np.full(s.shape, far, np.int64)
    for d in range(1, min(radius, nx - 1) + 1):  # x pass: the nearest voxel of the other class along the row
        differs = s[:, :, d:] != s[:, :, :-d]
        for view in (g[:, :, d:], g[:, :, :-d]):
            np.minimum(view, np.where(differs, d * d, far), out=view)
    h = R._axis_pass(g, s, 1, radius)
    return ((s.astype(np.uint16) << 15) | h.astype(np.uint16)).reshape(nzl, ny * nx)


def halos_np(z_ranges, radius, planes):
    """[(below, above)] per slab, cut out of the slabs' planes stacked into the whole grid's (None where there are none)"""
    whole = np.concatenate(planes)
    nz = z_ranges[-1][1]
    out = []
    for z0, z1 in z_ranges:
        nb, na = min(radius, z0), min(radius, nz - z1)
        out.append((whole[z0 - nb:z0] if nb else None, whole[z1:z1 + na] if na else None))
    return out


def finish_np(h, below, above, dims_slab, radius, resolution, sdf, cnt):
    """(signed int32 field, sdf after the rewrite) of the slab"""
    nx, ny, nzl = dims_slab
    parts = [p for p in (below, h, above) if p is not None]
    ext = np.concatenate(parts).reshape(-1, ny, nx)
    nb = 0 if below is None else len(below)
    cls, val = (ext >> 15).astype(bool), (ext & 0x7fff).astype(np.int64)
    k = R._axis_pass(val, cls, 0, radius)[nb:nb + nzl]
    d2 = np.where(k > radius * radius, R.far_of(radius), k).reshape(-1)
    s = cls[nb:nb + nzl].reshape(-1)
    phi = R.phi_of(d2, radius, resolution)
    out = np.asarray(sdf, np.float32).reshape(-1).copy()
    touched = np.asarray(cnt).reshape(-1) >= 1
    out[touched] = np.where(s, -phi, phi)[touched]
    return np.where(s, -d2, d2).astype(np.int32), out


def slab_flow_np(case, bounds, resolution=1.0):
    """(field, sdf) of the whole grid, put together from the slabs' results"""
    name, dims, sdf, cnt, iso, radius = case
    zr = list(zip(bounds[:-1], bounds[1:]))
    sd = [(dims[0], dims[1], z1 - z0) for z0, z1 in zr]
    planes = [planes_np(slab_of(sdf, dims, *z), slab_of(cnt, dims, *z), d, iso, radius) for z, d in zip(zr, sd)]
    halos = halos_np(zr, radius, planes)
    parts = [finish_np(planes[i], halos[i][0], halos[i][1], sd[i], radius, resolution, slab_of(sdf, dims, *zr[i]),
                       slab_of(cnt, dims, *zr[i])) for i in range(len(zr))]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def edge_planes(z_ranges, radius, planes):
    """(bottoms, tops): what every slab exports, its lowest and highest min(radius, own slices) planes"""
    ms = [min(radius, z1 - z0) for z0, z1 in z_ranges]
    return [p[:m] for p, m in zip(planes, ms)], [p[len(p) - m:] for p, m in zip(planes, ms)]
