"""The states the distance-field tests share (tests/test_distance_cpu.py: host function against the numpy restatement;
tests/test_gpu_distance.py: the device against it): random states on awkward dims, as test_gpu_components.random_state
makes them -- untouched voxels, NaNs, sdf == iso, a count of 0 over a valid sdf --, and the named cases.  A case is
(name, dims, sdf, cnt, iso, radius); the reference of every case is computed once (reference_of) and never changed."""
import numpy as np

import distance_ref as R
from vacancy_amd.capi import CarverOption, UpdateOption

LOWEST = np.finfo(np.float32).min
RANDOM_DIMS = [(8, 8, 8), (9, 10, 17), (65, 9, 9), (70, 23, 19), (130, 7, 5), (7, 130, 5), (5, 7, 130)]
LONG_DIMS = RANDOM_DIMS[4:]  # one axis longer than 127 + 1: a distance of 127 fits along it
RADII = (1, 3, 12)
ISOS = (0.0, 0.25)


def box_option(dims, uo=None, resolution=1.0):
    """A grid of exactly `dims` voxels centred on the origin.  resolution: a small multiple of 1/8, so that the halves of
    the extents are exact floats and (int)(extent / resolution) is `dims`."""
    h = [d * resolution / 2.0 for d in dims]
    return CarverOption(bb_min=[-x for x in h], bb_max=h, resolution=resolution, update_option=uo or UpdateOption())


def random_state(dims, density, iso, seed):
    rng = np.random.RandomState(seed)
    n = dims[0] * dims[1] * dims[2]
    solid = rng.rand(n) < density
    mag = (0.3 + 0.7 * rng.rand(n)).astype(np.float32)      # |sdf| >= 0.3: clear of every iso level used
    sdf = np.where(solid, -mag, mag).astype(np.float32)
    cnt = rng.randint(1, 4, n).astype(np.int32)
    r = rng.rand(n)
    untouched = r < 0.02
    sdf[untouched], cnt[untouched] = LOWEST, 0
    sdf[(r >= 0.02) & (r < 0.03)] = np.nan
    sdf[(r >= 0.03) & (r < 0.08)] = np.float32(iso)          # exactly the iso level as a float: not solid
    cnt[(r >= 0.08) & (r < 0.09)] = 0                        # a count of 0 over a valid sdf: not solid either
    return sdf, cnt


def state_from_mask(solid, cnt=None):
    solid = np.asarray(solid, bool).reshape(-1)
    sdf = np.where(solid, np.float32(-0.5), np.float32(0.5)).astype(np.float32)
    return sdf, (np.ones(solid.size, np.int32) if cnt is None else cnt)


def one_voxel_at_the_end(dims):
    """One solid voxel at index 1 of the long axis: the distances along that axis run 1 .. 128, so index 128 holds exactly
    127^2 -- the largest exact value, at the edge of the byte and of the 16 bits -- and index 129 is FAR."""
    nx, ny, nz = dims
    s = np.zeros((nz, ny, nx), bool)
    at = [nz // 2, ny // 2, nx // 2]
    at[2 - int(np.argmax(dims))] = 1
    s[tuple(at)] = True
    return state_from_mask(s)


def random_cases(dims):
    k = RANDOM_DIMS.index(dims)
    for i, iso in enumerate(ISOS):
        for j, radius in enumerate(RADII):
            density = (0.3, 0.05, 0.9)[(i + j + k) % 3]
            sdf, cnt = random_state(dims, density, iso, 1000 + 10 * k + 3 * i + j)
            yield ("random density %g iso %g R %d" % (density, iso, radius), dims, sdf, cnt, iso, radius)
        if dims in LONG_DIMS:  # sparse, so that the distances are long
            sdf, cnt = random_state(dims, 0.002, iso, 2000 + 10 * k + i)
            yield ("sparse iso %g R 127" % iso, dims, sdf, cnt, iso, 127)
    if dims in LONG_DIMS:
        sdf, cnt = one_voxel_at_the_end(dims)
        yield ("one voxel at the end, R 127", dims, sdf, cnt, 0.0, 127)


def named_cases():
    out = []
    n = 8 * 8 * 8
    out.append(("nothing solid", (8, 8, 8), np.full(n, 0.5, np.float32), np.ones(n, np.int32), 0.0, 3))
    out.append(("everything solid", (8, 8, 8), np.full(n, -0.5, np.float32), np.ones(n, np.int32), 0.0, 3))
    s = np.zeros((9, 9, 20), bool)
    s[4, 4, 10] = True
    out.append(("one solid voxel",) + ((20, 9, 9),) + state_from_mask(s) + (0.0, 3))
    # the row's second word holds one voxel and 63 bits that belong to nobody
    out.append(("65 wide, all solid", (65, 9, 9)) + state_from_mask(np.ones(65 * 81, bool)) + (0.0, 12))
    s = np.zeros((9, 9, 65), bool)
    s[:, :, 64] = True
    out.append(("65 wide, the last column solid", (65, 9, 9)) + state_from_mask(s) + (0.0, 12))
    s = np.zeros((9, 10, 17), bool)
    s[:, :, 0:6] = True
    out.append(("slab at x = 0", (17, 10, 9)) + state_from_mask(s) + (0.0, 4))
    return out


_refs = {}


def reference_of(case, resolution=1.0):
    """(signed int32 field, sdf after Redistance) of a case, computed once; callers must not write into the arrays"""
    name, dims, sdf, cnt, iso, radius = case
    key = (name, dims, iso, radius, resolution)
    if key not in _refs:
        d2, out = R.reference(sdf, cnt, dims, iso, radius, resolution)
        d2.setflags(write=False)
        out.setflags(write=False)
        _refs[key] = (d2, out)
    return _refs[key]
