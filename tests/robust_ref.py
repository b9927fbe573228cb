"""Restatement of the robust carve (include/vacancy_hip.h, "robust carve") that shares no arithmetic with the kernel.

The samples of a view come from the CPU oracle: a fresh OracleGrid with the same option carves that ONE view; where its
update_num is 1 the view contributes a sample, and its sdf is the sample.  The top list then runs in numpy, view by view,
with K columns of values and view indices, using only the comparison `>`; result and blame follow from the definition.
"""
import numpy as np

import oracle_lib as O

F = np.float32
LOWEST = np.finfo(np.float32).min


def samples(option, views, sdfs):
    """(has [n_views, n_voxels] bool, val [n_views, n_voxels] float32) on the whole grid of `option`."""
    prev = O.set_num_threads(1)  # (grids of a few thousand voxels: the OpenMP barriers would cost more than the work)
    try:
        has, val = [], []
        for v, s in zip(views, sdfs):
            g = O.OracleGrid(option)
            g.carve(v, s)
            sdf, cnt = g.download()
            g.close()
            assert cnt.max(initial=0) <= 1
            has.append(cnt == 1)
            val.append(sdf)
    finally:
        O.set_num_threads(prev)
    return np.array(has, bool).reshape(len(views), -1), np.array(val, F).reshape(len(views), -1)


def top_list(has, val, k):
    """The top list of every voxel after all views: (t [n, k], view index [n, k] (-1 where empty), samples [n])."""
    nv, n = has.shape
    t = np.full((n, k), LOWEST, F)
    ix = np.full((n, k), -1, np.int64)
    cnt = np.zeros(n, np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(nv):
            d = val[i]
            held = np.minimum(cnt, k)
            pos = np.full(n, -1, np.int64)
            rows = np.nonzero(has[i] & (held < k))[0]                       # 1. append ...
            t[rows, held[rows]], ix[rows, held[rows]], pos[rows] = d[rows], i, held[rows]
            rows = np.nonzero(has[i] & (held == k) & (d > t[:, k - 1]))[0]  # ... or replace the last entry, or drop
            t[rows, k - 1], ix[rows, k - 1], pos[rows] = d[rows], i, k - 1
            for j in range(k - 1, 0, -1):                                   # 2. swap upwards while d > predecessor
                rows = np.nonzero((pos == j) & (d > t[:, j - 1]))[0]
                t[rows, j], ix[rows, j] = t[rows, j - 1], ix[rows, j - 1]
                t[rows, j - 1], ix[rows, j - 1], pos[rows] = d[rows], i, j - 1
            cnt += has[i]
    return t, ix, cnt


def robust_from_samples(has, val, tolerate, iso=0.0):
    """(sdf float32 [n], update_num int32 [n], overruled int64 [n_views]) of the voxels the columns stand for."""
    nv, n = has.shape
    k = tolerate + 1
    t, ix, cnt = top_list(has, val, k)
    keep = np.minimum(cnt, k) - 1
    sdf = np.where(cnt > 0, t[np.arange(n), np.maximum(keep, 0)], F(LOWEST)).astype(F)
    overruled = np.zeros(nv, np.int64)
    with np.errstate(invalid="ignore"):
        solid = (cnt > 0) & (sdf.astype(np.float64) < iso)
        for j in range(k - 1):
            sel = solid & (j < keep) & (t[:, j].astype(np.float64) >= iso)
            overruled += np.bincount(ix[sel, j], minlength=nv)
    return sdf, cnt.astype(np.int32), overruled


def robust(option, views, sdfs, tolerate, iso=0.0):
    has, val = samples(option, views, sdfs)
    return robust_from_samples(has, val, tolerate, iso)


def assert_sdf_equal(got, want, ctx=""):
    """Bit equality, except that a NaN only has to be a NaN: sign and payload of a GENERATED NaN (inf - inf, 0 * inf in the
    bilinear sum over poisoned taps) are not defined by IEEE 754 and differ between x86 and gfx950 (as in
    test_gpu_parity.test_view_dropping_is_exact)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), "%s: NaN voxels differ (%d)" % (ctx, int((ng != nw).sum()))
    bg, bw = np.where(ng, 0, got.view(np.uint32)), np.where(nw, 0, want.view(np.uint32))
    assert np.array_equal(bg, bw), "%s: %d sdf values differ" % (ctx, int((bg != bw).sum()))
