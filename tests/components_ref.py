"""numpy restatement of the component definitions of include/vacancy_hip.h (vcy_label_components / vcy_keep_components):

  solid      update_num >= 1 and (double)sdf < iso_level   (an untouched voxel and a NaN are not solid)
  adjacency  the six axis neighbours inside the grid
  label      the smallest global voxel id z*nx*ny + y*nx + x of the component
  order      n_voxels descending, ties by label ascending

Everything is integer arithmetic on the mask, so the device's results are compared with these for equality.
Arrays are flat in the reference's order (x fastest); dims = (nx, ny, nz)."""
import numpy as np


def solid_mask(sdf, cnt, iso):
    with np.errstate(invalid="ignore"):
        return (np.asarray(sdf, np.float32).astype(np.float64) < float(iso)) & (np.asarray(cnt) >= 1)


def label_volume(solid, dims):
    """Label (int64) of every voxel, -1 where not solid.  Runs along x are numbered in id order in one vectorised
    step (a run's first voxel is its smallest id); the runs are then joined over y and z by hooking roots onto smaller
    roots and pointer jumping until nothing changes (the number of trees at least halves per round)."""
    nx, ny, nz = dims
    n = nx * ny * nz
    s = np.asarray(solid, bool).reshape(nz, ny, nx)
    start = s.copy()
    start[:, :, 1:] &= ~s[:, :, :-1]
    first = np.flatnonzero(start.reshape(-1)).astype(np.int64)       # id of every run's first voxel, ascending
    run = (np.cumsum(start.reshape(-1), dtype=np.int64) - 1).reshape(nz, ny, nx)  # run number of a SOLID voxel
    nruns = len(first)
    codes = []
    for lo, hi in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))),
                   ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        m = s[lo] & s[hi]
        codes.append(run[hi][m] * nruns + run[lo][m])
    codes = np.unique(np.concatenate(codes)) if nruns else np.zeros(0, np.int64)
    a, b = (codes // nruns, codes % nruns) if nruns else (codes, codes)
    parent = np.arange(nruns, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        diff = lo != hi
        if not diff.any():
            break
        np.minimum.at(parent, hi[diff], lo[diff])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    lab = np.full(n, -1, np.int64)
    flat = s.reshape(-1)
    lab[flat] = first[parent[run.reshape(-1)[flat]]]
    return lab


def components(labels, dims):
    """The sorted component list of a label array: dict of "label", "n_voxels" (int64), "bb_min", "bb_max" (int32 [n, 3])."""
    nx, ny, nz = dims
    vox = np.flatnonzero(labels >= 0)
    if len(vox) == 0:
        return {"label": np.zeros(0, np.int64), "n_voxels": np.zeros(0, np.int64),
                "bb_min": np.zeros((0, 3), np.int32), "bb_max": np.zeros((0, 3), np.int32)}
    lab = labels[vox]
    order = np.argsort(lab, kind="stable")
    lab, vox = lab[order], vox[order]
    first = np.flatnonzero(np.concatenate([[True], lab[1:] != lab[:-1]]))
    uniq = lab[first]
    count = np.diff(np.concatenate([first, [len(lab)]])).astype(np.int64)
    xyz = np.stack([vox % nx, (vox // nx) % ny, vox // (nx * ny)], 1)
    mn = np.minimum.reduceat(xyz, first, axis=0).astype(np.int32)
    mx = np.maximum.reduceat(xyz, first, axis=0).astype(np.int32)
    rank = np.lexsort((uniq, -count))  # n_voxels descending, then label ascending
    return {"label": uniq[rank], "n_voxels": count[rank], "bb_min": mn[rank], "bb_max": mx[rank]}


def reference(sdf, cnt, dims, iso):
    """(component list, per-voxel labels) of a state."""
    lab = label_volume(solid_mask(sdf, cnt, iso), dims)
    return components(lab, dims), lab


def kept(comps, largest=1, min_voxels=0):
    """Which components of the sorted list vcy_keep_components keeps (bool per component)."""
    n = len(comps["label"])
    rank_ok = np.ones(n, bool) if largest <= 0 else np.arange(n) < largest
    return rank_ok & (comps["n_voxels"] >= min_voxels)


def filter_state(sdf, labels, comps, largest=1, min_voxels=0, fill_sdf=1.0):
    """What vcy_keep_components leaves: (new sdf, removed voxel mask, removed components, removed voxels)."""
    keep = kept(comps, largest, min_voxels)
    gone = np.isin(labels, comps["label"][~keep])
    out = np.array(sdf, np.float32, copy=True)
    out[gone] = np.float32(fill_sdf)
    return out, gone, int((~keep).sum()), int(comps["n_voxels"][~keep].sum())


def subset(comps, mask):
    return {k: v[mask] for k, v in comps.items()}


def assert_components_equal(got, want, ctx=""):
    for k in ("label", "n_voxels", "bb_min", "bb_max"):
        assert got[k].shape == want[k].shape, "%s %s: %d components against %d" % (ctx, k, len(got[k]), len(want[k]))
        assert np.array_equal(got[k], want[k]), "%s %s differs" % (ctx, k)
