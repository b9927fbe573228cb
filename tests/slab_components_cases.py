"""Shared by tests/test_seam_components.py (host merge, no GPU) and tests/test_gpu_slab_components.py: where the grids are
cut, and the numpy restatement of what a slab reports before the merge (tests/components_ref.py on the slab's own
slices, ids made global)."""
import numpy as np

import components_ref as R

DIMS = [(9, 10, 17), (70, 23, 19), (130, 7, 5)]
DENSITIES = (0.2, 0.31, 0.5, 0.9)


def equal_cuts(nz, count):
    base, rem = divmod(nz, count)
    return [s * base + min(s, rem) for s in range(count)] + [nz]


def cuts_for(nz):
    """Equal slabs of 2, 3 and 4, a slab of 2 slices at either end, and a cut after every second slice; every slab has
    at least 2 slices (what a slab context needs)."""
    out = [equal_cuts(nz, k) for k in (2, 3, 4) if nz >= 2 * k]
    out += [[0, 2, nz], [0, nz - 2, nz], list(range(0, nz - 1, 2)) + [nz]]
    uniq = []
    for b in out:
        if b not in uniq and all(b1 - b0 >= 2 for b0, b1 in zip(b[:-1], b[1:])):
            uniq.append(b)
    return uniq


def slab_labels(solid, dims, z0, z1):
    """Provisional labels of the slab [z0, z1): int64 per voxel of the slab, global ids, -1 where not solid."""
    nx, ny, _ = dims
    s = nx * ny
    lab = R.label_volume(np.asarray(solid, bool)[z0 * s:z1 * s], (nx, ny, z1 - z0))
    return np.where(lab >= 0, lab + z0 * s, -1)


def slab_list(lab, dims, z0, z1):
    """The list a slab reports: its pieces with global labels and boxes."""
    nx, ny, nz = dims
    full = np.full(nx * ny * nz, -1, np.int64)
    full[z0 * nx * ny:z1 * nx * ny] = lab
    return R.components(full, dims)


def seam_pairs(lower_lab, upper_lab, dims):
    """(label below, label above) of EVERY voxel pair across the seam, duplicates left in."""
    s = dims[0] * dims[1]
    a, b = lower_lab[-s:], upper_lab[:s]
    m = (a >= 0) & (b >= 0)
    return np.stack([a[m], b[m]], 1).astype(np.int64)


def cut_volume(solid, dims, bounds):
    """(lists, pairs, labs) of a solid mask cut at `bounds`."""
    labs = [slab_labels(solid, dims, z0, z1) for z0, z1 in zip(bounds[:-1], bounds[1:])]
    lists = [slab_list(l, dims, z0, z1) for l, z0, z1 in zip(labs, bounds[:-1], bounds[1:])]
    pairs = [seam_pairs(labs[i], labs[i + 1], dims) for i in range(len(labs) - 1)]
    return lists, pairs, labs
