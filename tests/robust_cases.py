"""Scenes of the robust-carve tests, shared by the CPU test of the restatement and the GPU test of the kernel: grids, modes,
view sets (the views of test_gpu_render.py: pinhole and orthographic, a shrunk and a one-pixel ROI, a camera that looks
away from the grid) and adversarial SDF images after the recipe of test_gpu_parity.test_view_dropping_is_exact (white
noise, plateaus of exact ties, NaN / +-inf / lowest() pixels)."""
import numpy as np

import test_gpu_render as TR
from vacancy_amd.capi import CarverOption, UpdateOption

F = np.float32
W, H = TR.W, TR.H  # 48 x 40

# kwargs of UpdateOption (always kMax).  The default mode is compiled into the kernel, every other takes the run-time path.
MODES = {
    "default": dict(),
    "nn": dict(sdf_interp=0),
    "outside_max": dict(update_outside=1),
    "trunc": dict(use_truncation=True, truncation_band=0.2),
    "nn_outside_trunc": dict(sdf_interp=0, update_outside=1, use_truncation=True, truncation_band=0.2),
}

# (65, 9, 17) crosses the 64-lane word and the brick edges; (257, 3, 2): a second block of a row with one live lane
DIMS = [(65, 9, 17), (24, 20, 17), (1, 1, 1), (257, 3, 2)]

VIEW_SETS = {
    "pinhole": ["pinhole_outside", "roi_shrunk", "pinhole_inside", "pinhole_away", "roi_one_pixel"],
    "ortho": ["ortho_axis", "ortho_negx", "ortho_oblique"],
    "mixed": ["pinhole_outside", "ortho_oblique", "roi_shrunk", "ortho_axis", "pinhole_inside", "pinhole_away", "ortho_negx",
              "roi_one_pixel"],
}


def option_for(dims, mode="default"):
    dims = tuple(dims)
    ext = TR.BOX[dims] if dims in TR.BOX else tuple(d + 0.3 for d in dims)
    h = [e / 2.0 for e in ext]
    return CarverOption(bb_min=[-x for x in h], bb_max=h, resolution=1.0, update_option=UpdateOption(**MODES[mode]))


def sdf_image(kind, seed, w=W, h=H):
    """kind 0: a smooth signed distance to a disc; 1: white noise (below -1 too: the truncation test); 2: plateaus, many
    exact ties; 3: the smooth image poisoned with NaN, +-inf and lowest()."""
    rng = np.random.RandomState(1000 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cx, cy, r = w * (0.35 + 0.3 * rng.rand()), h * (0.35 + 0.3 * rng.rand()), min(w, h) * (0.2 + 0.25 * rng.rand())
    base = ((np.hypot(xx - cx, yy - cy) - r) / (0.5 * max(w, h))).astype(F)
    if kind == 1:
        base = rng.uniform(-1.5, 1.0, base.shape).astype(F)
    elif kind == 2:
        base = (np.round(base * 4) / 4).astype(F)
    elif kind == 3:
        base[rng.rand(h, w) < 0.02] = np.nan
        base[rng.rand(h, w) < 0.02] = np.inf
        base[rng.rand(h, w) < 0.02] = np.finfo(np.float32).min
        base[rng.rand(h, w) < 0.02] = -np.inf
    return np.ascontiguousarray(base)


def scene(dims, set_name, n_views):
    """(views, sdf images): the views of the set taken in turn, every index with an image of its own."""
    table = TR.views_for(tuple(dims))
    names = VIEW_SETS[set_name]
    views = [table[names[i % len(names)]] for i in range(n_views)]
    sdfs = [sdf_image(i % 4 if n_views > 1 else 3, 7 * i + len(names)) for i in range(n_views)]
    return views, sdfs


# (set, n_views): 1 and 2 views leave n <= m; 70 lies beyond the fused kernel's 64 views and beyond 64-bit masks
CALLS = [("mixed", 1), ("mixed", 2), ("pinhole", 5), ("ortho", 5), ("mixed", 70)]
