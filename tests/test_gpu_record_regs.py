"""Footprint records kept in registers: the fused carve launch against the per-view generic kernel, bit for bit.

The kMax instances of the fused kernel with raw tiles and a brick per wave keep the 8-byte footprint record of view v in
lane v and take it apart per processed view (v_readlane + scalar unpack, carve_fused.h: unpack_footprint_scalar); the
other instances keep a TileInfo per view in LDS.  Every case below carves the same views with the fused launch ("fused" 1,
raw tiles forced with "tile" 1) and with the per-view generic kernel ("fused" 0) and compares sdf and update_num after
every launch; where views can be dropped, the fused launch also runs with "cull" 0.  What the cases are after:

  - 2, 31, 32, 33, 63 and 64 views on a fresh slab: the lanes around 32 and lane 63 hold records, and 64 views is the
    special case of the view mask;
  - a second launch of 5 views over the carved slab: not fresh, brick minima valid, waves that return early;
  - cameras so close that a brick's footprint exceeds 15 x 15 pixels: records without a tile, the generic sampler;
  - an ROI inside the grid's footprint: tiles that end at the ROI's last column and row (edge bits), views that are not
    `sure`, so the checked loop forms the tile bounds from the record itself;
  - an 8192 x 16 image with the footprint in its last columns: tx0 at the top of its 13-bit field;
  - kMax, the unit-weight average with truncation and the weight 0.37 (instances that keep the LDS TileInfo);
  - "recordbytes" forced small (a launch in several chunks), "prologue" 1 (records made in the kernel's own prologue)
    and "rowkernel" 4 (the few-view flavour).

Grids of 40 x 24 x 24 (rows of whole bricks) and 36 x 20 x 20 voxels (scalar state I/O, clamped lanes), images of
160 x 120 with 0.74 pixels per voxel."""
import functools
import math

import numpy as np
import pytest

import oracle_lib as O
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import CarverOption, UpdateOption, make_view

gpu = pytest.mark.gpu

W, H = 160, 120
GRIDS = {"40x24x24": (40, 24, 24), "36x20x20": (36, 20, 20)}
MODES = {
    "max": dict(),
    "wa_unit_trunc": dict(voxel_update=1, use_truncation=True, truncation_band=0.1),
    "wa_037": dict(voxel_update=1, voxel_update_weight=0.37),
}
FAR = 140.0   # 0.74 pixels per voxel: a brick's footprint stays below 15 pixels
NEAR = 50.0   # 2.1 pixels per voxel: 8 voxels alone span more than 15


def grid_option(grid, mode):
    nx, ny, nz = GRIDS[grid]
    return CarverOption(bb_min=(-nx / 2.0, -ny / 2.0, -nz / 2.0), bb_max=(nx / 2.0, ny / 2.0, nz / 2.0), resolution=1.0,
                        update_option=UpdateOption(**MODES[mode]))


def camera(i, n, dist):
    """w2c of camera i of n on a Fibonacci sphere of radius `dist`, looking at the origin (synth.sphere_views)."""
    y = 1.0 - 2.0 * (i + 0.5) / n
    r = math.sqrt(max(0.0, 1.0 - y * y))
    phi = i * math.pi * (3.0 - math.sqrt(5.0))
    d = np.array([r * math.cos(phi), y, r * math.sin(phi)])
    return synth.affine_inverse(synth.lookat_c2w(dist * d, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))).astype(np.float32)


def image(i, w, h, offset):
    """A smooth SDF image, different for every view; values within about offset +- 1.1."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    return (0.6 * np.sin(xx * 0.11 + i) + 0.5 * np.cos(yy * 0.13 - 0.7 * i) + offset).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(kind, n):
    """([view], [image]) of n views."""
    f = synth.focal_from_fov_y(H, 60.0)
    cx, cy = np.float32(W / 2 - 0.5), np.float32(H / 2 - 0.5)
    offs = np.random.RandomState(5).uniform(-0.6, 0.6, 64)
    views, imgs = [], []
    for i in range(n):
        if kind == "far":
            views.append(make_view(camera(i, n, FAR), f, f, cx, cy, W, H))
            imgs.append(image(i, W, H, offs[i]))
        elif kind == "low":  # over a carved slab: four views below everything it holds, one that raises voxels
            views.append(make_view(camera(i, n, FAR), f, f, cx, cy, W, H))
            imgs.append(image(i, W, H, 0.9 if i == 2 else -3.5))
        elif kind == "near":  # every other camera so close that a whole brick does not fit a raw tile
            views.append(make_view(camera(i, n, NEAR if i % 2 else FAR), f, f, cx, cy, W, H))
            imgs.append(image(i, W, H, offs[i]))
        elif kind == "roi":  # the grid projects to about 65..95 x 51..69: the ROI cuts it on all four sides
            views.append(make_view(camera(i, n, FAR), f, f, cx, cy, W, H, roi_min=(70, 52), roi_max=(92, 66)))
            imgs.append(image(i, W, H, offs[i]))
        elif kind == "wide":  # 8192 x 16, 0.35 pixels per voxel, the grid's centre at column 8187.5
            fw = np.float32(0.35 * FAR)
            views.append(make_view(camera(i, n, FAR), fw, fw, np.float32(8187.5), np.float32(7.5), 8192, 16))
            imgs.append(image(i, 8192, 16, offs[i]))
        else:
            raise KeyError(kind)
    return views, imgs


def carve(grid, mode, kind, launches, params):
    """The states after every launch: [(sdf, update_num)]."""
    dev = vc.VoxelCarver(grid_option(grid, mode))
    assert dev.Init(), vc.last_error()
    for k, v in params:
        dev.set_param(k, v)
    out = []
    for li, count in enumerate(launches):
        # the first launch carves the "far" scene when another one follows (the slab the second launch finds)
        views, imgs = scene("far" if (li == 0 and len(launches) > 1) else kind, count)
        ptrs = [dev.upload_sdf(im) for im in imgs]
        assert dev.CarveBatchDevice(views, ptrs), vc.last_error()
        out.append(dev.download())
        for p in ptrs:
            dev.free_device(p)
    dev.close()
    return out


@functools.lru_cache(maxsize=None)
def reference(grid, mode, kind, launches):
    """The per-view generic kernel, one launch of it per view ("fused" 0) -- computed once, never modified."""
    out = carve(grid, mode, kind, list(launches), (("fused", 0),))
    for s, u in out:
        s.setflags(write=False)
        u.setflags(write=False)
    return out


def assert_same(got, want, ctx):
    assert len(got) == len(want)
    for li, ((ds, du), (rs, ru)) in enumerate(zip(got, want)):
        assert np.array_equal(du, ru), "%s launch %d: update_num differs at %d voxels" % (ctx, li, int((du != ru).sum()))
        bd, br = ds.view(np.uint32), rs.view(np.uint32)
        assert np.array_equal(bd, br), "%s launch %d: sdf bits differ at %d voxels" % (ctx, li, int((bd != br).sum()))


def check(grid, mode, kind, launches, extra=(), culls=(1, 0)):
    want = reference(grid, mode, kind, tuple(launches))
    for cull in culls:
        params = (("fused", 1), ("tile", 1), ("cull", cull)) + tuple(extra)
        assert_same(carve(grid, mode, kind, launches, params), want, "%s %s %s %s %s" % (grid, mode, kind, launches, params))
    return want


@gpu
@pytest.mark.parametrize("n", [2, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_view_counts_on_a_fresh_slab(grid, mode, n):
    (s, u), = check(grid, mode, "far", [n])
    assert int((u > 0).sum()) > u.size // 2, "the views touch too little of the grid"
    if mode == "max" and n >= 31:  # later views lie below what earlier ones left: there is something to drop
        assert int(u.max()) < n


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_second_launch_over_the_carved_slab(grid, mode):
    first, second = check(grid, mode, "low", [32, 5])
    changed = second[1] != first[1]
    assert changed.any(), "the second launch changes nothing"
    if mode == "max":  # (the averages take every sample that is not truncated)
        assert not changed.all(), "the second launch changes every voxel: no brick for a wave to leave early"


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_footprints_beyond_the_raw_tile(grid, mode):
    check(grid, mode, "near", [12])


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_roi_inside_the_footprint(grid, mode):
    check(grid, mode, "roi", [33])


@gpu
@pytest.mark.parametrize("mode", ["max", "wa_unit_trunc"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_footprint_in_the_last_columns_of_a_wide_image(grid, mode):
    check(grid, mode, "wide", [3])


@gpu
@pytest.mark.parametrize("extra", [(("recordbytes", 4000),), (("prologue", 1),)], ids=["recordbytes", "prologue"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_chunked_records_and_the_kernel_prologue(grid, mode, extra):
    check(grid, mode, "far", [32], extra)
    check(grid, mode, "roi", [33], extra, culls=(1,))


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_few_view_flavour(grid, mode):
    check(grid, mode, "low", [32, 4], (("rowkernel", 4),))


# ---- the scenes hold what the cases are after (CPU: the oracle's voxel positions, projected as the reference does) ------

def footprints(grid, view):
    """Per wave brick of the grid: (min and max of floor(u), min and max of floor(v), voxels inside the ROI, voxels)."""
    nx, ny, nz = GRIDS[grid]
    orc = O.OracleGrid(grid_option(grid, "max"))
    pos = orc.positions().astype(np.float32)
    orc.close()
    m = np.array(list(view.w2c), np.float32).reshape(3, 4)
    pc = [m[i, 3] + (m[i, 0] * pos[:, 0] + (m[i, 1] * pos[:, 1] + m[i, 2] * pos[:, 2])) for i in range(3)]
    u = np.float32(view.fx) / pc[2] * pc[0] + np.float32(view.cx)
    v = np.float32(view.fy) / pc[2] * pc[1] + np.float32(view.cy)
    inside = (u >= view.roi_min[0]) & (v >= view.roi_min[1]) & (u <= view.roi_max[0]) & (v <= view.roi_max[1])
    i = np.arange(len(pos))
    brick = ((i // (nx * ny)) // 8 * ((ny + 7) // 8) + (i // nx) % ny // 8) * ((nx + 7) // 8) + (i % nx) // 8
    out = []
    for b in range(int(brick.max()) + 1):
        sel = brick == b
        fu, fv = np.floor(u[sel]), np.floor(v[sel])
        out.append((int(fu.min()), int(fu.max()), int(fv.min()), int(fv.max()), int(inside[sel].sum()), int(sel.sum())))
    return out


@pytest.mark.parametrize("grid", list(GRIDS))
def test_the_scenes_hold_what_the_cases_are_after(grid):
    for view in scene("far", 33)[0]:  # every footprint fits a raw tile: at most 15 pixels with the second tap
        assert all(x1 - x0 + 2 <= 15 and y1 - y0 + 2 <= 15 and n_in == n for x0, x1, y0, y1, n_in, n in footprints(grid, view))
    near = scene("near", 12)[0]
    assert any(max(x1 - x0, y1 - y0) + 2 > 15 for x0, x1, y0, y1, _, _ in footprints(grid, near[1])), "every brick fits a raw tile"
    cut_right = cut_below = cut = whole = 0
    for view in scene("roi", 33)[0]:
        for x0, x1, y0, y1, n_in, n in footprints(grid, view):
            cut += 0 < n_in < n
            whole += n_in == n
            cut_right += n_in > 0 and x0 <= view.roi_max[0] <= x1   # the tile ends at the ROI's last column
            cut_below += n_in > 0 and y0 <= view.roi_max[1] <= y1   # ... row
    assert cut > 0 and whole > 0 and cut_right > 0 and cut_below > 0, (cut, whole, cut_right, cut_below)
    top = beyond = 0
    for view in scene("wide", 3)[0]:
        for x0, x1, y0, y1, n_in, n in footprints(grid, view):
            assert x0 >= 8176 - 8
            top += n_in > 0 and x0 >= 8184       # tx0 needs all 13 bits and its top bits are ones
            beyond += 0 < n_in < n and x1 > 8191  # voxels beyond the image's last column
    assert top > 0 and beyond > 0, (top, beyond)
