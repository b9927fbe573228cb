"""The step between two views' runs of the fused carve kernel: fused launches against the per-view kernel, bit for bit.

The kMax instances that keep their footprint records in registers carry, between two runs, a mask of the live views
still ahead and the next view's state as scalars (its record's tile word, the 32-bit offset of its view record), request
the next tile from one batch of the view's fields with 32-bit offsets from the image's base, and re-bound by ANDing the
mask with a ballot (carve_fused_kernel.h, carve_fused.h "the step between two views' runs").  Every case carves the same
views with the fused launch ("fused" 1, raw tiles forced with "tile" 1, "cull" 1 and 0) and with the per-view generic
kernel ("fused" 0) and compares sdf and update_num after every launch.  With "paircount" on, the fused launches also say
how many (brick, view) pairs they processed: fewer with "cull" 1 than with 0, and not none -- the bounds dropped views and
left views, so the mask was narrowed and walked.  What the cases are after, beyond tests/test_gpu_record_regs.py:

  - views whose images differ in width, height and ROI, interleaved in one launch (160 x 120, 96 x 64, 128 x 40 with a
    ROI): per-view request fields, 32-bit offsets from different image bases;
  - footprints in the last columns and rows of an image WITHOUT a ROI (the principal point shifted to the corner): tile
    windows clamped in x only, in y only and in both, at 0.2, 0.5, 0.9 and 1.7 pixels per voxel (1 to 4 row groups up
    to 0.9; at 1.7 most footprints exceed the raw tile: records without a tile, which are never dropped);
  - image levels in an order (0, -1, 2, 1, 3, -2, 2.5, ...) in which the view whose tile is in flight becomes droppable
    by the run in front of it and a later one does not: the re-bound moves the request;
  - the same at the mask's edges in a 64-view launch: views 31 and 32 fall and 33 is requested, 62 falls and 63 is
    requested, and 63 -- the last view -- falls and none remains;
  - an uploaded state in which the bricks of one half of the grid are above every view (the mask is empty at the start)
    and the others are raised by the last of 64 views only (the mask holds the top bit alone);
  - 65 views: two launches, the second of one view, over the slab the first left.

Grids of 40 x 24 x 24 and 36 x 20 x 20 voxels (as in test_gpu_record_regs.py), images of at most 160 x 120."""
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
FAR = 140.0
PPVS = [0.2, 0.5, 0.9, 1.7]  # pixels per voxel of the clamped-tile cases: 1, 2, 3 and 4 row groups
SPLIT_X = 16                 # "lastonly": voxels with x below it lie above every view (whole bricks: 16 = 2 x 8)


def grid_option(grid):
    nx, ny, nz = GRIDS[grid]
    return CarverOption(bb_min=(-nx / 2.0, -ny / 2.0, -nz / 2.0), bb_max=(nx / 2.0, ny / 2.0, nz / 2.0), resolution=1.0,
                        update_option=UpdateOption())


def camera(i, n, dist):
    """w2c of camera i of n on a Fibonacci sphere of radius `dist`, looking at the origin (synth.sphere_views)."""
    y = 1.0 - 2.0 * (i + 0.5) / n
    r = math.sqrt(max(0.0, 1.0 - y * y))
    phi = i * math.pi * (3.0 - math.sqrt(5.0))
    d = np.array([r * math.cos(phi), y, r * math.sin(phi)])
    return synth.affine_inverse(synth.lookat_c2w(dist * d, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))).astype(np.float32)


def level_image(i, w, h, level, amp):
    """A constant level plus a ripple of amplitude `amp`, different for every view."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    ripple = (0.6 * np.sin(xx * 0.11 + i) + 0.5 * np.cos(yy * 0.13 - 0.7 * i)) / 1.1
    return (amp * ripple + level).astype(np.float32)


REBOUND_LEVELS = [0.0, -1.0, 2.0, 1.0, 3.0, -2.0, 2.5, 3.5, 0.5, 4.0, 3.8, 4.5]


def edge_levels(last_falls):
    """64 levels: rising slowly, with steps at 30, 33 and 61 that the views right behind them lie below."""
    lv = [0.02 * i for i in range(30)] + [2.0, 1.0, 1.0, 3.0] + [3.0 + 0.02 * (i - 33) for i in range(34, 61)] + [5.0]
    return lv + ([6.0, 4.0] if last_falls else [4.0, 6.0])


@functools.lru_cache(maxsize=None)
def scene(kind):
    """([view], [image], amplitude of the ripple)."""
    f = synth.focal_from_fov_y(H, 60.0)  # 0.74 pixels per voxel at FAR
    centre = lambda w, h: (np.float32(w / 2 - 0.5), np.float32(h / 2 - 0.5))
    views, imgs = [], []
    if kind == "mixed":
        levels = [0.0, 0.5, 1.0, -3.0, 1.5, 2.0, -3.0, 2.5, 3.0, -3.0, 3.5, 4.0]
        for i, lv in enumerate(levels):
            if i % 3 == 0:
                w, h, fi, roi = W, H, f, {}
            elif i % 3 == 1:
                w, h, fi, roi = 96, 64, np.float32(0.5 * FAR), {}
            else:  # the grid projects to about 55..72 x 12..27: the ROI cuts it on all four sides
                w, h, fi, roi = 128, 40, np.float32(0.4 * FAR), dict(roi_min=(60, 15), roi_max=(68, 23))
            cx, cy = centre(w, h)
            views.append(make_view(camera(i, len(levels), FAR), fi, fi, cx, cy, w, h, **roi))
            imgs.append(level_image(i, w, h, lv, 0.3))
        return views, imgs
    if kind.startswith("clamp"):
        fi = np.float32(float(kind[5:]) * FAR)
        levels = [0.0, 1.0, 2.0, -3.0, 3.0, 4.0]
        cx0, cy0 = centre(W, H)
        for i, lv in enumerate(levels):  # the grid's centre 6 pixels from the last column (views 0, 1), row (2, 3), both (4, 5)
            cx = np.float32(W - 7) if i // 2 in (0, 2) else cx0
            cy = np.float32(H - 7) if i // 2 in (1, 2) else cy0
            views.append(make_view(camera(i, len(levels), FAR), fi, fi, cx, cy, W, H))
            imgs.append(level_image(i, W, H, lv, 0.3))
        return views, imgs
    levels, amp = {"rebound": (REBOUND_LEVELS, 0.15), "edges_next": (edge_levels(False), 0.08),
                   "edges_last": (edge_levels(True), 0.08), "lastonly": ([-5.0] * 63 + [5.0], 0.1),
                   "65": ([0.03 * i for i in range(64)] + [3.0], 0.3)}[kind]
    cx, cy = centre(W, H)
    for i, lv in enumerate(levels):
        views.append(make_view(camera(i, len(levels), FAR), f, f, cx, cy, W, H))
        imgs.append(level_image(i, W, H, lv, amp))
    return views, imgs


def initial_state(grid, kind):
    """(sdf, update_num) to upload before the views, or None for a fresh slab."""
    if kind != "lastonly":
        return None
    nx, ny, nz = GRIDS[grid]
    x = np.arange(nx * ny * nz) % nx
    return np.where(x < SPLIT_X, 10.0, 0.0).astype(np.float32), np.ones(nx * ny * nz, np.int32)


def carve(grid, kind, params):
    """(sdf, update_num) after the launch, (processed, total) pairs of the last fused launch (None without "paircount")."""
    dev = vc.VoxelCarver(grid_option(grid))
    assert dev.Init(), vc.last_error()
    for k, v in params:
        dev.set_param(k, v)
    state = initial_state(grid, kind)
    if state is not None:
        dev.upload(*state)
    views, imgs = scene(kind)
    ptrs = [dev.upload_sdf(im) for im in imgs]
    assert dev.CarveBatchDevice(views, ptrs), vc.last_error()
    out = dev.download()
    pairs = dev.last_carve_pairs()[:2] if ("paircount", 1) in params else None
    for p in ptrs:
        dev.free_device(p)
    dev.close()
    return out, pairs


@functools.lru_cache(maxsize=None)
def reference(grid, kind):
    """The per-view generic kernel, one launch of it per view ("fused" 0) -- computed once, never modified."""
    (s, u), _ = carve(grid, kind, (("fused", 0),))
    s.setflags(write=False)
    u.setflags(write=False)
    return s, u


def check(grid, kind, extra=()):
    """Both fused launches equal the reference; returns {cull: (processed, total)}."""
    rs, ru = reference(grid, kind)
    assert int((ru > 0).sum()) > 0, "the views touch nothing"
    pairs = {}
    for cull in (1, 0):
        params = (("fused", 1), ("tile", 1), ("cull", cull), ("paircount", 1)) + tuple(extra)
        (ds, du), pairs[cull] = carve(grid, kind, params)
        ctx = "%s %s %s" % (grid, kind, params)
        assert np.array_equal(du, ru), "%s: update_num differs at %d voxels" % (ctx, int((du != ru).sum()))
        bd, br = ds.view(np.uint32), rs.view(np.uint32)
        assert np.array_equal(bd, br), "%s: sdf bits differ at %d voxels" % (ctx, int((bd != br).sum()))
    print("%s %s: pairs processed / total, cull 1: %d / %d, cull 0: %d / %d" % ((grid, kind) + pairs[1] + pairs[0]))
    return pairs


def assert_dropped_some_not_all(pairs, bricks_min=1):
    """Not vacuous: the bounds dropped pairs ("cull" 1 processed fewer than "cull" 0) and left at least `bricks_min`."""
    (p1, t1), (p0, t0) = pairs[1], pairs[0]
    assert t1 == t0 and p0 <= t0
    assert p1 < p0, "no pair was dropped: %d of %d" % (p1, t1)
    assert p1 >= bricks_min, "too few pairs were processed: %d of %d" % (p1, t1)


def n_bricks(grid):
    nx, ny, nz = GRIDS[grid]
    return ((nx + 7) // 8) * ((ny + 7) // 8) * ((nz + 7) // 8)


@gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_mixed_images_in_one_launch(grid):
    assert_dropped_some_not_all(check(grid, "mixed"), 2 * n_bricks(grid))
    check(grid, "mixed", (("prologue", 1),))  # (the records made in the kernel's own prologue)


@gpu
@pytest.mark.parametrize("ppv", PPVS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_clamped_tiles_without_a_roi(grid, ppv):
    pairs = check(grid, "clamp%s" % ppv)
    if ppv < 1.0:
        assert_dropped_some_not_all(pairs)
    else:
        # 1.7 pixels per voxel: nearly every footprint exceeds the raw tile, and a record without a tile carries no bound
        # (it is never dropped); what the case adds is such records among the views ahead, at the image's edge
        assert 0 < pairs[1][0] <= pairs[0][0] == pairs[0][1], pairs


@gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_rebound_moves_the_request(grid):
    pairs = check(grid, "rebound")
    # levels 0, 2, 3, 3.5, 4, 4.5 rise above everything in front of them: every brick processes at least those six views
    # and drops at least -1, 1, -2 and 0.5 (each a whole level below a view in front of it)
    assert_dropped_some_not_all(pairs, 6 * n_bricks(grid))
    assert pairs[1][0] <= (len(REBOUND_LEVELS) - 4) * n_bricks(grid)


@gpu
@pytest.mark.parametrize("kind", ["edges_next", "edges_last"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_rebound_at_the_edges_of_the_mask(grid, kind):
    pairs = check(grid, kind)
    # views 0, 30, 33, 61 and the higher one of 62 / 63 rise above everything in front of them; 31, 32 and the lower one
    # of 62 / 63 lie a whole level below the view in front of them
    assert_dropped_some_not_all(pairs, 5 * n_bricks(grid))
    assert pairs[1][0] <= 61 * n_bricks(grid)


@gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_bricks_nothing_touches_and_bricks_only_the_last_view_touches(grid):
    pairs = check(grid, "lastonly")
    nx, ny, nz = GRIDS[grid]
    raised = ((nx + 7) // 8 - SPLIT_X // 8) * ((ny + 7) // 8) * ((nz + 7) // 8)  # the bricks at level 0
    # exactly: nothing in the bricks at level 10, the last view alone (level 5 against views at -5) in the others
    assert pairs[1][0] == raised, pairs
    assert pairs[0][0] == pairs[0][1] == 64 * n_bricks(grid), pairs
    s, u = reference(grid, "lastonly")
    x = np.arange(s.size) % nx
    assert (u[x < SPLIT_X] == 1).all() and (s[x < SPLIT_X] == 10.0).all() and (u[x >= SPLIT_X] == 2).all()


@gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_65_views_are_two_launches(grid):
    pairs = check(grid, "65")
    # (the pairs are the LAST launch's: one view over the slab the first 64 left, raised everywhere by it)
    assert pairs[0][1] == n_bricks(grid) and pairs[1][0] > 0
    s, u = reference(grid, "65")
    assert int(u.max()) > 1


# ---- the scenes hold what the cases are after (CPU: the oracle's voxel positions, projected as the reference does) ------

def footprints(grid, view):
    """Per wave brick: (min and max of floor(u), min and max of floor(v), voxels inside the image / ROI, voxels)."""
    nx, ny, nz = GRIDS[grid]
    orc = O.OracleGrid(grid_option(grid))
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
    # mixed: three image shapes, every grid voxel inside the two images without a ROI, the ROI cutting bricks
    views, imgs = scene("mixed")
    assert {(v.width, v.height) for v in views} == {(160, 120), (96, 64), (128, 40)}
    assert all(im.shape == (v.height, v.width) for v, im in zip(views, imgs))
    for i, view in enumerate(views):
        fp = footprints(grid, view)
        if i % 3 != 2:
            assert all(n_in == n for _, _, _, _, n_in, n in fp)
        else:
            assert any(0 < n_in < n for _, _, _, _, n_in, n in fp) and any(n_in == n for _, _, _, _, n_in, n in fp)
    # clamped tiles: bricks that lie inside the image and fit a raw tile (at most 15 pixels with the second tap), whose
    # 16-pixel window crosses the last column only / the last row only / both.  With these oblique cameras a brick's
    # footprint is 4 - 5 pixels high at 0.2 pixels per voxel, 6 - 9 at 0.5 and 9 - 14 at 0.9: one and two, two and three,
    # three and four row groups; at 1.7 most footprints exceed the raw tile (records without a tile among the views
    # ahead), and the few that fit have four.
    all_groups = set()
    for ppv in PPVS:
        views, _ = scene("clamp%s" % ppv)
        seen, beyond = set(), 0
        for i, view in enumerate(views):
            for x0, x1, y0, y1, n_in, n in footprints(grid, view):
                tw, th = x1 - x0 + 2, y1 - y0 + 2  # (the tile reaches one pixel beyond the last floor: the second tap)
                beyond += n_in == n and max(tw, th) > 15
                if n_in == n and tw <= 15 and th <= 15 and x1 + 1 <= W - 1 and y1 + 1 <= H - 1:
                    cl = (x0 + 15 > W - 1, y0 + 15 > H - 1)
                    seen.add(cl)
                    if cl != (False, False):
                        all_groups.add((th >> 2) + 1)
        if ppv < 1.0:
            assert {(True, False), (False, True), (True, True)} <= seen and beyond == 0, (ppv, seen, beyond)
        else:
            assert beyond > 0, ppv
    assert all_groups == {1, 2, 3, 4}, all_groups
    # the levels: a view said to fall lies a ripple's width below the view said to make it fall
    for kind, falls in (("rebound", [(1, 0), (3, 2), (5, 4), (8, 7)]), ("edges_next", [(31, 30), (32, 30), (62, 61)]),
                        ("edges_last", [(31, 30), (32, 30), (63, 62)]), ("lastonly", [(62, 63)])):
        _, imgs = scene(kind)
        for low, high in falls:
            assert float(imgs[low].max()) < float(imgs[high].min()) - 0.5, (kind, low, high)
    for kind, stays in (("rebound", [(2, 1), (4, 3), (7, 6), (9, 8), (11, 10)]), ("edges_next", [(33, 32), (63, 62), (31, 29)]),
                        ("edges_last", [(33, 32), (62, 61), (63, 61 - 1)])):
        _, imgs = scene(kind)
        for later, earlier in stays:  # ... and a view said to stay lies above everything in front of it
            assert float(imgs[later].min()) > max(float(im.max()) for im in imgs[:earlier + 1]), (kind, later, earlier)
    assert len(scene("65")[0]) == 65 and len(scene("edges_next")[0]) == 64
    s, u = initial_state(grid, "lastonly")
    assert s.size == np.prod(GRIDS[grid]) and set(np.unique(s)) == {0.0, 10.0} and SPLIT_X % 8 == 0
