"""State carried across a change of path inside one wave's view loop, against the CPU oracle bit for bit.

The fused carve kernel keeps a brick's sdf / update_num in registers over all views of a launch, and every view takes
one of several paths through the loop body: the first touch of an untouched brick, the select-free runs (loops of their
own: consecutive `sure` views stay inside them), the checked loop with or without voxels the staged tile does not
cover.  What can go wrong there and nowhere else is the state on its way from one path to the next.  The base sequence
below makes consecutive views of the same brick take different paths:

  1. a view every brick is `sure` in (first touch);
  2. the same camera with a shrunk ROI: some bricks are clipped (checked loop, voxels outside the tile);
  3. a `sure` view from a camera next to the first (with truncation, view 1 has left voxels untouched);
  4. a camera inside the grid: voxels behind and exactly on the camera plane (depth outside the fast-division range);
  5. view 1 again (processed or dropped, changes nothing under kMax);
  6. an image with a NaN and an infinity inside the footprints (no bound);
  7. a `sure` view that raises only some voxels;
  8. a `sure` view that raises every voxel.

It is carved in launches of 1, 2, 8, 33 (cycling the eight) and 64 views and as two launches of 4 (the state is written
back and reloaded in between), and once starting with view 2, so that under kMax a `sure` view (3) meets bricks that are
only partly touched; on a grid of 3 x 2 x 2 bricks and on one whose rows are no multiple of 8 voxels (scalar state
I/O), in five update modes and once with two-byte counters.  The fused launch with raw 16 x 16 tiles ("tile" 1: the
instances whose loop holds the tile wait, the buffer swap and the prefetches), the same without view dropping, the fused
launch with the tile kind the host picks (raw for the launches of 1 and 2 views -- the one-view and few-view flavours --
and the big tile for every launch that holds view 4) and the per-view kernel must all give the oracle's state.  The CPU
test at the end checks, from the oracle's projections, that the scene really holds a brick inside the ROI of view 1, a
brick cut by the ROI of view 2, a voxel at or behind the camera plane of view 4, footprints below 15 pixels, and which
tile kind the host's rule picks for every launch."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from vacancy_amd import carver as vc
from vacancy_amd.capi import VCY_INTERP_NN, CarverOption, UpdateOption, make_view

W, H = 96, 72
GRIDS = {"24x16x16": 24, "20x16x16": 20}
MODES = {
    "max": dict(),
    "max_limit": dict(voxel_max_update_num=3),  # reached by the fourth change of a voxel: the CHECKMAX instance
    "wa_unit_trunc": dict(voxel_update=1, use_truncation=True, truncation_band=0.1),
    "wa_037": dict(voxel_update=1, voxel_update_weight=0.37),
    "nn": dict(sdf_interp=VCY_INTERP_NN),
}
# launches (numbers of views, cycling the eight) of a run
# launches (first view of the run, numbers of views cycling the eight)
RUNS = {"1": (0, [1]), "2": (0, [2]), "8": (0, [8]), "33": (0, [33]), "64": (0, [64]), "4+4": (0, [4, 4]),
        "8_from_view2": (1, [8])}
# ("fused", "cull", "tile"): the fused launch on raw tiles, the same without view dropping, the fused launch with the
# tile kind the host picks (host_picks_big_tile below), the per-view kernel
CONFIGS = [(1, 1, 1), (1, 0, 1), (1, 1, 0), (0, 1, 0)]


def grid_option(nx, **uo):
    return CarverOption(bb_min=(-nx / 2.0, -8.0, -8.0), bb_max=(nx / 2.0, 8.0, 8.0), resolution=1.0,
                        update_option=UpdateOption(**uo))


def base_sequence():
    """[(view, image)] x 8.  Cameras A / A2 look down +z from 100 voxels away: 0.8 pixels per voxel at the grid's centre, a
    brick's footprint is below 15 pixels and the host picks raw tiles; camera B sits inside the grid."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    cam_a = np.array([[1, 0, 0, 0.3], [0, 1, 0, -0.2], [0, 0, 1, 100.0]], np.float32)
    c, s = np.float32(np.cos(0.05)), np.float32(np.sin(0.05))
    cam_a2 = np.array([[c, 0, s, 1.0], [0, 1, 0, 0.5], [-s, 0, c, 102.0]], np.float32)
    cam_b = np.array([[1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, 2.5]], np.float32)  # pc.z = z + 2.5: 0 at z = -2.5
    f, cx, cy = 80.0, 47.5, 35.5
    full = lambda m: make_view(m, f, f, cx, cy, W, H)
    i1 = (0.5 * np.sin(xx * 0.21) + 0.4 * np.cos(yy * 0.17) + 0.2).astype(np.float32)
    i1[(xx - 44) ** 2 + (yy - 33) ** 2 < 16] -= 2.0  # (below -1: skipped by the truncating average)
    i2 = (0.5 * i1 + 0.6).astype(np.float32)
    i3 = (0.3 * np.cos(xx * 0.13 + yy * 0.11) + 0.5).astype(np.float32)
    i4 = (0.2 + 0.01 * xx - 0.005 * yy).astype(np.float32)
    i6 = (i3 + 0.25).astype(np.float32)
    i6[35, 47] = np.nan
    i6[30, 52] = np.inf
    i7 = i1.copy()
    i7[xx > 50] += 3.0
    i8 = (6.0 + 0.01 * xx + 0.02 * yy).astype(np.float32)
    return [(full(cam_a), i1),
            (make_view(cam_a, f, f, cx, cy, W, H, roi_min=(43, 27), roi_max=(53, 36)), i2),
            (full(cam_a2), i3),
            (full(cam_b), i4),
            (full(cam_a), i1),
            (full(cam_a), i6),
            (full(cam_a), i7),
            (full(cam_a), i8)]


def project(pos, view):
    """The oracle's projection of its voxel positions (orc_carve: the reference's operations in fp32, in its order)."""
    m = np.array(list(view.w2c), np.float32).reshape(3, 4)
    p = pos.astype(np.float32)
    with np.errstate(all="ignore"):
        pc = [m[i, 3] + (m[i, 0] * p[:, 0] + (m[i, 1] * p[:, 1] + m[i, 2] * p[:, 2])) for i in range(3)]
        u = np.float32(view.fx) / pc[2] * pc[0] + np.float32(view.cx)
        v = np.float32(view.fy) / pc[2] * pc[1] + np.float32(view.cy)
        inside = (u >= view.roi_min[0]) & (v >= view.roi_min[1]) & (u <= view.roi_max[0]) & (v <= view.roi_max[1])
    return pc[2], inside & ~(pc[2] < 0), u, v


def host_picks_big_tile(views):
    """The tile kind of a fused launch when "tile" is 0 (launch_carve_fused): pixels per voxel at the slab's centre -- the
    origin, for these grids -- of the view that has the most, and the big tile when 8 sqrt(3) of them + 3 exceed 15."""
    worst = np.float32(0)
    for v in views:
        pz = np.float32(v.w2c[11])  # t.z + R[2] . (0, 0, 0)
        worst = max(worst, np.float32(max(v.fx, v.fy)) / pz if pz > 0 else np.float32(np.inf))
    return bool(np.float32(8.0) * np.float32(1.7320508) * worst + np.float32(3.0) > np.float32(15.0))


SNAPSHOTS = (1, 2, 3, 4, 5, 6, 7, 8, 33, 64)


@functools.lru_cache(maxsize=None)
def oracle_states(grid, mode, max_update=None, start=0):
    """{views carved: (sdf, update_num)} of the cycled base sequence, begun at view `start` + 1 -- computed once per
    (grid, mode, start), never modified."""
    uo = dict(MODES[mode])
    if max_update is not None:
        uo["voxel_max_update_num"] = max_update
    orc = O.OracleGrid(grid_option(GRIDS[grid], **uo))
    assert orc.dims == (GRIDS[grid], 16, 16)
    seq = base_sequence()
    out = {}
    for i in range(max(SNAPSHOTS)):
        orc.carve(*seq[(start + i) % 8])
        if i + 1 in SNAPSHOTS:
            s, u = orc.download()
            s.setflags(write=False)
            u.setflags(write=False)
            out[i + 1] = (s, u)
    orc.close()
    return out


def assert_state_equal(ds, du, os_, ou, ctx):
    """Bit for bit; NaN voxels only need to be NaN on both sides (their payload is not pinned down)."""
    assert np.array_equal(du, ou), "%s update_num differs at %d voxels" % (ctx, int((du != ou).sum()))
    nan_d, nan_o = np.isnan(ds), np.isnan(os_)
    assert np.array_equal(nan_d, nan_o), ctx + " NaN voxels differ"
    bd, bo = np.where(nan_d, 0, ds.view(np.uint32)), np.where(nan_o, 0, os_.view(np.uint32))
    assert np.array_equal(bd, bo), "%s sdf bits differ at %d voxels" % (ctx, int((bd != bo).sum()))


def run_on_device(grid, mode, launches, count_bytes=1, max_update=None, start=0):
    uo = dict(MODES[mode])
    if max_update is not None:
        uo["voxel_max_update_num"] = max_update
    states = oracle_states(grid, mode, max_update, start)
    seq = base_sequence()
    for fused, cull, tile in CONFIGS:
        dev = vc.VoxelCarver(grid_option(GRIDS[grid], **uo))
        assert dev.Init(), vc.last_error()
        dev.set_param("fused", fused)
        dev.set_param("cull", cull)
        dev.set_param("tile", tile)
        if count_bytes != 1:
            dev.set_param("lazycount", 0)  # (the counters at their final width from the start)
        assert dev.get_param("count_bytes") == count_bytes
        imgs = [dev.upload_sdf(im) for _, im in seq]
        done = 0
        for n in launches:
            idx = [(start + done + i) % 8 for i in range(n)]
            assert dev.CarveBatchDevice([seq[i][0] for i in idx], [imgs[i] for i in idx]), vc.last_error()
            done += n
            ctx = "%s %s fused %d cull %d tile %d after %d views" % (grid, mode, fused, cull, tile, done)
            assert_state_equal(*dev.download(), *states[done], ctx)
        assert dev.get_param("count_bytes") == count_bytes
        for p in imgs:
            dev.free_device(p)
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_state_across_path_changes(grid, mode, run):
    start, launches = RUNS[run]
    run_on_device(grid, mode, launches, start=start)


@pytest.mark.gpu
def test_state_across_path_changes_two_byte_counters():
    """A limit of 1000 updates needs two-byte counters: the kernel instances of carve_fused_u16."""
    run_on_device("24x16x16", "max", [8], count_bytes=2, max_update=1000)
    run_on_device("20x16x16", "wa_unit_trunc", [4, 4], count_bytes=2, max_update=1000)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_scene_takes_the_paths(grid):
    """From the oracle's projections: a brick with every voxel inside the ROI of view 1, a brick with voxels on both sides
    of the ROI of view 2, a voxel at or behind the camera plane of view 4, footprints below 15 pixels; the tile kind the
    host picks for every launch of the runs; and the oracle's states show that the views do what the sequence says."""
    nx = GRIDS[grid]
    orc = O.OracleGrid(grid_option(nx))
    pos = orc.positions()
    orc.close()
    seq = base_sequence()
    i = np.arange(len(pos))
    brick = ((i // (nx * 16)) // 8 * 2 + (i // nx) % 16 // 8) * ((nx + 7) // 8) + (i % nx) // 8
    nb = int(brick.max()) + 1
    assert nb == ((nx + 7) // 8) * 4
    per_brick = lambda mask: np.bincount(brick, weights=mask, minlength=nb)
    size = per_brick(np.ones(len(pos)))
    _, in1, _, _ = project(pos, seq[0][0])
    assert int((per_brick(in1) == size).sum()) >= 1, "view 1: no brick with every voxel inside the ROI"
    _, in2, _, _ = project(pos, seq[1][0])
    n2 = per_brick(in2)
    assert int(((n2 > 0) & (n2 < size)).sum()) >= 1, "view 2: no brick cut by the ROI"
    assert int((n2 == size).sum()) >= 1, "view 2: no brick wholly inside the ROI (first touch -> run)"
    z4, _, _, _ = project(pos, seq[3][0])
    assert int((z4 <= 0).sum()) >= 1, "view 4: no voxel at or behind the camera plane"
    assert int((z4 == 0).sum()) >= 1 and int((z4 < 0).sum()) >= 1 and int((z4 > 0).sum()) >= 1
    # footprints of the bricks in every view but 4: the pixels their taps read span fewer than 15 in x and in y
    for k in (0, 1, 2, 4, 5, 6, 7):
        _, _, u, v = project(pos, seq[k][0])
        for b in range(nb):
            sel = brick == b
            for c in (u[sel], v[sel]):
                assert int(np.floor(c.max())) + 1 - int(np.floor(c.min())) + 1 < 15, (k, b)
    # the tile kind the host picks ("tile" 0): raw for the launches of one and two views, big wherever view 4 is carved
    views = [vw for vw, _ in seq]
    for name, (start, launches) in RUNS.items():
        done = 0
        for n in launches:
            idx = [(start + done + j) % 8 for j in range(n)]
            done += n
            assert host_picks_big_tile([views[j] for j in idx]) == (3 in idx), (name, idx)
    assert not host_picks_big_tile(views[:2]) and host_picks_big_tile(views)
    # what the views do, in the oracle's states
    st = oracle_states(grid, "max")
    assert int((st[1][1] == 0).sum()) == 0, "kMax: view 1 leaves voxels untouched"
    for k in (2, 3, 4):
        assert not np.array_equal(st[k - 1][1], st[k][1]), "kMax: view %d changes nothing" % k
    assert np.array_equal(st[5][1], st[4][1]), "kMax: the repeat of view 1 changes a voxel"
    assert int(np.isinf(st[6][0]).sum()) > 0, "the infinity of view 6 reaches no voxel"
    up7 = st[7][1] > st[6][1]
    assert 0 < int(up7.sum()) < len(pos), "view 7 raises no voxel, or every voxel"
    assert int((st[8][0] >= 6.0).sum()) == len(pos), "view 8 does not raise every voxel"
    tr = oracle_states(grid, "wa_unit_trunc")
    assert int((tr[1][1] == 0).sum()) > 0, "truncation: view 1 leaves no voxel untouched"
    assert int(np.isnan(tr[8][0]).sum()) > 0, "the NaN of view 6 reaches no voxel"
    # begun at view 2, kMax: the clipped view leaves bricks partly touched, and view 3 -- every voxel of them inside its
    # ROI -- touches the rest
    st2 = oracle_states(grid, "max", None, 1)
    t1 = per_brick(st2[1][1] > 0)
    partly = (t1 > 0) & (t1 < size)
    assert int(partly.sum()) >= 1, "begun at view 2: no brick is partly touched after it"
    _, in3, _, _ = project(pos, seq[2][0])
    assert int((per_brick(in3) == size)[partly].sum()) >= 1, "view 3 does not cover a partly touched brick"
    assert int((st2[2][1] == 0).sum()) == 0, "view 3 leaves voxels untouched"
    lim = oracle_states(grid, "max_limit")
    assert int(lim[64][1].max()) == 4, "the update limit is not reached"
