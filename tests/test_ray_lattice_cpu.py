"""CPU-only: the scenes of tests/ray_lattice_scenes.py hold what they are for, and the per-pixel model of the kernel's
walk (tests/ray_walk_model.py) tells the kernel's tie rules apart on them.

  * the model, unmutated, equals the numpy restatement (tests/render_ref.py) on every (grid, view, state), whole grid and
    z-slabs, with "rayskip" on and off: depth bits, voxel ids, entry axes;
  * the class counts of ray_lattice_scenes.classify reach their floors: ties of two and three axes, ties on two brick
    planes in sparse states, rays that start on planes, hits at t == -0.0;
  * every mutant of the model changes pixels on the whole-grid scenes and on the slab scenes named for it -- but
    entry_gt, which is equivalent (see test_mutants_change_pixels).

Measured when this was written (24x16x16 | 20x16x16; pixels of 1920 per view, summed over the scenes of MUTANT_SCENES):
  two-axis ties per view 997 .. 1919 | 977 .. 1919, three-axis ties on corner_out, negz, perm 514 .. 617 | 514 .. 565,
  ties on two brick planes at density 0.004 21 .. 118 | 27 .. 128; corner_in at density 0.3: 1000 hits at +0.0, 960 of
  them at t == -0.0, 920 rays start inside a solid voxel.
  mutant      whole grid   slabs
  step_le     2762 | 2762   306 | 278
  brick_le     162 |  204   119 | 119
  count_flip  2629 | 2629   162 |  99
  count_lt    2549 | 2549   164 | 111
  entry_gt       0 |    0     0 |   0
  neg_zero    1920 | 1920  1920 | 1920
  start_le    3360 | 3360  3840 | 3840
  still_lt     239 |  239   103 | 108
Over ALL scenes of the 24-wide grid (rayskip 1) the mutants change 4148, 342, 9630, 7469, 0, 960, 6720 and 681 pixels;
brick_le changes 20 to 92 pixels per view on the corner_cut states and 5 | 2 on all other states together."""
import numpy as np
import pytest

import ray_lattice_scenes as R
import ray_walk_model as M
import render_ref as RR

ENTRY_VIEWS = ["corner_out", "negz", "perm", "neg_all", "on_far_face", "corner_out_roi", "negz_fxfy"]   # start outside

# mutant -> (whole-grid scenes (view, state, rayskip), slab scenes (view, state, cut set; rayskip 1)): the scenes that
# discriminate it, so that the test stays short; entry_gt runs where rays enter from outside
MUTANT_SCENES = {
    "step_le": ([("corner_in", "random_0.3", 1), ("on_face", "all_solid", 0)], [("on_face", "random_0.03", "at_5_11")]),
    "brick_le": ([(v, "corner_cut", 1) for v in ("on_face", "corner_out", "corner_in")],
                 [("on_face", "corner_cut", "at_8"), ("negz", "corner_cut", "at_5_11"), ("corner_out", "corner_cut", "at_5")]),
    "count_flip": ([("on_face", "random_0.3", 1), ("perm", "all_solid", 1)],
                   [("on_far_face", "random_0.03", "at_8"), ("perm", "random_0.03", "at_5")]),
    "count_lt": ([("on_face", "random_0.3", 1), ("on_far_face", "all_solid", 1)],
                 [("on_far_face", "random_0.03", "at_8"), ("on_far_face", "random_0.03", "at_5")]),
    "entry_gt": ([(v, s, 1) for v in ENTRY_VIEWS for s in ("random_0.3", "random_0.03", "all_solid")],
                 [(v, s, "at_5_11") for v in ENTRY_VIEWS for s in ("random_0.03", "corner_cut")]),
    "neg_zero": ([("corner_in", "random_0.3", 1), ("corner_in", "random_0.3", 0)],
                 [("corner_in", "random_0.3", "at_5"), ("corner_in", "random_0.3", "at_5_11")]),
    "start_le": ([("corner_in", "random_0.3", 1), ("on_face", "all_solid", 0)],
                 [("corner_in", "random_0.3", "at_5"), ("corner_in", "random_0.3", "at_5_11")]),
    "still_lt": ([("corner_in", "all_solid", 1), ("on_far_face", "random_0.3", 0), ("on_face", "random_0.3", 1)],
                 [("corner_in", "random_0.03", "at_5_11"), ("on_far_face", "random_0.03", "at_5")]),
}

_rays = {}


def rays_of(grid, vn):
    if (grid, vn) not in _rays:
        _rays[grid, vn] = M.Rays(R.views(grid)[vn], R.planes_of(grid), R.dims_of(grid))
    return _rays[grid, vn]


def differing(a, b):
    return int(((a[0].view(np.uint32) != b[0].view(np.uint32)) | (a[1] != b[1]) | (a[2] != b[2])).sum())


def own(sn, vn):
    return vn if sn == "corner_cut" else None


def slabs_of(cut):
    b = R.CUT_SETS[cut]
    return list(zip(b[:-1], b[1:]))


# ---- 1. the scenes ---------------------------------------------------------------------------------------------------

def test_views_are_exact():
    for grid in R.GRID_NAMES:
        R.planes_of(grid)                                    # (asserts that every plane is an integer)
        assert R.dims_of(grid) == RR.grid_dims(list(R.option(grid).bb_min), list(R.option(grid).bb_max), 1.0)
        for vn, v in R.views(grid).items():
            o, d, roi = RR.rays(v)
            assert np.array_equal(o, np.round(o)) and len(np.unique(o, axis=1).T) == 1, vn   # an integer camera centre
            f = max(v.fx, v.fy)
            assert np.array_equal(d * f, np.round(d * f)), vn   # d is a multiple of 1 / f: exact
            assert int(roi.sum()) == (1920 if vn != "corner_out_roi" else 36 * 32)
        signs = {vn: tuple(sorted(set(np.sign(RR.rays(v)[1][2]).astype(int).tolist()))) for vn, v in R.views(grid).items()}
        assert signs["corner_out"] == (1,) and signs["negz"] == (-1,) and signs["neg_all"] == (-1,)
        assert signs["perm"] == (-1, 0, 1)                   # z is an image axis there: all three signs of s_z


@pytest.mark.parametrize("grid", R.GRID_NAMES)
def test_trace_is_the_restatement(grid):
    """The walk with notes gives the images of render_ref.render: its notes are notes on the restatement's paths."""
    for vn, v in R.views(grid).items():
        for sn in R.STATE_NAMES:
            solid = R.solid_of(grid, sn, own(sn, vn))
            tr = R.trace(v, R.planes_of(grid), R.dims_of(grid), solid)
            assert differing((tr["depth"], tr["voxel"], tr["axis"]), R.want(grid, vn, sn)) == 0, (vn, sn)


def test_render_by_sorting_is_the_restatement():
    """(what tests/test_gpu_render_long_axis.py takes for its one view along 12 282 cells) -- on scenes full of ties"""
    grid = "20x16x16"
    for vn, sn in (("corner_in", "random_0.3"), ("corner_in", "random_0.004"), ("on_face", "random_0.03"), ("perm", "random_0.03"),
                   ("on_far_face", "all_solid"), ("neg_all", "corner_cut"), ("corner_out_roi", "random_0.03")):
        got = R.render_by_sorting(R.views(grid)[vn], R.planes_of(grid), R.dims_of(grid), R.solid_of(grid, sn, own(sn, vn)))
        assert differing(got, R.want(grid, vn, sn)) == 0, (vn, sn)


@pytest.mark.parametrize("grid", R.GRID_NAMES)
def test_class_floors(grid):
    planes, dims, views = R.planes_of(grid), R.dims_of(grid), R.views(grid)
    cuts = sorted({z for b in R.CUT_SETS.values() for z in b[1:-1]})
    sz_at_cut = set()
    for vn, v in views.items():
        empty = R.classify(v, planes, dims, None, cuts)
        sparse = R.classify(v, planes, dims, R.solid_of(grid, "random_0.004"))
        print(grid, vn, empty, "density 0.004: tie_brick %d" % sparse["tie_brick"])
        if vn != "corner_in":
            assert empty["tie2"] >= 500, (vn, empty)
        if vn in ("corner_out", "negz", "perm"):
            assert empty["tie3"] >= 50, (vn, empty)
        assert sparse["tie_brick"] >= 10, (vn, sparse)
        assert empty["tie_inside"] >= 500, (vn, empty)
        assert int(R.solid_of(grid, "corner_cut", vn).sum()) >= 5, vn
        if empty["tie_at_cut"] >= 50:                        # ties on the planes the slabs are cut at, by the sign of s_z
            sz_at_cut |= set(np.sign(RR.rays(v)[1][2]).astype(int).tolist())
    assert sz_at_cut >= {-1, 1}, sz_at_cut
    # the camera on a lattice corner inside the grid
    dense = R.classify(views["corner_in"], planes, dims, R.solid_of(grid, "random_0.3"))
    print(grid, "corner_in at density 0.3", dense)
    assert dense["start_on_plane"] == 1920 and dense["still_on_plane"] >= 80
    want = R.want(grid, "corner_in", "random_0.3")
    assert (want[1] >= 0).all() and not want[0].view(np.uint32).any(), "a hit of corner_in is not at depth +0.0"
    assert dense["hit_negzero"] >= 400 and dense["hit_inside"] >= 400 and dense["hit_zero"] >= dense["hit_negzero"]
    # the camera on the grid's corner: the rays of the column u == cx and the row v == cy stand still on an axis whose
    # origin is P[0] (inside) or P[n] (outside: a miss whatever is solid)
    near = R.classify(views["on_face"], planes, dims, R.solid_of(grid, "all_solid"))
    far = R.classify(views["on_far_face"], planes, dims, R.solid_of(grid, "all_solid"))
    assert near["still_on_plane"] >= 80 and far["still_on_plane"] >= 80
    o, d, _ = RR.rays(views["on_face"])
    assert near["hit_zero"] == int(((d[0] >= 0) & (d[1] >= 0)).sum()) >= 1000 and near["hit_inside"] == 0
    o, d, _ = RR.rays(views["on_far_face"])
    still_out = ((d[0] == 0) & (o[0] == planes[0][-1])) | ((d[1] == 0) & (o[1] == planes[1][-1]))
    assert still_out.sum() >= 80 and (R.want(grid, "on_far_face", "all_solid")[1].reshape(-1)[still_out] == -1).all()
    o, d, _ = RR.rays(views["on_face"])
    still_in = (((d[0] == 0) & (d[1] >= 0)) | ((d[1] == 0) & (d[0] >= 0))).reshape(R.H, R.W)
    assert still_in.sum() >= 70
    assert (R.want(grid, "on_face", "all_solid")[1][still_in] >= 0).all()


def test_slab_cuts_are_tied_on():
    """The views tie on the very planes the slabs of CUT_SETS are cut at, with s_z > 0 and with s_z < 0."""
    for grid in R.GRID_NAMES:
        for k in (5, 8, 11):
            up = R.classify(R.views(grid)["corner_out"], R.planes_of(grid), R.dims_of(grid), None, (k,))["tie_at_cut"]
            down = R.classify(R.views(grid)["negz"], R.planes_of(grid), R.dims_of(grid), None, (k,))["tie_at_cut"]
            assert up >= 20 and down >= 20, (grid, k, up, down)


# ---- 2. the model equals the restatement -----------------------------------------------------------------------------

@pytest.mark.parametrize("grid", R.GRID_NAMES)
def test_model_equals_restatement_whole_grid(grid):
    for vn in R.VIEW_NAMES:
        for sn in R.STATE_NAMES:
            solid = R.solid_of(grid, sn, own(sn, vn))
            for rayskip in (1, 0):
                got = M.cast(rays_of(grid, vn), solid, None, rayskip)
                assert differing(got, R.want(grid, vn, sn)) == 0, (grid, vn, sn, rayskip)


@pytest.mark.parametrize("grid", R.GRID_NAMES)
def test_model_equals_restatement_slabs(grid):
    hits = 0
    for vn in R.VIEW_NAMES:
        for sn in R.SLAB_STATES:
            solid = R.solid_of(grid, sn, own(sn, vn))
            for z in sorted({z for cut in R.CUT_SETS for z in slabs_of(cut)}):
                want = R.want(grid, vn, sn, None, z)
                hits += int((want[1] >= 0).sum())
                for rayskip in (1, 0):
                    assert differing(M.cast(rays_of(grid, vn), solid, z, rayskip), want) == 0, (grid, vn, sn, z, rayskip)
    assert hits > 1000


# ---- 3. the mutants --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant", M.MUTANTS)
@pytest.mark.parametrize("grid", R.GRID_NAMES)
def test_mutants_change_pixels(grid, mutant):
    """entry_gt is equivalent.  When two out-of-range axes come into range at one t and the entry jump picks the LOWER as
    its event, count_before leaves the higher one plane short (for it axis_first is false), so it is still out of range;
    the next round's entry jump has that axis alone, takes its plane at the same t, and counts nothing more on the lower
    axis, whose next plane lies later: cell, t_in and a_in come out as if the higher axis had been picked at once."""
    whole, slab = MUTANT_SCENES[mutant]
    n_whole = n_slab = 0
    for vn, sn, rayskip in whole:
        solid = R.solid_of(grid, sn, own(sn, vn))
        n_whole += differing(M.cast(rays_of(grid, vn), solid, None, rayskip, mutant), R.want(grid, vn, sn))
    for vn, sn, cut in slab:
        solid = R.solid_of(grid, sn, own(sn, vn))
        for z in slabs_of(cut):
            n_slab += differing(M.cast(rays_of(grid, vn), solid, z, 1, mutant), R.want(grid, vn, sn, None, z))
    print(grid, mutant, "changes", n_whole, "pixels on whole-grid scenes,", n_slab, "on slab scenes")
    if mutant == "entry_gt":
        assert n_whole == 0 and n_slab == 0
    else:
        assert n_whole >= 10 and n_slab >= 10
