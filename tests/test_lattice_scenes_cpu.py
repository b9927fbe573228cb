"""What keeps test_gpu_lattice.py from being vacuous, shown from the CPU oracle alone (no GPU, never the device): the
numpy restatement of the samplers equals the oracle on every lattice view; the views put voxels exactly on every decision
edge, in bricks of both kinds; every mutant of the restatement changes what the oracle computes; and the truncation meets
samples of exactly -1 and of the float below it.  The counts are printed once (-s)."""
import numpy as np
import pytest

import lattice_scenes as L
from vacancy_amd.capi import VCY_INTERP_BILINEAR, VCY_INTERP_NN

GRIDS = list(L.GRIDS)
PINHOLE = [n for n in L.VIEW_NAMES if not L.VIEWS[n][7]]
ORTHO = [n for n in L.VIEW_NAMES if L.VIEWS[n][7]]
OUTSIDE_MAX = 1  # vcy_update_option::update_outside (0: NONE)

# the issue's table for the 24 x 16 x 16 grid: (half, integer, roi_min, roi_max, z_zero, z_negative, tie_even)
TABLE = {
    "pin_ties": (384, 184, 0, 0, 0, 0, 288),
    "pin_int_roi": (0, 710, 44, 31, 0, 0, 0),
    "pin_half": (192, 999, 0, 0, 0, 0, 96),
    "ortho_ties": (5760, 0, 0, 0, 384, 384, 4320),
    "ortho_int_roi": (0, 2880, 405, 405, 384, 384, 0),
}

# mutant -> (nearest neighbour?, update_outside, truncation, the views whose one-view state it must change)
MUTANTS = {
    "half_even": (True, 0, False, ["pin_ties", "ortho_ties", "pin_big", "pin_half", "pin_fxfy", "pin_div3"]),
    "floor_half": (True, 0, False, ["pin_below_half"]),
    "strict_max": (False, OUTSIDE_MAX, False, ["pin_int_roi", "ortho_int_roi"]),
    "strict_min": (False, OUTSIDE_MAX, False, ["pin_int_roi", "ortho_int_roi", "pin_neg"]),
    "no_clamp": (False, 0, False, ["pin_int_roi", "ortho_int_roi"]),
    "le_trunc": (False, 0, True, ["pin_int_roi", "ortho_int_roi", "pin_half", "pin_neg", "pin_fxfy", "pin_div3"]),
}


def state_differs(a, b):
    """Voxels at which two (sdf, update_num) states differ; NaN equals NaN."""
    nan_a, nan_b = np.isnan(a[0]), np.isnan(b[0])
    bits = np.where(nan_a, 0, a[0].view(np.uint32)) != np.where(nan_b, 0, b[0].view(np.uint32))
    return int(((a[1] != b[1]) | (nan_a != nan_b) | bits).sum())


@pytest.mark.parametrize("grid", GRIDS)
def test_restatement_equals_the_oracle(grid):
    """Fresh grid, one view, kMax, update_outside NONE: sample_np with the reference's rule IS the oracle's sdf, for both
    samplers and every view; with update_outside MAX and with the truncation too, since the mutants are judged there."""
    pos = L.positions(grid)
    assert bool(((pos * 2) % 2 == 1).all()), "the voxel centres are no half-integers"
    for name, view, img in L.scene():
        for nn in (False, True):
            interp = VCY_INTERP_NN if nn else VCY_INTERP_BILINEAR
            for kw, uo in ((dict(), dict()), (dict(outside_max=True), dict(update_outside=OUTSIDE_MAX)),
                           (dict(truncation=True), dict(use_truncation=True, truncation_band=0.1))):
                mine = L.one_view_state(view, img, pos, nn, **kw)
                want = L.oracle_one_view(grid, view, img, sdf_interp=interp, **uo)
                assert state_differs(mine, want) == 0, (grid, name, nn, kw)


def test_every_class_is_reached():
    counts = {g: {n: {k: int(m.sum()) for k, m in L.classify(L.make(n), L.positions(g)).items()} for n in L.VIEW_NAMES}
              for g in GRIDS}
    keys = ("half", "tie_even", "integer", "roi_min", "roi_max", "below_half", "negative", "z_zero", "z_negative")
    for g in GRIDS:
        print("\n%s  %-15s %s" % (g, "view", " ".join("%10s" % k for k in keys)))
        for n in L.VIEW_NAMES:
            print("%s  %-15s %s" % (" " * len(g), n, " ".join("%10d" % counts[g][n][k] for k in keys)))
    for n, row in TABLE.items():
        c = counts["24x16x16"][n]
        got = (c["half"], c["integer"], c["roi_min"], c["roi_max"], c["z_zero"], c["z_negative"], c["tie_even"])
        assert got == row, (n, got, row)
    for g in GRIDS:
        c = counts[g]
        for k in ("half", "tie_even", "integer", "roi_min", "roi_max"):
            assert max(c[n][k] for n in PINHOLE) >= 16 and max(c[n][k] for n in ORTHO) >= 16, (g, k)
        # pc.z == 0 and < 0: orthographic only (a pinhole camera inside the grid is test_gpu_view_loop_paths' view 4);
        # u < 0 next to a ROI above 0 and the float below .5: pinhole only -- both need cx, which ortho does not read
        for k in ("z_zero", "z_negative"):
            assert max(c[n][k] for n in ORTHO) >= 16, (g, k)
        assert c["pin_neg"]["negative"] >= 16 and c["pin_below_half"]["negative"] >= 16, g
        assert c["pin_below_half"]["below_half"] >= 16, g  # (a whole column of 16 voxels and more)
        # the trap of the issue: ties whose floor is odd round alike under both rules -- pin_big's are all even
        assert c["pin_big"]["tie_even"] == c["pin_big"]["half"] >= 16, g
    # u == cx on a whole column along z: pc.x == 0 exactly on the plane x = -5.5
    for g in GRIDS:
        pos = L.positions(g)
        _, ins, u, _ = L.project(pos, L.make("pin_below_half"))
        col = ins & (u == L.BELOW_HALF) & (pos[:, 1] == 1.5)
        assert int(col.sum()) == 16 and len(set(pos[col, 2].tolist())) == 16, g


def test_host_tile_rule_picks_raw_tiles_for_two_views():
    """"tile" 0: raw tiles for the views at or below 0.85 pixels per voxel.  (pin_half is NOT one of them: fy = 64 over a
    depth of 64.5 is 0.99 pixels per voxel in y, and the rule takes the larger focal length.)"""
    raw = [n for n in L.VIEW_NAMES if not L.host_picks_big_tile([L.make(n)])]
    for n in raw:
        t, fx, fy = L.VIEWS[n][0], L.VIEWS[n][1], L.VIEWS[n][2]
        assert max(fx, fy) / t[2] <= 0.85, n
    assert len(raw) >= 2 and "pin_fxfy" in raw and "pin_div3" in raw, raw
    assert L.host_picks_big_tile([L.make(n) for n in L.VIEW_NAMES if not L.VIEWS[n][7]])


@pytest.mark.parametrize("grid", GRIDS)
def test_every_mutant_changes_the_oracle_state(grid):
    """The reference rule equals the oracle (first test); a mutant must differ from it in every view listed for it, or a
    kernel with that defect would pass test_gpu_lattice.py."""
    pos = L.positions(grid)
    lines = []
    for rule, (nn, outside, trunc, expected) in MUTANTS.items():
        uo = dict(sdf_interp=VCY_INTERP_NN if nn else VCY_INTERP_BILINEAR, update_outside=outside)
        if trunc:
            uo.update(use_truncation=True, truncation_band=0.1)
        diffs = {}
        for name, view, img in L.scene():
            want = L.oracle_one_view(grid, view, img, **uo)
            mutant = L.one_view_state(view, img, pos, nn, rule, outside_max=bool(outside), truncation=trunc)
            diffs[name] = state_differs(mutant, want)
        lines.append("%s %-10s %s" % (grid, rule, " ".join("%s=%d" % kv for kv in diffs.items() if kv[1])))
        for name in expected:
            assert diffs[name] > 0, (grid, rule, name, "the mutant changes nothing")
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("grid", GRIDS)
def test_classes_lie_in_sure_bricks_and_in_cut_bricks(grid):
    """Every coordinate class has a voxel in a brick the documented rule makes `sure` (the select-free run) and in a brick
    that a ROI edge cuts (the checked loop and its hand-over to sample_generic).  A voxel ON a ROI edge can never lie in a
    `sure` brick -- the rule wants the hull clear of the edge by the margin -- so roi_min / roi_max need the cut brick
    only; and the ties and integers must also reach a `sure` brick whose footprint fits the raw tile."""
    pos = L.positions(grid)
    brick, nb = L.brick_of(grid)
    in_sure, in_raw, in_cut = {}, {}, {}
    for name in L.VIEW_NAMES:
        view = L.make(name)
        rep = L.brick_report(grid, view)
        for k, m in L.classify(view, pos).items():
            held = np.bincount(brick, weights=m, minlength=nb) > 0
            in_sure[k] = in_sure.get(k, 0) + int((held & rep["sure"]).sum())
            in_raw[k] = in_raw.get(k, 0) + int((held & rep["sure_raw"]).sum())
            in_cut[k] = in_cut.get(k, 0) + int((held & rep["cut"]).sum())
    for k in ("half", "tie_even", "integer", "below_half"):
        assert in_sure[k] >= 1 and in_raw[k] >= 1, (grid, k, "no sure brick holds a voxel of the class")
    for k in ("half", "tie_even", "integer", "below_half", "roi_min", "roi_max"):
        assert in_cut[k] >= 1, (grid, k, "no cut brick holds a voxel of the class")
    assert in_sure["roi_min"] == 0 and in_sure["roi_max"] == 0
    # u < 0 and pc.z < 0: next to sampled voxels inside one brick
    assert in_cut["negative"] >= 1 and in_cut["z_negative"] >= 1, grid


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nn", [False, True])
def test_truncation_meets_minus_one_and_the_float_below(grid, nn):
    """Under truncation the oracle keeps a voxel whose sample is exactly -1 and skips one whose sample is the float below
    it: both occur, through voxels with integer coordinates (the sample is the pixel)."""
    interp = VCY_INTERP_NN if nn else VCY_INTERP_BILINEAR
    kept = skipped = 0
    for name, view, img in L.scene():
        plain = L.oracle_one_view(grid, view, img, sdf_interp=interp)
        trunc = L.oracle_one_view(grid, view, img, sdf_interp=interp, use_truncation=True, truncation_band=0.1)
        at, below = plain[0] == L.MINUS_ONE, plain[0] == L.BELOW_MINUS_ONE
        assert bool((trunc[1][at] == 1).all()) and bool((trunc[0][at] == L.MINUS_ONE).all()), name
        assert bool((trunc[1][below] == 0).all()), name
        if not nn:  # the bilinear sum reaches them only where lu == lv == 0
            both = L.classify(view, L.positions(grid))["integer_both"]
            assert bool(both[at | below].all()), name
        kept, skipped = kept + int(at.sum()), skipped + int(below.sum())
    print("\n%s nn %d: %d voxels take exactly -1 (kept), %d the float below (skipped)" % (grid, nn, kept, skipped))
    assert kept >= 1 and skipped >= 1
