"""The float-class scenes (tests/float_class_scenes.py) do what test_gpu_float_classes.py needs of them -- shown from the
CPU oracle alone, without a GPU:

  - the views select the three tile paths by the host's rule, and the cut ROIs do cut the grid's projection;
  - the final states hold, at touched voxels, a denormal, -0, +inf, -inf, NaN, and lowest() under update_num > 0;
  - every named defect, emulated by transforming the INPUTS, changes the oracle's state at one voxel or more after one
    of the four batches: a kernel with that defect cannot pass the comparison with the oracle;
  - the exact-zero bilinear weight makes a NaN out of an image without one (0 * inf);
  - max_element restates std::max_element, and the oracle's outside voxels hold exactly that value."""
import numpy as np
import pytest

import depth_ref as DR
import float_class_scenes as S

F = np.float32
ids3 = lambda d: "%dx%dx%d" % d  # noqa: E731


def touched_classes(sdf, cnt):
    t = cnt > 0
    with np.errstate(invalid="ignore"):
        return {
            "denormal": int((t & (np.abs(sdf) < S.FLT_MIN) & (sdf != 0)).sum()),
            "minus_zero": int((t & (sdf == 0) & np.signbit(sdf)).sum()),
            "plus_inf": int((t & (sdf == np.inf)).sum()),
            "minus_inf": int((t & (sdf == -np.inf)).sum()),
            "nan": int((t & np.isnan(sdf)).sum()),
            "lowest_touched": int((t & (sdf == S.LOWEST)).sum()),
        }


@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_views_take_the_three_tile_paths_and_the_rois_cut(dims):
    vs, pos = S.views(dims), S.positions(dims)
    side = {name: max(8.0 * 1.7320508 * S.pixels_per_voxel(dims, vs[i]) + 3.0 for i in idx) for name, idx in S.BATCHES.items()}
    assert side["ppv07"] <= 15.0                             # the raw 16 x 16 tile
    assert side["ppv2"] > 15.0 and side["ppv2"] ** 2 <= 2048  # the 2048-pixel tile
    assert side["ppv5"] ** 2 > 2048                           # footprints beyond it: sample_generic
    assert side["ortho"] > 15.0
    for name, idx in S.BATCHES.items():
        assert len({bool(vs[i].is_ortho) for i in idx}) == 1, name  # one projection model per launch
    for i, v in enumerate(vs):
        assert v.roi_min[0] > 0 and v.roi_min[1] > 0  # pixel [0, 0] (the whole column 0) lies outside
        _, ins, _, _ = S.project(pos, v)
        assert ins.sum() > 0, i
        if i % 2 == 0:
            assert ins.sum() < len(ins), "view %d: the ROI cuts nothing" % i
    # the planted cells lie inside ROI_CUT, the four central ones inside ROI_TIGHT
    for k in range(16):
        (bx, by), (ix, iy) = S.planted_pixels(k)
        roi = S.ROI_TIGHT if k < 4 else S.ROI_CUT
        assert roi[0][0] <= bx and ix <= roi[1][0] and roi[0][1] <= by and iy <= roi[1][1], k


@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_final_states_reach_every_class(dims):
    total = {}
    per_set = {}
    for s in S.SETS:
        for opt in S.OPTIONS:
            got = touched_classes(*S.oracle_final(dims, opt, s))
            for k, v in got.items():
                total[k] = total.get(k, 0) + v
                per_set[s, k] = per_set.get((s, k), 0) + v
    for k, v in total.items():
        assert v > 0, "no final state of %s holds a touched voxel of class %s" % (dims, k)
    # ... and where the sets are made for a class, they reach it themselves
    assert per_set["denormals", "denormal"] > 0 and per_set["zeros", "minus_zero"] > 0
    assert per_set["huge", "plus_inf"] > 0 and per_set["huge", "lowest_touched"] > 0 and per_set["huge", "nan"] > 0
    assert per_set["inf", "plus_inf"] > 0 and per_set["inf", "minus_inf"] > 0 and per_set["inf", "nan"] > 0
    assert per_set["nan", "nan"] > 0 and per_set["max_sdf", "nan"] > 0
    # the overflow of the weighted average: the huge set holds no +inf, its unit-weight average makes many
    assert not any(np.isposinf(im).any() for im in S.image_set("huge"))
    assert touched_classes(*S.oracle_final(dims, "wa_w1", "huge"))["plus_inf"] > 100


@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_uploaded_state_holds_every_class_and_is_carved_on(dims):
    sdf, cnt = S.special_state(dims)
    with np.errstate(invalid="ignore"):
        for c in range(4):
            sel = sdf[cnt == c]
            assert np.isnan(sel).any() and np.isposinf(sel).any() and np.isneginf(sel).any() and (sel == S.LOWEST).any()
            assert ((sel == 0) & np.signbit(sel)).any() and ((np.abs(sel) < S.FLT_MIN) & (sel != 0)).any()
        assert ((cnt == 0) & (sdf == F(0.5))).any()  # a count of 0 over a valid value
    which = sum((S.BATCHES[b] for b in S.UPLOAD_FOLLOW), ())
    for opt in S.OPTIONS:
        for s in S.SETS:
            after = S.oracle_carve(dims, opt, S.image_set(s), which, state=(sdf, cnt))
            assert S.differ(after, (sdf, cnt)) > 0, (opt, s)
            assert touched_classes(*after)["nan"] > 0, (opt, s)  # (a NaN state stays one under both update rules)


# (defect, set, option): the oracle's state must change under the transformed inputs
DEFECT_CASES = [
    ("denormal_flush", "denormals", "kmax"), ("denormal_flush", "denormals", "wa_w1"),
    ("denormal_flush", "denormals", "kmax_trunc_nn"),
    ("lost_sign_of_zero", "zeros", "kmax"), ("lost_sign_of_zero", "zeros", "kmax_trunc_nn"),
    ("nan_ignoring_maximum", "max_sdf", "kmax_outside"), ("nan_ignoring_maximum", "max_sdf", "wa_w05_outside"),
    ("nan_ignoring_maximum", "nan", "kmax_outside"), ("nan_ignoring_maximum", "nan", "wa_w05_outside"),
    ("wrong_zero_of_maximum", "max_sdf", "kmax_outside"), ("wrong_zero_of_maximum", "zeros", "kmax_outside"),
    ("saturation", "inf", "kmax"), ("saturation", "inf", "wa_w1"), ("saturation", "max_sdf", "kmax_outside"),
]


@pytest.mark.parametrize("defect,set_name,opt", DEFECT_CASES)
@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_an_emulated_defect_changes_the_oracles_state(dims, defect, set_name, opt):
    images = S.image_set(set_name)
    none = np.zeros((S.H, S.W), np.int32)
    assert any(S.differ((S.DEFECTS[defect](im), none), (im, none)) > 0 for im in images), "the defect does not touch the inputs"
    # (the device is compared after every batch, so a difference in any of the four states would be seen)
    n = [S.differ(a, b) for a, b in zip(S.oracle_states(dims, opt, set_name), S.oracle_states(dims, opt, set_name, defect))]
    assert max(n) > 0, "%s would go unseen on %s / %s" % (defect, set_name, opt)


@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_defects_outside_the_roi_show_only_through_max_sdf(dims):
    """Without update_outside = kMax pixel [0, 0] is read by nothing: the NaN-ignoring maximum changes no state."""
    for s in ("max_sdf", "nan"):
        assert S.differ(S.oracle_final(dims, "kmax", s), S.oracle_final(dims, "kmax", s, "nan_ignoring_maximum")) == 0


@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_a_weight_of_exactly_zero_meets_an_inf(dims):
    img = S.zero_weight_image()
    assert not np.isnan(img).any() and not np.isneginf(img).any() and np.isposinf(img).any()
    v = S.views(dims)[6]
    _, ins, u, w = S.project(S.positions(dims), v)
    on_column = ins & (u == F(S.AXIS_COLUMN))
    assert on_column.sum() >= dims[1] * dims[2] // 2
    images = list(S.image_set("inf"))
    assert np.array_equal(images[6].view(np.uint32), img.view(np.uint32))
    sdf, cnt = S.oracle_carve(dims, "kmax", images, which=[6])
    nan = np.isnan(sdf)
    assert nan.any() and (nan <= on_column).all(), "a NaN that 0 * inf does not explain"
    assert np.isposinf(sdf).any()  # (a positive weight times inf next to it)


def test_max_element_is_std_max_element():
    rng = np.random.RandomState(5)
    a = rng.uniform(-1, 1, 50).astype(F)
    assert S.max_element(a) == (a.max(), int(a.argmax()))
    a[7] = a[31] = F(2.0)
    assert S.max_element(a) == (F(2.0), 7)                      # the first of equal maxima
    a[3] = np.nan
    assert S.max_element(a) == (F(2.0), 7)                      # a NaN that is not first never wins
    a[0] = np.nan
    m, i = S.max_element(a)
    assert np.isnan(m) and i == 0                               # the first pixel a NaN: nothing compares greater
    z = np.array([-1.0, -0.0, 0.0, -2.0], F)
    m, i = S.max_element(z)
    assert i == 1 and np.signbit(m)                             # +0 == -0: the first zero wins, with its sign
    m, i = S.max_element(z[::-1].copy())
    assert i == 1 and not np.signbit(m)
    assert S.max_element(np.full(5, -np.inf, F)) == (F(-np.inf), 0)


@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_the_oracles_outside_voxels_hold_max_element(dims):
    """One view on a fresh grid with update_outside = kMax: the voxels in front of the camera and outside the ROI hold
    *std::max_element of the image -- NaN, +inf, -inf and either zero included."""
    pos = S.positions(dims)
    for s in ("max_sdf", "zeros", "nan"):
        images = S.image_set(s)
        for i, v in enumerate(S.views(dims)):
            z, ins, _, _ = S.project(pos, v)
            out = ~ins & ~(z < 0)
            if not out.any():
                continue
            sdf, cnt = S.oracle_carve(dims, "kmax_outside", images, which=[i])
            m, _ = S.max_element(images[i])
            assert (cnt[out] == 1).all()
            if np.isnan(m):
                assert np.isnan(sdf[out]).all(), (s, i)
            else:
                assert (sdf[out].view(np.uint32) == m.view(np.uint32)).all(), (s, i)


# ---- depth -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_minus_zero_depth_is_no_measurement(dims):
    opt = S.option_for(dims)
    vs = list(S.views(dims))
    depths = [S.depth_image(v, i) for i, v in enumerate(vs)]
    for d in depths:
        assert ((d == 0) & np.signbit(d)).any() and np.isposinf(d).any() and (d == S.FLT_MAX).any()
        assert ((np.abs(d) < S.FLT_MIN) & (d != 0)).any()
    band = 200.0  # (wider than every camera depth: a depth of zero taken for a measurement gives a sample in -1 .. 0)
    stats = {}
    want = DR.carve_depth(opt, vs, depths, band, stats=stats)
    assert stats["invalid"] > 0 and stats["clamped"] > 0 and stats["between"] > 0
    wrong = DR.carve_depth(opt, vs, [S.minus_zero_is_a_measurement(d) for d in depths], band)
    assert S.differ(want, wrong) > 0
