"""The seam merge of the sharded connected components on the host (no GPU): vcy_merge_components_host through
vacancy_amd.dist.merge_components.  numpy volumes are cut at given z bounds, every slab's sub-volume is labelled by
tests/components_ref.py with ids made global, the seam pairs are taken by numpy with their duplicates, and the merged
list and the per-slab maps have to EQUAL components_ref.reference on the whole volume."""
import numpy as np
import pytest

import components_ref as R
import slab_components_cases as S
from vacancy_amd import capi
from vacancy_amd import dist as vdist


def check_merge(solid, dims, bounds, ctx):
    solid = np.asarray(solid, bool).reshape(-1)
    want_lab = R.label_volume(solid, dims)
    want = R.components(want_lab, dims)
    lists, pairs, _ = S.cut_volume(solid, dims, bounds)
    merged, maps = vdist.merge_components(lists, pairs)
    R.assert_components_equal(merged, want, ctx)
    assert len(maps) == len(lists)
    for s, (l, m) in enumerate(zip(lists, maps)):
        # a provisional label is a voxel of its piece: the whole volume's label there is the merged label
        assert np.array_equal(m, want_lab[l["label"]]), "%s: the map of slab %d differs" % (ctx, s)
    return want, lists, pairs, maps


@pytest.mark.parametrize("dims", S.DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_random_volumes(dims):
    n = dims[0] * dims[1] * dims[2]
    cuts = S.cuts_for(dims[2])
    assert any(b1 - b0 == 2 for b in cuts for b0, b1 in zip(b[:-1], b[1:]))
    crossing = dups = 0
    for k, density in enumerate(S.DENSITIES):
        solid = np.random.RandomState(40 + k).rand(n) < density
        for bounds in cuts:
            want, lists, pairs, _ = check_merge(solid, dims, bounds, "%s density %g cuts %s" % (dims, density, bounds))
            assert len(want["label"]) > (1 if density < 0.9 else 0)  # (0.9: one body, and sometimes nothing else)
            crossing += sum(len(l["label"]) for l in lists) - len(want["label"])
            dups += sum(len(p) - len(np.unique(p, axis=0)) for p in pairs if len(p))
    assert crossing > 0, "no component of any volume crossed a seam"
    assert dups > 0, "no pair list had a duplicate"


def volume(dims):
    return np.zeros(dims[::-1], bool)  # [z][y][x]


def test_chain_across_three_seams():
    dims = (6, 3, 8)
    s = volume(dims)
    # a staircase: one step per slab, each joined to the next through one voxel column
    s[0:2, 0, 0:2] = True
    s[2:4, 0, 1:3] = True
    s[4:6, 0, 2:4] = True
    s[6:8, 0, 3:5] = True
    s[7, 2, 5] = True       # and a speck that joins nothing
    want, lists, _, maps = check_merge(s, dims, [0, 2, 4, 6, 8], "chain")
    assert want["label"].tolist() == [0, 7 * 18 + 2 * 6 + 5] and want["n_voxels"].tolist() == [16, 1]
    assert want["bb_min"][0].tolist() == [0, 0, 0] and want["bb_max"][0].tolist() == [4, 0, 7]
    assert [len(l["label"]) for l in lists] == [1, 1, 1, 2]
    assert [m[0] for m in maps] == [0, 0, 0, 0]


@pytest.mark.parametrize("arms_below", [True, False])
def test_u_shape_meets_only_in_the_other_slab(arms_below):
    """Two pieces of one slab that are one component only through the neighbouring slab, in either direction; the smallest
    id lies in the arms' slab once and in the bar's slab once."""
    dims = (5, 3, 4)
    s = volume(dims)
    arms, bar = ((0, 2), 2) if arms_below else ((2, 4), 1)
    s[arms[0]:arms[1], 1, 0] = True
    s[arms[0]:arms[1], 1, 4] = True
    s[bar, 1, :] = True
    want, lists, _, maps = check_merge(s, dims, [0, 2, 4], "U arms_below=%s" % arms_below)
    assert len(want["label"]) == 1 and want["n_voxels"].tolist() == [9]
    assert want["label"].tolist() == [5 if arms_below else 15 + 5]
    two, one = (lists[0], lists[1]) if arms_below else (lists[1], lists[0])
    assert len(two["label"]) == 2 and len(one["label"]) == 1
    assert all((m == want["label"][0]).all() for m in maps)


def test_equal_sizes_in_different_slabs_order_by_label():
    dims = (6, 4, 8)
    s = volume(dims)
    s[5:7, 2:4, 3:6] = True   # 12 voxels in the upper slab
    s[1:3, 0:2, 0:3] = True   # 12 voxels in the lower one
    s[3:5, 0, 5] = True       # 2 voxels across the seam
    want, lists, pairs, _ = check_merge(s, dims, [0, 4, 8], "tie")
    assert want["n_voxels"].tolist() == [12, 12, 2] and want["label"][0] < want["label"][1]
    assert want["label"][0] == 24 + 0 and want["label"][1] == 5 * 24 + 2 * 6 + 3
    assert len(pairs[0]) == 1


def test_empty_lists_and_duplicates():
    dims = (4, 3, 6)
    s = volume(dims)
    merged, maps = vdist.merge_components(*S.cut_volume(s.reshape(-1), dims, [0, 2, 4, 6])[:2])
    assert len(merged["label"]) == 0 and merged["bb_min"].shape == (0, 3) and [len(m) for m in maps] == [0, 0, 0]
    s[2:6, :, :] = True       # the lowest slab stays empty; the seam above it has no pairs
    want, lists, pairs, _ = check_merge(s, dims, [0, 2, 4, 6], "empty slab")
    assert len(lists[0]["label"]) == 0 and len(pairs[0]) == 0 and len(pairs[1]) == 12
    assert want["label"].tolist() == [24] and want["n_voxels"].tolist() == [48]
    # one slab: the list comes back as it is
    merged, maps = vdist.merge_components([want], [])
    R.assert_components_equal(merged, want, "one slab")
    assert maps[0].tolist() == [24]


def test_unknown_label_is_an_error():
    dims = (4, 3, 4)
    s = volume(dims)
    s[:, 1, 1] = True
    lists, pairs, _ = S.cut_volume(s.reshape(-1), dims, [0, 2, 4])
    vdist.merge_components(lists, pairs)
    for side in (0, 1):
        bad = pairs[0].copy()
        bad[0, side] += 1
        with pytest.raises(RuntimeError) as e:
            vdist.merge_components(lists, [bad])
        assert e.value.rc == capi.VCY_ERR_INVALID_ARG and "did not report" in str(e.value)
    # a label of the right slab on the wrong side of the pair
    with pytest.raises(RuntimeError):
        vdist.merge_components(lists, [pairs[0][:, ::-1]])
