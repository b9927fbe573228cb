"""The expected values of the silhouette edge table (silhouette_cases.py), proven without a GPU: the oracle's SDF
builder against the definition it restates, and the product's host restatement against the oracle -- bit for bit, on
every case."""
import numpy as np

import oracle_lib as O
import silhouette_cases as S
from vacancy_amd import carver

FLT_MAX = np.finfo(np.float32).max
MAX_BRUTE_PIXELS = 4096


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def brute_distance(mask, rmin, rmax, seed_is_255):
    """min |dx| + |dy| over the seeds inside the ROI, for every ROI pixel, in int64; None when the ROI holds no seed."""
    roi = mask[rmin[1]:rmax[1] + 1, rmin[0]:rmax[0] + 1]
    ys, xs = np.nonzero((roi == 255) == seed_is_255)
    if len(xs) == 0:
        return None
    sx, sy = xs.astype(np.int64), ys.astype(np.int64)
    py, px = (a.ravel().astype(np.int64) for a in np.indices(roi.shape))
    out = np.empty(roi.size, np.int64)
    for i in range(0, roi.size, 512):  # pixels x seeds, 512 pixels at a time
        d = np.abs(px[i:i + 512, None] - sx[None, :]) + np.abs(py[i:i + 512, None] - sy[None, :])
        out[i:i + 512] = d.min(axis=1)
    return out.reshape(roi.shape)


def as_float(d, shape):
    return np.full(shape, FLT_MAX, np.float32) if d is None else d.astype(np.float32)


def brute_images(mask, rmin, rmax):
    """(DistanceTransformL1, untruncated unnormalised MakeSignedDistanceField) by the definition: 0 outside the ROI,
    FLT_MAX where the ROI holds no seed, the sign as voxel_carver.cc:176-203 takes it."""
    roi = mask[rmin[1]:rmax[1] + 1, rmin[0]:rmax[0] + 1]
    to_non255 = as_float(brute_distance(mask, rmin, rmax, False), roi.shape)  # 0 on the pixels != 255 themselves
    to_255 = as_float(brute_distance(mask, rmin, rmax, True), roi.shape)
    dist = np.zeros(mask.shape, np.float32)
    dist[rmin[1]:rmax[1] + 1, rmin[0]:rmax[0] + 1] = to_non255
    neg = np.where(to_non255 > 0, -to_non255, to_non255)                        # :176-182
    sdf = np.zeros(mask.shape, np.float32)
    sdf[rmin[1]:rmax[1] + 1, rmin[0]:rmax[0] + 1] = np.where(roi == 255, neg, to_255)  # :184-203
    return dist, sdf


def test_table_holds_what_the_edges_need():
    names = {c[0] for c in S.cases()}
    for rw in S.ROW_WIDTHS:
        for rx0 in S.ROW_LEFT_EDGES:
            for pad in (0, 3):
                tag = "rows/rw%d_x%d_pad%d/" % (rw, rx0, pad)
                want = ["%s_%s" % (s, p) for s in "ns" for p in ("first", "last", "only_outside")] + ["noise0.02", "noise0.5"]
                if rw >= 64:
                    want += ["n_lane63", "s_lane63"]
                if rw >= 65:
                    want += ["%s_lane%s" % (s, p) for s in "ns" for p in ("64", "63+64")]
                assert all(tag + k in names for k in want), tag
                c = S.case(tag + "n_first")
                assert c[1].shape == (3 + (5 if pad else 0), rx0 + rw + pad) and c[3][1] - c[2][1] == 2
                assert c[2][0] == rx0 and c[3][0] - rx0 + 1 == rw
    for rh in S.COL_HEIGHTS:
        for ry0 in S.COL_TOP_EDGES:
            c = S.case("cols/rh%d_y%d/n_middle_row" % (rh, ry0))
            assert c[2][1] == ry0 and c[3][1] - ry0 + 1 == rh and c[3][0] - c[2][0] + 1 == 5
            roi = c[1][c[2][1]:c[3][1] + 1, c[2][0]:c[3][0] + 1]
            assert int((roi != 255).any(axis=1).sum()) == 1  # one row holds every seed of the inside distance
    # the `only_outside` cases: the raw distance is +-FLT_MAX although seeds touch the ROI on every side that has a margin
    c = S.case("rows/rw65_x63_pad3/n_only_outside")
    raw = S.oracle_image(c, False, False, 0.1)
    assert (raw[c[2][1]:c[3][1] + 1, c[2][0]:c[3][0] + 1] == -FLT_MAX).all() and c[1][c[2][1], c[2][0] - 1] == 0
    c = S.case("rows/rw65_x63_pad3/s_only_outside")
    assert (S.oracle_image(c, False, False, 0.1)[c[2][1]:c[3][1] + 1, c[2][0]:c[3][0] + 1] == FLT_MAX).all()
    # the scratch-reuse pair: max |v| = FLT_MAX, then a few pixels
    a, b = S.scratch_pair()
    assert a[1].shape == b[1].shape
    assert np.abs(S.oracle_image(a, False, False, 0.1)).max() == FLT_MAX
    assert 1 < np.abs(S.oracle_image(b, False, False, 0.1)).max() < 40


def test_oracle_equals_the_brute_force_definition():
    checked = 0
    for name, mask, rmin, rmax in S.cases():
        assert (rmax[0] - rmin[0] + 1) * (rmax[1] - rmin[1] + 1) <= MAX_BRUTE_PIXELS, name  # no case is left out
        dist, sdf = brute_images(mask, rmin, rmax)
        assert np.array_equal(bits(O.distance_transform_l1(mask, rmin, rmax)), bits(dist)), name
        assert np.array_equal(bits(S.oracle_image((name, mask, rmin, rmax), False, False, 0.1)), bits(sdf)), name
        checked += 1
    assert checked == len(S.cases())


def test_host_restatement_equals_oracle_on_the_table():
    runs = 0
    for c in S.cases():
        name, mask, rmin, rmax = c
        assert np.array_equal(bits(carver.distance_transform_l1(mask, rmin, rmax)),
                              bits(O.distance_transform_l1(mask, rmin, rmax))), name
        for norm, trunc, band in S.settings(name):
            got = carver.make_sdf(mask, rmin, rmax, norm, trunc, band)
            assert np.array_equal(bits(got), bits(S.oracle_image(c, norm, trunc, band))), (name, norm, trunc, band)
            runs += 1
    assert runs >= 6 * len(S.cases()) + 2 * len(S.EQUALITY_BANDS)
