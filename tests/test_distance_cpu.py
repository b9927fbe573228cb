"""The distance field of the hull without a GPU: the two statements of tests/distance_ref.py against each other (brute
force over all pairs of voxels == the separable evaluation), the serial host function of the library
(vcy_distance_field_host) against the restatement, bit for bit, on every case the GPU test uses, and the facts about the
closing that include/vacancy_hip.h quotes."""
import numpy as np
import pytest

import distance_cases as K
import distance_ref as R
from vacancy_amd import capi
from vacancy_amd import carver as vc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# (dims, density, R)
BRUTE_GRIDS = [((7, 6, 5), 0.3, 3), ((17, 10, 9), 0.05, 4), ((20, 6, 6), 0.9, 5), ((4, 4, 4), 0.0, 3), ((8, 9, 10), 0.02, 12)]


@pytest.mark.parametrize("dims,density,radius", BRUTE_GRIDS, ids=lambda v: str(v))
def test_brute_force_equals_separable(dims, density, radius):
    rng = np.random.RandomState(sum(dims) + radius)
    solid = rng.rand(dims[0] * dims[1] * dims[2]) < density
    brute, sep = R.brute_d2(solid, dims, radius), R.separable_d2(solid, dims, radius)
    assert np.array_equal(brute, sep)
    assert brute.min() >= 1
    if density == 0.0:
        assert (brute == R.far_of(radius)).all()
    else:
        assert solid.any() and (brute <= radius * radius).any()
    # ... and through the state: signs, phi
    sdf, cnt = K.state_from_mask(solid)
    a, b = R.reference(sdf, cnt, dims, 0.0, radius, brute=True), R.reference(sdf, cnt, dims, 0.0, radius)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    assert ((a[0] < 0) == solid).all()


def test_brute_force_equals_separable_on_a_random_state():
    dims, iso, radius = (9, 10, 7), 0.25, 4
    sdf, cnt = K.random_state(dims, 0.3, iso, 5)
    a, b = R.reference(sdf, cnt, dims, iso, radius, brute=True), R.reference(sdf, cnt, dims, iso, radius)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    untouched = cnt == 0
    assert untouched.any() and np.array_equal(bits(a[1][untouched]), bits(sdf[untouched]))
    assert (a[0][untouched] > 0).all() and (a[0][np.isnan(sdf)] > 0).all()


def check_host(case, resolution=1.0):
    name, dims, sdf, cnt, iso, radius = case
    want_d2, want_sdf = K.reference_of(case, resolution)
    d2, out = vc.distance_field_host(K.box_option(dims, resolution=resolution), sdf, cnt, iso, radius)
    assert np.array_equal(d2, want_d2), "%s %s: %d field values differ" % (name, dims, (d2 != want_d2).sum())
    assert np.array_equal(bits(out), bits(want_sdf)), "%s %s: sdf bits differ" % (name, dims)
    return d2


@pytest.mark.parametrize("dims", K.RANDOM_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_host_function_equals_restatement_random(dims):
    for case in K.random_cases(dims):
        d2 = check_host(case)
        far = R.far_of(case[5])
        assert (np.abs(d2) < far).any()
        if "one voxel" in case[0]:  # the largest exact value, and FAR next to it
            assert (d2 == 127 * 127).any() and (d2 == far).any()


def test_host_function_equals_restatement_named():
    for case in K.named_cases():
        d2 = check_host(case)
        far = R.far_of(case[5])
        if case[0] == "nothing solid":
            assert (d2 == far).all()
        if case[0] in ("everything solid", "65 wide, all solid"):
            assert (d2 == -far).all()
        if case[0] == "one solid voxel":
            assert (np.abs(d2) < far).any() and (d2 == far).any() and (d2 < 0).sum() == 1
        if case[0] == "slab at x = 0":  # the border is not a feature: the slab's depth counts from its open face alone
            f = d2.reshape(9, 10, 17)
            assert (f[:, :, 0] == -far).all() and (f[:, :, 5] == -1).all() and (f[:, :, 6] == 1).all()
    check_host(K.named_cases()[2], resolution=0.375)


def test_host_function_refusals():
    name, dims, sdf, cnt, iso, _ = K.named_cases()[2]
    for radius in (0, 128, -3):
        with pytest.raises(RuntimeError) as e:
            vc.distance_field_host(K.box_option(dims), sdf, cnt, iso, radius)
        assert e.value.rc == capi.VCY_ERR_INVALID_ARG and "radius" in str(e.value)
    with pytest.raises(ValueError):
        vc.distance_field_host(K.box_option(dims), sdf[:-1], cnt[:-1], iso, 3)


# ---- the closing ---------------------------------------------------------------------------------------------------------

def test_closing_fills_the_gap():
    sdf, cnt, dims, gap = R.two_blocks()
    before = R.solid_mask(sdf, cnt, 0.0)
    assert before.sum() == 250 and gap.sum() == 50 and not (before & gap).any()
    closed = R.solid_mask(R.close_hull(sdf, cnt, dims, 1.3), cnt, 0.0)
    assert np.array_equal(closed, before | gap) and closed.sum() == 300
    # ... and the host function composes to the same state
    r, big_r = vc.close_hull_plan(1.3, 1.0)
    assert (r, big_r) == R.close_plan(1.3, 1.0)
    s = sdf
    for level in (0.0, r, -r):
        s = vc.distance_field_host(K.box_option(dims), s, cnt, level, big_r)[1]
    assert np.array_equal(bits(s), bits(R.close_hull(sdf, cnt, dims, 1.3)))


def test_closing_ties_at_one_and_a_half():
    """(1.5 + 0.5)^2 = 4 is a squared voxel distance: both steps treat it alike and the closing shrinks the blocks."""
    sdf, cnt, dims, gap = R.two_blocks()
    closed = R.solid_mask(R.close_hull(sdf, cnt, dims, 1.5), cnt, 0.0)
    assert closed.sum() == 90
    for rv in (0.5, 1.5, 2.5, 0.0, -1.0, 126.0):
        with pytest.raises(ValueError):
            vc.close_hull_plan(rv, 1.0)
    for rv in (1.3, 2.3, 2.0, 125.0):
        vc.close_hull_plan(rv, 1.0)


@pytest.mark.parametrize("seed", range(5))
def test_closing_is_extensive(seed):
    dims = (12, 11, 10)
    rng = np.random.RandomState(40 + seed)
    solid = rng.rand(dims[0] * dims[1] * dims[2]) < (0.1, 0.3, 0.5, 0.7, 0.2)[seed]
    sdf, cnt = K.state_from_mask(solid)
    closed = R.solid_mask(R.close_hull(sdf, cnt, dims, 1.3), cnt, 0.0)
    assert not (solid & ~closed).any(), "the closing removed %d solid voxels" % (solid & ~closed).sum()
