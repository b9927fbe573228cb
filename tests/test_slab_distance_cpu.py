"""The distance field of the hull across z-slabs without a GPU: the two host halves of the library
(vcy_distance_slab_planes_host, vcy_distance_slab_finish_host) with the seam assembly of vacancy_amd.dist.distance_halos
between them, against the WHOLE grid's reference (distance_cases.reference_of) bit for bit -- the int32 field and the sdf
after the rewrite --, on every case of tests/slab_distance_cases.py under every cut of z; the numpy restatement of the slab
flow against the same reference; distance_halos alone; the refusals."""
import numpy as np
import pytest

import distance_cases as K
import slab_distance_cases as S
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host_flow(case, bounds, resolution=1.0):
    """planes_host per slab, distance_halos, finish_host per slab: (field, sdf, the slabs' planes)"""
    name, dims, sdf, cnt, iso, radius = case
    opt = K.box_option(dims, resolution=resolution)
    zr = list(zip(bounds[:-1], bounds[1:]))
    planes = [vc.distance_slab_planes_host(opt, z, S.slab_of(sdf, dims, *z), S.slab_of(cnt, dims, *z), iso, radius) for z in zr]
    bottoms, tops = S.edge_planes(zr, radius, planes)
    bottoms[0], tops[-1] = None, None  # nobody needs them
    halos = vdist.distance_halos(zr, radius, bottoms, tops)
    parts = [vc.distance_slab_finish_host(opt, z, planes[i], halos[i][0], halos[i][1], radius, S.slab_of(sdf, dims, *z),
                                          S.slab_of(cnt, dims, *z)) for i, z in enumerate(zr)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), planes


def check_flow(case, bounds, resolution=1.0):
    ctx = "%s %s cut %s" % (case[0], case[1], bounds)
    want_d2, want_sdf = K.reference_of(case, resolution)
    d2, out, planes = host_flow(case, bounds, resolution)
    assert np.array_equal(d2, want_d2), "%s: %d field values differ" % (ctx, (d2 != want_d2).sum())
    assert np.array_equal(bits(out), bits(want_sdf)), ctx + ": sdf bits differ"
    return planes


NAMED = K.named_cases()


@pytest.mark.parametrize("k", range(len(NAMED)), ids=[c[0].replace(" ", "_") for c in NAMED])
def test_host_halves_equal_the_whole_grid_named(k):
    case = NAMED[k]
    for bounds in S.cuts_of(case[1][2]):
        check_flow(case, bounds)


@pytest.mark.parametrize("dims", S.SLAB_RANDOM_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_host_halves_equal_the_whole_grid_random(dims):
    cuts = S.cuts_of(dims[2])
    assert any(z1 - z0 == 2 for b in cuts for z0, z1 in zip(b[:-1], b[1:]))
    assert any(2 in b for b in cuts) and any(dims[2] - 2 in b for b in cuts)
    seen_far_seam = False
    for case in K.random_cases(dims):
        for bounds in cuts:
            check_flow(case, bounds)
        if "one voxel" in case[0]:  # 127^2 reaches index 128 from index 1: across every seam of every cut
            seen_far_seam = (K.reference_of(case)[0] == 127 * 127).any()
    assert seen_far_seam == (dims in K.LONG_DIMS)


def test_resolution_that_rounds():
    check_flow(NAMED[2], [0, 2, 7, 9], resolution=0.375)


def test_a_halo_spans_three_slabs():
    """(9, 10, 17) at R = 12 under [0, 6, 8, 10, 17]: the slab [8, 10) needs 8 planes below -- [6, 8) and [0, 6) -- and 7
    above, and hands none of its own to itself; dropping the farther neighbour must be noticed."""
    case = [c for c in K.random_cases((9, 10, 17)) if c[5] == 12][0]
    bounds = [0, 6, 8, 10, 17]
    assert bounds in S.cuts_of(17)
    planes = check_flow(case, bounds)
    zr = list(zip(bounds[:-1], bounds[1:]))
    bottoms, tops = S.edge_planes(zr, 12, planes)
    halos = vdist.distance_halos(zr, 12, bottoms, tops)
    assert [None if b is None else len(b) for b, _ in halos] == [None, 6, 8, 10]
    assert [None if a is None else len(a) for _, a in halos] == [11, 9, 7, None]
    whole = np.concatenate(planes)
    assert np.array_equal(halos[2][0], whole[0:8]) and np.array_equal(halos[2][1], whole[10:17])
    # the near neighbour alone is not enough: the field of the slab [8, 10) changes
    name, dims, sdf, cnt, iso, radius = case
    opt = K.box_option(dims)
    with pytest.raises(RuntimeError) as e:
        vc.distance_slab_finish_host(opt, (8, 10), planes[2], halos[2][0][6:], halos[2][1], radius, S.slab_of(sdf, dims, 8, 10),
                                     S.slab_of(cnt, dims, 8, 10))
    assert e.value.rc == capi.VCY_ERR_INVALID_ARG and "planes" in str(e.value)


@pytest.mark.parametrize("radius", (1, 3, 12, 127))
def test_distance_halos_against_slicing_the_whole_grid(radius):
    nz, sl = 23, 6
    rng = np.random.RandomState(radius)
    whole = rng.randint(0, 65536, (nz, sl)).astype(np.uint16)
    for bounds in S.cuts_of(nz) + [[0, 2, 4, 6, 8, 10, 23], [0, 21, 23], list(range(0, 23, 2)) + [23]]:
        zr = list(zip(bounds[:-1], bounds[1:]))
        planes = [whole[z0:z1] for z0, z1 in zr]
        bottoms, tops = S.edge_planes(zr, radius, planes)
        bottoms[0], tops[-1] = None, None
        got = vdist.distance_halos(zr, radius, bottoms, tops)
        want = S.halos_np(zr, radius, planes)
        for (z0, z1), (gb, ga), (wb, wa) in zip(zr, got, want):
            assert (gb is None) == (wb is None) and (ga is None) == (wa is None), (bounds, z0, z1)
            assert gb is None or np.array_equal(gb, wb), (bounds, z0, z1)
            assert ga is None or np.array_equal(ga, wa), (bounds, z0, z1)
            assert (0 if gb is None else len(gb)) == min(radius, z0) and (0 if ga is None else len(ga)) == min(radius, nz - z1)


def test_numpy_restatement_of_the_slab_flow():
    for case in NAMED + list(K.random_cases((9, 10, 17))):
        want_d2, want_sdf = K.reference_of(case)
        for bounds in S.cuts_of(case[1][2]):
            d2, out = S.slab_flow_np(case, bounds)
            assert np.array_equal(d2, want_d2) and np.array_equal(bits(out), bits(want_sdf)), (case[0], bounds)


def test_host_planes_equal_the_restatement():
    for case in NAMED + list(K.random_cases((70, 23, 19))):
        name, dims, sdf, cnt, iso, radius = case
        opt = K.box_option(dims)
        for z in ((0, dims[2]), (2, dims[2] - 2)):
            got = vc.distance_slab_planes_host(opt, z, S.slab_of(sdf, dims, *z), S.slab_of(cnt, dims, *z), iso, radius)
            want = S.planes_np(S.slab_of(sdf, dims, *z), S.slab_of(cnt, dims, *z), (dims[0], dims[1], z[1] - z[0]), iso, radius)
            assert np.array_equal(got, want), (name, z)


def test_refusals():
    name, dims, sdf, cnt, iso, _ = NAMED[2]  # (20, 9, 9)
    opt = K.box_option(dims)
    z = (2, 7)
    s, c = S.slab_of(sdf, dims, *z), S.slab_of(cnt, dims, *z)
    h = vc.distance_slab_planes_host(opt, z, s, c, iso, 3)
    sl = dims[0] * dims[1]
    two, three = np.zeros((2, sl), np.uint16), np.zeros((3, sl), np.uint16)
    vc.distance_slab_finish_host(opt, z, h, two, two, 3, s, c)  # min(3, 2) below, min(3, 9 - 7) above
    for below, above in ((three, two), (two, three), (None, two), (two, None), (two[:1], two)):
        with pytest.raises(RuntimeError) as e:
            vc.distance_slab_finish_host(opt, z, h, below, above, 3, s, c)
        assert e.value.rc == capi.VCY_ERR_INVALID_ARG and "planes" in str(e.value)
    for radius in (0, 128, -3):
        with pytest.raises(RuntimeError) as e:
            vc.distance_slab_planes_host(opt, z, s, c, iso, radius)
        assert e.value.rc == capi.VCY_ERR_INVALID_ARG and "radius" in str(e.value)
        with pytest.raises(RuntimeError) as e:
            vc.distance_slab_finish_host(opt, z, h, two, two, radius, s, c)
        assert e.value.rc == capi.VCY_ERR_INVALID_ARG and "radius" in str(e.value)
    for bad in ((7, 2), (-1, 4), (5, 10)):
        with pytest.raises((RuntimeError, ValueError)):
            vc.distance_slab_planes_host(opt, bad, s, c, iso, 3)
    with pytest.raises(ValueError):
        vc.distance_slab_planes_host(opt, z, s[:-1], c[:-1], iso, 3)
