"""The host half of the ray-cast over z-slabs (no GPU): vcy_render_merge_host and vcy_hull_agreement_host.  Slab images
come from the numpy restatement (tests/render_ref.py) on the solid mask restricted to a slab's slices -- the definition
of a slab image --; the yardstick is the restatement on the whole mask.  Depths are compared as uint32 bits."""
import ctypes as C

import numpy as np
import pytest

import render_ref as RR
import slab_render_cases as S
from vacancy_amd import capi
from vacancy_amd import carver as vc


def merge(view, images):
    return vc.render_merge_host(view, [{"depth": d, "voxel": v, "axis": a} for d, v, a in images])


@pytest.mark.parametrize("dims", S.DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_merge_equals_the_whole_grid(dims):
    c = S.case(dims)
    n = 0
    for cut, bounds in S.cut_sets(dims[2]).items():
        for sn in c["states"]:
            for vn, view in c["views"].items():
                images = [S.slab_image(dims, sn, vn, z0, z1) for z0, z1 in S.slabs_of(bounds)]
                S.assert_images_equal(merge(view, images), c["want"][sn, vn], "%s %s %s cut %s" % (dims, sn, vn, cut))
                n += sum(int((v >= 0).sum()) for _, v, _ in images[1:])
    assert n > 0   # (slabs above the first one do hit)


def test_ties_in_depth_go_to_the_first_slab_along_the_ray():
    dims = S.TIE_DIMS
    c = S.case(dims)
    solid = S.solid_of(dims, "all_solid")
    assert solid.all()
    for name, (view, sz) in S.tie_views().items():
        _, d, roi = RR.rays(view)
        assert np.all(np.sign(d[2][roi]) == sz)
        want = RR.render(view, c["planes"], dims, solid)
        for cut in S.TIE_CUTS:
            bounds = S.cut_sets(dims[2])[cut]
            images = [RR.render(view, c["planes"], dims, S.slab_solid(solid, dims, z0, z1)) for z0, z1 in S.slabs_of(bounds)]
            tied = S.tied_pixels(images, want[1])
            assert tied.sum() > 0, "%s, cut %s: no pixel hits two slabs at equal depth -- the case shows nothing" % (name, cut)
            got = merge(view, images)
            assert np.array_equal(got["voxel"][tied], want[1][tied]) and np.array_equal(got["axis"][tied], want[2][tied])
            assert np.all(want[2][tied] == 0)   # the x crossing sorts before the z crossing of the same t
            S.assert_images_equal(got, want, "tie %s cut %s" % (name, cut))


@pytest.mark.parametrize("width", [48, 64, 70])
def test_agreement_from_hit_bits(width):
    dims = (24, 20, 17)
    c = S.case(dims)
    solid = S.solid_of(dims, "random")
    rng = np.random.RandomState(width)
    e = float(max(dims))
    pos = np.array([1.3, 0.9, -1.7]) * e
    f = 34.0 * float(np.linalg.norm(pos)) / e
    for roi in (None, ((5, 4), (width - 9, S.H - 7))):
        view = S.look(pos, (0.0, 0.0, 0.0), f, roi=roi, w=width)
        slabs = [RR.render(view, c["planes"], dims, S.slab_solid(solid, dims, z0, z1))[1] for z0, z1 in ((0, 3), (3, 11), (11, 17))]
        hits = [S.pack_hits(v, view) for v in slabs]
        for h in hits:   # (the function reads no padding bit: set them all)
            if width % 64:
                h[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(width % 64)
        mask = (rng.rand(S.H, width) < 0.5).astype(np.uint8) * 3
        union = np.where(np.any([v >= 0 for v in slabs], axis=0), 0, -1)
        want = RR.agreement(view, union, mask)
        assert want[0] > 0 and want[1] > 0 and want[2] > 0
        assert vc.hull_agreement_host(view, hits, mask).tolist() == want
        assert vc.hull_agreement_host(view, hits[:1], mask).tolist() == RR.agreement(view, slabs[0], mask)
        whole = RR.render(view, c["planes"], dims, solid)[1]
        assert np.array_equal(whole >= 0, union >= 0)   # the OR of the slabs' silhouettes is the whole grid's


def test_argument_errors():
    lib = capi.load()
    view = S.case((9, 8, 7))["views"]["pinhole_outside"]
    px = S.W * S.H
    depth, voxel, axis = np.zeros(px, np.float32), np.full(px, -1, np.int64), np.zeros(px, np.uint8)
    dout, vout, aout = np.zeros(px, np.float32), np.zeros(px, np.int64), np.zeros(px, np.uint8)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data)  # noqa: E731
    null = (C.c_void_p * 1)(None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bad = capi.VCY_ERR_INVALID_ARG
    ok = lib.vcy_render_merge_host
    assert ok(C.byref(view), 1, one(depth), one(voxel), one(axis), p(dout), p(vout), p(aout)) == 0
    assert np.all(np.isposinf(dout)) and np.all(vout == -1) and np.all(aout == 255)
    assert ok(C.byref(view), 1, None, one(voxel), None, None, p(vout), None) == 0      # depth and axis left out as a whole
    assert ok(C.byref(view), 1, None, one(voxel), None, None, None, None) == 0
    assert ok(None, 1, one(depth), one(voxel), one(axis), p(dout), p(vout), p(aout)) == bad
    assert ok(C.byref(view), 0, one(depth), one(voxel), one(axis), p(dout), p(vout), p(aout)) == bad
    assert ok(C.byref(view), -1, one(depth), one(voxel), one(axis), p(dout), p(vout), p(aout)) == bad
    assert ok(C.byref(view), 1, one(depth), None, one(axis), p(dout), p(vout), p(aout)) == bad
    assert ok(C.byref(view), 1, one(depth), null, one(axis), p(dout), p(vout), p(aout)) == bad
    assert ok(C.byref(view), 1, null, one(voxel), one(axis), p(dout), p(vout), p(aout)) == bad
    assert ok(C.byref(view), 1, one(depth), one(voxel), null, p(dout), p(vout), p(aout)) == bad
    assert ok(C.byref(view), 1, one(depth), one(voxel), one(axis), None, p(vout), p(aout)) == bad
    assert ok(C.byref(view), 1, one(depth), one(voxel), one(axis), p(dout), p(vout), None) == bad
    hits, mask, counts = np.zeros((S.H, 1), np.uint64), np.zeros(px, np.uint8), np.zeros(3, np.int64)
    agree = lib.vcy_hull_agreement_host
    assert agree(C.byref(view), 1, one(hits), p(mask), p(counts)) == 0 and counts.tolist() == [0, 0, 0]
    assert agree(None, 1, one(hits), p(mask), p(counts)) == bad
    assert agree(C.byref(view), 0, one(hits), p(mask), p(counts)) == bad
    assert agree(C.byref(view), 1, None, p(mask), p(counts)) == bad
    assert agree(C.byref(view), 1, null, p(mask), p(counts)) == bad
    assert agree(C.byref(view), 1, one(hits), None, p(counts)) == bad
    assert agree(C.byref(view), 1, one(hits), p(mask), None) == bad
    for change in ("nan", "fx", "width", "roi"):
        v = capi.View.from_buffer_copy(view)
        if change == "nan":
            v.w2c[3] = float("nan")
        elif change == "fx":
            v.fx = 0.0
        elif change == "width":
            v.width = 0
        else:
            v.roi_max[1] = S.H
        assert ok(C.byref(v), 1, one(depth), one(voxel), one(axis), p(dout), p(vout), p(aout)) == bad, change
        assert agree(C.byref(v), 1, one(hits), p(mask), p(counts)) == bad, change
    assert "view" in vc.last_error()
