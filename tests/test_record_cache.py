"""Footprint records kept across launches ("recordcache"): a context that carves the same cameras again skips the pre-pass.

A footprint record is geometry (tile origin and size, edge bits, `sure`) and one bound; only the bound depends on the
images.  With "recordcache" 1 (the default) a context remembers which launch its record buffer describes, and a kMax
launch of the general flavour that finds its own cameras, slab and buffer there runs no pre-pass: the carve kernel's
prologue looks the bounds up itself, through the helpers the pre-pass uses (carve_fused_plan.h: fused_reuses_records;
carve_fused_kernel.h: kStateStaleBounds).  "recordcache" 0 is the path as it was, and the second implementation here:

  - the same batch three times over a reset grid, 1 / 9 / 32 / 64 views: sdf and update_num bit-identical call for call
    between "recordcache" 1 and 0 and to "cull" 0, and the SAME pairs processed ("paircount"), not merely the same result;
  - the images change between calls -- in place in the same device buffers, and as new buffers, one image with a NaN and
    a +inf inside the footprints -- while the cameras stay: still reused, still identical (also with update_outside = kMax,
    where the bound of a tile that is not `sure` takes the view's current max_sdf);
  - every field of the key, changed one at a time, makes the next launch run the pre-pass again
    (vcy_get_param "recordcache_hits" stands still exactly there) and the results equal a fresh context's;
  - the launches that must not reuse -- a listed launch of few views over a carved grid, weighted average, "tile" 2,
    chunked records, the few-view flavour, the one-view flavour -- leave the counter alone and equal "recordcache" 0;
  - carving over a carved grid without a reset (the early-return test compares the in-kernel bound with the kept brick
    minima), against "recordcache" 0 and against the per-view kernel.

Grids of 64^3 and 60^3 voxels (a ragged x edge: 7.5 bricks per row), images of 320 x 240, kMax with and without
truncation."""
import functools
import math

import numpy as np
import pytest

from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import (VCY_OUTSIDE_MAX, VCY_OUTSIDE_NONE, VCY_UPDATE_MAX, VCY_UPDATE_WEIGHTED_AVERAGE, CarverOption,
                              UpdateOption, make_view)

gpu = pytest.mark.gpu

W, H = 320, 240
GRIDS = [64, 60]
DIST = 280.0  # 0.74 pixels per voxel: every footprint fits the raw tile


def option(n, trunc=False, update=VCY_UPDATE_MAX, outside=VCY_OUTSIDE_NONE):
    h = n / 2.0
    uo = UpdateOption(voxel_update=update, update_outside=outside, use_truncation=trunc, truncation_band=0.1)
    return CarverOption(bb_min=(-h, -h, -h), bb_max=(h, h, h), resolution=1.0, update_option=uo)


def camera(i, n, dist=DIST, shift=(0.0, 0.0, 0.0)):
    """w2c of camera i of n on a Fibonacci sphere of radius `dist`, looking at the origin, moved by `shift`."""
    y = 1.0 - 2.0 * (i + 0.5) / n
    r = math.sqrt(max(0.0, 1.0 - y * y))
    phi = i * math.pi * (3.0 - math.sqrt(5.0))
    d = np.array([r * math.cos(phi), y, r * math.sin(phi)])
    return synth.affine_inverse(synth.lookat_c2w(dist * d + np.asarray(shift), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))).astype(np.float32)


F = synth.focal_from_fov_y(H, 60.0)
CX, CY = np.float32(W / 2 - 0.5), np.float32(H / 2 - 0.5)


def rig(n_views, moved=None, fy_of=None, roi_of=None):
    """n_views cameras; `moved`: that camera 3 units aside; `fy_of`: that camera with fy != fx; `roi_of`: ... with a ROI
    that cuts the grid's projection (about 136..183 x 96..143)."""
    views = []
    for i in range(n_views):
        w2c = camera(i, n_views, shift=(3.0, 0.0, 0.0) if i == moved else (0.0, 0.0, 0.0))
        fy = np.float32(F * 1.01) if i == fy_of else F
        roi = dict(roi_min=(140, 100), roi_max=(175, 150)) if i == roi_of else {}
        views.append(make_view(w2c, F, fy, CX, CY, W, H, **roi))
    return views


def images(n_views, seed, special=False):
    """A level per view plus a ripple; the levels rise and fall so that views are dropped, re-bounds move the request and
    (with truncation) whole views lie below -1.  `special`: view 2 holds a NaN and view 5 (or the last) a +inf where
    the grid projects to."""
    levels = [0.0, -1.0, 2.0, 1.0, 3.0, -2.5, 2.5, 3.5, 0.5, 4.0, 3.8, 4.5]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for i in range(n_views):
        ripple = (0.6 * np.sin(xx * 0.11 + i + seed) + 0.5 * np.cos(yy * 0.13 - 0.7 * i + 2 * seed)) / 1.1
        lv = levels[(i + 5 * seed) % len(levels)] + 0.01 * (i // len(levels))
        out.append((0.3 * ripple + lv).astype(np.float32))
    if special:
        out[min(2, n_views - 1)][H // 2 + 3, W // 2 - 4] = np.nan
        out[min(5, n_views - 1)][H // 2 - 6, W // 2 + 7] = np.inf
    return out


class Session:
    """A context with "paircount" on and the given knobs; carve() -> (sdf, update_num, (processed, total) pairs)."""

    def __init__(self, opt, params=(), z_range=None):
        self.dev = vc.VoxelCarver(opt, z_range=z_range)
        assert self.dev.Init(), vc.last_error()
        self.dev.set_param("paircount", 1)
        for k, v in params:
            self.dev.set_param(k, v)
        self.bufs = []

    def upload(self, imgs):
        ptrs = [self.dev.upload_sdf(im) for im in imgs]
        self.bufs += ptrs
        return ptrs

    def carve(self, views, ptrs, reset=True, pairs=True):
        if reset:
            self.dev.reset()
        assert self.dev.CarveBatchDevice(views, ptrs), vc.last_error()
        s, u = self.dev.download()
        return s, u, (self.dev.last_carve_pairs()[:2] if pairs else None)

    def hits(self):
        return self.dev.get_param("recordcache_hits")

    def close(self):
        for p in self.bufs:
            self.dev.free_device(p)
        self.dev.close()


def same(a, b, what):
    (sa, ua, pa), (sb, ub, pb) = a, b
    assert np.array_equal(ua, ub), "%s: update_num differs at %d voxels" % (what, int((ua != ub).sum()))
    ba, bb = sa.view(np.uint32), sb.view(np.uint32)
    assert np.array_equal(ba, bb), "%s: sdf bits differ at %d voxels" % (what, int((ba != bb).sum()))
    if pa is not None and pb is not None:
        assert pa == pb, "%s: pairs processed / total %s against %s" % (what, pa, pb)


def fresh_result(opt, views, imgs, params=(), z_range=None):
    """What a fresh context without the cache gives for one call."""
    s = Session(opt, (("recordcache", 0),) + tuple(params), z_range)
    out = s.carve(views, s.upload(imgs))
    s.close()
    return out


# ---- 1. reuse is exact ------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("trunc", [False, True], ids=["kmax", "kmax_trunc"])
@pytest.mark.parametrize("n_views", [1, 9, 32, 64])
@pytest.mark.parametrize("n", GRIDS)
def test_reuse_is_exact(n, n_views, trunc):
    assert n_views <= 64  # (one fused launch holds up to 64 views: fused_max_views)
    opt, views, imgs = option(n, trunc), rig(n_views), images(n_views, 0)
    runs = {}
    for rc in (1, 0):
        s = Session(opt, (("recordcache", rc),))
        ptrs = s.upload(imgs)
        runs[rc] = [s.carve(views, ptrs) for _ in range(3)]
        # a launch of one view takes the one-view flavour, which does not reuse; the others hit on calls two and three
        assert s.hits() == (2 if rc == 1 and n_views > 1 else 0), (rc, n_views, s.hits())
        s.close()
    for call in range(3):
        same(runs[1][call], runs[0][call], "%d^3, %d views, call %d, recordcache 1 / 0" % (n, n_views, call))
    s = Session(opt, (("cull", 0),))
    ref = s.carve(views, s.upload(imgs))
    s.close()
    for call in range(3):
        same(runs[1][call][:2] + (None,), ref, "%d^3, %d views, call %d against cull 0" % (n, n_views, call))
    p1, t1 = runs[1][2][2]
    assert int((ref[1] > 0).sum()) > 0 and 0 < p1 <= t1 == ref[2][1]
    if n_views >= 9:
        assert p1 < ref[2][0], "no pair was dropped: the bounds were never compared"


# ---- 2. images change, cameras do not ---------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mode", ["kmax", "kmax_trunc", "kmax_outside_max"])
@pytest.mark.parametrize("n", GRIDS)
def test_images_change_cameras_do_not(n, mode):
    opt = option(n, trunc=mode == "kmax_trunc", outside=VCY_OUTSIDE_MAX if mode == "kmax_outside_max" else VCY_OUTSIDE_NONE)
    # (view 4 with a ROI that cuts the grid's projection: tiles that are not `sure`, whose bound takes max_sdf)
    views = rig(12, roi_of=4)
    a, b, c = images(12, 0), images(12, 1), images(12, 2, special=True)
    runs = {}
    for rc in (1, 0):
        s = Session(opt, (("recordcache", rc),))
        ptrs = s.upload(a)
        out = [s.carve(views, ptrs)]
        for p, im in zip(ptrs, b):  # new contents in the same device buffers
            s.dev.memcpy_h2d(p, im)
        out.append(s.carve(views, ptrs))
        out.append(s.carve(views, s.upload(c)))  # new buffers; a NaN and a +inf inside the footprints
        assert s.hits() == (2 if rc == 1 else 0)
        runs[rc] = out
        s.close()
    for call in range(3):
        same(runs[1][call], runs[0][call], "%d^3 %s call %d" % (n, mode, call))
    assert not np.array_equal(runs[0][0][0].view(np.uint32), runs[0][1][0].view(np.uint32)), "the images did not matter"
    same(runs[1][2], fresh_result(opt, views, c), "%d^3 %s: the last call against a fresh context" % (n, mode))


# ---- 3. every key field invalidates -----------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("trunc", [False, True], ids=["kmax", "kmax_trunc"])
@pytest.mark.parametrize("n", GRIDS)
def test_every_key_field_invalidates(n, trunc):
    opt = option(n, trunc)
    nv = 12
    imgs = images(nv, 0)
    base = rig(nv)
    s = Session(opt)
    ptrs = s.upload(imgs)

    def step(what, views, p, im, want_hit, params=()):
        """One carve over a reset grid: the counter moves exactly when `want_hit`, the result is a fresh context's."""
        before = s.hits()
        out = s.carve(views, p)
        assert s.hits() - before == (1 if want_hit else 0), "%s: recordcache_hits %d -> %d" % (what, before, s.hits())
        same(out, fresh_result(opt, views, im, params), "%d^3 %s" % (n, what))

    step("first call", base, ptrs, imgs, False)
    step("same cameras", base, ptrs, imgs, True)
    for what, views in (("one camera's translation", rig(nv, moved=3)), ("one focal length (fx != fy)", rig(nv, fy_of=7)),
                        ("a ROI", rig(nv, roi_of=5))):
        step(what, views, ptrs, imgs, False)
        step(what + ", again", views, ptrs, imgs, True)
    # the view count (other cameras as well: a rig of nine)
    nine = rig(9)
    step("the view count", nine, ptrs[:9], imgs[:9], False)
    step("the view count, again", nine, ptrs[:9], imgs[:9], True)
    # "cull" 0 makes records without bounds for a launch that may not reuse: nothing is remembered
    s.dev.set_param("cull", 0)
    step("cull 0", nine, ptrs[:9], imgs[:9], False, (("cull", 0),))
    s.dev.set_param("cull", 1)
    step("cull 1 after cull 0", nine, ptrs[:9], imgs[:9], False)
    step("cull 1, again", nine, ptrs[:9], imgs[:9], True)
    # "prologue" 1 makes its footprints in the kernel and does not touch the record buffer: it neither reuses nor
    # invalidates -- the next launch with records finds the rig of nine still there
    s.dev.set_param("prologue", 1)
    step("prologue 1", nine, ptrs[:9], imgs[:9], False, (("prologue", 1),))
    s.dev.set_param("prologue", 0)
    step("prologue 0 after prologue 1", nine, ptrs[:9], imgs[:9], True)
    # a batch of other views in between
    step("another batch", base, ptrs, imgs, False)
    step("the first batch again", nine, ptrs[:9], imgs[:9], False)
    step("the first batch, once more", nine, ptrs[:9], imgs[:9], True)
    s.close()
    # the z-range: a second context over a slab of the grid (whole brick layers and a ragged one)
    for zr in ((16, 48), (8, n - 3)):
        z = Session(opt, z_range=zr)
        zp = z.upload(imgs)
        for call, want in enumerate((0, 1, 2)):
            out = z.carve(base, zp)
            assert z.hits() == want
            same(out, fresh_result(opt, base, imgs, z_range=zr), "%d^3 slab %s call %d" % (n, zr, call))
        z.close()


# ---- 4. launches that must not reuse ----------------------------------------------------------------------------------

MUST_NOT = {
    # name: (update, knobs, views per launch)
    "weighted_average": (VCY_UPDATE_WEIGHTED_AVERAGE, (), 9),
    "tile2": (VCY_UPDATE_MAX, (("tile", 2),), 9),
    "recordbytes": (VCY_UPDATE_MAX, (("recordbytes", 4000),), 9),
    "rowkernel": (VCY_UPDATE_MAX, (("rowkernel", -1),), 6),
    "oneview": (VCY_UPDATE_MAX, (), 1),
}


@gpu
@pytest.mark.parametrize("trunc", [False, True], ids=["plain", "trunc"])
@pytest.mark.parametrize("case", list(MUST_NOT))
@pytest.mark.parametrize("n", GRIDS)
def test_launches_that_must_not_reuse(n, case, trunc):
    update, knobs, nv = MUST_NOT[case]
    opt, views, imgs = option(n, trunc, update), rig(nv), images(nv, 0)
    runs = {}
    for rc in (1, 0):
        s = Session(opt, (("recordcache", rc),) + knobs)
        ptrs = s.upload(imgs)
        runs[rc] = [s.carve(views, ptrs) for _ in range(3)]
        # (the few-view flavour needs rows of whole bricks: at 60^3 "rowkernel" -1 selects the general flavour after all,
        # and that launch is one that reuses -- plan_fused_launch, tests/fused_plan_host_check.cpp "rowkernel -1, nx 60")
        takes_flavour = case != "rowkernel" or n % 8 == 0
        assert s.hits() == (0 if takes_flavour or rc == 0 else 2), (case, rc, s.hits())
        s.close()
    for call in range(3):
        same(runs[1][call], runs[0][call], "%d^3 %s call %d" % (n, case, call))


@gpu
@pytest.mark.parametrize("trunc", [False, True], ids=["kmax", "kmax_trunc"])
@pytest.mark.parametrize("n", GRIDS)
def test_a_listed_launch_does_not_reuse(n, trunc):
    """Four views over a carved grid build the live list, which reads the bounds from the records: the pre-pass runs."""
    opt, views, imgs = option(n, trunc), rig(12), images(12, 0)
    few, few_imgs = rig(4), images(4, 1)
    runs = {}
    for rc in (1, 0):
        s = Session(opt, (("recordcache", rc),))
        ptrs, fptrs = s.upload(imgs), s.upload(few_imgs)
        out = [s.carve(views, ptrs)]
        h0 = s.hits()
        out += [s.carve(few, fptrs, reset=False) for _ in range(3)]  # (the second and third would find their own key)
        assert s.hits() == h0 == 0, (rc, h0, s.hits())
        runs[rc] = out
        s.close()
    for call in range(4):
        same(runs[1][call], runs[0][call], "%d^3 listed, call %d" % (n, call))


# ---- 5. carve over a carved grid --------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("trunc", [False, True], ids=["kmax", "kmax_trunc"])
@pytest.mark.parametrize("n", GRIDS)
def test_carve_over_a_carved_grid(n, trunc):
    opt, views = option(n, trunc), rig(12)
    sets = [images(12, 0), images(12, 1), images(12, 2, special=True), images(12, 1)]
    runs = {}
    for name, params in (("cache", (("recordcache", 1),)), ("nocache", (("recordcache", 0),)), ("perview", (("fused", 0),))):
        s = Session(opt, params)
        ptrs = [s.upload(im) for im in sets]
        s.dev.reset()
        runs[name] = [s.carve(views, p, reset=False, pairs=name != "perview") for p in ptrs]
        assert s.hits() == (3 if name == "cache" else 0), (name, s.hits())
        s.close()
    for call in range(len(sets)):
        same(runs["cache"][call], runs["nocache"][call], "%d^3 carved grid, call %d, recordcache 1 / 0" % (n, call))
        same(runs["cache"][call], runs["perview"][call], "%d^3 carved grid, call %d, against the per-view kernel" % (n, call))
    # (not vacuous: over the carved grid the early-return test and the bounds drop pairs, and the last call -- images the
    # grid has seen -- changes nothing)
    (p1, t1), (p3, t3) = runs["cache"][1][2], runs["cache"][3][2]
    assert 0 < p1 < t1 and p3 < t3
    assert np.array_equal(runs["cache"][3][0].view(np.uint32), runs["cache"][2][0].view(np.uint32))
