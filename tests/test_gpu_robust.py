"""The robust carve on the device (vcy_carve_robust_device / _silhouettes, carve_robust.hip) against the numpy restatement of
its definition (tests/robust_ref.py): sdf bits, update_num and overruled are compared for equality, for m = 0 .. 3.  Then
what does not go through the restatement: m = 0 against the ordinary carve, z-slabs against the whole grid, the state's
bookkeeping against a context that got the same state through upload, the refusals, a property of a scene with one blank
mask, and the example.  (A NaN only has to be a NaN: robust_ref.assert_sdf_equal says why.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import oracle_lib as O
import robust_cases as RC
import robust_ref as R
import test_gpu_render as TR
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import CarverOption, UpdateOption
from vacancy_amd.sharded import ShardedVoxelCarver

pytestmark = pytest.mark.gpu

F = np.float32
LOWEST = np.finfo(np.float32).min
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")
ISO = [0.0, 0.25, -0.25, 0.0]  # per m; +-0.25 is a plateau value of the tie images: exact equality with the iso level

_cache = {}


def case(dims, mode, set_name, n_views):
    """Option, views, images and the restatement's samples: computed once."""
    key = (tuple(dims), mode, set_name, n_views)
    if key not in _cache:
        opt = RC.option_for(dims, mode)
        views, sdfs = RC.scene(dims, set_name, n_views)
        has, val = R.samples(opt, views, sdfs)
        _cache[key] = dict(opt=opt, views=views, sdfs=sdfs, has=has, val=val)
    return _cache[key]


def make_dev(opt, dims=None, z_range=None):
    dev = vc.VoxelCarver(opt, z_range=z_range)
    assert dev.Init(), vc.last_error()
    if dims is not None:
        assert dev.dims == tuple(dims), (dev.dims, dims)
    return dev


def assert_equals(dev, got, want, ctx):
    sdf, cnt, over = want
    ds, du = dev.download()
    assert np.array_equal(du, cnt), "%s: %d update_num differ" % (ctx, int((du != cnt).sum()))
    R.assert_sdf_equal(ds, sdf, ctx)
    assert got["overruled"].dtype == np.int64 and np.array_equal(got["overruled"], over), (ctx, got["overruled"], over)
    assert ((du == 0) <= (ds == F(LOWEST))).all(), ctx  # update_num == 0 implies sdf == lowest()


# ---- 1. equality with the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(RC.MODES))
@pytest.mark.parametrize("dims", RC.DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_equals_restatement(dims, mode):
    blamed = 0
    for set_name, nv in RC.CALLS:
        c = case(dims, mode, set_name, nv)
        dev = make_dev(c["opt"], dims)
        ptrs = [dev.upload_sdf(s) for s in c["sdfs"]]
        for m in range(4):
            got = dev.CarveRobustDevice(c["views"], ptrs, m, ISO[m])
            want = R.robust_from_samples(c["has"], c["val"], m, ISO[m])
            assert_equals(dev, got, want, (dims, mode, set_name, nv, m))
            assert got["device_ms"] > 0.0
            blamed += int(want[2].sum())
            if nv <= m:  # n <= m: the smallest sample is kept, such a voxel is never carved by a sample below the iso level
                assert want[1].max(initial=0) <= m and (nv > 1 or not want[2].any())
        for p in ptrs:
            dev.free_device(p)
    assert blamed > 0 or dims == (1, 1, 1), "no case of this grid exercises the blame"


# ---- 2. m = 0 is the ordinary carve ----------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("mode,set_name,nv", [("default", "pinhole", 5), ("default", "ortho", 5), ("trunc", "mixed", 70),
                                              ("nn_outside_trunc", "pinhole", 5)])
def test_m0_equals_the_ordinary_carve(mode, set_name, nv, fused):
    dims = (65, 9, 17)
    opt = RC.option_for(dims, mode)
    views, sdfs = RC.scene(dims, set_name, nv)
    dev, other = make_dev(opt, dims), make_dev(opt, dims)
    other.set_param("fused", fused)
    p1, p2 = [dev.upload_sdf(s) for s in sdfs], [other.upload_sdf(s) for s in sdfs]
    got = dev.CarveRobustDevice(views, p1, 0)
    assert other.CarveBatchDevice(views, p2), vc.last_error()
    ds, du = dev.download()
    os_, ou = other.download()
    R.assert_sdf_equal(ds, os_, (mode, set_name, fused))
    assert np.array_equal(du > 0, ou > 0) and (du >= ou).all()  # (samples against changes of the value)
    assert not got["overruled"].any()


# ---- 3. z-slabs --------------------------------------------------------------------------------------------------------

def discs(n, seed=5):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:RC.H, 0:RC.W]
    out = []
    for i in range(n):
        cx, cy, r = RC.W * (0.3 + 0.4 * rng.rand()), RC.H * (0.3 + 0.4 * rng.rand()), 6 + 10 * rng.rand()
        out.append(np.where(np.hypot(xx - cx, yy - cy) <= r, 255, 0).astype(np.uint8))
    out[n // 2][:] = 0  # one blank frame
    return out


@pytest.mark.parametrize("mode", ["default", "nn_outside_trunc"])
def test_z_slabs_give_the_whole_grid(mode):
    dims, m, iso = (24, 20, 17), 3, 0.0
    c = case(dims, mode, "mixed", 70)
    nxy = dims[0] * dims[1]
    whole = make_dev(c["opt"], dims)
    ptrs = [whole.upload_sdf(s) for s in c["sdfs"]]
    got = whole.CarveRobustDevice(c["views"], ptrs, m, iso)
    ws, wu = whole.download()
    total = np.zeros(70, np.int64)
    for z0, z1 in ((0, 5), (5, 11), (11, 17)):
        slab = make_dev(c["opt"], dims, z_range=(z0, z1))
        part = slab.CarveRobustDevice(c["views"], ptrs, m, iso)  # (same device: the whole grid's images)
        ss, su = slab.download()
        assert np.array_equal(su, wu[z0 * nxy:z1 * nxy]), (z0, z1)
        R.assert_sdf_equal(ss, ws[z0 * nxy:z1 * nxy], (z0, z1))
        cols = slice(z0 * nxy, z1 * nxy)
        assert np.array_equal(part["overruled"], R.robust_from_samples(c["has"][:, cols], c["val"][:, cols], m, iso)[2])
        total += part["overruled"]
    assert np.array_equal(total, got["overruled"])
    # (with update_outside = kMax nearly every voxel has three samples of max_sdf: nothing is solid, nobody is blamed)
    assert total.sum() > 0 or mode != "default"
    for p in ptrs:
        whole.free_device(p)


def test_sharded_silhouettes_equal_the_single_context_and_the_restatement():
    dims, m = (24, 20, 17), 1
    opt = RC.option_for(dims, "trunc")
    views = RC.scene(dims, "mixed", 9)[0]
    masks = discs(9)
    single = make_dev(opt, dims)
    got = single.CarveRobustSilhouettes(views, masks, m)
    u = opt.update_option
    sdfs = [O.make_sdf(mk, tuple(v.roi_min), tuple(v.roi_max), bool(opt.sdf_minmax_normalize), bool(u.use_truncation),
                       u.truncation_band) for v, mk in zip(views, masks)]
    assert_equals(single, got, R.robust(opt, views, sdfs, m), "silhouettes")
    sh = ShardedVoxelCarver(opt, [0], slabs_per_device=3)
    assert sh.Init(), vc.last_error()
    part = sh.CarveRobustSilhouettes(views, masks, m)
    assert np.array_equal(part["overruled"], got["overruled"]) and part["overruled"].sum() > 0
    ss, su = single.download()
    ps = [c.download() for c in sh.slabs]
    assert np.array_equal(np.concatenate([p[1] for p in ps]), su)
    assert np.array_equal(np.concatenate([p[0] for p in ps]).view(np.uint32), ss.view(np.uint32))
    sh.close()


# ---- 4. counter widths -------------------------------------------------------------------------------------------------

def ring_views(n, e, w, h):
    out = []
    for i in range(n):
        a = 2.0 * np.pi * i / n
        pos = np.array([np.cos(a) * 1.9, 0.35 * np.sin(3.0 * a), np.sin(a) * 1.9]) * e
        out.append(TR.look(pos, (0.0, 0.0, 0.0), 0.25 * w * float(np.linalg.norm(pos)) / e, w=w, h=h))
    return out


def test_300_views_need_two_byte_counters():
    dims, w, h = (24, 20, 17), 16, 12
    opt = RC.option_for(dims)
    views = ring_views(300, 24.0, w, h)
    sdfs = [RC.sdf_image(2 if i % 3 else 0, i, w, h) for i in range(300)]
    has, val = R.samples(opt, views, sdfs)
    dev = make_dev(opt, dims)
    ptrs = [dev.upload_sdf(s) for s in sdfs]
    for m in (0, 3):
        want = R.robust_from_samples(has, val, m, 0.0)
        assert want[1].max() > 255  # the premise: counts that one byte cannot hold
        got = dev.CarveRobustDevice(views, ptrs, m, 0.0)
        assert dev.get_param("count_bytes") == 2
        assert_equals(dev, got, want, ("u16", m))
    # ... and back to one byte with a call of few views, as a reset followed by a carve would
    got = dev.CarveRobustDevice(views[:5], ptrs[:5], 1, 0.0)
    assert dev.get_param("count_bytes") == 1
    assert_equals(dev, got, R.robust_from_samples(has[:5], val[:5], 1, 0.0), "u8 again")
    for p in ptrs:
        dev.free_device(p)


def test_four_byte_counters():
    dims = (65, 9, 17)
    c = case(dims, "default", "pinhole", 5)
    opt = RC.option_for(dims)
    opt.update_option.voxel_max_update_num = 70000
    dev = make_dev(opt, dims)
    dev.set_param("lazycount", 0)
    assert dev.get_param("count_bytes") == 4
    ptrs = [dev.upload_sdf(s) for s in c["sdfs"]]
    got = dev.CarveRobustDevice(c["views"], ptrs, 2, 0.0)
    assert dev.get_param("count_bytes") == 4
    assert_equals(dev, got, R.robust_from_samples(c["has"], c["val"], 2, 0.0), "u32")  # (the cap is not applied: same samples)
    for p in ptrs:
        dev.free_device(p)


# ---- 5. the state's bookkeeping ----------------------------------------------------------------------------------------

def test_later_calls_see_the_state_as_after_an_upload():
    dims, m = (24, 20, 17), 1
    c = case(dims, "default", "ortho", 5)  # (a hull of a few thousand voxels inside a touched grid)
    a, b = make_dev(c["opt"], dims), make_dev(c["opt"], dims)
    ptrs = [a.upload_sdf(s) for s in c["sdfs"]]
    # a context that is not fresh, with a view still queued: the call replaces all of it
    assert a.CarveBatchDevice(c["views"][:3], ptrs[:3]), vc.last_error()
    assert a.ExtractIsoSurface(0.0)["faces"].shape[1] == 3
    a.LabelComponents(0.0)
    assert a.Carve(c["views"][0], c["sdfs"][0]), vc.last_error()
    got = a.CarveRobustDevice(c["views"], ptrs, m, 0.0)
    want = R.robust_from_samples(c["has"], c["val"], m, 0.0)
    assert_equals(a, got, want, "replaced")
    assert 1000 < int(((want[1] > 0) & (want[0] < 0)).sum()) < int((want[1] > 0).sum())
    fresh = make_dev(c["opt"], dims)
    fresh.CarveRobustDevice(c["views"], ptrs, m, 0.0)
    assert a.state_diff(fresh) == 0
    b.upload(*a.download())
    ma, mb = a.ExtractIsoSurface(0.0), b.ExtractIsoSurface(0.0)
    assert len(ma["faces"]) > 0 and np.array_equal(ma["faces"], mb["faces"]) and np.array_equal(ma["keys"], mb["keys"])
    assert np.array_equal(ma["vertices"].view(np.uint32), mb["vertices"].view(np.uint32))
    table = TR.views_for(dims)
    rv = [table["pinhole_outside"], table["ortho_oblique"]]
    for x, y in zip(a.RenderHull(rv, 0.0, voxel_ids=True), b.RenderHull(rv, 0.0, voxel_ids=True)):
        assert np.array_equal(x["depth"].view(np.uint32), y["depth"].view(np.uint32)) and np.array_equal(x["voxel"], y["voxel"])
        assert np.isfinite(x["depth"]).any()
    la, lb = a.LabelComponents(0.0, labels=True), b.LabelComponents(0.0, labels=True)
    for k in ("label", "n_voxels", "bb_min", "bb_max", "labels"):
        assert np.array_equal(la[k], lb[k]), k
    assert len(la["label"]) > 0
    # a following ordinary carve, fused and per view
    for fused in (1, 0):
        a.set_param("fused", fused)
        b.set_param("fused", fused)
        pb = [b.upload_sdf(s) for s in c["sdfs"][:3]]
        assert a.CarveBatchDevice(c["views"][:3], ptrs[:3]) and b.CarveBatchDevice(c["views"][:3], pb), vc.last_error()
        (sa, ua), (sb, ub) = a.download(), b.download()
        assert np.array_equal(ua, ub) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), fused
    for p in ptrs:
        a.free_device(p)


def test_a_failure_of_queued_views_is_reported():
    dims = (24, 20, 17)
    c = case(dims, "default", "pinhole", 5)
    dev = make_dev(c["opt"], dims)
    ptrs = [dev.upload_sdf(s) for s in c["sdfs"]]
    assert dev.Carve(c["views"][0], c["sdfs"][0]), vc.last_error()  # queued
    dev.set_param("inject_carve_failure", 1)
    with pytest.raises(RuntimeError, match="injected") as e:
        dev.CarveRobustDevice(c["views"], ptrs, 1, 0.0)
    assert e.value.rc == capi.VCY_ERR_INTERNAL
    got = dev.CarveRobustDevice(c["views"], ptrs, 1, 0.0)  # ... once
    assert_equals(dev, got, R.robust_from_samples(c["has"], c["val"], 1, 0.0), "after the failure")
    for p in ptrs:
        dev.free_device(p)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

def raw_call(dev, entry, views, pointers, tolerate, iso, over):
    n = len(views)
    arr = (capi.View * max(n, 1))(*views)
    ptrs = (C.c_void_p * max(n, 1))(*pointers)
    return getattr(dev._lib, entry)(dev.ctx, n, arr, ptrs, tolerate, iso, over.ctypes.data_as(C.c_void_p))


def test_refusals_leave_state_and_outputs_untouched():
    dims = (24, 20, 17)
    c = case(dims, "default", "pinhole", 5)
    views, sdfs = c["views"], c["sdfs"]
    dev = make_dev(c["opt"], dims)
    ptrs = [dev.upload_sdf(s).value for s in sdfs]
    masks = [np.zeros((RC.H, RC.W), np.uint8) for _ in views]
    mptr = [mk.ctypes.data for mk in masks]
    assert dev.CarveBatchDevice(views[:2], ptrs[:2]), vc.last_error()
    before = dev.download()
    bad_roi = capi.View.from_buffer_copy(views[1])
    bad_roi.roi_max[0] = RC.W
    narrow = CarverOption(bb_min=list(c["opt"].bb_min), bb_max=list(c["opt"].bb_max), resolution=1.0,
                          update_option=UpdateOption(voxel_max_update_num=10))
    average = CarverOption(bb_min=list(c["opt"].bb_min), bb_max=list(c["opt"].bb_max), resolution=1.0,
                           update_option=UpdateOption(voxel_update=1))
    dn, da = make_dev(narrow, dims), make_dev(average, dims)
    for entry, pp in (("vcy_carve_robust_device", ptrs), ("vcy_carve_robust_silhouettes", mptr)):
        cases = [
            ("tolerate -1", dev, views, pp, -1, "tolerate"),
            ("tolerate 4", dev, views, pp, 4, "tolerate"),
            ("no views", dev, [], [], 1, "views"),
            ("1025 views", dev, [views[0]] * 1025, [pp[0]] * 1025, 1, "views"),
            ("weighted average", da, views, pp, 1, "kMax"),
            ("null image", dev, views, pp[:2] + [None] + pp[3:], 1, "null"),
            ("ROI outside the image", dev, [views[0], bad_roi] + views[2:], pp, 1, "ROI"),
            ("300 views on one-byte counters", dn, [views[0]] * 300, [pp[0]] * 300, 1, "counters"),
        ]
        for name, ctx, vs, ps, tol, text in cases:
            over = np.full(1100, -7, np.int64)
            assert raw_call(ctx, entry, vs, ps, tol, 0.0, over) == capi.VCY_ERR_INVALID_ARG, (entry, name)
            assert text in vc.last_error(), (entry, name, vc.last_error())
            assert (over == -7).all(), (entry, name)
    after = dev.download()
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32))
    for other in (dn, da):
        s, u = other.download()
        assert not u.any() and (s == F(LOWEST)).all()
    # without a place for the counts the state is the same
    over = np.full(5, -7, np.int64)
    assert raw_call(dev, "vcy_carve_robust_device", views, ptrs, 2, 0.0, over) == 0, vc.last_error()
    want = R.robust_from_samples(c["has"], c["val"], 2, 0.0)
    assert np.array_equal(over, want[2])
    arr = (capi.View * 5)(*views)
    assert dev._lib.vcy_carve_robust_device(dev.ctx, 5, arr, (C.c_void_p * 5)(*ptrs), 2, 0.0, None) == 0, vc.last_error()
    assert_equals(dev, {"overruled": want[2]}, want, "no overruled array")
    for p in ptrs:
        dev.free_device(p)


# ---- 7. a property that does not share the restatement's arithmetic ---------------------------------------------------

def test_one_blank_mask_no_longer_removes_the_object():
    n, nv, bad = 32, 8, 3
    opt = synth.sphere_option(n)  # (no truncation)
    views, masks = synth.sphere_views(n, nv, RC.W, RC.H)
    corrupted = list(masks)
    corrupted[bad] = np.zeros_like(masks[bad])
    # the premise and the claims on the restatement first: every voxel lies in every image
    sdfs = [O.make_sdf(mk) for mk in corrupted]
    has, val = R.samples(opt, views, sdfs)
    assert has.all()
    ref = R.robust_from_samples(has, val, 1, 0.0)
    assert ref[2][bad] == int((ref[0] < 0).sum()) > 0 and ref[2].sum() == ref[2][bad]

    clean = make_dev(opt)
    assert clean.CarveBatchSilhouettes(views, masks), vc.last_error()
    cs, cu = clean.download()
    clean_solid = (cu >= 1) & (cs < 0)
    assert clean_solid.sum() > 1000
    ordinary = make_dev(opt)
    assert ordinary.CarveBatchSilhouettes(views, corrupted), vc.last_error()
    os_, ou = ordinary.download()
    assert not ((ou >= 1) & (os_ < 0)).any()  # the ordinary carve loses the sphere

    dev = make_dev(opt)
    got = dev.CarveRobustSilhouettes(views, corrupted, 1)
    ds, du = dev.download()
    assert (du == nv).all()  # the premise, on the device
    solid = (du >= 1) & (ds < 0)
    assert (solid >= clean_solid).all()  # contains the clean hull: the second largest is at most the clean maximum
    assert got["overruled"][bad] == int(solid.sum()) > 0
    assert got["overruled"].sum() == got["overruled"][bad]  # every other view's count is 0
    assert_equals(dev, got, ref, "blank mask")


# ---- 8. the example ----------------------------------------------------------------------------------------------------

def test_bunny_example_names_the_blank_mask(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    bad = 2
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "--tolerate", "1", "--blank-view", str(bad)],
                         check=True, capture_output=True, text=True)
    rows = [l.split() for l in run.stdout.splitlines() if l.startswith("ROBUST view")]
    assert len(rows) == 6, run.stdout
    counts = [int(r[4]) for r in rows]  # ROBUST view <i> overruled <n>
    assert [r[2] for r in rows] == [str(i) for i in range(6)]
    assert all(counts[bad] > x for i, x in enumerate(counts) if i != bad), counts
    assert os.path.getsize(str(tmp_path / "surface_robust.ply")) > 1000
    # ... and they are what Python gets on the same views
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    masks = B.load_masks()
    masks[bad] = np.zeros_like(masks[bad])
    dev = make_dev(B.bunny_option(10.0))
    assert dev.CarveRobustSilhouettes(views, masks, 1)["overruled"].tolist() == counts
    miss = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "--tolerate"], capture_output=True, text=True)
    assert miss.returncode == 10 and "--tolerate needs a number" in miss.stderr
