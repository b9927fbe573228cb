"""The ray-cast of the hull from z-slab contexts and the sharded carver (vcy_render_hull_slab, the SLAB instances of
render.hip, and the host merge) against the numpy restatement on the solid mask restricted to a slab's slices
(tests/render_ref.py, tests/slab_render_cases.py): depth BITS, voxel ids, entry axes and packed hit bits are compared for
equality, with brick skipping on and off; the sharded carver against the single context; and, independent of the
restatement, the merged silhouette of a carved bunny against the silhouettes it was carved from.

A context cannot own a slab that starts at z = 1 (a slab above the first keeps two halo slices below it: vcy_create), so
of the cut {1} only the slab [0, 1) runs on the device, and the cut at every z leaves [1, 2) out; the merge of those cuts
takes the restatement's image in that one place.  The cut {2} stands next to them."""
import ctypes as C

import numpy as np
import pytest

import bunny_data as B
import render_ref as RR
import slab_render_cases as S
import test_gpu_render as T
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import sharded

pytestmark = pytest.mark.gpu

LOWEST = np.finfo(np.float32).min
VIEWS = ["pinhole_inside", "pinhole_away", "ortho_axis", "ortho_negx", "ortho_oblique", "roi_shrunk", "roi_one_pixel"]
# (dims, cut set, states): every cut of the nz = 17 grids on two states, the cut at every z on the small grid and, on one
# sparse state, on a grid of several bricks
CASES = [(d, cut, ("random", "cluster")) for d in ((65, 9, 17), (24, 20, 17))
         for cut in ("one", "at_1", "at_nz-1", "at_8", "at_9", "at_3_11", "at_2")]
CASES += [((9, 8, 7), "every_z", ("random", "cluster")), ((24, 20, 17), "every_z", ("cluster",))]


def bounds_of(dims, cut):
    return [0, 2, dims[2]] if cut == "at_2" else S.cut_sets(dims[2])[cut]


def can_exist(z0):
    return z0 == 0 or z0 >= 2


def slab_state(dims, sn, z0, z1):
    sdf, cnt, iso = S.case(dims)["states"][sn]
    s = dims[0] * dims[1]
    return sdf[z0 * s:z1 * s], cnt[z0 * s:z1 * s], iso


def assert_slab_images(got, want, view, ctx):
    S.assert_images_equal(got, want, ctx)
    assert np.array_equal(got["hits"], S.pack_hits(want[1], view)), "%s: hit bits differ" % ctx


# ---- 1. slab contexts against the restatement --------------------------------------------------------------------------

@pytest.mark.parametrize("rayskip", [1, 0])
@pytest.mark.parametrize("dims,cut,states", CASES, ids=["%dx%dx%d-%s" % (d + (cut,)) for d, cut, _ in CASES])
def test_slab_equals_restatement(dims, cut, states, rayskip):
    c = S.case(dims)
    views = [c["views"][vn] for vn in VIEWS]
    bounds = bounds_of(dims, cut)
    hits = 0
    for sn in states:
        merged_in = [[] for _ in VIEWS]
        for z0, z1 in S.slabs_of(bounds):
            want = [S.slab_image(dims, sn, vn, z0, z1) for vn in VIEWS]
            if can_exist(z0):
                dev = S.make_dev(c["opt"], dims, z_range=(z0, z1))
                dev.set_param("rayskip", rayskip)
                sdf, cnt, iso = slab_state(dims, sn, z0, z1)
                dev.upload(sdf, cnt)
                got = dev.RenderHullSlab(views, iso, voxel_ids=True, axes=True, hits=True)
                for vn, v, g, w in zip(VIEWS, views, got, want):
                    assert_slab_images(g, w, v, "%s %s %s slab [%d, %d) rayskip %d" % (dims, sn, vn, z0, z1, rayskip))
                    hits += int((g["voxel"] >= 0).sum())
                s2, c2 = dev.download()
                assert np.array_equal(S.bits(s2), S.bits(sdf)) and np.array_equal(c2, cnt), "rendering changed the state"
                assert dev.last_render_ms() >= 0.0
                dev.close()
            else:
                got = [{"depth": d, "voxel": v, "axis": a} for d, v, a in want]
            for j, g in enumerate(got):
                merged_in[j].append(g)
        for vn, v, parts in zip(VIEWS, views, merged_in):
            S.assert_images_equal(vc.render_merge_host(v, parts), c["want"][sn, vn], "%s %s %s merged over %s" % (dims, sn, vn, cut))
    assert hits > 0


@pytest.mark.parametrize("width", [48, 70])
def test_hit_bits_and_their_padding(width):
    dims = (24, 20, 17)
    c = S.case(dims)
    e = float(max(dims))
    pos = np.array([1.3, 0.9, -1.7]) * e
    f = 34.0 * float(np.linalg.norm(pos)) / e
    views = [S.look(pos, (0.0, 0.0, 0.0), f, roi=roi, w=width) for roi in (None, ((5, 4), (width - 9, S.H - 7)))]
    sdf, cnt, iso = slab_state(dims, "random", 3, 11)
    dev = S.make_dev(c["opt"], dims, z_range=(3, 11))
    dev.upload(sdf, cnt)
    solid = S.slab_solid(S.solid_of(dims, "random"), dims, 3, 11)
    words = (width + 63) // 64
    lib = capi.load()
    for v in views:
        want = RR.render(v, c["planes"], dims, solid)
        hits = np.full((S.H, words), 0xA5A5A5A5A5A5A5A5, np.uint64)   # (every word has to be written)
        voxel = np.empty((S.H, width), np.int64)
        hp, vp = (C.c_void_p * 1)(hits.ctypes.data), (C.c_void_p * 1)(voxel.ctypes.data)
        assert lib.vcy_render_hull_slab(dev.ctx, iso, 1, (capi.View * 1)(v), None, vp, None, hp) == 0, vc.last_error()
        assert np.array_equal(voxel, want[1])
        assert np.array_equal(hits, S.pack_hits(want[1], v))
        unpacked = np.unpackbits(hits.view(np.uint8), axis=1, bitorder="little")
        assert np.array_equal(unpacked[:, :width] != 0, want[1] >= 0) and not unpacked[:, width:].any()
        assert (want[1] >= 0).sum() > 20
        if v.roi_min[0] > 0:
            assert not unpacked[:, :v.roi_min[0]].any() and not unpacked[:v.roi_min[1]].any()
        # only the hit bits: nothing else is asked for
        only = np.full((S.H, words), 7, np.uint64)
        assert lib.vcy_render_hull_slab(dev.ctx, iso, 1, (capi.View * 1)(v), None, None, None, (C.c_void_p * 1)(only.ctypes.data)) == 0
        assert np.array_equal(only, hits)


# ---- 2. a context that owns the whole grid ----------------------------------------------------------------------------

@pytest.mark.parametrize("dims", T.ALL_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_whole_grid_context_equals_render_hull(dims):
    c = S.case(dims)
    dev = S.make_dev(c["opt"], dims)
    names = list(c["views"])
    vs = [c["views"][vn] for vn in names]
    for rayskip in (1, 0):
        dev.set_param("rayskip", rayskip)
        for sn, (sdf, cnt, iso) in c["states"].items():
            dev.upload(sdf, cnt)
            old = dev.RenderHull(vs, iso, voxel_ids=True, axes=True)
            new = dev.RenderHullSlab(vs, iso, voxel_ids=True, axes=True, hits=True)
            for vn, v, a, b in zip(names, vs, old, new):
                assert_slab_images(b, (a["depth"], a["voxel"], a["axis"]), v, "%s %s %s" % (dims, sn, vn))
                S.assert_images_equal(b, c["want"][sn, vn], "%s %s %s against the restatement" % (dims, sn, vn))


# ---- 3. freshness ------------------------------------------------------------------------------------------------------

def all_misses(g):
    return np.all(np.isposinf(g["depth"])) and np.all(g["voxel"] == -1) and np.all(g["axis"] == 255) and not g["hits"].any()


def slab_want(dev, opt, view, z0, z1, iso=0.0):
    """The restatement's image of what the slab context holds now."""
    sdf, cnt = dev.download()
    nx, ny, nz = dev.dims
    solid = np.zeros(nx * ny * nz, bool)
    solid[z0 * nx * ny:z1 * nx * ny] = RR.solid_mask(sdf, cnt, iso)
    return RR.render(view, RR.option_planes(opt), dev.dims, solid), solid


def test_fresh_slab_and_stale_bit_planes():
    n, opt, views, masks = T.sphere_scene(6)
    z0, z1 = 9, 20
    dev = S.make_dev(opt, (n, n, n), z_range=(z0, z1))
    cam = views[5]
    kw = dict(voxel_ids=True, axes=True, hits=True)
    assert all_misses(dev.RenderHullSlab(cam, 0.0, **kw))
    sdf, cnt = dev.download()                                    # the fill, as it would have been written
    assert np.all(sdf == LOWEST) and not cnt.any()
    dev.reset()
    for i in range(2):
        assert dev.CarveSilhouette(views[i], masks[i]), vc.last_error()   # (queued: the render applies them)
    first = dev.RenderHullSlab(cam, 0.0, **kw)
    want, _ = slab_want(dev, opt, cam, z0, z1)
    assert_slab_images(first, want, cam, "two views")
    assert (first["voxel"] >= 0).sum() > 0
    assert dev.CarveSilhouette(views[2], masks[2]), vc.last_error()     # a carve
    second = dev.RenderHullSlab(cam, 0.0, **kw)
    want2, solid = slab_want(dev, opt, cam, z0, z1)
    assert not np.array_equal(want2[1], want[1]), "the third view does not change this image: the test shows nothing"
    assert_slab_images(second, want2, cam, "after one more view")
    sdf, cnt = dev.download()                                           # an upload: a floater in the slab's first voxel
    assert not solid[z0 * n * n]
    sdf[0], cnt[0] = -0.5, 1
    dev.upload(sdf, cnt)
    want3, solid3 = slab_want(dev, opt, cam, z0, z1)
    assert solid3[z0 * n * n]
    assert_slab_images(dev.RenderHullSlab(cam, 0.0, **kw), want3, cam, "floater")
    pieces = dev.LabelComponentsSlab(0.0)                               # the component filter on the slab
    order = np.argsort(-pieces["n_voxels"], kind="stable")
    assert len(order) >= 2
    assert dev.KeepComponentsSlab(pieces["label"][order[1:]])["removed_voxels"] >= 1
    want4, solid4 = slab_want(dev, opt, cam, z0, z1)
    assert not solid4[z0 * n * n]
    assert_slab_images(dev.RenderHullSlab(cam, 0.0, **kw), want4, cam, "after KeepComponentsSlab")
    want5, _ = slab_want(dev, opt, cam, z0, z1, iso=-0.3)               # another iso level on the same state
    assert_slab_images(dev.RenderHullSlab(cam, -0.3, **kw), want5, cam, "iso -0.3")
    dev.reset()
    assert all_misses(dev.RenderHullSlab(cam, 0.0, **kw))


# ---- 4. batches --------------------------------------------------------------------------------------------------------

def test_sixty_five_views_take_two_launches_and_sizes_may_differ():
    dims = (24, 20, 17)
    c = S.case(dims)
    z0, z1 = 3, 11
    dev = S.make_dev(c["opt"], dims, z_range=(z0, z1))
    sdf, cnt, iso = slab_state(dims, "random", z0, z1)
    dev.upload(sdf, cnt)
    solid = S.slab_solid(S.solid_of(dims, "random"), dims, z0, z1)
    ang = np.linspace(0.0, 2.0 * np.pi, 65, endpoint=False)
    views = [S.look((60.0 * np.cos(a), 25.0 + 10.0 * np.sin(3 * a), 60.0 * np.sin(a)), (0.0, 0.0, 0.0), 30.0, w=16, h=16) for a in ang]
    kw = dict(voxel_ids=True, axes=True, hits=True)
    batch = dev.RenderHullSlab(views, iso, **kw)
    assert len(batch) == 65
    n_hit = 0
    for k in (0, 1, 31, 63, 64):           # (63 | 64: the last view of the first launch, the only one of the second)
        assert_slab_images(batch[k], RR.render(views[k], c["planes"], dims, solid), views[k], "view %d of 65" % k)
        n_hit += int((batch[k]["voxel"] >= 0).sum())
    assert n_hit > 0
    for k in range(65):
        one = dev.RenderHullSlab(views[k], iso, **kw)
        assert_slab_images(one, (batch[k]["depth"], batch[k]["voxel"], batch[k]["axis"]), views[k], "single call %d" % k)
        assert np.array_equal(one["hits"], batch[k]["hits"])
    small = S.look((30.0, 20.0, -40.0), (0.0, 0.0, 0.0), 40.0, w=17, h=9)
    wide = S.look((30.0, 20.0, -40.0), (0.0, 0.0, 0.0), 60.0, w=70, h=40)
    names = list(c["views"])
    mixed = dev.RenderHullSlab([c["views"][names[0]], small, wide, c["views"][names[5]]], iso, **kw)
    assert mixed[1]["depth"].shape == (9, 17) and mixed[1]["hits"].shape == (9, 1) and mixed[2]["hits"].shape == (40, 2)
    assert_slab_images(mixed[1], RR.render(small, c["planes"], dims, solid), small, "17 x 9")
    assert_slab_images(mixed[2], RR.render(wide, c["planes"], dims, solid), wide, "70 x 40")
    assert_slab_images(mixed[0], S.slab_image(dims, "random", names[0], z0, z1), c["views"][names[0]], "mixed 0")
    assert_slab_images(mixed[3], S.slab_image(dims, "random", names[5], z0, z1), c["views"][names[5]], "mixed 3")


# ---- 5. the sharded carver against the single context -------------------------------------------------------------------

def check_sharded(dev, sh, views, masks, ctx):
    want = dev.RenderHull(views, 0.0, voxel_ids=True, axes=True)
    got = sh.RenderHull(views, 0.0, voxel_ids=True, axes=True)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        S.assert_images_equal(a, (b["depth"], b["voxel"], b["axis"]), "%s view %d" % (ctx, k))
        assert a["device_ms"] >= 0.0
    assert sum(int((b["voxel"] >= 0).sum()) for b in want) > 100
    one = sh.RenderHull(views[0])
    assert set(one) == {"depth", "device_ms"} and np.array_equal(S.bits(one["depth"]), S.bits(want[0]["depth"]))
    counts = sh.HullAgreement(views, masks)
    assert counts.dtype == np.int64 and np.array_equal(counts, dev.HullAgreement(views, masks)), ctx
    return got


@pytest.mark.parametrize("slabs", [1, 2, 3, 5, "planned"])
def test_sharded_sphere(slabs):
    n, opt, views, masks = T.sphere_scene()
    sdfs = [vc.make_sdf(m) for m in masks]
    dev = S.make_dev(opt, (n, n, n))
    sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=3 if slabs == "planned" else slabs)
    if slabs == "planned":
        bounds = sh.plan(views, sdfs)
        assert len(bounds) == 4
    assert sh.Init(), vc.last_error()
    for c in [dev] + sh.slabs:
        for v, s in zip(views, sdfs):
            assert c.Carve(v, s), vc.last_error()
    check_sharded(dev, sh, views, masks, "sphere in %s slabs" % slabs)
    sh.close()


@pytest.mark.parametrize("slabs", [1, 2, 3, 5])
def test_sharded_bunny_and_its_silhouettes(slabs):
    views, masks = T.bunny_inputs()
    opt = B.bunny_option(10.0)
    dev = S.make_dev(opt)
    sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=slabs)
    assert sh.Init(), vc.last_error()
    assert dev.CarveBatchSilhouettes(views, masks), vc.last_error()
    assert sh.CarveBatchSilhouettes(views, masks), vc.last_error()
    got = check_sharded(dev, sh, views, masks, "bunny in %d slabs" % slabs)
    # independent of the restatement: the merged silhouette lies on the silhouettes the hull was carved from
    pos = dev.positions()
    diff = [opt.bb_max[a] - opt.bb_min[a] for a in range(3)]
    pitch = max(diff[a] / dev.dims[a] for a in range(3))
    counts = sh.HullAgreement(views, masks)
    for k, (view, mask, g) in enumerate(zip(views, masks, got)):
        _, _, z = T.carve_projection(view, pos)
        z_min = float(z.min())
        assert z_min > 0
        r = int(np.ceil(0.5 * np.sqrt(3.0) * pitch * float(max(view.fx, view.fy)) / z_min)) + 1
        hull = g["voxel"] >= 0
        assert hull.sum() > 1000
        m = mask != 0
        out = np.argwhere(hull & ~m)            # hull pixels off the silhouette: each within r pixels of it
        my, mx = np.nonzero(m)
        for at in range(0, len(out), 64):
            blk = out[at:at + 64]
            d2 = (blk[:, 0, None] - my[None, :]) ** 2 + (blk[:, 1, None] - mx[None, :]) ** 2
            assert d2.min(axis=1).max() <= r * r, (k, r, float(np.sqrt(d2.min(axis=1).max())))
        assert counts[k].tolist() == RR.agreement(view, g["voxel"], mask), k
        assert counts[k][0] > 0.8 * (counts[k][0] + counts[k][1])
    sh.close()


def test_old_entry_points_still_refuse_a_slab():
    dims = (9, 8, 7)
    c = S.case(dims)
    sdf, cnt, iso = slab_state(dims, "random", 2, 7)
    slab = S.make_dev(c["opt"], dims, z_range=(2, 7))
    slab.upload(sdf, cnt)
    view = c["views"]["pinhole_outside"]
    with pytest.raises(RuntimeError, match="whole grid"):
        slab.RenderHull(view, iso)
    got = slab.RenderHullSlab(view, iso, voxel_ids=True, axes=True, hits=True)
    assert_slab_images(got, S.slab_image(dims, "random", "pinhole_outside", 2, 7), view, "after the refusal")
    lib = capi.load()
    assert lib.vcy_render_hull_slab(slab.ctx, iso, 0, (capi.View * 1)(view), None, None, None, None) == capi.VCY_ERR_INVALID_ARG
    bad = capi.View.from_buffer_copy(view)
    bad.roi_max[1] = S.H
    assert lib.vcy_render_hull_slab(slab.ctx, iso, 1, (capi.View * 1)(bad), None, None, None, None) == capi.VCY_ERR_INVALID_ARG
