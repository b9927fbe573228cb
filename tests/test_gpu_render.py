"""The ray-cast of the hull on the device (vcy_render_hull / vcy_hull_agreement, render.hip) against the numpy restatement
of its definition (tests/render_ref.py): depth BITS, voxel ids and entry axes are compared for equality; brick skipping
against the flat walk; and two checks that do not share the restatement's arithmetic -- projected voxel centres must be
covered, and the hull of a carved scene must lie on the silhouettes it was carved from."""
import ctypes as C
import math

import numpy as np
import pytest

import bunny_data as B
import render_ref as RR
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import CarverOption, UpdateOption, make_view

pytestmark = pytest.mark.gpu

F = np.float32
LOWEST = np.finfo(np.float32).min
W, H = 48, 40
# dims -> extent of the box per axis: (9, 8, 7) and (24, 20, 17) have diff / resolution truncate (pitch != resolution),
# (65, 9, 17) crosses the 64-voxel word and the brick edges, (1, 1, 1) is a box of 1.5 with one voxel of 1
BOX = {(9, 8, 7): (9.5, 8.3, 7.9), (65, 9, 17): (65.0, 9.0, 17.0), (24, 20, 17): (24.4, 20.2, 17.3), (1, 1, 1): (1.5, 1.5, 1.5)}
ALL_DIMS = list(BOX)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def grid_option(dims, scale=1.0):
    h = [scale * e / 2.0 for e in BOX[tuple(dims)]]
    return CarverOption(bb_min=[-x for x in h], bb_max=h, resolution=scale)


def make_dev(opt, dims=None, z_range=None):
    dev = vc.VoxelCarver(opt, z_range=z_range)
    assert dev.Init(), vc.last_error()
    if dims is not None:
        assert dev.dims == tuple(dims), (dev.dims, dims)
    return dev


def look(pos, target, f=30.0, ortho=False, roi=None, up=(0.0, 1.0, 0.1), w=W, h=H):
    w2c = synth.affine_inverse(synth.lookat_c2w(pos, target, up))
    if ortho:  # a pixel is a world unit: put the target in the middle of the image
        w2c[0, 3] += w / 2.0
        w2c[1, 3] += h / 2.0
    rmin, rmax = roi if roi else (None, None)
    return make_view(w2c.astype(F), F(f), F(f * 1.07), F(w / 2.0 - 0.3), F(h / 2.0 + 0.2), w, h, rmin, rmax, ortho)


def views_for(dims, scale=1.0):
    """name -> view; the grid is centred on the origin with extent about dims * scale."""
    e = scale * float(max(dims))
    d = np.array(dims, np.float64) * scale
    out_pos = np.array([1.3, 0.9, -1.7]) * e
    dist = float(np.linalg.norm(out_pos))
    f_out = 34.0 * dist / e
    ident = np.zeros((3, 4), F)
    ident[:, :3] = np.eye(3)
    ident[:, 3] = (W // 2, H // 2, e + 3.0)   # integer offsets: rays run along voxel centres or cell planes, d = (0, 0, 1)
    return {
        "pinhole_outside": look(out_pos, (0.1 * e, -0.05 * e, 0.02 * e), f_out),
        "pinhole_inside": look(d * (0.13, 0.21, -0.17), (e, 0.4 * e, 0.3 * e), 25.0),
        "pinhole_away": look(out_pos, 2.0 * out_pos, f_out),
        "ortho_axis": make_view(ident, 1.0, 1.0, 0.0, 0.0, W, H, is_ortho=True),
        "ortho_negx": look((e + 2.0, 0.0, 0.0), (0.0, 0.0, 0.0), ortho=True, up=(0.0, 0.0, 1.0)),
        "ortho_oblique": look(np.array([1.0, 0.7, -1.2]) * e, (0.0, 0.0, 0.0), ortho=True),
        "roi_shrunk": look(out_pos, (0.1 * e, -0.05 * e, 0.02 * e), f_out, roi=((5, 4), (40, 33))),
        "roi_one_pixel": look(out_pos, (0.1 * e, -0.05 * e, 0.02 * e), f_out, roi=((24, 20), (24, 20))),
    }


def states_for(dims):
    """name -> (sdf, cnt, iso)"""
    nx, ny, nz = dims
    n = nx * ny * nz
    out = {}
    for name, density, iso, seed in (("random", 0.3, 0.0, 1), ("dense_iso", 0.6, -0.05, 2), ("thin_iso", 0.08, 0.0125, 3)):
        rng = np.random.RandomState(seed)
        solid = rng.rand(n) < density
        mag = (0.1 + 0.9 * rng.rand(n)).astype(F)
        sdf = np.where(solid, -mag, mag).astype(F)
        cnt = rng.randint(1, 4, n).astype(np.int32)
        r = rng.rand(n)
        sdf[r < 0.02], cnt[r < 0.02] = LOWEST, 0                 # untouched
        sdf[(r >= 0.02) & (r < 0.04)] = np.nan
        sdf[(r >= 0.04) & (r < 0.08)] = F(iso)                   # exactly the iso level: solid iff float(iso) < iso
        cnt[(r >= 0.08) & (r < 0.10)] = 0                        # a count of 0 over a valid sdf
        out[name] = (sdf, cnt, iso)
    # a cluster in one corner region and three lone voxels: most bricks hold nothing
    rng = np.random.RandomState(4)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    box = (x >= nx // 2) & (x < nx // 2 + max(1, nx // 4)) & (y < max(1, ny // 3)) & (z >= nz // 3)
    solid = (box & (rng.rand(nz, ny, nx) < 0.5)).reshape(-1)
    solid[rng.randint(0, n, 3)] = True
    out["cluster"] = (np.where(solid, F(-0.5), F(0.5)).astype(F), np.ones(n, np.int32), 0.0)
    out["empty_hull"] = (np.full(n, 0.5, F), np.ones(n, np.int32), 0.0)
    out["all_solid"] = (np.full(n, -0.5, F), np.ones(n, np.int32), 0.0)
    return out


_cache = {}


def case(dims):
    """Option, plane tables, views, states and the restatement's images of every (state, view): computed once."""
    dims = tuple(dims)
    if dims not in _cache:
        opt = grid_option(dims)
        planes = RR.option_planes(opt)
        views, states = views_for(dims), states_for(dims)
        want = {}
        for sn, (sdf, cnt, iso) in states.items():
            solid = RR.solid_mask(sdf, cnt, iso)
            for vn, v in views.items():
                want[sn, vn] = RR.render(v, planes, dims, solid)
        _cache[dims] = dict(opt=opt, planes=planes, views=views, states=states, want=want)
    return _cache[dims]


def assert_images_equal(got, want, ctx):
    d, v, a = want
    assert np.array_equal(got["voxel"], v), "%s: %d voxel ids differ" % (ctx, int((got["voxel"] != v).sum()))
    assert np.array_equal(bits(got["depth"]), bits(d)), "%s: %d depths differ" % (ctx, int((bits(got["depth"]) != bits(d)).sum()))
    assert np.array_equal(got["axis"], a), "%s: %d axes differ" % (ctx, int((got["axis"] != a).sum()))


# ---- 1. equality with the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize("rayskip", [1, 0])
@pytest.mark.parametrize("dims", ALL_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_equals_restatement(dims, rayskip):
    c = case(dims)
    dev = make_dev(c["opt"], dims)
    dev.set_param("rayskip", rayskip)
    assert dev.get_param("rayskip") == rayskip
    names = list(c["views"])
    hits = 0
    for sn, (sdf, cnt, iso) in c["states"].items():
        dev.upload(sdf, cnt)   # (one context through all states: every upload must make the kept bit planes stale)
        got = dev.RenderHull([c["views"][vn] for vn in names], iso, voxel_ids=True, axes=True)
        for vn, g in zip(names, got):
            assert_images_equal(g, c["want"][sn, vn], "%s %s %s rayskip %d" % (dims, sn, vn, rayskip))
            hits += int((g["voxel"] >= 0).sum())
            if sn == "empty_hull" or vn == "pinhole_away":
                assert np.all(np.isposinf(g["depth"])) and np.all(g["voxel"] == -1) and np.all(g["axis"] == 255)
        s2, c2 = dev.download()
        assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt), "rendering changed the state"
        assert dev.last_render_ms() >= 0.0
    assert hits > 0
    if max(dims) > 1:  # the cases are not vacuous: every kind of entry occurs somewhere
        seen = set()
        for (sn, vn), (d, v, a) in c["want"].items():
            seen |= set(np.unique(a).tolist())
        assert seen >= {0, 1, 2, 3, 255}, seen


# ---- 2. skipping on equals skipping off ------------------------------------------------------------------------------

_bunny = {}


def bunny_inputs():
    if not _bunny:
        _bunny["views"] = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
        _bunny["masks"] = B.load_masks()
    return _bunny["views"], _bunny["masks"]


def test_skip_equals_flat_walk():
    for dims in ALL_DIMS:
        c = case(dims)
        dev = make_dev(c["opt"], dims)
        vs = list(c["views"].values())
        for sn, (sdf, cnt, iso) in c["states"].items():
            dev.upload(sdf, cnt)
            res = []
            for rayskip in (1, 0):
                dev.set_param("rayskip", rayskip)
                res.append(dev.RenderHull(vs, iso, voxel_ids=True, axes=True))
            for a, b in zip(*res):
                assert np.array_equal(bits(a["depth"]), bits(b["depth"])) and np.array_equal(a["voxel"], b["voxel"]) and \
                    np.array_equal(a["axis"], b["axis"]), (dims, sn)


def test_skip_equals_flat_walk_on_the_bunny():
    views, masks = bunny_inputs()
    dev = make_dev(B.bunny_option(10.0))
    assert dev.CarveBatchSilhouettes(views, masks), vc.last_error()
    res, counts = [], []
    for rayskip in (1, 0):
        dev.set_param("rayskip", rayskip)
        res.append(dev.RenderHull(views, 0.0, voxel_ids=True, axes=True))
        counts.append(dev.HullAgreement(views, masks))
    for a, b in zip(*res):
        assert np.array_equal(bits(a["depth"]), bits(b["depth"])) and np.array_equal(a["voxel"], b["voxel"]) and \
            np.array_equal(a["axis"], b["axis"])
        assert (a["voxel"] >= 0).sum() > 1000
    assert np.array_equal(counts[0], counts[1])
    for v, m, a, cnt in zip(views, masks, res[0], counts[0]):
        assert cnt.tolist() == RR.agreement(v, a["voxel"], m)
        assert cnt[0] > 0.8 * (cnt[0] + cnt[1])   # the hull covers the silhouette it was carved from, up to its voxel size


# ---- 3. independent of the arithmetic: projected voxel centres are covered ---------------------------------------------

def carve_projection(view, pos):
    """The carve's own projection of world points (voxel_carver.cc:453, camera.cc:131-137 | 201-205), float32."""
    m = np.array(list(view.w2c), F).reshape(3, 4)
    px, py, pz = (pos[:, k].astype(F) for k in range(3))
    pc = [m[r, 3] + (m[r, 0] * px + (m[r, 1] * py + m[r, 2] * pz)) for r in range(3)]
    if view.is_ortho:
        return pc[0], pc[1], pc[2]
    with np.errstate(all="ignore"):
        return (F(view.fx) / pc[2]) * pc[0] + F(view.cx), (F(view.fy) / pc[2]) * pc[1] + F(view.cy), pc[2]


@pytest.mark.parametrize("name", ["pinhole_outside", "ortho_axis", "ortho_negx", "ortho_oblique", "roi_shrunk"])
def test_projected_centres_are_covered(name):
    dims, scale = (9, 8, 7), 2.5   # voxels of about 2.6 world units: at least 2 pixels in every view below
    opt = grid_option(dims, scale)
    dev = make_dev(opt, dims)
    view = views_for(dims, scale)[name]
    sdf, cnt, iso = states_for(dims)["random"]
    dev.upload(sdf, cnt)
    solid = RR.solid_mask(sdf, cnt, iso)
    pos = dev.positions()
    u, v, z = carve_projection(view, pos)
    pitch = min(BOX[dims][a] * scale / dims[a] for a in range(3))
    if not view.is_ortho:
        assert min(view.fx, view.fy) * pitch / float(z.max()) >= 2.0
    assert pitch >= 2.0 and float(z.min()) > 0.0
    got = dev.RenderHull(view, iso)
    pu, pv = np.floor(u + F(0.5)).astype(int), np.floor(v + F(0.5)).astype(int)
    in_roi = (pu >= view.roi_min[0]) & (pu <= view.roi_max[0]) & (pv >= view.roi_min[1]) & (pv <= view.roi_max[1])
    idx = np.nonzero(solid & in_roi)[0]
    assert len(idx) > 20
    d = got["depth"][pv[idx], pu[idx]]
    # the pixel's ray passes the centre at depth z within half a pixel, a quarter of a voxel: inside the voxel's cell
    assert np.all(np.isfinite(d)), "%d solid voxels project to pixels the hull does not cover" % int((~np.isfinite(d)).sum())
    assert np.all(d <= z[idx]), "the hull lies behind %d solid voxels" % int((d > z[idx]).sum())


# ---- 4. consistency with the carve -----------------------------------------------------------------------------------

def sphere_scene(n_views=8):
    n = 24
    views, masks = synth.sphere_views(n, n_views, W, H)
    return n, synth.sphere_option(n, UpdateOption(voxel_update=capi.VCY_UPDATE_MAX)), views, masks


def ref_images(dev, opt, views, iso=0.0):
    sdf, cnt = dev.download()
    solid = RR.solid_mask(sdf, cnt, iso)
    planes = RR.option_planes(opt)
    return [RR.render(v, planes, dev.dims, solid) for v in views], solid


def test_hull_of_a_carved_scene_lies_on_its_silhouettes():
    n, opt, views, masks = sphere_scene()
    dev = make_dev(opt, (n, n, n))
    assert dev.CarveBatchSilhouettes(views, masks), vc.last_error()
    pos = dev.positions()
    got = dev.RenderHull(views, 0.0, voxel_ids=True)
    counts = dev.HullAgreement(views, masks)
    diff = [opt.bb_max[a] - opt.bb_min[a] for a in range(3)]
    pitch = max(diff[a] / dev.dims[a] for a in range(3))   # the voxel pitch of the scene, diff / n
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for k, (view, mask, g) in enumerate(zip(views, masks, got)):
        _, _, z = carve_projection(view, pos)
        z_min = float(z.min())
        assert z_min > 0
        # a hull pixel's ray passes a solid voxel's cell, so within half its diagonal of the centre, and a centre with
        # a negative bilinear sample lies next to a silhouette pixel
        r = math.ceil(0.5 * math.sqrt(3.0) * pitch * float(max(view.fx, view.fy)) / z_min) + 1
        hull = g["voxel"] >= 0
        assert hull.sum() > 20
        mu, mv = uu[mask != 0], vv[mask != 0]
        d2 = (uu[hull][:, None] - mu[None, :]) ** 2 + (vv[hull][:, None] - mv[None, :]) ** 2
        assert d2.min(axis=1).max() <= r * r, (k, r, float(np.sqrt(d2.min(axis=1).max())))
        assert counts[k].tolist() == RR.agreement(view, g["voxel"], mask), k
        assert counts[k][0] > 0


# ---- 5. freshness ----------------------------------------------------------------------------------------------------

def test_render_follows_the_state():
    n, opt, views, masks = sphere_scene(6)
    dev = make_dev(opt, (n, n, n))
    cam = views[5]
    fresh = dev.RenderHull(cam, 0.0, voxel_ids=True, axes=True)          # nothing carved: all misses
    assert np.all(np.isposinf(fresh["depth"])) and np.all(fresh["voxel"] == -1) and np.all(fresh["axis"] == 255)
    assert dev.HullAgreement([cam], [masks[5]]).tolist() == [[0, int((masks[5] != 0).sum()), 0]]
    for i in range(2):
        assert dev.CarveSilhouette(views[i], masks[i]), vc.last_error()   # (queued: the render applies them)
    first = dev.RenderHull(cam, 0.0, voxel_ids=True, axes=True)
    (want,), _ = ref_images(dev, opt, [cam])
    assert_images_equal(first, want, "two views")
    assert (first["voxel"] >= 0).sum() > 0
    assert dev.CarveSilhouette(views[2], masks[2]), vc.last_error()
    second = dev.RenderHull(cam, 0.0, voxel_ids=True, axes=True)
    (want2,), solid = ref_images(dev, opt, [cam])
    assert not np.array_equal(want2[1], want[1]), "the third view does not change this image: the test shows nothing"
    assert_images_equal(second, want2, "after one more view")
    # the filter: add a floater, render, remove it
    sdf, cnt = dev.download()
    assert not solid[0]
    sdf[0], cnt[0] = -0.5, 1
    dev.upload(sdf, cnt)
    assert_images_equal(dev.RenderHull(cam, 0.0, voxel_ids=True, axes=True), ref_images(dev, opt, [cam])[0][0], "floater")
    assert dev.KeepComponents(0.0, largest=1)["removed_voxels"] >= 1
    kept = dev.RenderHull(cam, 0.0, voxel_ids=True, axes=True)
    (want3,), solid3 = ref_images(dev, opt, [cam])
    assert not solid3[0]
    assert_images_equal(kept, want3, "after KeepComponents")
    # another iso level on the same state
    (want4,), _ = ref_images(dev, opt, [cam], iso=-0.3)
    assert_images_equal(dev.RenderHull(cam, -0.3, voxel_ids=True, axes=True), want4, "iso -0.3")
    dev.reset()
    again = dev.RenderHull(cam, 0.0, voxel_ids=True, axes=True)
    assert np.all(again["voxel"] == -1) and np.all(np.isposinf(again["depth"])) and np.all(again["axis"] == 255)
    assert dev.CarveSilhouette(views[0], masks[0]), vc.last_error()
    assert_images_equal(dev.RenderHull(cam, 0.0, voxel_ids=True, axes=True), ref_images(dev, opt, [cam])[0][0], "after reset")


# ---- 6. batch --------------------------------------------------------------------------------------------------------

def test_batch_equals_single_calls_and_null_outputs():
    dims = (24, 20, 17)
    c = case(dims)
    dev = make_dev(c["opt"], dims)
    sdf, cnt, iso = c["states"]["random"]
    dev.upload(sdf, cnt)
    names = list(c["views"])
    assert len(names) == 8
    vs = [c["views"][vn] for vn in names]
    batch = dev.RenderHull(vs, iso, voxel_ids=True, axes=True)
    for v, b, vn in zip(vs, batch, names):
        one = dev.RenderHull(v, iso, voxel_ids=True, axes=True)
        assert_images_equal(one, (b["depth"], b["voxel"], b["axis"]), vn)
    # NULL arrays and NULL entries: only what is asked for is written
    lib = capi.load()
    n = len(vs)
    arr = (capi.View * n)(*vs)
    depth = [np.full((H, W), -7.0, F) for _ in vs]
    axis = [np.full((H, W), 77, np.uint8) for _ in vs]
    dp = (C.c_void_p * n)(*[None if k % 2 else depth[k].ctypes.data for k in range(n)])
    ap = (C.c_void_p * n)(*[axis[k].ctypes.data if k == 3 else None for k in range(n)])
    assert lib.vcy_render_hull(dev.ctx, iso, n, arr, dp, None, ap) == 0, vc.last_error()
    for k in range(n):
        if k % 2:
            assert np.all(depth[k] == F(-7.0))
        else:
            assert np.array_equal(bits(depth[k]), bits(batch[k]["depth"]))
        assert np.array_equal(axis[k], batch[k]["axis"]) if k == 3 else np.all(axis[k] == 77)
    assert lib.vcy_render_hull(dev.ctx, iso, n, arr, None, None, None) == 0
    # views of different sizes in one launch
    small = look((30.0, 20.0, -40.0), (0.0, 0.0, 0.0), 40.0, w=17, h=9)
    mixed = dev.RenderHull([vs[0], small, vs[5]], iso, voxel_ids=True, axes=True)
    assert mixed[1]["depth"].shape == (9, 17)
    assert_images_equal(mixed[1], RR.render(small, c["planes"], dims, RR.solid_mask(sdf, cnt, iso)), "17 x 9")
    assert_images_equal(mixed[0], c["want"]["random", names[0]], "mixed 0")
    assert_images_equal(mixed[2], c["want"]["random", names[5]], "mixed 2")


# ---- 7. refusals -----------------------------------------------------------------------------------------------------

def test_refusals():
    dims = (9, 8, 7)
    c = case(dims)
    sdf, cnt, iso = c["states"]["random"]
    view = c["views"]["pinhole_outside"]
    nxy = dims[0] * dims[1]
    slab = make_dev(c["opt"], dims, z_range=(2, 7))
    whole = make_dev(c["opt"], dims)
    slab.upload(sdf[2 * nxy:], cnt[2 * nxy:])
    with pytest.raises(RuntimeError, match="whole grid"):
        slab.RenderHull(view, iso)
    lib = capi.load()
    arr = (capi.View * 1)(view)
    mask = np.zeros((H, W), np.uint8)
    counts = np.zeros(3, np.int64)
    mp = (C.c_void_p * 1)(mask.ctypes.data)
    assert lib.vcy_hull_agreement(slab.ctx, iso, 1, arr, mp, counts.ctypes.data_as(C.c_void_p)) == capi.VCY_ERR_UNSUPPORTED
    assert lib.vcy_render_hull(slab.ctx, iso, 1, arr, None, None, None) == capi.VCY_ERR_UNSUPPORTED
    s2, c2 = slab.download()
    assert np.array_equal(bits(s2), bits(sdf[2 * nxy:])) and np.array_equal(c2, cnt[2 * nxy:])
    whole.upload(sdf, cnt)
    for change in ("nan", "fx", "fy", "width", "height", "roi"):
        v = capi.View.from_buffer_copy(view)
        if change == "nan":
            v.w2c[3] = float("nan")
        elif change == "fx":
            v.fx = 0.0
        elif change == "fy":
            v.fy = 0.0
        elif change == "width":
            v.width = 0
        elif change == "height":
            v.height = -1
        else:
            v.roi_max[1] = H
        assert lib.vcy_render_hull(whole.ctx, iso, 1, (capi.View * 1)(v), None, None, None) == capi.VCY_ERR_INVALID_ARG, change
    assert lib.vcy_render_hull(whole.ctx, iso, 0, arr, None, None, None) == capi.VCY_ERR_INVALID_ARG
    s2, c2 = whole.download()
    assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt)
    assert_images_equal(whole.RenderHull(view, iso, voxel_ids=True, axes=True), c["want"]["random", "pinhole_outside"], "after the refusals")
