"""Connected components of the hull on the device (vcy_label_components / vcy_keep_components, components.hip) against
the numpy restatement of their definitions (tests/components_ref.py).  The definitions are integer arithmetic on the
solid mask, so every labelling assertion is EQUALITY: of the sorted component list (label, n_voxels, boxes) and of the
label of every voxel; the filter is checked byte for byte against the reference-filtered state, and through every
reader of the state behind it (marching cubes with and without brick skipping and normals, ExtractVoxel, one more carve)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bunny_data as B
import components_ref as R
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import CarverOption, UpdateOption

pytestmark = pytest.mark.gpu

LOWEST = np.finfo(np.float32).min
KEEP_RULES = [dict(largest=1, min_voxels=0), dict(largest=0, min_voxels=20), dict(largest=2, min_voxels=5)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box_option(dims, uo=None):
    """A grid of exactly `dims` voxels of size 1 centred on the origin (halves of small integers are exact floats)."""
    h = [d / 2.0 for d in dims]
    return CarverOption(bb_min=[-x for x in h], bb_max=h, resolution=1.0, update_option=uo or UpdateOption())


def make_dev(dims, uo=None):
    dev = vc.VoxelCarver(box_option(dims, uo))
    assert dev.Init(), vc.last_error()
    assert dev.dims == tuple(dims), (dev.dims, dims)
    return dev


def state_from_mask(solid, cnt=None):
    sdf = np.where(solid, np.float32(-0.5), np.float32(0.5)).astype(np.float32)
    return sdf, (np.ones(solid.size, np.int32) if cnt is None else cnt)


def check_labels(dev, sdf, cnt, iso, ctx=""):
    """Labels `dev` (which holds sdf, cnt) and compares list and per-voxel labels with the reference; returns both."""
    want, want_lab = R.reference(sdf, cnt, dev.dims, iso)
    got = dev.LabelComponents(iso, labels=True)
    R.assert_components_equal(got, want, ctx)
    bad = int((got["labels"] != want_lab).sum())
    assert bad == 0, "%s: the labels of %d voxels differ from the reference" % (ctx, bad)
    assert got["device_ms"] >= 0.0
    return want, want_lab


def random_state(dims, density, iso, seed):
    rng = np.random.RandomState(seed)
    n = dims[0] * dims[1] * dims[2]
    solid = rng.rand(n) < density
    mag = (0.1 + 0.9 * rng.rand(n)).astype(np.float32)      # |sdf| >= 0.1: clear of every iso level used
    sdf = np.where(solid, -mag, mag).astype(np.float32)
    cnt = rng.randint(1, 4, n).astype(np.int32)
    r = rng.rand(n)
    untouched = r < 0.02
    sdf[untouched], cnt[untouched] = LOWEST, 0
    sdf[(r >= 0.02) & (r < 0.03)] = np.nan
    sdf[(r >= 0.03) & (r < 0.08)] = np.float32(iso)          # exactly the iso level as a float: solid iff float(iso) < iso
    cnt[(r >= 0.08) & (r < 0.09)] = 0                        # a count of 0 over a valid sdf: not solid either
    return sdf, cnt


RANDOM_DIMS = [(8, 8, 8), (9, 10, 17), (65, 9, 9), (70, 23, 19), (130, 7, 5)]


# ---- 1. random states on awkward dims ------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", RANDOM_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_random_states(dims):
    dev = make_dev(dims)
    for k, (density, iso) in enumerate(itertools.product((0.2, 0.31, 0.5, 0.9), (0.0, 0.0125, -0.05))):
        sdf, cnt = random_state(dims, density, iso, 100 + k)
        dev.upload(sdf, cnt)
        want, _ = check_labels(dev, sdf, cnt, iso, "%s density %g iso %g" % (dims, density, iso))
        assert len(want["label"]) > 0
        s2, c2 = dev.download()
        assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt), "labelling changed the state"


# ---- 2. serpentine ---------------------------------------------------------------------------------------------------

def serpentine(n):
    """A 1-voxel-wide path through an n^3 grid: along x in every second row of every second slice, joined by single
    voxels alternately at the far and the near end, slices joined the same way -- it enters and leaves every brick."""
    s = np.zeros((n, n, n), bool)  # [z][y][x]
    end_y = 0
    for zi, z in enumerate(range(0, n, 2)):
        rows = list(range(0, n, 2))
        if zi % 2:
            rows.reverse()
        x_end = 0
        for ri, y in enumerate(rows):
            s[z, y, :] = True
            x_end = n - 1 if (ri % 2 == 0) else 0
            if ri + 1 < len(rows):
                s[z, (y + rows[ri + 1]) // 2, x_end] = True
        end_y = rows[-1]
        if z + 2 < n:
            s[z + 1, end_y, x_end] = True
    return s.reshape(-1)


@pytest.mark.parametrize("complement", [False, True])
def test_serpentine(complement):
    n = 24
    solid = serpentine(n)
    path_len = int(solid.sum())
    if complement:
        solid = ~solid
    sdf, cnt = state_from_mask(solid)
    dev = make_dev((n, n, n))
    dev.upload(sdf, cnt)
    want, lab = check_labels(dev, sdf, cnt, 0.0, "serpentine")
    if not complement:
        assert want["label"].tolist() == [0] and want["n_voxels"].tolist() == [path_len]
        assert want["bb_min"].tolist() == [[0, 0, 0]] and want["bb_max"].tolist() == [[n - 1, n - 2, n - 2]]
    again = dev.LabelComponents(0.0, labels=True)
    R.assert_components_equal(again, want, "second labelling")
    assert np.array_equal(again["labels"], lab)


# ---- 3. checkerboard, diagonal contact -------------------------------------------------------------------------------

def test_checkerboard():
    dims = (17, 9, 10)
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    solid = ((x + y + z) % 2 == 0).reshape(-1)
    sdf, cnt = state_from_mask(solid)
    dev = make_dev(dims)
    dev.upload(sdf, cnt)
    want, _ = check_labels(dev, sdf, cnt, 0.0, "checkerboard")
    n = nx * ny * nz
    assert len(want["label"]) == (n + 1) // 2
    assert np.array_equal(want["label"], np.flatnonzero(solid)) and (want["n_voxels"] == 1).all()


def test_blocks_touching_at_a_brick_corner():
    dims = (16, 16, 16)
    s = np.zeros(dims[::-1], bool)
    s[6:8, 6:8, 6:8] = True
    s[8:10, 8:10, 8:10] = True   # meets the first block at the corner (8, 8, 8) only -- also a corner of eight bricks
    sdf, cnt = state_from_mask(s.reshape(-1))
    dev = make_dev(dims)
    dev.upload(sdf, cnt)
    want, _ = check_labels(dev, sdf, cnt, 0.0, "corner contact")
    assert want["n_voxels"].tolist() == [8, 8]
    assert want["label"].tolist() == [(6 * 16 + 6) * 16 + 6, (8 * 16 + 8) * 16 + 8]


# ---- 4. degenerate ---------------------------------------------------------------------------------------------------

def test_all_solid_and_none_solid():
    dims = (9, 10, 17)
    n = dims[0] * dims[1] * dims[2]
    dev = make_dev(dims)
    sdf, cnt = state_from_mask(np.ones(n, bool))
    dev.upload(sdf, cnt)
    want, _ = check_labels(dev, sdf, cnt, 0.0, "all solid")
    assert want["label"].tolist() == [0] and want["n_voxels"].tolist() == [n]
    assert want["bb_min"].tolist() == [[0, 0, 0]] and want["bb_max"].tolist() == [[8, 9, 16]]
    sdf, cnt = state_from_mask(np.zeros(n, bool))
    dev.upload(sdf, cnt)
    got = dev.LabelComponents(0.0, labels=True)
    assert len(got["label"]) == 0 and got["bb_min"].shape == (0, 3) and (got["labels"] == -1).all()
    r = dev.KeepComponents(0.0)
    assert (r["removed_components"], r["removed_voxels"]) == (0, 0)


@pytest.mark.parametrize("how", ["init", "reset"])
def test_untouched_context(how):
    """Nothing carved since the fill: the empty list, and the context goes on exactly like one that was never asked."""
    n, nv = 24, 2
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, nv, 160, 120)
    dev, plain = vc.VoxelCarver(opt), vc.VoxelCarver(opt)
    assert dev.Init() and plain.Init(), vc.last_error()
    if how == "reset":
        for d in (dev, plain):
            assert d.CarveSilhouette(views[0], masks[0]), vc.last_error()
            d.sync()
            d.reset()
    got = dev.LabelComponents(0.0, labels=True)
    assert len(got["label"]) == 0 and (got["labels"] == -1).all()
    assert dev.KeepComponents(0.0, largest=1)["removed_voxels"] == 0
    assert dev.get_param("brick_min_valid") == plain.get_param("brick_min_valid") == 0
    for d in (dev, plain):
        assert d.CarveSilhouette(views[1], masks[1]), vc.last_error()
        d.sync()
    assert dev.get_param("brick_min_valid") == plain.get_param("brick_min_valid") == 1
    assert dev.state_diff(plain) == 0


# ---- 5. ties ---------------------------------------------------------------------------------------------------------

def two_blocks_state():
    dims = (12, 9, 10)
    s = np.zeros(dims[::-1], bool)
    s[1:4, 1:4, 1:4] = True
    s[5:8, 4:7, 7:10] = True
    return dims, state_from_mask(s.reshape(-1))


def test_ties_go_to_the_lower_label():
    dims, (sdf, cnt) = two_blocks_state()
    dev = make_dev(dims)
    dev.upload(sdf, cnt)
    want, lab = check_labels(dev, sdf, cnt, 0.0, "two blocks")
    assert want["n_voxels"].tolist() == [27, 27] and want["label"][0] < want["label"][1]
    r = dev.KeepComponents(0.0, largest=1)
    assert (r["removed_components"], r["removed_voxels"]) == (1, 27)
    s2, _ = dev.download()
    gone = lab == want["label"][1]
    assert (s2[gone] == 1.0).all() and np.array_equal(bits(s2[~gone]), bits(sdf[~gone]))


# ---- 6. counter widths -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_update,width", [(300, 2), (70000, 4)])
def test_counter_widths(max_update, width):
    n, nv = 24, 3
    uo = UpdateOption(voxel_max_update_num=max_update)
    dev = vc.VoxelCarver(synth.sphere_option(n, uo))
    assert dev.Init(), vc.last_error()
    dev.set_param("lazycount", 0)
    views, masks = synth.sphere_views(n, nv, 160, 120)
    for i in range(nv):
        assert dev.CarveSilhouette(views[i], masks[i]), vc.last_error()
    sdf, cnt = dev.download()
    assert dev.get_param("count_bytes") == width
    want, _ = check_labels(dev, sdf, cnt, 0.0, "u%d counters" % (8 * width))
    assert len(want["label"]) >= 1
    # the same with counters the library cannot take as implied by the sdf (an upload), read at this width
    cnt2 = cnt.copy()
    cnt2[::7] = 0
    dev.upload(sdf, cnt2)
    assert dev.get_param("count_bytes") == width
    check_labels(dev, sdf, cnt2, 0.0, "u%d counters, uploaded" % (8 * width))


# ---- 7. carved scenes ------------------------------------------------------------------------------------------------

_bunny = {}


def bunny_inputs():
    if not _bunny:
        _bunny["views"] = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
        _bunny["masks"] = B.load_masks()
    return _bunny["views"], _bunny["masks"]


def carve_bunny(res, mode, nv, defer=1, sync=True):
    views, masks = bunny_inputs()
    dev = vc.VoxelCarver(B.bunny_option(res, UpdateOption(**B.MODES[mode])))
    assert dev.Init(), vc.last_error()
    dev.set_param("defer", defer)
    for i in range(nv):
        assert dev.CarveSilhouette(views[i], masks[i]), vc.last_error()
    if sync:
        dev.sync()
    return dev


_ref_cache = {}


def bunny_reference(key, dev):
    """(sdf, cnt, components, labels) of a carved bunny state, computed once per (res, mode, views)."""
    if key not in _ref_cache:
        sdf, cnt = dev.download()
        comps, lab = R.reference(sdf, cnt, dev.dims, 0.0)
        for a in (sdf, cnt, lab):
            a.setflags(write=False)
        _ref_cache[key] = (sdf, cnt, comps, lab)
    return _ref_cache[key]


BUNNY_STATES = list(itertools.product((10.0, 2.5), ("default", "tsdf"), (2, 6)))


@pytest.mark.parametrize("defer", [1, 0])
@pytest.mark.parametrize("res,mode,nv", BUNNY_STATES)
def test_bunny(res, mode, nv, defer):
    # "defer" 1: the call comes right behind CarveSilhouette, no sync -- the queued views have to be applied first
    dev = carve_bunny(res, mode, nv, defer, sync=False)
    got = dev.LabelComponents(0.0, labels=True)
    sdf, cnt, want, want_lab = bunny_reference((res, mode, nv), dev)
    s2, c2 = dev.download()
    assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt)
    R.assert_components_equal(got, want, "bunny")
    assert np.array_equal(got["labels"], want_lab)
    assert want["n_voxels"][0] > 1000


# ---- 8. filter exactness ---------------------------------------------------------------------------------------------

def assert_mesh_equal(a, b, ctx):
    for k in ("vertices", "faces", "keys"):
        assert a[k].shape == b[k].shape, "%s %s: %s against %s" % (ctx, k, a[k].shape, b[k].shape)
    assert np.array_equal(bits(a["vertices"]), bits(b["vertices"])), ctx + " vertex bits"
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["keys"], b["keys"]), ctx + " faces / keys"
    if "normals" in a:
        assert np.array_equal(bits(a["normals"]), bits(b["normals"])), ctx + " vertex normals"
        assert np.array_equal(bits(a["face_normals"]), bits(b["face_normals"])), ctx + " face normals"


CARVE_PATHS = [(1, 1), (1, 0), (0, 1), (0, 0)]  # ("fused", "cull")


def check_filter(dev, other, sdf, cnt, iso, rule, views, masks, rot, was_valid, full_voxel_mesh, fill=1.0):
    """`dev` holds (sdf, cnt); `other` is a second context of the same options that gets the numpy-filtered state."""
    comps, lab = R.reference(sdf, cnt, dev.dims, iso)
    want_sdf, gone, want_nc, want_nv = R.filter_state(sdf, lab, comps, fill_sdf=fill, **rule)
    assert dev.get_param("brick_min_valid") == was_valid
    r = dev.KeepComponents(iso, fill_sdf=fill, **rule)
    assert (r["removed_components"], r["removed_voxels"]) == (want_nc, want_nv)
    assert dev.get_param("brick_min_valid") == was_valid
    assert np.array_equal(dev.download_labels(), lab), "download_labels is not the labelling before the removal"
    s2, c2 = dev.download()
    assert np.array_equal(c2, cnt), "update_num changed"
    changed = bits(s2) != bits(sdf)
    assert not (changed & ~gone).any(), "a voxel outside the removed components changed"
    assert (bits(s2[gone]) == bits(np.float32(fill))).all(), "a removed voxel does not hold fill_sdf"
    assert np.array_equal(bits(s2), bits(want_sdf))
    keep = R.kept(comps, **rule)
    after = dev.LabelComponents(iso, labels=True)
    R.assert_components_equal(after, R.subset(comps, keep), "labelling after the filter")
    assert np.array_equal(after["labels"], np.where(gone, -1, lab))
    # every reader of the state, against a context that got the filtered state from outside
    other.upload(want_sdf, cnt)
    for skip in (0, 2):
        dev.set_param("mcskip", skip)
        other.set_param("mcskip", skip)
        for normals in (False, True):
            assert_mesh_equal(dev.ExtractIsoSurface(iso, True, normals=normals),
                              other.ExtractIsoSurface(iso, True, normals=normals), "mcskip %d normals %s" % (skip, normals))
    for inside_empty in (True, False):
        if inside_empty or full_voxel_mesh:
            a, b = dev.ExtractVoxel(inside_empty), other.ExtractVoxel(inside_empty)
            assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(bits(a["vertices"]), bits(b["vertices"]))
        else:  # (a million cubes: the kept voxels are compared, of which the cubes are a host-side function)
            assert np.array_equal(dev.extract_voxel_ids(inside_empty), other.extract_voxel_ids(inside_empty))
    # one more view through every carve path; the first one is the one that meets the recomputed minima
    for k in range(4):
        fused, cull = CARVE_PATHS[(k + rot) % 4]
        for d in (dev, other):
            d.set_param("fused", fused)
            d.set_param("cull", cull)
            assert d.CarveSilhouette(views[k % len(views)], masks[k % len(views)]), vc.last_error()
            d.sync()
        assert dev.state_diff(other) == 0, "fused %d cull %d" % (fused, cull)


@pytest.mark.parametrize("rule", range(3))
@pytest.mark.parametrize("dims", [(9, 10, 17), (70, 23, 19)], ids=lambda d: "%dx%dx%d" % d)
def test_filter_random(dims, rule):
    iso = 0.0125
    sdf, cnt = random_state(dims, 0.31, iso, 7)
    dev, other = make_dev(dims), make_dev(dims)
    dev.upload(sdf, cnt)
    views, masks = synth.sphere_views(max(dims), 2, 160, 120)
    check_filter(dev, other, sdf, cnt, iso, KEEP_RULES[rule], views, masks, rule, 0, True, fill=0.75)


@pytest.mark.parametrize("rule", range(3))
def test_filter_ties(rule):
    dims, (sdf, cnt) = two_blocks_state()
    dev, other = make_dev(dims), make_dev(dims)
    dev.upload(sdf, cnt)
    views, masks = synth.sphere_views(max(dims), 2, 160, 120)
    check_filter(dev, other, sdf, cnt, 0.0, KEEP_RULES[rule], views, masks, rule, 0, True)


@pytest.mark.parametrize("rule", range(3))
@pytest.mark.parametrize("res,mode,nv", BUNNY_STATES)
def test_filter_bunny(res, mode, nv, rule):
    dev = carve_bunny(res, mode, nv)
    sdf, cnt, _, _ = bunny_reference((res, mode, nv), dev)
    other = vc.VoxelCarver(dev.option)
    assert other.Init(), vc.last_error()
    views, masks = bunny_inputs()
    views, masks = views[2:4], masks[2:4]
    # a carved scene: the brick minima were valid, and have to be afterwards (the brick-skipping extraction and the
    # carve inside check_filter are the proof that they are also right)
    check_filter(dev, other, sdf, cnt, 0.0, KEEP_RULES[rule], views, masks, rule, 1, res >= 10.0)


# ---- 9. the mesh belongs to what was kept ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["default", "tsdf"])
def test_mesh_of_the_kept_component(mode):
    dev = carve_bunny(10.0, mode, 2)
    dev.set_param("meshkeys", 1)
    sdf, cnt, comps, lab = bunny_reference((10.0, mode, 2), dev)
    assert len(comps["label"]) >= 2, "the scene has no floater to remove"
    before = dev.ExtractIsoSurface(0.0, True)
    dev.KeepComponents(0.0, largest=1)
    m = dev.ExtractIsoSurface(0.0, True)
    assert 0 < len(m["vertices"]) < len(before["vertices"])
    solid = lab >= 0
    ka, kb = m["keys"][:, 0], m["keys"][:, 1]
    assert (solid[ka] != solid[kb]).all(), "an edge with a vertex has exactly one solid end"
    inside = np.where(solid[ka], ka, kb)
    assert (lab[inside] == comps["label"][0]).all()


# ---- 10. errors ------------------------------------------------------------------------------------------------------

def test_slab_context_is_unsupported():
    n = 24
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, 1, 160, 120)
    dev = vc.VoxelCarver(opt, z_range=(8, 24))
    assert dev.Init(), vc.last_error()
    assert dev.CarveSilhouette(views[0], masks[0]), vc.last_error()
    sdf, cnt = dev.download()
    lib = capi.load()
    p, k = C.POINTER(capi.Component)(), C.c_int64(5)
    assert lib.vcy_label_components(dev.ctx, 0.0, C.byref(p), C.byref(k)) == capi.VCY_ERR_UNSUPPORTED
    assert k.value == 0 and not p
    a, b = C.c_int64(5), C.c_int64(5)
    assert lib.vcy_keep_components(dev.ctx, 0.0, 1, 0, 1.0, C.byref(a), C.byref(b)) == capi.VCY_ERR_UNSUPPORTED
    assert "whole grid" in vc.last_error()
    s2, c2 = dev.download()
    assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt)


def test_fill_and_label_argument_errors():
    dims, (sdf, cnt) = two_blocks_state()
    dev = make_dev(dims)
    dev.upload(sdf, cnt)
    lib = capi.load()
    lab = np.empty(sdf.size, np.int64)
    assert lib.vcy_download_labels(dev.ctx, lab.ctypes.data_as(C.c_void_p)) == capi.VCY_ERR_INVALID_ARG
    for iso, fill in ((0.0, -0.25), (0.5, 0.25), (0.0, float("nan")), (0.0, float("inf")), (0.0, float("-inf"))):
        a, b = C.c_int64(5), C.c_int64(5)
        rc = lib.vcy_keep_components(dev.ctx, iso, 1, 0, fill, C.byref(a), C.byref(b))
        assert rc == capi.VCY_ERR_INVALID_ARG, (iso, fill)
        with pytest.raises(RuntimeError):
            dev.KeepComponents(iso, fill_sdf=fill)
    s2, c2 = dev.download()
    assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt)
    # fill_sdf == iso_level is allowed: not below it
    assert dev.KeepComponents(0.0, largest=1, fill_sdf=0.0)["removed_components"] == 1


# ---- 11. one larger grid ---------------------------------------------------------------------------------------------

def test_256_balls_bridge_and_specks():
    n = 256
    z, y, x = np.ogrid[0:n, 0:n, 0:n]

    def ball(c, r):
        return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r * r

    rc = 25                                  # smaller than a and b together: the joined pair is the largest component
    a, b, c = ball((60, 60, 60), 30), ball((180, 60, 60), 20), ball((128, 190, 170), rc)
    bridge = np.zeros((n, n, n), bool)
    bridge[60, 60, 90:161] = True           # (x from ball a's rim at 90 to ball b's at 160, across words and bricks)
    specks = np.zeros((n, n, n), bool)
    rng = np.random.RandomState(3)
    ids = []
    while len(ids) < 50:                     # isolated voxels in the empty slab z >= 230, two apart at least
        p = (int(rng.randint(230, 256)), int(rng.randint(0, 256)), int(rng.randint(0, 256)))
        if all(abs(p[0] - q[0]) + abs(p[1] - q[1]) + abs(p[2] - q[2]) > 1 for q in ids):
            ids.append(p)
            specks[p] = True
    joined = a | b | bridge
    solid = joined | c | specks
    assert not (joined & c).any() and c[:230].sum() == c.sum() and joined.sum() > c.sum() > 1
    sdf, cnt = state_from_mask(solid.reshape(-1))
    dev = make_dev((n, n, n))
    dev.upload(sdf, cnt)
    got = dev.LabelComponents(0.0)
    assert len(got["label"]) == 52
    assert got["n_voxels"][:2].tolist() == [int(joined.sum()), int(c.sum())]
    assert (got["n_voxels"][2:] == 1).all() and (np.diff(got["label"][2:]) > 0).all()
    assert got["label"][0] == int(np.flatnonzero(joined.reshape(-1))[0])
    assert got["bb_min"][0].tolist() == [30, 30, 30] and got["bb_max"][0].tolist() == [200, 90, 90]
    assert got["bb_min"][1].tolist() == [128 - rc, 190 - rc, 170 - rc]
    assert got["bb_max"][1].tolist() == [128 + rc, 190 + rc, 170 + rc]
    r = dev.KeepComponents(0.0, largest=1)
    assert (r["removed_components"], r["removed_voxels"]) == (51, int(c.sum()) + 50)
    after = dev.LabelComponents(0.0)
    assert after["n_voxels"].tolist() == [int(joined.sum())]
    s2, _ = dev.download()
    assert np.array_equal(s2 < 0, joined.reshape(-1))
