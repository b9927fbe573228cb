"""The distance field of the hull on the device (vcy_distance_field / vcy_redistance, distance.hip) against the numpy
restatement of its definition (tests/distance_ref.py).  Squared voxel distances are integers and phi is one float per
integer, so every assertion is EQUALITY -- float bits compared as uint32: of the signed field, of the state Redistance
leaves, and, behind the writer, of everything every reader of the state returns (marching cubes with and without brick
skipping and normals, the labelling, the ray-cast with its cached bit planes, ExtractVoxel, one more carve)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import distance_cases as K
import distance_ref as R
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import sharded as vs
from vacancy_amd import synth
from vacancy_amd.capi import UpdateOption

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_dev(dims, uo=None, resolution=1.0, z_range=None):
    dev = vc.VoxelCarver(K.box_option(dims, uo, resolution), z_range=z_range)
    assert dev.Init(), vc.last_error()
    assert dev.dims == tuple(dims), (dev.dims, dims)
    return dev


def check_case(dev, case, resolution=1.0):
    """Uploads the case, compares DistanceField and the state after Redistance with the reference; returns the field."""
    name, dims, sdf, cnt, iso, radius = case
    ctx = "%s %s" % (name, dims)
    want_d2, want_sdf = K.reference_of(case, resolution)
    dev.upload(sdf, cnt)
    d2 = dev.DistanceField(iso, radius)
    assert np.array_equal(d2, want_d2), "%s: %d field values differ" % (ctx, (d2 != want_d2).sum())
    s1, c1 = dev.download()
    assert np.array_equal(bits(s1), bits(sdf)) and np.array_equal(c1, cnt), ctx + ": DistanceField changed the state"
    r = dev.Redistance(iso, radius)
    s2, c2 = dev.download()
    assert np.array_equal(c2, cnt), ctx + ": update_num changed"
    untouched = cnt == 0
    assert np.array_equal(bits(s2[untouched]), bits(sdf[untouched])), ctx + ": an untouched voxel changed"
    bad = bits(s2) != bits(want_sdf)
    assert not bad.any(), "%s: the sdf bits of %d voxels differ" % (ctx, bad.sum())
    assert r["rewritten"] == int((cnt >= 1).sum()) and r["device_ms"] > 0.0
    return d2


# ---- 1. random states on awkward dims --------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", K.RANDOM_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_random_states(dims):
    dev = make_dev(dims)
    for case in K.random_cases(dims):
        d2 = check_case(dev, case)
        far = R.far_of(case[5])
        assert (np.abs(d2) < far).any()
        if "one voxel" in case[0]:
            assert (d2 == 127 * 127).any() and (d2 == far).any()


# ---- 2. named cases ------------------------------------------------------------------------------------------------------

NAMED = K.named_cases()


@pytest.mark.parametrize("k", range(len(NAMED)), ids=[c[0].replace(" ", "_") for c in NAMED])
def test_named(k):
    case = NAMED[k]
    d2 = check_case(make_dev(case[1]), case)
    far = R.far_of(case[5])
    if case[0] == "nothing solid":
        assert (d2 == far).all()
    if case[0] in ("everything solid", "65 wide, all solid"):  # (the padding bits of the second word are no features)
        assert (d2 == -far).all()
    if case[0] == "one solid voxel":
        assert (np.abs(d2) < far).any() and (d2 == far).any() and (d2 < 0).sum() == 1
    if case[0] == "slab at x = 0":  # the border is not a feature
        f = d2.reshape(9, 10, 17)
        assert (f[:, :, 0] == -far).all() and (f[:, :, 5] == -1).all() and (f[:, :, 6] == 1).all()


def test_resolution_that_rounds():
    case = NAMED[2]
    check_case(make_dev(case[1], resolution=0.375), case, resolution=0.375)
    want = K.reference_of(case, 0.375)[1]
    assert np.float32(0.5 * 0.375) in np.abs(want) and len(np.unique(want)) > 6


@pytest.mark.parametrize("top,width", [(3, 1), (300, 2), (66000, 4)])
def test_counter_widths(top, width):
    dims = (70, 23, 19)
    sdf, cnt = K.random_state(dims, 0.3, 0.0, 77)
    cnt = cnt.copy()
    cnt[np.nonzero(cnt)[0][::5]] = top
    dev = make_dev(dims, UpdateOption(voxel_max_update_num=70000))
    check_case(dev, ("u%d counters" % (8 * width), dims, sdf, cnt, 0.0, 3))
    assert dev.get_param("count_bytes") == width


# ---- 3. the writer against every reader ------------------------------------------------------------------------------------

def assert_mesh_equal(a, b, ctx):
    for k in ("vertices", "faces", "keys", "normals", "face_normals"):
        assert a[k].shape == b[k].shape, "%s %s: %s against %s" % (ctx, k, a[k].shape, b[k].shape)
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["keys"], b["keys"]), ctx + " faces / keys"
    for k in ("vertices", "normals", "face_normals"):
        assert np.array_equal(bits(a[k]), bits(b[k])), "%s %s bits" % (ctx, k)


def test_writer_against_every_reader():
    dims, res, radius = (70, 23, 19), 1.0, 3
    sdf, cnt = K.random_state(dims, 0.2, 0.0, 9)
    case = ("readers", dims, sdf, cnt, 0.0, radius)
    _, want_sdf = K.reference_of(case, res)
    a, b = make_dev(dims), make_dev(dims)
    views, masks = synth.sphere_views(max(dims), 2, 160, 120)
    a.upload(sdf, cnt)
    # the ray-cast first, at an iso level where the OLD field has other solid voxels: its bit planes are cached
    old = a.RenderHull(views[:1], 1.0)[0]["depth"]
    a.Redistance(0.0, radius)
    assert a.get_param("brick_min_valid") == 0  # the declared row: minima lost
    b.upload(np.array(want_sdf), cnt)
    assert a.state_diff(b) == 0
    new_a, new_b = a.RenderHull(views[:1], 1.0)[0]["depth"], b.RenderHull(views[:1], 1.0)[0]["depth"]
    assert np.array_equal(bits(new_a), bits(new_b)), "the bit planes of the old field were used"
    assert not np.array_equal(bits(new_a), bits(old)), "the case does not tell the two fields apart"
    for iso in (-0.7 * res, 0.0, 0.7 * res):
        for skip in (1, 0):
            a.set_param("mcskip", skip)
            b.set_param("mcskip", skip)
            ma, mb = a.ExtractIsoSurface(iso, True, normals=True), b.ExtractIsoSurface(iso, True, normals=True)
            assert_mesh_equal(ma, mb, "iso %g mcskip %d" % (iso, skip))
            assert len(ma["vertices"]) > 100
    la, lb = a.LabelComponents(0.0, labels=True), b.LabelComponents(0.0, labels=True)
    for k in ("label", "n_voxels", "bb_min", "bb_max", "labels"):
        assert np.array_equal(la[k], lb[k]), k
    assert len(la["label"]) > 0
    for inside_empty in (True, False):
        va, vb = a.ExtractVoxel(inside_empty), b.ExtractVoxel(inside_empty)
        assert np.array_equal(va["faces"], vb["faces"]) and np.array_equal(bits(va["vertices"]), bits(vb["vertices"]))
    # one more fused kMax carve, through the live list
    for d in (a, b):
        d.set_param("fused", 1)
        d.set_param("livelist", 1)
        assert d.CarveSilhouette(views[1], masks[1]), vc.last_error()
        d.sync()
    assert a.state_diff(b) == 0


def test_redistance_after_a_carve_keeps_later_carves_exact():
    """A carved scene (valid brick minima before, lost after), then another view: equal to a context that got the
    redistanced state from outside."""
    n = 24
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, 3, 160, 120)
    a, b = vc.VoxelCarver(opt), vc.VoxelCarver(opt)
    assert a.Init() and b.Init(), vc.last_error()
    for i in range(2):
        assert a.CarveSilhouette(views[i], masks[i]), vc.last_error()
    a.sync()
    assert a.get_param("brick_min_valid") == 1
    sdf, cnt = a.download()
    want_d2, want_sdf = R.reference(sdf, cnt, a.dims, 0.0, 5, opt.resolution)
    assert np.array_equal(a.DistanceField(0.0, 5), want_d2)
    assert a.get_param("brick_min_valid") == 1  # a reader declares nothing
    assert a.Redistance(0.0, 5)["rewritten"] == int((cnt >= 1).sum())
    assert a.get_param("brick_min_valid") == 0
    s2, c2 = a.download()
    assert np.array_equal(bits(s2), bits(want_sdf)) and np.array_equal(c2, cnt)
    b.upload(want_sdf, cnt)
    for d in (a, b):
        assert d.CarveSilhouette(views[2], masks[2]), vc.last_error()
        d.sync()
    assert a.state_diff(b) == 0


# ---- 4. refusals, the fresh context ------------------------------------------------------------------------------------------

def test_radius_out_of_range():
    name, dims, sdf, cnt, iso, _ = NAMED[2]
    dev = make_dev(dims)
    dev.upload(sdf, cnt)
    lib = capi.load()
    d2 = np.full(sdf.size, 7, np.int32)
    for radius in (0, 128):
        n = C.c_int64(5)
        assert lib.vcy_distance_field(dev.ctx, 0.0, radius, d2.ctypes.data) == capi.VCY_ERR_INVALID_ARG
        assert "radius" in vc.last_error() and (d2 == 7).all()
        assert lib.vcy_redistance(dev.ctx, 0.0, radius, C.byref(n)) == capi.VCY_ERR_INVALID_ARG
        assert n.value == 0
        with pytest.raises(RuntimeError):
            dev.Redistance(0.0, radius)
    s2, c2 = dev.download()
    assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt)


def test_slab_context_is_unsupported():
    n = 24
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, 1, 160, 120)
    dev, twin = vc.VoxelCarver(opt, z_range=(8, 24)), vc.VoxelCarver(opt, z_range=(8, 24))
    assert dev.Init() and twin.Init(), vc.last_error()
    for d in (dev, twin):
        assert d.CarveSilhouette(views[0], masks[0]), vc.last_error()
        d.sync()
    lib = capi.load()
    d2 = np.full(dev.slab_voxels, 7, np.int32)
    k = C.c_int64(5)
    assert lib.vcy_distance_field(dev.ctx, 0.0, 3, d2.ctypes.data) == capi.VCY_ERR_UNSUPPORTED
    assert "whole grid" in vc.last_error() and (d2 == 7).all()
    assert lib.vcy_redistance(dev.ctx, 0.0, 3, C.byref(k)) == capi.VCY_ERR_UNSUPPORTED
    assert "whole grid" in vc.last_error() and k.value == 0
    assert dev.state_diff(twin) == 0


def test_fresh_context():
    n = 24
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, 1, 160, 120)
    dev, plain = vc.VoxelCarver(opt), vc.VoxelCarver(opt)
    assert dev.Init() and plain.Init(), vc.last_error()
    assert (dev.DistanceField(0.0, 5) == 26).all()
    r = dev.Redistance(0.0, 5)
    assert r["rewritten"] == 0 and r["device_ms"] == 0.0
    assert dev.get_param("brick_min_valid") == plain.get_param("brick_min_valid") == 0
    for d in (dev, plain):
        assert d.CarveSilhouette(views[0], masks[0]), vc.last_error()
        d.sync()
    assert dev.get_param("brick_min_valid") == plain.get_param("brick_min_valid") == 1
    assert dev.state_diff(plain) == 0


# ---- 5. the closing ------------------------------------------------------------------------------------------------------

def test_close_hull():
    sdf, cnt, dims, gap = R.two_blocks()
    dev = make_dev(dims)
    dev.upload(sdf, cnt)
    steps = dev.CloseHull(1.3)
    assert [s["rewritten"] for s in steps] == [sdf.size] * 3
    want = R.close_hull(sdf, cnt, dims, 1.3)
    s2, c2 = dev.download()
    assert np.array_equal(bits(s2), bits(want)) and np.array_equal(c2, cnt)
    solid = R.solid_mask(s2, c2, 0.0)
    assert solid.sum() == 300 and np.array_equal(solid, R.solid_mask(sdf, cnt, 0.0) | gap)
    assert (dev.DistanceField(0.0, 1) < 0).sum() == 300
    with pytest.raises(ValueError):
        dev.CloseHull(1.5)
    s3, _ = dev.download()
    assert np.array_equal(bits(s3), bits(s2)), "the refused radius changed the state"


def test_sharded_carver_one_slab_only():
    sdf, cnt, dims, gap = R.two_blocks()
    opt = K.box_option(dims)
    one = vs.ShardedVoxelCarver(opt, [0], 1)
    assert one.Init(), vc.last_error()
    one.slabs[0].upload(sdf, cnt)
    want_d2, _ = R.reference(sdf, cnt, dims, 0.0, 4)
    assert np.array_equal(one.DistanceField(0.0, 4), want_d2)
    one.CloseHull(1.3)
    assert np.array_equal(bits(one.slabs[0].download()[0]), bits(R.close_hull(sdf, cnt, dims, 1.3)))
    two = vs.ShardedVoxelCarver(opt, [0], 2)
    assert two.Init(), vc.last_error()
    for call in (lambda: two.DistanceField(0.0, 4), lambda: two.Redistance(0.0, 4), lambda: two.CloseHull(1.3)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "whole grid in one context" in str(e.value)
    one.close()
    two.close()


# ---- 6. the C++ layer ------------------------------------------------------------------------------------------------------

def test_bunny_example_offsets_what_python_offsets(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "--redistance", "4", "--offset", "2.0"],
                         check=True, capture_output=True, text=True)
    row = [l.split() for l in run.stdout.splitlines() if l.startswith("REDISTANCE")]
    assert len(row) == 1, run.stdout
    # REDISTANCE radius <R> offset <mm> verts <n> faces <m>
    assert row[0][1:6:2] == ["radius", "offset", "verts"] and row[0][2] == "4" and float(row[0][4]) == 2.0, row
    ply = tmp_path / "surface_offset.ply"
    assert ply.exists() and ply.stat().st_size > 1000

    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    masks = B.load_masks()
    dev = vc.VoxelCarver(B.bunny_option(10.0))
    assert dev.Init(), vc.last_error()
    for v, m in zip(views, masks):
        assert dev.CarveSilhouette(v, m), vc.last_error()
    hull = dev.ExtractIsoSurface(0.0, True)
    dev.Redistance(0.0, 4)
    grown = dev.ExtractIsoSurface(2.0, True)
    assert int(row[0][6]) == len(grown["vertices"]) and int(row[0][8]) == len(grown["faces"])
    # (2 mm is less than half a voxel: the surface moves along the edges it already crosses)
    assert len(grown["vertices"]) > 1000 and not np.array_equal(bits(grown["vertices"]), bits(hull["vertices"]))
    header = open(str(ply), "rb").read(400).decode("ascii", "replace")
    assert "element vertex %d" % len(grown["vertices"]) in header
