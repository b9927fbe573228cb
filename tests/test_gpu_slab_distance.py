"""The distance field of the hull across z-slabs on the device (vcy_distance_slab_begin / _planes, vcy_distance_field_slab,
vcy_redistance_slab; the composition of vacancy_amd.dist and the members of ShardedVoxelCarver) against the WHOLE grid's
reference (tests/distance_ref.py through distance_cases.reference_of).  One device; the slabs are contexts with a z_range.
Squared voxel distances are integers and phi is one float per integer, so every assertion is EQUALITY -- float bits
compared as uint32: of the planes against the host half, of the slabs' fields and states put together against the
reference, and, behind the writer, of what the readers of the state return against a whole-grid context after Redistance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import distance_cases as K
import distance_ref as R
import slab_distance_cases as S
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist
from vacancy_amd import sharded as vs
from vacancy_amd import synth
from vacancy_amd.capi import UpdateOption

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_slabs(dims, bounds, uo=None, resolution=1.0):
    opt = K.box_option(dims, uo, resolution)
    out = []
    for z in zip(bounds[:-1], bounds[1:]):
        dev = vc.VoxelCarver(opt, z_range=z)
        assert dev.Init(), vc.last_error()
        assert dev.dims == tuple(dims) and dev.z_range == z, (dev.dims, dev.z_range)
        out.append(dev)
    return out


def upload(slabs, dims, sdf, cnt):
    for dev in slabs:
        dev.upload(S.slab_of(sdf, dims, *dev.z_range), S.slab_of(cnt, dims, *dev.z_range))


def download(slabs):
    parts = [dev.download() for dev in slabs]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def check_case(slabs, case, resolution=1.0):
    """Uploads the case into the slabs; the slabs' fields and their states after the rewrite, put together, against the
    whole grid's reference.  Returns the field."""
    name, dims, sdf, cnt, iso, radius = case
    ctx = "%s %s cut %s" % (name, dims, [dev.z_range for dev in slabs])
    want_d2, want_sdf = K.reference_of(case, resolution)
    upload(slabs, dims, sdf, cnt)
    r = vdist.distance_field_slabs(slabs, 0, 1, iso, radius)
    d2 = np.concatenate(r["fields"])
    assert np.array_equal(d2, want_d2), "%s: %d field values differ" % (ctx, (d2 != want_d2).sum())
    s1, c1 = download(slabs)
    assert np.array_equal(bits(s1), bits(sdf)) and np.array_equal(c1, cnt), ctx + ": the field changed the state"
    w = vdist.redistance_slabs(slabs, 0, 1, iso, radius)
    s2, c2 = download(slabs)
    assert np.array_equal(c2, cnt), ctx + ": update_num changed"
    bad = bits(s2) != bits(want_sdf)
    assert not bad.any(), "%s: the sdf bits of %d voxels differ" % (ctx, bad.sum())
    sl = dims[0] * dims[1]
    assert w["rewritten"] == [int((cnt[z0 * sl:z1 * sl] >= 1).sum()) for z0, z1 in (dev.z_range for dev in slabs)], ctx
    assert r["device_ms"] > 0.0 and w["device_ms"] > 0.0
    seams = len(slabs) - 1
    assert (r["plane_bytes"] > 0) == (seams > 0) and r["plane_bytes"] <= 2 * seams * 2 * sl * radius
    return d2


# ---- 1. the planes against the host half ---------------------------------------------------------------------------------

def test_planes_equal_the_host_half():
    dims = (70, 23, 19)
    slabs = make_slabs(dims, [0, 2, 10, 19])
    for case in K.random_cases(dims):
        name, _, sdf, cnt, iso, radius = case
        upload(slabs, dims, sdf, cnt)
        for dev in slabs:
            z0, z1 = dev.z_range
            assert dev.DistanceSlabBegin(iso, radius) > 0.0
            want = vc.distance_slab_planes_host(dev.option, dev.z_range, S.slab_of(sdf, dims, z0, z1),
                                                S.slab_of(cnt, dims, z0, z1), iso, radius)
            assert np.array_equal(dev.DistanceSlabPlanes(z0, z1), want), (name, z0, z1)
            assert np.array_equal(dev.DistanceSlabPlanes(z1 - 1, z1), want[-1:]) and len(dev.DistanceSlabPlanes(z0, z0)) == 0
            for bad in ((z0 - 1, z1), (z0, z1 + 1), (z1, z0)):
                with pytest.raises(RuntimeError) as e:
                    dev.DistanceSlabPlanes(*bad)
                assert e.value.rc == capi.VCY_ERR_INVALID_ARG


# ---- 2. the cases of the CPU test under every cut ------------------------------------------------------------------------

NAMED = K.named_cases()
NAMED_DIMS = sorted({c[1] for c in NAMED})


@pytest.mark.parametrize("dims", NAMED_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_named(dims):
    for bounds in S.cuts_of(dims[2]):
        slabs = make_slabs(dims, bounds)
        for case in NAMED:
            if case[1] == dims:
                check_case(slabs, case)


@pytest.mark.parametrize("dims", S.SLAB_RANDOM_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_random_states(dims):
    for bounds in S.cuts_of(dims[2]):
        slabs = make_slabs(dims, bounds)
        for case in K.random_cases(dims):
            d2 = check_case(slabs, case)
            assert (np.abs(d2) < R.far_of(case[5])).any()


def test_resolution_that_rounds():
    case = NAMED[2]
    check_case(make_slabs(case[1], [0, 2, 7, 9], resolution=0.375), case, resolution=0.375)


def test_whole_grid_context_runs_the_slab_calls():
    case = NAMED[5]
    name, dims, sdf, cnt, iso, radius = case
    d2 = check_case(make_slabs(dims, [0, dims[2]]), case)
    whole = make_slabs(dims, [0, dims[2]])[0]
    whole.upload(sdf, cnt)
    assert np.array_equal(whole.DistanceField(iso, radius), d2)


# ---- 3. shapes at which the windowed z pass takes another path -------------------------------------------------------------

# (dims, the cut, R): the window crosses a 64-slice tile and x has a partial second tile; the 128-slice tile with an
# extended column longer than 128; a slab thinner than R in a thin grid
EXTRA = [((70, 9, 150), 70, 4), ((70, 9, 140), 50, 40), ((130, 7, 5), 2, 12)]


@pytest.mark.parametrize("dims,cut,radius", EXTRA, ids=lambda v: str(v))
def test_extra_shapes(dims, cut, radius):
    # sparse, so that the distances are long: they reach across the seam
    sdf, cnt = K.random_state(dims, {4: 0.05, 12: 0.02, 40: 0.0003}[radius], 0.0, 300 + radius)
    d2 = check_case(make_slabs(dims, [0, cut, dims[2]]), ("extra shape R %d" % radius, dims, sdf, cnt, 0.0, radius))
    assert (np.abs(d2) < R.far_of(radius)).any() and (np.abs(d2) > 4).any()


def test_the_largest_distance_across_a_seam():
    dims = (5, 7, 130)
    case = [c for c in K.random_cases(dims) if "one voxel" in c[0]][0]
    assert case[5] == 127
    d2 = check_case(make_slabs(dims, [0, 64, 130]), case)
    upper = d2.reshape(130, 7, 5)[64:]
    assert (upper == 127 * 127).any() and (upper == R.far_of(127)).any() and (d2 < 0).sum() == 1


@pytest.mark.parametrize("top,width", [(3, 1), (300, 2), (66000, 4)])
def test_counter_widths(top, width):
    dims = (70, 23, 19)
    sdf, cnt = K.random_state(dims, 0.3, 0.0, 77)
    cnt = cnt.copy()
    cnt[np.nonzero(cnt)[0][::5]] = top
    slabs = make_slabs(dims, [0, 2, 11, 19], UpdateOption(voxel_max_update_num=70000))
    check_case(slabs, ("u%d counters" % (8 * width), dims, sdf, cnt, 0.0, 3))
    assert [dev.get_param("count_bytes") for dev in slabs] == [width] * 3


# ---- 4. a fresh slab beside a carved one ------------------------------------------------------------------------------------

def test_fresh_slab_beside_a_carved_one():
    dims, iso, radius = (24, 24, 24), 0.0, 5
    sdf, cnt = K.random_state(dims, 0.3, iso, 11)
    sl = dims[0] * dims[1]
    sdf[:12 * sl], cnt[:12 * sl] = K.LOWEST, 0  # what the fresh slab holds
    want_d2, want_sdf = R.reference(sdf, cnt, dims, iso, radius)
    fresh, carved = make_slabs(dims, [0, 12, 24])
    plain = make_slabs(dims, [0, 12, 24])[0]
    carved.upload(sdf[12 * sl:], cnt[12 * sl:])
    assert fresh.get_param("fresh") == 1 and carved.get_param("fresh") == 0
    r = vdist.distance_field_slabs([fresh, carved], 0, 1, iso, radius)
    assert np.array_equal(np.concatenate(r["fields"]), want_d2)
    assert (r["fields"][0] < R.far_of(radius)).any(), "the fresh slab does not see its neighbour's solid voxels"
    assert (r["fields"][0] > 0).all() and fresh.get_param("fresh") == 1
    # alone, a fresh slab is FAR everywhere
    fresh.DistanceSlabBegin(iso, radius)
    assert (fresh.DistanceSlabPlanes(0, 12) == R.far_of(radius)).all()
    w = vdist.redistance_slabs([fresh, carved], 0, 1, iso, radius)
    assert w["rewritten"] == [0, int((cnt[12 * sl:] >= 1).sum())]
    # (the writer ended the carved slab's tag; the fresh slab wrote nothing and its tag still stands)
    assert fresh.RedistanceSlab(None, np.zeros((radius, sl), np.uint16)) == {"rewritten": 0, "device_ms": 0.0}
    assert fresh.get_param("fresh") == 1 and fresh.get_param("brick_min_valid") == plain.get_param("brick_min_valid") == 0
    assert np.array_equal(bits(carved.download()[0]), bits(want_sdf[12 * sl:]))
    # the lazy fill has survived: one view carved into it and into a context nothing has touched give equal states
    views, masks = synth.sphere_views(24, 1, 160, 120)
    for d in (fresh, plain):
        assert d.CarveSilhouette(views[0], masks[0]), vc.last_error()
        d.sync()
    assert fresh.get_param("brick_min_valid") == plain.get_param("brick_min_valid")
    assert fresh.state_diff(plain) == 0


# ---- 5. the tag and the refusals ------------------------------------------------------------------------------------------

def refused(call):
    with pytest.raises(RuntimeError) as e:
        call()
    assert e.value.rc == capi.VCY_ERR_INVALID_ARG, str(e.value)
    return str(e.value)


def test_tag_and_refusals():
    dims, iso = (9, 10, 17), 0.0
    sdf, cnt = K.random_state(dims, 0.3, iso, 21)
    sl = dims[0] * dims[1]
    lower, dev = make_slabs(dims, [0, 8, 17])
    twin = make_slabs(dims, [0, 8, 17])[1]
    upload([lower, dev], dims, sdf, cnt)
    twin.upload(sdf[8 * sl:], cnt[8 * sl:])
    planes = lambda n: np.zeros((n, sl), np.uint16)  # noqa: E731
    # nothing begun yet
    assert "vcy_distance_slab_begin" in refused(lambda: dev.DistanceSlabPlanes(8, 17))
    refused(lambda: dev.DistanceFieldSlab(planes(3), None))
    refused(lambda: dev.RedistanceSlab(planes(3), None))
    for radius in (0, 128):
        assert "radius" in refused(lambda: dev.DistanceSlabBegin(iso, radius))
    # a wrong number of planes
    dev.DistanceSlabBegin(iso, 3)
    for below, above in ((planes(2), None), (planes(4), None), (None, None), (planes(3), planes(1))):
        assert "planes" in refused(lambda: dev.DistanceFieldSlab(below, above))
        assert "planes" in refused(lambda: dev.RedistanceSlab(below, above))
    assert dev.state_diff(twin) == 0
    # another radius replaces the tag
    dev.DistanceSlabBegin(iso, 5)
    refused(lambda: dev.DistanceFieldSlab(planes(3), None))
    lower.DistanceSlabBegin(iso, 5)
    want = R.reference(sdf, cnt, dims, iso, 5)[0]
    assert np.array_equal(dev.DistanceFieldSlab(lower.DistanceSlabPlanes(3, 8), None), want[8 * sl:])
    assert dev.last_distance_ms() > 0.0
    # an upload between begin and the finish
    dev.upload(sdf[8 * sl:], cnt[8 * sl:])
    assert "written" in refused(lambda: dev.DistanceSlabPlanes(8, 17))
    refused(lambda: dev.DistanceFieldSlab(planes(5), None))
    refused(lambda: dev.RedistanceSlab(planes(5), None))
    assert dev.state_diff(twin) == 0
    # a carve, queued or applied
    views, masks = synth.sphere_views(17, 1, 160, 120)
    dev.DistanceSlabBegin(iso, 5)
    for d in (dev, twin):
        assert d.CarveSilhouette(views[0], masks[0]), vc.last_error()
    refused(lambda: dev.DistanceSlabPlanes(8, 17))
    refused(lambda: dev.RedistanceSlab(planes(5), None))
    dev.sync()
    twin.sync()
    refused(lambda: dev.DistanceFieldSlab(planes(5), None))
    assert dev.state_diff(twin) == 0
    # the writer ends its own tag
    dev.DistanceSlabBegin(iso, 5)
    assert dev.RedistanceSlab(planes(5), None)["rewritten"] > 0
    refused(lambda: dev.RedistanceSlab(planes(5), None))


def test_whole_grid_calls_still_refuse_a_slab():
    dims = (9, 10, 17)
    sdf, cnt = K.random_state(dims, 0.3, 0.0, 22)
    dev, twin = make_slabs(dims, [0, 8, 17])[1], make_slabs(dims, [0, 8, 17])[1]
    sl = dims[0] * dims[1]
    for d in (dev, twin):
        d.upload(sdf[8 * sl:], cnt[8 * sl:])
    lib = capi.load()
    d2 = np.full(dev.slab_voxels, 7, np.int32)
    k = C.c_int64(5)
    assert lib.vcy_distance_field(dev.ctx, 0.0, 3, d2.ctypes.data) == capi.VCY_ERR_UNSUPPORTED
    assert "whole grid" in vc.last_error() and (d2 == 7).all()
    assert lib.vcy_redistance(dev.ctx, 0.0, 3, C.byref(k)) == capi.VCY_ERR_UNSUPPORTED
    assert "whole grid" in vc.last_error() and k.value == 0
    assert dev.state_diff(twin) == 0
    two = vs.ShardedVoxelCarver(K.box_option(dims), [0], 2)
    assert two.Init(), vc.last_error()
    for call in (lambda: two.DistanceField(0.0, 4), lambda: two.Redistance(0.0, 4), lambda: two.CloseHull(1.3)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "whole grid in one context" in str(e.value)
    two.close()


# ---- 6. the writer against the readers, through the sharded carver --------------------------------------------------------

def make_sharded(dims, bounds, sdf, cnt):
    sv = vs.ShardedVoxelCarver(K.box_option(dims), [0], len(bounds) - 1, z_bounds=bounds)
    assert sv.Init(), vc.last_error()
    assert sv.z_ranges == list(zip(bounds[:-1], bounds[1:]))
    upload(sv.slabs, dims, sdf, cnt)
    return sv


def assert_mesh_equal(a, b, ctx):
    for k in ("vertices", "faces", "keys", "normals", "face_normals"):
        assert a[k].shape == b[k].shape, "%s %s: %s against %s" % (ctx, k, a[k].shape, b[k].shape)
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["keys"], b["keys"]), ctx + " faces / keys"
    for k in ("vertices", "normals", "face_normals"):
        assert np.array_equal(bits(a[k]), bits(b[k])), "%s %s bits" % (ctx, k)


@pytest.mark.parametrize("bounds", [[0, 8, 19], [0, 2, 11, 19]], ids=str)
def test_writer_against_the_readers(bounds):
    dims, radius = (70, 23, 19), 3
    sdf, cnt = K.random_state(dims, 0.2, 0.0, 9)
    case = ("readers", dims, sdf, cnt, 0.0, radius)
    want_d2, want_sdf = K.reference_of(case)
    whole = vc.VoxelCarver(K.box_option(dims))
    assert whole.Init(), vc.last_error()
    whole.upload(sdf, cnt)
    sv = make_sharded(dims, bounds, sdf, cnt)
    views, masks = synth.sphere_views(max(dims), 2, 160, 120)
    # the ray-cast first, at an iso level where the OLD field has other solid voxels: its bit planes are cached per slab
    old = sv.RenderHull(views[:1], 1.0)[0]["depth"]
    assert np.array_equal(sv.DistanceFieldSlabs(0.0, radius), want_d2)
    w = sv.RedistanceSlabs(0.0, radius)
    assert sum(w["rewritten"]) == whole.Redistance(0.0, radius)["rewritten"] == int((cnt >= 1).sum())
    assert w["device_ms"] > 0.0 and w["plane_bytes"] > 0
    assert [c.get_param("brick_min_valid") for c in sv.slabs] == [0] * len(sv.slabs)
    assert np.array_equal(bits(download(sv.slabs)[0]), bits(want_sdf))
    new, ref = sv.RenderHull(views[:1], 1.0)[0]["depth"], whole.RenderHull(views[:1], 1.0)[0]["depth"]
    assert np.array_equal(bits(new), bits(ref)), "the bit planes of the old field were used"
    assert not np.array_equal(bits(new), bits(old)), "the case does not tell the two fields apart"
    for iso in (0.0, 0.7):
        ma, mb = sv.ExtractIsoSurface(iso, True, normals=True), whole.ExtractIsoSurface(iso, True, normals=True)
        assert_mesh_equal(ma, mb, "iso %g" % iso)
        assert len(ma["vertices"]) > 100
    la, lb = sv.LabelComponents(0.0, labels=True), whole.LabelComponents(0.0, labels=True)
    for k in ("label", "n_voxels", "bb_min", "bb_max", "labels"):
        assert np.array_equal(la[k], lb[k]), k
    assert len(la["label"]) > 0
    # one more fused kMax carve
    for d in sv.slabs + [whole]:
        d.set_param("fused", 1)
        assert d.CarveSilhouette(views[1], masks[1]), vc.last_error()
        d.sync()
    sa, ca = download(sv.slabs)
    sb, cb = whole.download()
    assert np.array_equal(bits(sa), bits(sb)) and np.array_equal(ca, cb)
    sv.close()


# ---- 7. the closing ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bounds", [[0, 6, 13], [0, 4, 9, 13], [0, 2, 11, 13]], ids=str)
def test_close_hull_slabs(bounds):
    sdf, cnt, dims, gap = R.two_blocks()
    sv = make_sharded(dims, bounds, sdf, cnt)
    steps = sv.CloseHullSlabs(1.3)
    assert [sum(s["rewritten"]) for s in steps] == [sdf.size] * 3
    want = R.close_hull(sdf, cnt, dims, 1.3)
    s2, c2 = download(sv.slabs)
    assert np.array_equal(bits(s2), bits(want)) and np.array_equal(c2, cnt)
    solid = R.solid_mask(s2, c2, 0.0)
    assert solid.sum() == 300 and np.array_equal(solid, R.solid_mask(sdf, cnt, 0.0) | gap)
    assert (sv.DistanceFieldSlabs(0.0, 1) < 0).sum() == 300
    with pytest.raises(ValueError):
        sv.CloseHullSlabs(1.5)
    assert np.array_equal(bits(download(sv.slabs)[0]), bits(s2)), "the refused radius changed the state"
    sv.close()


# ---- 8. the C++ layer ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args,tag", [(["10", "2", "--redistance", "4", "--offset", "2.0"], "SLAB_REDISTANCE"),
                                      (["10", "3", "--close", "1.3"], "SLAB_CLOSE")], ids=["redistance", "close"])
def test_bunny_example_over_slabs(tmp_path, args, tag):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path)] + args, check=True, capture_output=True, text=True)
    rows = [l.split() for l in run.stdout.splitlines() if l.startswith("SLAB_")]
    assert len(rows) == 1 and rows[0][0] == tag, run.stdout
    assert rows[0][1:3] == ["slabs", args[1]] and rows[0][-2:] == ["identical", "1"], rows
    assert int(rows[0][rows[0].index("verts") + 1]) > 1000
    # the single context's own line stands beside it
    assert sum(l.startswith(tag[5:] + " ") for l in run.stdout.splitlines()) == 1, run.stdout
