"""The device SDF builder (vacancy_amd/csrc/sdf2d.hip) and every batch path in front of it at their hand-made edges:
the table of silhouette_cases.py through vcy_make_sdf_device and -- shuffled, so that the 32 jobs of a launch differ
in size and ROI -- through vcy_make_sdf_batch_device; the max |v| cell when scratch memory is reused; views of
different size, intrinsics and ROI through the streamed and the sharded carve; the staging pool shared by two entry
points.  Every comparison is with the oracle, bit for bit, over the whole image (pixels outside the ROI are 0)."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as O
import silhouette_cases as S
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import UpdateOption

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5C3F00D
TSDF = dict(voxel_update=1, use_truncation=True, truncation_band=0.1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def carver_of(n=16, z_range=None, **kw):
    dev = vc.VoxelCarver(synth.sphere_option(n, UpdateOption(**kw)), z_range=z_range)
    assert dev.Init(), vc.last_error()
    return dev


def assert_image(got, want, ctx):
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        y, x = bad[0]
        raise AssertionError("%s: %d of %d pixels differ, first at (x %d, y %d): %r, oracle %r"
                             % (ctx, len(bad), got.size, x, y, got[y, x], want[y, x]))


# ---- single images ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize,truncate", [(True, False), (False, False), (True, True), (False, True)])
def test_single_image_builder_on_the_table(normalize, truncate):
    """vcy_make_sdf_device, every case of the table (the equality bands on their case)."""
    dev = carver_of()
    runs = 0
    for c in S.cases():
        name, mask, rmin, rmax = c
        for norm, trunc, band in S.settings(name):
            if (norm, trunc) != (normalize, truncate):
                continue
            d = dev.make_sdf_device(mask, rmin, rmax, norm, trunc, band)
            got = dev.download_image(d, mask.shape)
            dev.free_device(d)
            assert_image(got, S.oracle_image(c, norm, trunc, band), "%s band %g" % (name, band))
            runs += 1
    assert runs == (len(S.cases()) * len(S.BANDS) + len(S.EQUALITY_BANDS) if truncate else len(S.cases()))


# ---- heterogeneous batches into caller-owned images ----------------------------------------------------------------------

def batch_into(dev, batch, truncate, band, ctx):
    """vcy_make_sdf_batch_device of `batch` (cases) into ONE allocation -- image i at its own offset, w * h * 4 bytes
    rounded up to 256, 256 guard bytes in front of, between and behind the images, everything pre-filled with a sentinel:
    every image equals the oracle's, every other byte still holds the sentinel."""
    offs, pos = [], 256
    for _, mask, _, _ in batch:
        offs.append(pos)
        pos += (mask.size * 4 + 255) // 256 * 256 + 256
    buf = C.c_void_p()
    assert dev._lib.vcy_device_alloc(dev.ctx, pos, C.byref(buf)) == 0, vc.last_error()
    try:
        dev.memcpy_h2d(buf, np.full(pos // 4, SENTINEL, np.uint32))
        ok = dev.make_sdf_batch_into([S.view_of(c) for c in batch], [c[1] for c in batch], [buf.value + o for o in offs])
        assert ok, vc.last_error()
        after = dev.download_image(buf, (pos // 4,)).view(np.uint32)
    finally:
        dev.free_device(buf)
    untouched = np.ones(pos // 4, bool)
    for i, (c, o) in enumerate(zip(batch, offs)):
        h, w = c[1].shape
        untouched[o // 4:o // 4 + w * h] = False
        got = after[o // 4:o // 4 + w * h].view(np.float32).reshape(h, w)
        assert_image(got, S.oracle_image(c, True, truncate, band), "%s: image %d of %d (%s)" % (ctx, i, len(batch), c[0]))
    assert (after[untouched] == SENTINEL).all(), "%s: %d guard words overwritten" % (ctx, int((after[untouched] != SENTINEL).sum()))


def shuffled_batches():
    """The table in a fixed random order, cut into batches of 1, 31, 32, 33 and 65 cases (the truncation-equality case
    in the second group of the last one) and then all of it in one call."""
    table = S.cases()
    order = [table[i] for i in np.random.RandomState(7).permutation(len(table))]
    out, first = [], 0
    for n in (1, 31, 32, 33, 65):
        out.append(order[first:first + n])
        first += n
    out[-1][40] = S.case(S.EQUALITY_NAME)
    out.append(order)
    for b in out[1:]:  # every launch of 32 jobs mixes sizes and ROIs
        for g in range(0, len(b), 32):
            assert len({(c[1].shape, c[2], c[3]) for c in b[g:g + 32]}) > min(8, len(b[g:g + 32]) // 2)
    return out


@pytest.mark.parametrize("truncate", [False, True])
def test_heterogeneous_batches_into_caller_owned_images(truncate):
    band = S.EQUALITY_BANDS[0]
    dev = carver_of(use_truncation=truncate, truncation_band=band)
    for batch in shuffled_batches():
        batch_into(dev, batch, truncate, band, "batch of %d" % len(batch))


# ---- the max |v| cell when scratch is reused ------------------------------------------------------------------------------

def test_scratch_reuse_across_groups_and_calls():
    """max |v| is reduced by atomicMax into a cell of the scratch memory that sdf_rows_kernel resets: a view that
    inherits the cell of an all-255 image (FLT_MAX) must still be normalised by its own maximum -- as job 0 of the
    second group of a batch, as the second of two vcy_make_sdf_device calls, as the second of two vcy_carve_silhouette
    calls on one context."""
    full, blob = S.scratch_pair()
    h, w = S.SCRATCH_SHAPE
    rng = np.random.RandomState(12)
    filler = [("scratch/filler%d" % i, (rng.rand(h, w) < 0.5).astype(np.uint8) * 255, (0, 0), (w - 1, h - 1))
              for i in range(31)]
    dev = carver_of()
    batch_into(dev, [full] + filler + [blob], False, 0.1, "33 views of one size")
    for c in (full, blob):
        d = dev.make_sdf_device(c[1], c[2], c[3], True, False, 0.1)
        got = dev.download_image(d, c[1].shape)
        dev.free_device(d)
        assert_image(got, S.oracle_image(c, True, False, 0.1), "make_sdf_device " + c[0])
    views, _ = synth.sphere_views(16, 2, w, h)
    orc = O.OracleGrid(dev.option)
    for v, c in zip(views, (full, blob)):
        ok, sdf = dev.CarveSilhouette(v, c[1], return_sdf=True)
        assert ok, vc.last_error()
        assert_image(sdf, S.oracle_image(c, True, False, 0.1), "CarveSilhouette " + c[0])
        orc.carve(v, S.oracle_image(c, True, False, 0.1))
    assert_state(dev.download(), orc.download(), "two CarveSilhouette calls")


# ---- carves from views that differ in size, intrinsics and ROI ----------------------------------------------------------

MIXED_N = 24
MIXED_SIZES = ((40, 30), (64, 64), (65, 17), (130, 9), (96, 72))


def assert_state(got, want, ctx):
    (gs, gu), (ws, wu) = got, want
    assert np.array_equal(gu, wu), "%s: update_num differs in %d voxels" % (ctx, int((gu != wu).sum()))
    assert np.array_equal(bits(gs), bits(ws)), "%s: sdf differs in %d voxels" % (ctx, int((bits(gs) != bits(ws)).sum()))


def mixed_views(nv=33, sizes=MIXED_SIZES, n=MIXED_N):
    """synth.sphere_views, but every view with its own image size, focal length (fx == fy) and principal point; a
    third of the views with a sub-ROI whose left edge is no multiple of 64; silhouettes: the sphere's disc with noise, every
    fourth one noise alone."""
    rng = np.random.RandomState(21)
    radius, dist = 0.35 * n, 2.0 * n
    lim = radius * radius / (dist * dist - radius * radius)
    views, masks = [], []
    for i in range(nv):
        w, h = sizes[i % len(sizes)]
        f = synth.focal_from_fov_y(h, 40.0 + 2.5 * (i % 7))
        cx = np.float32(np.float32(w) * np.float32(0.5) - np.float32(0.5) + np.float32(1.25 * (i % 3 - 1)))
        cy = np.float32(np.float32(h) * np.float32(0.5) - np.float32(0.5) + np.float32(0.75 * (i % 4 - 1.5)))
        y = 1.0 - 2.0 * (i + 0.5) / nv
        r = math.sqrt(max(0.0, 1.0 - y * y))
        phi = i * math.pi * (3.0 - math.sqrt(5.0))
        c2w = synth.lookat_c2w(dist * np.array([r * math.cos(phi), y, r * math.sin(phi)]), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        rmin = rmax = None
        if i % 3 == 1:
            rmin = ((65 if w >= 96 else 3) + i % 5, 1 + i % 2)
            rmax = (w - 2 - i % 4, h - 2)
        views.append(vc.make_view(synth.affine_inverse(c2w).astype(np.float32), f, f, cx, cy, w, h, rmin, rmax))
        if i % 4 == 3:
            mask = np.where(rng.rand(h, w) < 0.5, 255, 0).astype(np.uint8)
        else:
            uu = (np.arange(w, dtype=np.float64) - float(cx)) / float(f)
            vv = (np.arange(h, dtype=np.float64) - float(cy)) / float(f)
            mask = np.where(uu[None, :] ** 2 + vv[:, None] ** 2 <= lim, 255, 0).astype(np.uint8)
            flip = rng.rand(h, w) < 0.03
            mask[flip] = S.VALUES[rng.randint(0, len(S.VALUES), int(flip.sum()))]
        masks.append(mask)
    assert sum(1 for v in views if v.roi_min[0] % 64) >= nv // 3 and len({(v.width, v.height) for v in views}) == len(sizes)
    return views, masks


def view_rois(v):
    return tuple(v.roi_min), tuple(v.roi_max)


_oracle_states = {}


def oracle_state(key, kw, views, masks, n=MIXED_N):
    """The oracle's per-view loop (MakeSignedDistanceField + Carve per view) -- once per key, shared, read-only."""
    if key not in _oracle_states:
        uo = UpdateOption(**kw)
        orc = O.OracleGrid(synth.sphere_option(n, uo))
        for v, m in zip(views, masks):
            orc.carve(v, O.make_sdf(m, *view_rois(v), normalize=True, use_truncation=bool(uo.use_truncation),
                                    band=uo.truncation_band))
        s, u = orc.download()
        s.setflags(write=False)
        u.setflags(write=False)
        _oracle_states[key] = (s, u)
    return _oracle_states[key]


MODES = {"kmax": dict(), "tsdf": TSDF}


@pytest.mark.parametrize("mode", list(MODES))
def test_streamed_carve_with_mixed_views(mode):
    """vcy_carve_batch_silhouettes, 33 views (two chunks), no two neighbours of one size."""
    views, masks = mixed_views()
    dev = carver_of(MIXED_N, **MODES[mode])
    assert dev.CarveBatchSilhouettes(views, masks), vc.last_error()
    assert_state(dev.download(), oracle_state(("mixed", mode), MODES[mode], views, masks), "streamed " + mode)


def z_slabs(count, kw):
    from vacancy_amd import dist as vdist
    return [carver_of(MIXED_N, z_range=vdist.slab_range(MIXED_N, r, count), **kw) for r in range(count)]


def slab_states(slabs):
    parts = [c.download() for c in slabs]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.mark.parametrize("split,mode", [(0, "kmax"), (1, "kmax"), (1, "tsdf")])
def test_sharded_producer_with_mixed_views(split, mode, monkeypatch):
    """vcy_carve_batch_silhouettes_sharded over three z-slabs: one producer for the device (split 0) and one producer
    rank per slab (split 1: share, slot and gather layout of three devices)."""
    views, masks = mixed_views()
    monkeypatch.setenv("VCY_TEST_SPLIT_PRODUCERS", str(split))
    slabs = z_slabs(3, MODES[mode])
    try:
        assert vc.carve_batch_silhouettes_sharded(slabs, views, masks)
        assert_state(slab_states(slabs), oracle_state(("mixed", mode), MODES[mode], views, masks),
                     "sharded split %d %s" % (split, mode))
    finally:
        vc.capi.load().vcy_halo_shutdown()  # releases the producer groups as well


@pytest.mark.parametrize("mode", list(MODES))
def test_one_rank_producer_with_mixed_views(mode):
    """vacancy_amd.dist.carve_silhouettes_sharded with world == 1: vcy_make_sdf_batch_device builds every chunk's images
    in place, slots sized by the largest image of the call."""
    from vacancy_amd import dist as vdist
    views, masks = mixed_views()
    slabs = z_slabs(3, MODES[mode])
    info = vdist.carve_silhouettes_sharded(slabs, 0, 1, views, masks, chunk=16)
    assert info["views_built_by_this_rank"] == len(views)
    assert_state(slab_states(slabs), oracle_state(("mixed", mode), MODES[mode], views, masks), "one rank " + mode)
    vc.capi.load().vcy_halo_shutdown()


# ---- one staging pool, two entry points -----------------------------------------------------------------------------------

def test_pool_growth_and_shared_layout_on_one_context():
    """vcy_make_sdf_batch_device and vcy_carve_batch_silhouettes keep ONE device pool and ONE page-locked staging area
    in the context, laid out differently and grown on demand: small batch, larger carve, mixed batch, small carve."""
    dev = carver_of(MIXED_N, **TSDF)
    band = TSDF["truncation_band"]
    rng = np.random.RandomState(33)
    small = [("pool/40x30_%d" % i, (rng.rand(30, 40) < 0.2 + 0.1 * i).astype(np.uint8) * 255, (0, 0), (39, 29))
             for i in range(5)]
    batch_into(dev, small, True, band, "1: 40x30 batch")
    big_views, big_masks = mixed_views(34, ((96, 72),))
    assert dev.CarveBatchSilhouettes(big_views, big_masks), vc.last_error()
    assert_state(dev.download(), oracle_state("pool/96x72", TSDF, big_views, big_masks), "2: 96x72 carve")
    batch_into(dev, shuffled_batches()[4], True, band, "3: mixed batch")
    dev.reset()
    small_views, small_masks = mixed_views(7, ((40, 30),))
    assert dev.CarveBatchSilhouettes(small_views, small_masks), vc.last_error()
    assert_state(dev.download(), oracle_state("pool/40x30", TSDF, small_views, small_masks), "4: 40x30 carve")
