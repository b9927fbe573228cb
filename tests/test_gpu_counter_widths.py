"""update_num at the edges of its three storage widths, against the CPU oracle bit for bit.

A context keeps every voxel's update_num in 1, 2 or 4 bytes: one byte on a fresh grid, widened when the views applied
or the counts uploaded could need more (count_width_for / set_count_width, vcy_state.hip), up to the width that
voxel_max_update_num + 1 needs (a voxel is skipped once update_num > max, voxel_carver.cc:447-450).  Every kernel that
reads or writes the counters has one branch per width, and halo slices travel at the final ("wire") width and are
narrowed -- saturating -- into a narrower receiver.  Every case below asserts count_bytes before and after the
operation it tests, so the width it exercises is proven, not assumed; the counts sit where a wrap (256 -> 0,
65536 -> 0) would turn a carved voxel back into an untouched one."""
import numpy as np
import pytest

import oracle_lib as O
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist
from vacancy_amd import synth
from vacancy_amd.capi import CarverOption, UpdateOption

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _oracle_on_one_thread():
    """The grids here hold a few thousand voxels: the oracle's carve is fastest without OpenMP's fork and join (65 600
    views of 12^3: 3 s instead of 12 s)."""
    prev = O.set_num_threads(1)
    yield
    O.set_num_threads(prev)


def assert_state_equal(dev, orc, ctx=""):
    ds, du = dev.download()
    os_, ou = orc.download()
    assert np.array_equal(du, ou), "%s update_num differs at %d voxels" % (ctx, int((du != ou).sum()))
    assert np.array_equal(ds.view(np.uint32), os_.view(np.uint32)), \
        "%s sdf bits differ at %d voxels" % (ctx, int((ds.view(np.uint32) != os_.view(np.uint32)).sum()))


def assert_mesh_equal(dm, om, ctx=""):
    assert dm["vertices"].shape == om["vertices"].shape, (ctx, dm["vertices"].shape, om["vertices"].shape)
    assert dm["faces"].shape == om["faces"].shape, (ctx, dm["faces"].shape, om["faces"].shape)
    assert np.array_equal(dm["keys"], om["keys"]), ctx + " edge keys / vertex order differ"
    assert np.array_equal(dm["faces"], om["faces"]), ctx + " faces differ"
    assert np.array_equal(dm["vertices"].view(np.uint32), om["vertices"].view(np.uint32)), \
        ctx + " vertex bits differ"


def assert_voxel_mesh_equal(dv, ov, ctx=""):
    assert np.array_equal(dv["faces"], ov["faces"]), ctx + " voxel mesh faces differ"
    assert np.array_equal(dv["vertices"].view(np.uint32), ov["vertices"].view(np.uint32)), ctx + " voxel mesh vertices differ"


def widths(dev):
    return dev.get_param("count_bytes"), dev.get_param("count_bytes_final")


def assert_everything_equal(dev, orc, rng, ctx):
    """Full state, vcy_download_voxels at random ids, marching cubes (mcsweep 0/1 x mcskip 0/2) and ExtractVoxel /
    ExtractVoxelInto (inside_empty both ways): every reader of the counters at the context's current width."""
    assert_state_equal(dev, orc, ctx)
    os_, ou = orc.download()
    ids = rng.randint(0, orc.n, 257).astype(np.int64)
    ids[:2] = (0, orc.n - 1)
    gs, gu = dev.download_voxels(ids)
    assert np.array_equal(gu, ou[ids]), ctx + " download_voxels update_num"
    assert np.array_equal(gs.view(np.uint32), os_[ids].view(np.uint32)), ctx + " download_voxels sdf"
    ref = orc.marching_cubes(0.0, True)
    assert len(ref["faces"]) > 0, ctx
    for sweep in (0, 1):
        for skip in (0, 2):
            dev.set_param("mcsweep", sweep)
            dev.set_param("mcskip", skip)
            assert_mesh_equal(dev.ExtractIsoSurface(0.0, True), ref, "%s mcsweep %d mcskip %d" % (ctx, sweep, skip))
    for inside_empty in (False, True):
        ov = orc.extract_voxel(inside_empty)
        assert len(ov["faces"]) > 0, ctx
        assert_voxel_mesh_equal(dev.ExtractVoxel(inside_empty), ov, "%s ExtractVoxel(%s)" % (ctx, inside_empty))
        assert_voxel_mesh_equal(dev.ExtractVoxelInto(inside_empty), ov, "%s ExtractVoxelInto(%s)" % (ctx, inside_empty))


# ---- 1. uploaded counts at the edges of every width, then a few views through every carve path ---------------------

MODES = {
    "max": dict(),
    "wa_unit": dict(voxel_update=1),
    "wa_037": dict(voxel_update=1, voxel_update_weight=0.37),
    "tsdf": dict(voxel_update=1, use_truncation=True, truncation_band=0.1),
}

# (voxel_max_update_num, largest count uploaded, count_bytes after the upload, after the carve, final width)
EDGE_CASES = [
    (2, 3, 1, 1, 1),            # u8 forever
    (254, 255, 1, 1, 1),        # u8 saturated: counts at 255 > max stay 255 in the fused u8 instance
    (255, 255, 1, 2, 2),        # u8 -> u16 by the carve
    (255, 256, 2, 2, 2),        # u16 from the upload
    (65534, 65535, 2, 2, 2),    # u16 forever: counts at 65535 > max stay 65535 (a wrap would be a first touch)
    (65535, 65535, 2, 4, 4),    # u16 -> u32 by the carve: the per-view kernel takes over from the fused one
    (65535, 65536, 4, 4, 4),    # u32 from the upload
    (70000, 70001, 4, 4, 4),    # u32
    (70000, 255, 1, 2, 4),      # u8 -> u16 under a final width of 4
]

# (name, set_param values, views per call (0: one CarveDevice call))
PATHS = [
    ("fused", dict(), 3),
    ("fused_cull0", dict(cull=0), 3),
    ("oneview1", dict(defer=0, oneview=1), 0),
    ("oneview0", dict(defer=0, oneview=0), 0),
    ("perview", dict(fused=0), 3),
]


def edge_counts(rng, n, max_update, top):
    """Counts of every edge value up to `top` (0, 1, max - 1, max, max + 1, 255, 256, 65534 .. 65536), mixed per voxel;
    every one of them occurs, `top` included."""
    vals = sorted({v for v in (0, 1, 2, max_update - 1, max_update, max_update + 1, 255, 256, 65534, 65535, 65536)
                   if 0 <= v <= top})
    cnt = np.array(vals, np.int32)[rng.randint(0, len(vals), n)]
    cnt[rng.permutation(n)[: len(vals)]] = vals
    assert int(cnt.max()) == top
    return cnt


def edge_grid(update_option):
    # 67 x 9 x 7: rows of 64 + 3 voxels, slices of 603 (odd)
    return CarverOption(bb_min=(-33.5, -4.5, -3.5), bb_max=(33.5, 4.5, 3.5), resolution=1.0, update_option=update_option)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", EDGE_CASES, ids=["max%d_top%d" % c[:2] for c in EDGE_CASES])
def test_uploaded_edge_counts_through_every_carve_path(case, mode):
    max_update, top, w_upload, w_carve, w_final = case
    uo = UpdateOption(voxel_max_update_num=max_update, **MODES[mode])
    opt = edge_grid(uo)
    views, masks = synth.sphere_views(67, 3, 64, 48)
    sdfs = [O.make_sdf(m, use_truncation=bool(uo.use_truncation), band=uo.truncation_band) for m in masks]
    orc = O.OracleGrid(opt)
    assert orc.dims == (67, 9, 7)
    rng = np.random.RandomState(max_update + top)
    sdf = rng.uniform(-1, 1, orc.n).astype(np.float32)
    cnt = edge_counts(rng, orc.n, max_update, top)
    sdf[(cnt == 0) & (rng.rand(orc.n) < 0.5)] = np.finfo(np.float32).min  # (what an untouched voxel holds)
    for name, params, nv in PATHS:
        ctx = "max %d top %d %s %s" % (max_update, top, mode, name)
        dev = vc.VoxelCarver(opt)
        assert dev.Init(), vc.last_error()
        for k, v in params.items():
            dev.set_param(k, v)
        assert widths(dev) == (1, w_final), ctx
        dev.upload(sdf, cnt)
        orc.upload(sdf, cnt)
        assert widths(dev) == (w_upload, w_final), ctx + " after the upload"
        assert_state_equal(dev, orc, ctx + " uploaded")
        imgs = [dev.upload_sdf(s_) for s_ in sdfs]
        if nv:
            assert dev.CarveBatchDevice(views[:nv], imgs[:nv]), vc.last_error()
        else:
            assert dev.CarveDevice(views[0], imgs[0]), vc.last_error()
        for i in range(max(nv, 1)):
            orc.carve(views[i], sdfs[i])
        assert widths(dev) == (w_carve, w_final), ctx + " after the carve"
        saturated = cnt > max_update
        du = dev.download()[1]
        assert np.array_equal(du[saturated], cnt[saturated]), ctx + " a saturated counter moved"
        assert_everything_equal(dev, orc, rng, ctx)
        assert widths(dev) == (w_carve, w_final), ctx + " after the readers"
        for p in imgs:
            dev.free_device(p)
        dev.close()


def test_lazycount_0_converts_held_counts():
    """"lazycount" 0 on a context that holds state widens it in place (convert_counts 1 -> 2, 1 -> 4, 2 -> 4)."""
    rng = np.random.RandomState(3)
    for max_update, top, w_before, w_after in ((255, 255, 1, 2), (70000, 255, 1, 4), (70000, 65535, 2, 4)):
        opt = edge_grid(UpdateOption(voxel_max_update_num=max_update))
        orc = O.OracleGrid(opt)
        sdf = rng.uniform(-1, 1, orc.n).astype(np.float32)
        cnt = edge_counts(rng, orc.n, max_update, top)
        orc.upload(sdf, cnt)
        dev = vc.VoxelCarver(opt)
        assert dev.Init(), vc.last_error()
        dev.upload(sdf, cnt)
        assert widths(dev) == (w_before, w_after)
        dev.set_param("lazycount", 0)
        assert widths(dev) == (w_after, w_after)
        assert_everything_equal(dev, orc, rng, "lazycount 0 max %d top %d" % (max_update, top))


# ---- 2. a fresh grid carved across the 256th and the 65 536th view --------------------------------------------------

def test_fresh_grid_crosses_u8_u16_u32():
    n, ncam, w, h = 12, 6, 32, 24
    uo = UpdateOption(voxel_update=1, voxel_max_update_num=65535)  # unit weight: rcp_count for 1 / (n + 1)
    opt = synth.sphere_option(n, uo)
    cams, masks = synth.sphere_views(n, ncam, w, h)  # one focal length: the short-division check runs once
    sdfs = [O.make_sdf(m) for m in masks]
    total = 65600
    marks = (255, 256, 300, 65480, 65535, 65536, 65580, total)
    rng = np.random.RandomState(65536)

    orc = O.OracleGrid(opt)
    ref = {}
    done = 0
    for m in marks:
        for i in range(done, m):
            orc.carve(cams[i % ncam], sdfs[i % ncam])
        done = m
        ref[m] = orc.download()
    assert int(ref[total][1].max()) == 65536 and int(ref[total][1].min()) == 65536  # every voxel saw every view

    def carve_range(dev, imgs, a, b, batch=8192):
        for s in range(a, b, batch):
            e = min(b, s + batch)
            assert dev.CarveBatchDevice([cams[i % ncam] for i in range(s, e)], [imgs[i % ncam] for i in range(s, e)]), \
                vc.last_error()

    def same_as(dev, m, ctx):
        ds, du = dev.download()
        assert np.array_equal(du, ref[m][1]), "%s: update_num differs at %d voxels after %d views" % (
            ctx, int((du != ref[m][1]).sum()), m)
        assert np.array_equal(ds.view(np.uint32), ref[m][0].view(np.uint32)), "%s: sdf bits differ after %d views" % (ctx, m)

    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    assert widths(dev) == (1, 4)
    imgs = [dev.upload_sdf(s_) for s_ in sdfs]
    expect = {255: 1, 256: 2, 300: 2, 65480: 2, 65535: 2, 65536: 4, 65580: 4, total: 4}
    done = 0
    for m in marks:
        assert dev.get_param("count_bytes") == (1 if done < 256 else 2 if done < 65536 else 4), m
        carve_range(dev, imgs, done, m)
        done = m
        assert widths(dev) == (expect[m], 4), m
        same_as(dev, m, "batches")
    assert_everything_equal(dev, orc, rng, "after %d views" % total)  # (orc holds the state after `total` views)

    # the last views around 65 536 through per-view Carve() calls: queued (defer 1; can_defer looks at one view, the
    # flush of a queue that crosses the boundary goes to the per-view kernel) and applied one by one (defer 0)
    one_by_one = []
    for defer in (1, 0):
        d = vc.VoxelCarver(opt)
        assert d.Init(), vc.last_error()
        d.set_param("defer", defer)
        di = [d.upload_sdf(s_) for s_ in sdfs]
        carve_range(d, di, 0, 65480)
        assert widths(d) == (2, 4)
        for i in range(65480, 65580):
            assert d.Carve(cams[i % ncam], sdfs[i % ncam]), vc.last_error()
        same_as(d, 65580, "Carve() defer %d" % defer)
        assert widths(d) == (4, 4)
        one_by_one.append(d)
    assert one_by_one[0].state_diff(one_by_one[1]) == 0

    # reset: one byte again; 300 views widen into the spare array of another width
    dev.reset()
    assert widths(dev) == (1, 4)
    carve_range(dev, imgs, 0, 300)
    assert widths(dev) == (2, 4)
    same_as(dev, 300, "after reset")


# ---- 3. halo slices between slabs of different widths, wire width 4 -------------------------------------------------

SLAB_COUNTS = {  # per width: values that need it (the largest one), and values a narrower type would wrap to 0
    1: (0, 1, 2, 255),
    2: (0, 1, 256, 512, 65535),
    4: (0, 1, 256, 65536, 70001),
}


def halo_state(rng, dims, cut, w_lower, w_upper):
    n = dims[0] * dims[1] * dims[2]
    sl = dims[0] * dims[1]
    sdf = rng.uniform(-1, 1, n).astype(np.float32)
    cnt = np.empty(n, np.int32)
    lo = np.array(SLAB_COUNTS[w_lower], np.int32)
    up = np.array(SLAB_COUNTS[w_upper], np.int32)
    cnt[: cut * sl] = lo[rng.randint(0, len(lo), cut * sl)]
    cnt[cut * sl:] = up[rng.randint(0, len(up), n - cut * sl)]
    cnt[rng.randint(0, cut * sl)] = lo[-1]
    cnt[cut * sl + rng.randint(0, n - cut * sl)] = up[-1]
    # the converter's tail (2 * slice is not a multiple of 4): the lower slab's last voxels hold its widest values
    cnt[cut * sl - 3: cut * sl] = lo[-2:][rng.randint(0, 2, 3)]
    return sdf, cnt


@pytest.mark.parametrize("how", ["host", "copy", "rccl"])
def test_halo_exchange_at_wire_width_4(how):
    lib = vc.capi.load()
    opt = CarverOption(bb_min=(-6.5, -4.5, -6.0), bb_max=(6.5, 4.5, 6.0), resolution=1.0,
                       update_option=UpdateOption(voxel_max_update_num=70000))
    orc = O.OracleGrid(opt)
    dims = orc.dims
    assert dims == (13, 9, 12)  # slices of 117 voxels: 2 * 117 = 234 counters per halo
    nz, sl = dims[2], dims[0] * dims[1]
    ranges = [vdist.slab_range(nz, r, 2) for r in range(2)]
    cut = ranges[0][1]
    rng = np.random.RandomState(7)
    for w_lower in (1, 2, 4):
        for w_upper in (1, 2, 4):
            ctx = "%s lower u%d upper u%d" % (how, 8 * w_lower, 8 * w_upper)
            sdf, cnt = halo_state(rng, dims, cut, w_lower, w_upper)
            orc.upload(sdf, cnt)
            slabs = []
            for (z0, z1) in ranges:
                c = vc.VoxelCarver(opt, z_range=(z0, z1))
                assert c.Init(), vc.last_error()
                c.upload(sdf[z0 * sl: z1 * sl], cnt[z0 * sl: z1 * sl])
                slabs.append(c)
            assert [widths(c) for c in slabs] == [(w_lower, 4), (w_upper, 4)], ctx
            assert int(lib.vcy_halo_bytes(slabs[0].ctx)) == 2 * sl * 8
            if how == "host":
                gathered = np.concatenate([c.halo_pack_host() for c in slabs])
                for r, c in enumerate(slabs):
                    c.halo_unpack_host(gathered, r, 2)
            elif how == "copy":
                assert lib.vcy_halo_copy_from(slabs[0].ctx, None) == 0
                assert lib.vcy_halo_copy_from(slabs[1].ctx, slabs[0].ctx) == 0, vc.last_error()
            else:
                vc.halo_allgather(slabs)
            assert [widths(c) for c in slabs] == [(w_lower, 4), (w_upper, 4)], ctx + " after the exchange"
            for interp in (True, False):
                merged = vdist.merge_meshes([c.ExtractIsoSurface(0.0, interp) for c in slabs])
                assert_mesh_equal(merged, orc.marching_cubes(0.0, interp), ctx)
            for inside_empty in (False, True):
                ids = np.concatenate([c.extract_voxel_ids(inside_empty) for c in slabs])
                ov = orc.extract_voxel(inside_empty)
                assert len(ov["faces"]) > 0
                assert_voxel_mesh_equal(vc.voxel_cubes(opt, ids), ov, "%s inside_empty %s" % (ctx, inside_empty))
            assert [widths(c) for c in slabs] == [(w_lower, 4), (w_upper, 4)], ctx + " after the readers"


def test_state_diff_between_contexts_of_different_width():
    opt = CarverOption(bb_min=(-6.5, -4.5, -6.0), bb_max=(6.5, 4.5, 6.0), resolution=1.0,
                       update_option=UpdateOption(voxel_max_update_num=70000))
    rng = np.random.RandomState(9)
    n = 13 * 9 * 12
    sdf = rng.uniform(-1, 1, n).astype(np.float32)
    held = {}
    for w in (1, 2, 4):
        cnt = np.array(SLAB_COUNTS[w], np.int32)[rng.randint(0, len(SLAB_COUNTS[w]), n)]
        cnt[0] = SLAB_COUNTS[w][-1]
        for lazy in (1, 0):
            c = vc.VoxelCarver(opt)
            assert c.Init(), vc.last_error()
            c.upload(sdf, cnt)
            if not lazy:
                c.set_param("lazycount", 0)
            assert widths(c) == ((w if lazy else 4), 4)
            held[(w, lazy)] = (c, cnt)
    for (wa, la), (a, ca) in held.items():
        for (wb, lb), (b, cb) in held.items():
            assert a.state_diff(b) == int((ca != cb).sum()), (wa, la, wb, lb)
    # the same counts, different widths: nothing differs; one counter changed: one voxel differs
    a, ca = held[(1, 1)]
    for key in ((1, 0), (2, 1), (4, 1)):
        b = vc.VoxelCarver(opt)
        assert b.Init()
        wide = ca.copy()
        wide[-1] = SLAB_COUNTS[key[0]][-1]
        b.upload(sdf, wide)
        if not key[1]:
            b.set_param("lazycount", 0)
        assert widths(b) == ((key[0] if key[1] else 4), 4)
        assert b.state_diff(a) == int(wide[-1] != ca[-1])
        b.upload(sdf, ca)
        assert b.get_param("count_bytes") == (key[0] if key[1] else 4)  # (an upload never narrows)
        assert b.state_diff(a) == 0 and a.state_diff(b) == 0
