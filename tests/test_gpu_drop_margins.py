"""View dropping and brick skipping at the edges of their bounds, against the CPU oracle bit for bit.

The carve kernels skip a (wave brick, view) pair when an upper bound of every sample the brick can take is not above
the brick's minimum (kMax) or lies below the truncation limit, and compile the `dist < -1` test out where a lower bound
allows it (footprint_of, carve_fused_device.h); marching cubes does not read a brick whose kept minimum lies above the iso
level (mc_bits_bricks_kernel).  The smooth and noisy scenes of the other modules cannot tell a tight bound from one
that is a pixel short: here the images are needle scenes (needle_scenes.py), on which a pair must not be dropped only
because of one pixel on the outer ring of its footprint, and the states hold one low voxel per brick.  The CPU test at
the end checks that the scenes still put needles on those rings where the oracle shows that they matter."""
import numpy as np
import pytest

import needle_scenes as N
import oracle_lib as O
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist
from vacancy_amd.capi import CarverOption, UpdateOption, make_view


def assert_state_equal(ds, du, os_, ou, ctx):
    """Bit for bit; NaN voxels only need to be NaN on both sides (their payload is not pinned down)."""
    assert np.array_equal(du, ou), "%s update_num differs at %d voxels" % (ctx, int((du != ou).sum()))
    nan_d, nan_o = np.isnan(ds), np.isnan(os_)
    assert np.array_equal(nan_d, nan_o), ctx + " NaN voxels differ"
    bd, bo = np.where(nan_d, 0, ds.view(np.uint32)), np.where(nan_o, 0, os_.view(np.uint32))
    assert np.array_equal(bd, bo), "%s sdf bits differ at %d voxels" % (ctx, int((bd != bo).sum()))


def assert_mesh_equal(dm, om, ctx=""):
    assert dm["vertices"].shape == om["vertices"].shape, (ctx, dm["vertices"].shape, om["vertices"].shape)
    assert dm["faces"].shape == om["faces"].shape, (ctx, dm["faces"].shape, om["faces"].shape)
    assert np.array_equal(dm["keys"], om["keys"]), ctx + " edge keys / vertex order differ"
    assert np.array_equal(dm["faces"], om["faces"]), ctx + " faces differ"
    assert np.array_equal(dm["vertices"].view(np.uint32), om["vertices"].view(np.uint32)), ctx + " vertex bits differ"


def batches_of(nv, k):
    """Views in launches of k: consecutive launches carry different views, so the window planes of a view slot hold
    the previous launch's image wherever this launch does not rebuild them."""
    return [list(range(i, min(nv, i + k))) for i in range(0, nv, k)]


# (family, mode): every footprint size with kMax; borders and the ROI; max_sdf; the truncation drop; the truncating
# average's lower bound (general and unit weight); nearest-neighbour taps; fx != fy; orthographic
FUSED_CASES = [("raw", "max"), ("raw", "outside"), ("raw", "trunc"), ("raw", "tsdf_pits"), ("raw", "nn"),
               ("k8", "max"), ("k8", "roi"), ("k8", "outside"), ("k8", "trunc"), ("k8", "tsdf_pits"),
               ("k8", "wa_unit_pits"), ("k8", "tsdf_drop"), ("k8", "nn"), ("k8", "fxfy"),
               ("big", "max"), ("big", "fxfy"), ("big", "outside"), ("big", "trunc"),
               ("ortho", "max"), ("ortho", "tsdf_pits")]

# (cull, tile, prologue): raw / quad tiles from the pre-pass's records, big tiles, footprints in the kernel's prologue,
# and no dropping at all as the control
FUSED_CONFIGS = [(1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 0, 1), (0, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,mode", FUSED_CASES, ids=["%s-%s" % c for c in FUSED_CASES])
def test_multi_view_launches_on_needle_scenes(family, mode):
    sc = N.make_scene(family, mode)
    nv = len(sc["views"])
    batches = batches_of(nv, 8)
    after = N.oracle_run(sc, batches)
    before = N.oracle_run(sc, [[]])[0]
    assert not np.array_equal(after[-1][1], before[1]), "the scene changes nothing"
    drops = sc["kind"] != "pits"  # (a background at or above -1 in the weighted average: nothing to drop)
    for cull, tile, prologue in FUSED_CONFIGS:
        if family == "big" and tile == 1:
            continue  # (footprints wider than a raw tile: never dropped)
        ctx = "%s %s cull %d tile %d prologue %d" % (family, mode, cull, tile, prologue)
        dev = vc.VoxelCarver(sc["opt"])
        assert dev.Init(), vc.last_error()
        dev.set_param("cull", cull)
        dev.set_param("tile", tile)
        dev.set_param("prologue", prologue)
        dev.set_param("paircount", 1)
        if sc["state"] is None:
            v_init, i_init = N.init_view(sc)
            assert dev.CarveBatchDevice([v_init], [dev.upload_sdf(i_init)]), vc.last_error()
        else:
            dev.upload(*sc["state"])
        assert_state_equal(*dev.download(), *before, ctx + " before the needles")
        imgs = [dev.upload_sdf(s) for s in sc["images"]]
        processed = total = 0
        for b, (os_, ou) in zip(batches, after):
            assert dev.CarveBatchDevice([sc["views"][i] for i in b], [imgs[i] for i in b]), vc.last_error()
            p, t, _ = dev.last_carve_pairs()
            processed, total = processed + p, total + t
            assert_state_equal(*dev.download(), os_, ou, "%s after views %d..%d" % (ctx, b[0], b[-1]))
        if cull and drops:
            # (not vacuous: pairs were dropped -- at the benchmark's footprints most of them -- and the state changed)
            assert processed < (total // 2 if family == "raw" and tile != 1 else total), (ctx, processed, total)
        for p in imgs:
            dev.free_device(p)
        dev.close()


# single-view launches: (livelist, listrecords, recordbytes, rowkernel)
SINGLE_CONFIGS = [(1, 1, 0, -1), (0, 1, 0, -1), (1, 0, 0, -1), (1, 1, 2000, -1), (0, 0, 2000, 0), (1, 1, 0, 0)]
SINGLE_CASES = [("raw", "max"), ("raw", "trunc"), ("k8", "max"), ("k8", "roi"), ("k8", "trunc"), ("k8", "nn")]


@pytest.mark.gpu
@pytest.mark.parametrize("family,mode", SINGLE_CASES, ids=["%s-%s" % c for c in SINGLE_CASES])
def test_single_view_launches_on_needle_scenes(family, mode):
    """defer 0, oneview 1: one launch per view, dropped against the brick minima the previous launch left.  The state
    is carved, not uploaded (an upload turns the kept minima off): a view that sees the whole grid, one that changes
    nothing and rebuilds the minima, then the needle views."""
    sc = N.make_scene(family, mode)
    nv = min(len(sc["views"]), 16)
    v_init, i_init = N.init_view(sc)
    nothing = np.full_like(sc["images"][0], sc["bg"])
    orc = O.OracleGrid(sc["opt"])
    states = []
    orc.carve(v_init, i_init)
    assert int((orc.download()[1] == 0).sum()) == 0, "the first view leaves voxels untouched"
    orc.carve(sc["views"][0], nothing)
    states.append(orc.download())
    for i in range(nv):
        orc.carve(sc["views"][i], sc["images"][i])
        states.append(orc.download())
    orc.close()
    assert not np.array_equal(states[-1][1], states[0][1]), "the needles change nothing"
    for livelist, listrecords, recordbytes, rowkernel in SINGLE_CONFIGS:
        ctx = "%s %s livelist %d listrecords %d recordbytes %d rowkernel %d" % (family, mode, livelist, listrecords,
                                                                            recordbytes, rowkernel)
        dev = vc.VoxelCarver(sc["opt"])
        assert dev.Init(), vc.last_error()
        for k, v in (("defer", 0), ("oneview", 1), ("livelist", livelist), ("listrecords", listrecords),
                     ("recordbytes", recordbytes), ("rowkernel", rowkernel)):
            dev.set_param(k, v)
        assert dev.Carve(v_init, i_init), vc.last_error()
        assert dev.Carve(sc["views"][0], nothing), vc.last_error()
        assert dev.get_param("brick_min_valid") == 1, ctx
        assert_state_equal(*dev.download(), *states[0], ctx + " before the needles")
        for i in range(nv):
            assert dev.Carve(sc["views"][i], sc["images"][i]), vc.last_error()
            assert_state_equal(*dev.download(), *states[i + 1], "%s view %d" % (ctx, i))
        assert dev.get_param("brick_min_valid") == 1, ctx
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world,mode", [(2, "max"), (3, "max"), (3, "tsdf_pits")])
def test_z_slab_contexts_on_needle_scenes(world, mode):
    """Slabs of one grid seen from the side: every slab is a narrow band of image rows, and its window planes are only
    built over that band (FusedView::wrect).  Needles on the rows just inside and just outside every band; the launches
    alternate between two principal points, so the rows a launch does not rebuild hold the other launch's windows."""
    sc = N.make_scene("k8", mode, z_axis_view=True)
    n = sc["n"]
    nv = len(sc["views"])
    orc = O.OracleGrid(sc["opt"])
    pos = orc.positions()
    orc.close()
    cuts = [vdist.slab_range(n, r, world) for r in range(world)]
    for i, v in enumerate(sc["views"]):  # rows at the edges of every slab's band, +- 1 and 2
        M = np.array(list(v.w2c), np.float64).reshape(3, 4)
        pc = pos.astype(np.float64) @ M[:, :3].T + M[:, 3]
        wv = float(v.fy) / pc[:, 2] * pc[:, 1] + float(v.cy)
        zi = np.arange(len(pos)) // (n * n)
        val = N._needle_value(sc["kind"], i)
        xs = np.arange((i * 7) % 17, v.width, 17)
        for z0, z1 in cuts:
            sel = (zi >= z0) & (zi < z1)
            lo, hi = int(np.floor(wv[sel].min())), int(np.floor(wv[sel].max()))
            for y in (lo - 2, lo - 1, lo, hi + 1, hi + 2):
                if 0 <= y < v.height:
                    sc["images"][i][y, xs] = val
    batches = batches_of(nv, 6)
    after = N.oracle_run(sc, batches)
    slabs = []
    for z0, z1 in cuts:
        c = vc.VoxelCarver(sc["opt"], z_range=(z0, z1))
        assert c.Init(), vc.last_error()
        if sc["state"] is None:
            v_init, i_init = N.init_view(sc)
            assert c.CarveBatchDevice([v_init], [c.upload_sdf(i_init)]), vc.last_error()
        else:
            s, u = sc["state"]
            a, b = z0 * n * n, z1 * n * n
            c.upload(s[a:b], u[a:b])
        c.imgs = [c.upload_sdf(im) for im in sc["images"]]
        slabs.append(c)
    for b, (os_, ou) in zip(batches, after):
        for c in slabs:
            assert c.CarveBatchDevice([sc["views"][i] for i in b], [c.imgs[i] for i in b]), vc.last_error()
        ds = np.concatenate([c.download()[0] for c in slabs])
        du = np.concatenate([c.download()[1] for c in slabs])
        assert_state_equal(ds, du, os_, ou, "%d slabs %s after views %d..%d" % (world, mode, b[0], b[-1]))
    for c in slabs:
        for p in c.imgs:
            c.free_device(p)
        c.close()


# ---- marching cubes: one low voxel per brick ------------------------------------------------------------------------

MC_ISO = np.float32(0.25)


def _mc_grid(uo):
    # 64 x 32 x 32: rows of one 64-voxel word (the brick-row pass needs whole words), 8 x 4 x 4 bricks
    return CarverOption(bb_min=(-32.0, -16.0, -16.0), bb_max=(32.0, 16.0, 16.0), resolution=1.0, update_option=uo)


def _ortho_views():
    """Orthographic, axis-aligned: every voxel centre lands on a pixel exactly, so a voxel samples ONE pixel.  A looks
    along +z (pixel (x, y)), B along +x (pixel (z, y))."""
    a = np.array([[1, 0, 0, 31.5], [0, 1, 0, 15.5], [0, 0, 1, 100.0]], np.float32)
    b = np.array([[0, 0, 1, 15.5], [0, 1, 0, 15.5], [1, 0, 0, 100.0]], np.float32)
    return make_view(a, 1.0, 1.0, 0.0, 0.0, 64, 32, is_ortho=True), make_view(b, 1.0, 1.0, 0.0, 0.0, 32, 32, is_ortho=True)


def _low_voxels():
    """One low voxel in 32 of the 128 bricks, one per row y (so the pits of the two views meet only there): at a brick
    corner, on an edge, on a face and inside, the cells around it reaching into the neighbouring bricks."""
    spots = [(0, 0), (7, 7), (0, 3), (3, 0), (0, 5), (5, 7), (3, 4), (7, 0)]  # (x, z) in the brick; y: the row's
    out = []
    for y in range(32):
        bx, bz = (y * 3) % 8, (y * 5 + y // 8) % 4
        ox, oz = spots[(y + y // 8) % 8]
        out.append((bx * 8 + ox, y, bz * 8 + oz))
    return out


def _extract_both(dev, orc, isos, ctx):
    assert dev.get_param("brick_min_valid") == 1, ctx
    for iso in isos:
        om = orc.marching_cubes(iso, True)
        for skip in (2, 0):
            dev.set_param("mcskip", skip)
            assert_mesh_equal(dev.ExtractIsoSurface(iso, True), om, "%s iso %r mcskip %d" % (ctx, iso, skip))
        dev.set_param("mcskip", 2)


@pytest.mark.gpu
def test_brick_skipping_kmax_first_touch_from_pits():
    """kMax on a fresh grid: view A touches every voxel (1.0, pits at the chosen voxels), view B raises every other
    voxel; each chosen voxel ends at the iso level, one float below it, or well below it."""
    lo = np.float32(MC_ISO)
    just = np.nextafter(lo, np.float32(-1))
    values = [lo, just, np.float32(lo - 0.5)]
    opt = _mc_grid(UpdateOption())
    va, vb = _ortho_views()
    ia = np.ones((32, 64), np.float32)
    ib = np.ones((32, 32), np.float32)
    for k, (x, y, z) in enumerate(_low_voxels()):
        ia[y, x] = ib[y, z] = values[k % 3]
    orc = O.OracleGrid(opt)
    orc.carve(va, ia)
    orc.carve(vb, ib)
    os_, ou = orc.download()
    assert int((os_ < 0.5).sum()) == 32  # exactly the chosen voxels are low
    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    pa, pb = dev.upload_sdf(ia), dev.upload_sdf(ib)
    assert dev.CarveBatchDevice([va, vb], [pa, pb]), vc.last_error()
    assert_state_equal(*dev.download(), os_, ou, "kMax first touch")
    isos = [float(lo), float(lo) + 1e-9, float(lo) - 1e-9, float(just), float(just) - 1e-9]
    _extract_both(dev, orc, isos, "kMax")
    dev.free_device(pa)
    dev.free_device(pb)
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("weight", [1.0, 0.37])
def test_brick_skipping_after_weighted_average_lowers_single_voxels(weight):
    """Weighted average: two views leave every voxel at 1 (brick minima high), then two launches lower columns of
    voxels (C along z, D along x) -- by C alone to 0, by D alone to 0.25, where the columns cross to -0.5.  Every
    launch must lower the kept minimum of the bricks it lowers, or marching cubes skips them."""
    opt = _mc_grid(UpdateOption(voxel_update=1, voxel_update_weight=weight))
    va, vb = _ortho_views()
    one_a, one_b = np.ones((32, 64), np.float32), np.ones((32, 32), np.float32)
    ic, id_ = one_a.copy(), one_b.copy()
    for x, y, z in _low_voxels():
        ic[y, x] = id_[y, z] = np.float32(-2.0)
    orc = O.OracleGrid(opt)
    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    ptrs = [dev.upload_sdf(im) for im in (one_a, one_b, ic, id_)]
    for step, idx in enumerate(([0, 1], [0, 2], [3])):  # (the second launch: a view that keeps 1, then C)
        vs = [(va, vb, va, vb)[i] for i in idx]
        assert dev.CarveBatchDevice(vs, [ptrs[i] for i in idx]), vc.last_error()
        for i in idx:
            orc.carve((va, vb, va, vb)[i], (one_a, one_b, ic, id_)[i])
        ctx = "weight %g launch %d" % (weight, step)
        assert_state_equal(*dev.download(), *orc.download(), ctx)
        if step:
            _extract_both(dev, orc, [0.0, 0.1, 0.3, -0.25, 0.1 + 1e-9], ctx)
    assert int((orc.download()[0] < 0).sum()) == 32
    for p in ptrs:
        dev.free_device(p)
    dev.close()


# ---- the scenes reach the margins (CPU) ------------------------------------------------------------------------------

# floors of margin pairs with an effect, per family (about half of what the generator gives today)
MARGIN_FLOORS = {
    "raw": [("max", 650), ("trunc", 600), ("tsdf_pits", 750), ("outside", 430)],
    "k8": [("max", 350), ("roi", 300), ("trunc", 300), ("tsdf_pits", 300), ("nn", 120), ("fxfy", 300)],
    "big": [("max", 50), ("fxfy", 40), ("trunc", 40)],
    "ortho": [("max", 450), ("tsdf_pits", 450)],
}


@pytest.mark.parametrize("family", list(MARGIN_FLOORS))
def test_needle_scenes_reach_the_margins(family):
    """In float64: the pixels the bilinear samples of a brick can read form its tap rectangle; a margin pair is a
    (brick, view) pair with needles on the rectangle's outer ring and none inside.  The oracle must show the needles'
    effect in enough of them, and the tie view (image == the state's minimum) must change a voxel, or the GPU tests
    above would pass with a bound that is a pixel or a rounding step short."""
    total_hits = 0
    for mode, floor in MARGIN_FLOORS[family]:
        sc = N.make_scene(family, mode)
        nv = len(sc["views"])
        _, effect = N.oracle_run(sc, [list(range(nv))], effects=True)
        hits, pairs = N.margin_pairs(sc, effect)
        assert hits >= floor, (family, mode, hits, pairs)
        total_hits += hits
        if sc["kind"] == "needles" and N.MODES[mode]["uo"].get("sdf_interp", 1) == 1:
            assert int(effect[2].sum()) > 0, (family, mode, "the tie view changes nothing")
    assert total_hits >= 300, (family, total_hits)
