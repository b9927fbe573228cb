"""The carve kernels on the lattice scenes (lattice_scenes.py), against the CPU oracle bit for bit: voxels that project
exactly onto the nearest-neighbour tie, onto integers, onto roi_min and roi_max, onto the float below .5, next to pixels of
exactly -1 and poisoned pixels just outside the ROI.  The fused kernel answers such a voxel by one of several
implementations -- the select-free run of a `sure` tile, the checked loop over the staged tile, sample_generic for a voxel
the tile refuses, the per-view kernel -- and the depth carve, the robust carve and the vertex colouring carry samplers of
their own; every one of them must land on the reference's side of every equality.  test_lattice_scenes_cpu.py shows, from
the oracle alone, that the scenes reach those equalities and that a sampler with any of the named defects would differ.

Per update mode and grid: (a) every view alone on a fresh context, (b) all views in as few launches as one projection
model per launch allows (a mixed launch is the per-view kernel's: the config with "fused" 0 gets one), (c) one launch per
view with the state compared after each, (d) the sequence begun at its second view, where under kMax a view that is `sure`
everywhere (pin_half) meets the bricks the ROI view before it left partly touched."""
import functools

import numpy as np
import pytest

import color_cases as CC
import color_ref as CR
import depth_ref as DR
import lattice_scenes as L
import oracle_lib as O
import robust_ref as R
from test_gpu_view_loop_paths import assert_state_equal
from vacancy_amd import carver as vc
from vacancy_amd.capi import VCY_INTERP_NN

pytestmark = pytest.mark.gpu

GRIDS = list(L.GRIDS)
MODES = {
    "max": dict(),
    "nn": dict(sdf_interp=VCY_INTERP_NN),
    "max_limit": dict(voxel_max_update_num=3),
    "wa_unit_trunc": dict(voxel_update=1, use_truncation=True, truncation_band=0.1),
    "wa_037": dict(voxel_update=1, voxel_update_weight=0.37),
    "outside_max": dict(update_outside=1),
    "nn_trunc": dict(sdf_interp=VCY_INTERP_NN, use_truncation=True, truncation_band=0.1),
}
NV = len(L.VIEW_NAMES)
N_PIN = sum(1 for n in L.VIEW_NAMES if not L.VIEWS[n][7])  # the pinhole views come first, the orthographic ones last
assert all(L.VIEWS[n][7] == (i >= N_PIN) for i, n in enumerate(L.VIEW_NAMES))

# ("fused", "cull", "tile"): raw tiles, the same without view dropping, the tile kind the host picks, big tiles, the
# per-view kernel
CONFIGS = [dict(fused=1, cull=1, tile=1), dict(fused=1, cull=0, tile=1), dict(fused=1, cull=1, tile=0),
           dict(fused=1, cull=1, tile=2), dict(fused=0)]
# run (c) only -- test_gpu_drop_margins' single-view flavours (livelist, listrecords, recordbytes, rowkernel), on raw
# tiles: the one-view instance and the row kernel are not taken with big tiles
SINGLE_FLAVOURS = [dict(defer=0, oneview=1, tile=1, livelist=ll, listrecords=lr, recordbytes=rb, rowkernel=rk)
                   for ll, lr, rb, rk in [(1, 1, 0, -1), (0, 1, 0, -1), (1, 0, 0, -1), (1, 1, 2000, -1), (0, 0, 2000, 0),
                                          (1, 1, 0, 0)]]
PROLOGUE = dict(fused=1, cull=1, tile=1, prologue=1)


def launches_of(run):
    """[view indices of a launch] of a run; a fused launch holds one projection model."""
    pin, ortho = list(range(N_PIN)), list(range(N_PIN, NV))
    if run == "batch":
        return [pin, ortho]
    if run == "each":
        return [[i] for i in range(NV)]
    if run == "from_second":
        return [pin[1:], ortho, [0]]
    if run == "mixed":  # one call with both projection models: the per-view kernel
        return [pin + ortho]
    raise KeyError(run)


@functools.lru_cache(maxsize=None)
def oracle_after(grid, mode, order):
    """[(sdf, update_num) after each view of `order`] from a fresh grid -- computed once, never modified."""
    orc = O.OracleGrid(L.grid_option(grid, **MODES[mode]))
    sc = L.scene()
    out = []
    for i in order:
        orc.carve(sc[i][1], sc[i][2])
        s, u = orc.download()
        s.setflags(write=False)
        u.setflags(write=False)
        out.append((s, u))
    orc.close()
    return out


def make_dev(grid, mode, params, z_range=None):
    dev = vc.VoxelCarver(L.grid_option(grid, **MODES[mode]), z_range=z_range)
    assert dev.Init(), vc.last_error()
    for k, v in params.items():
        dev.set_param(k, v)
    return dev


def carve_and_compare(grid, mode, launches, params, host_images=False, with_div_level=False):
    """The launches on a fresh context with these parameters, the state compared with the oracle's after every launch."""
    sc = L.scene()
    order = tuple(i for la in launches for i in la)
    want = oracle_after(grid, mode, order)
    dev = make_dev(grid, mode, params)
    imgs = None if host_images else [dev.upload_sdf(im) for _, _, im in sc]
    done = 0
    for la in launches:
        if host_images:
            for i in la:
                assert dev.Carve(sc[i][1], sc[i][2]), vc.last_error()
        else:
            assert dev.CarveBatchDevice([sc[i][1] for i in la], [imgs[i] for i in la]), vc.last_error()
        done += len(la)
        ctx = "%s %s %r after %s" % (grid, mode, params, "+".join(L.VIEW_NAMES[i] for i in order[:done][-3:]))
        if with_div_level:
            ctx += " (div_level %d)" % dev.get_param("div_level")
        assert_state_equal(*dev.download(), *want[done - 1], ctx)
    for p in imgs or []:
        dev.free_device(p)
    dev.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", GRIDS)
def test_every_view_alone_on_a_fresh_context(grid, mode):
    """(a) the first touch: the state IS the sample, nothing masks it."""
    for i in range(NV):
        for params in CONFIGS:
            carve_and_compare(grid, mode, [[i]], params)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", GRIDS)
def test_all_views_in_one_launch_per_projection(grid, mode):
    """(b), and the mixed call through the per-view kernel."""
    for params in CONFIGS:
        carve_and_compare(grid, mode, launches_of("batch"), params)
    carve_and_compare(grid, mode, launches_of("mixed"), dict(fused=0))
    carve_and_compare(grid, mode, launches_of("mixed"), dict(fused=1))  # (not eligible: the same kernel, chosen by the library)
    carve_and_compare(grid, mode, launches_of("batch"), PROLOGUE)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", GRIDS)
def test_one_launch_per_view(grid, mode):
    """(c), also through the single-view flavours and with the footprints made in the kernel's prologue."""
    for params in CONFIGS + [PROLOGUE]:
        carve_and_compare(grid, mode, launches_of("each"), params)
    for params in SINGLE_FLAVOURS:
        carve_and_compare(grid, mode, launches_of("each"), params, host_images=True)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", GRIDS)
def test_sequence_begun_at_its_second_view(grid, mode):
    """(d)"""
    for params in CONFIGS:
        carve_and_compare(grid, mode, launches_of("from_second"), params)


@pytest.mark.parametrize("shortdiv", [1, 0])
@pytest.mark.parametrize("mode", ["max", "nn_trunc", "wa_unit_trunc"])
@pytest.mark.parametrize("grid", GRIDS)
def test_short_division_on_exact_quotients(grid, mode, shortdiv):
    """fx and pc.z both powers of two, 48 / 96, and inexact quotients on the slices around them: div_view<DIV> at both
    settings of "shortdiv"; a failure names the division sequence the launch used."""
    for tile in (1, 2):
        params = dict(fused=1, cull=1, tile=tile, shortdiv=shortdiv)
        carve_and_compare(grid, mode, launches_of("batch"), params, with_div_level=True)
        carve_and_compare(grid, mode, launches_of("each"), params, with_div_level=True)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cut", [8, 7], ids=["exact_slice_ends_lower_slab", "exact_slice_begins_upper_slab"])
def test_z_slabs_cut_at_the_exact_slice(cut, mode):
    """Two z-slab contexts; the slice with pc.z == 64 (z index 7) is the last of the lower slab or the first of the upper."""
    grid = "24x16x16"
    sc = L.scene()
    launches = launches_of("batch")
    want = oracle_after(grid, mode, tuple(i for la in launches for i in la))
    slabs = []
    for zr in ((0, cut), (cut, 16)):
        dev = make_dev(grid, mode, dict(), z_range=zr)
        assert dev.z_range == zr
        dev.imgs = [dev.upload_sdf(im) for _, _, im in sc]
        slabs.append(dev)
    done = 0
    for la in launches:
        for dev in slabs:
            assert dev.CarveBatchDevice([sc[i][1] for i in la], [dev.imgs[i] for i in la]), vc.last_error()
        done += len(la)
        parts = [dev.download() for dev in slabs]
        ds, du = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        assert_state_equal(ds, du, *want[done - 1], "slabs cut at %d, %s, after %d views" % (cut, mode, done))
    for dev in slabs:
        for p in dev.imgs:
            dev.free_device(p)
        dev.close()


# ---- the other kernels with a sampler of their own ----------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["max", "nn"])
@pytest.mark.parametrize("grid", GRIDS)
def test_robust_carve(grid, mode):
    """CarveRobustDevice at m = 0 and m = 1 against the restatement (robust_ref.py: the samples are the oracle's)."""
    sc = L.scene()
    views, sdfs = [v for _, v, _ in sc], [im for _, _, im in sc]
    opt = L.grid_option(grid, **MODES[mode])
    has, val = R.samples(opt, views, sdfs)
    dev = make_dev(grid, mode, dict())
    ptrs = [dev.upload_sdf(s) for s in sdfs]
    for m in (0, 1):
        got = dev.CarveRobustDevice(views, ptrs, m, 0.0)
        sdf, cnt, over = R.robust_from_samples(has, val, m, 0.0)
        ds, du = dev.download()
        ctx = "%s %s m = %d" % (grid, mode, m)
        assert np.array_equal(du, cnt), "%s: %d update_num differ" % (ctx, int((du != cnt).sum()))
        R.assert_sdf_equal(ds, sdf, ctx)
        assert np.array_equal(got["overruled"], over), (ctx, got["overruled"], over)
    for p in ptrs:
        dev.free_device(p)
    dev.close()


@pytest.mark.parametrize("mode", ["max", "wa_037"])
@pytest.mark.parametrize("grid", GRIDS)
def test_depth_carve(grid, mode):
    """CarveDepthDevice (depth_sample.h: its own roundf / clamp / ROI test) against depth_ref.py; finite depths on the
    sampled pixels, +inf / NaN / 0 just outside the ROI."""
    views = [L.make(n) for n in L.VIEW_NAMES]
    depths = [L.depth_image(n) for n in L.VIEW_NAMES]
    opt = L.grid_option(grid, **MODES[mode])
    band = 2.0
    stats = {}
    want = DR.carve_depth(opt, views, depths, band, stats=stats)
    assert stats["between"] > 1000 and stats["clamped"] > 0 and stats["dropped"] > 0, stats
    dev = make_dev(grid, mode, dict())
    ptrs = [dev.upload_sdf(d) for d in depths]
    dev.CarveDepthDevice(views, ptrs, band)
    ds, du = dev.download()
    ctx = "%s %s depth" % (grid, mode)
    assert np.array_equal(du, want[1]), "%s: %d update_num differ" % (ctx, int((du != want[1]).sum()))
    R.assert_sdf_equal(ds, want[0], ctx)
    # view by view on fresh contexts: the first touch of every view's own sampler
    for i, (v, d) in enumerate(zip(views, depths)):
        one = DR.carve_depth(opt, [v], [d], band)
        dev.reset()
        dev.CarveDepthDevice([v], [ptrs[i]], band)
        ds, du = dev.download()
        ctx = "%s %s depth, %s alone" % (grid, mode, L.VIEW_NAMES[i])
        assert np.array_equal(du, one[1]), "%s: %d update_num differ" % (ctx, int((du != one[1]).sum()))
        R.assert_sdf_equal(ds, one[0], ctx)
    for p in ptrs:
        dev.free_device(p)
    dev.close()


@pytest.mark.parametrize("interp", [CR.NN, CR.BILINEAR], ids=["nn", "bilinear"])
@pytest.mark.parametrize("grid", GRIDS)
def test_vertex_colours(grid, interp):
    """ColorVertices (color.hip: its own roundf / floorf / clamp / ROI test) against color_ref.py.  The vertices are the
    voxel centres of the tie, integer, ROI-edge and below-half classes of any view; the depth is supplied and the
    tolerance so large that no vertex is occluded: what is compared is the sampling."""
    pos = L.positions(grid)
    views = [L.make(n) for n in L.VIEW_NAMES]
    pick = np.zeros(len(pos), bool)
    for v in views:
        c = L.classify(v, pos)
        pick |= c["half"] | c["integer"] | c["roi_min"] | c["roi_max"] | c["below_half"]
    p = np.ascontiguousarray(pos[pick])
    assert len(p) > 1000
    photos = [L.photo(n) for n in L.VIEW_NAMES]
    depths = [np.zeros((L.H, L.W), np.float32) for _ in views]
    tol, fallback = 1.0e6, (1.0, 2.0, 3.0)
    dev = make_dev(grid, "max", dict())
    # all views together (the mean over the views that see the vertex), then each alone (the sample itself)
    for sel in [list(range(NV))] + [[i] for i in range(NV)]:
        vs, ph, dp = [views[i] for i in sel], [photos[i] for i in sel], [depths[i] for i in sel]
        want = CR.color_vertices(p, None, vs, ph, dp, CR.MEAN, interp, tol, 0.0, fallback)
        got = dev.ColorVertices(p, vs, ph, None, dp, CR.MEAN, interp, tol, 0.0, fallback)
        CC.assert_equal(got, want, "%s interp %d views %s" % (grid, interp, [L.VIEW_NAMES[i] for i in sel]))
        assert int(want[1].sum()) > 0
    dev.close()
