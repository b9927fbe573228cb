"""The ray-cast of the hull on the device where a ray's plane crossings TIE (render.hip: the one-crossing step, the brick
jump with count_before, the entry jump -- three implementations of "merged by (t, axis) ascending"), against the numpy
restatement (tests/render_ref.py) on the scenes of tests/ray_lattice_scenes.py: depth BITS, voxel ids and entry axes,
with "rayskip" on and off, for the whole grid, z-slab contexts with their host merge, the agreement counts and the
colouring's internal depth render.  tests/test_ray_lattice_cpu.py shows without a GPU what these scenes hold and which
wrong comparisons they tell apart."""
import numpy as np
import pytest

import color_cases as CC
import color_ref as CR
import ray_lattice_scenes as R
import render_ref as RR
import slab_render_cases as S
from test_gpu_render import assert_images_equal, bits, make_dev
from vacancy_amd import carver as vc

pytestmark = pytest.mark.gpu

F = np.float32
KW = dict(voxel_ids=True, axes=True)


def all_misses(g):
    return np.all(np.isposinf(g["depth"])) and np.all(g["voxel"] == -1) and np.all(g["axis"] == 255)


# ---- 1. the whole grid -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rayskip", [1, 0])
@pytest.mark.parametrize("grid", R.GRID_NAMES)
def test_whole_grid_equals_restatement(grid, rayskip):
    dims = R.dims_of(grid)
    dev = make_dev(R.option(grid), dims)
    dev.set_param("rayskip", rayskip)
    names = R.VIEW_NAMES
    vs = [R.views(grid)[vn] for vn in names]
    hits = 0
    for sn in R.COMMON_STATES:
        sdf, cnt, iso = R.state(grid, sn)
        dev.upload(sdf, cnt)   # (one context through all states: every upload must make the kept bit planes stale)
        for vn, g in zip(names, dev.RenderHull(vs, iso, **KW)):
            assert_images_equal(g, R.want(grid, vn, sn), "%s %s %s rayskip %d" % (grid, sn, vn, rayskip))
            hits += int((g["voxel"] >= 0).sum())
            assert sn != "empty_hull" or all_misses(g)
        s2, c2 = dev.download()
        assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt), "rendering changed the state"
    assert hits > 10000
    for own in names:          # the corner_cut state of every view: all views in one call, and its own view alone
        sdf, cnt, iso = R.corner_cut(grid, own)
        dev.upload(sdf, cnt)
        for vn, g in zip(names, dev.RenderHull(vs, iso, **KW)):
            assert_images_equal(g, R.want(grid, vn, "corner_cut", own), "%s corner_cut of %s in %s rayskip %d" % (grid, own, vn, rayskip))
        alone = dev.RenderHull(R.views(grid)[own], iso, **KW)
        assert_images_equal(alone, R.want(grid, own, "corner_cut"), "%s corner_cut %s alone rayskip %d" % (grid, own, rayskip))
        assert (alone["voxel"] >= 0).sum() >= 5, own


# ---- 2. z-slabs and their merge --------------------------------------------------------------------------------------

def slab_scenes():
    """(view, state, the view whose corner_cut state it is): the common states in every view, corner_cut in its own"""
    return [(vn, sn, vn if sn == "corner_cut" else None) for sn in R.SLAB_STATES for vn in R.VIEW_NAMES]


@pytest.mark.parametrize("rayskip", [1, 0])
@pytest.mark.parametrize("cut", list(R.CUT_SETS))
@pytest.mark.parametrize("grid", R.GRID_NAMES)
def test_slabs_equal_restatement_and_merge(grid, cut, rayskip):
    dims = R.dims_of(grid)
    nxy = dims[0] * dims[1]
    bounds = R.CUT_SETS[cut]
    parts = {}
    for z0, z1 in zip(bounds[:-1], bounds[1:]):
        dev = make_dev(R.option(grid), dims, z_range=(z0, z1))
        dev.set_param("rayskip", rayskip)
        for sn in R.SLAB_STATES:
            for own in (R.VIEW_NAMES if sn == "corner_cut" else [None]):
                sdf, cnt, iso = R.state(grid, sn, own)
                dev.upload(sdf[z0 * nxy:z1 * nxy], cnt[z0 * nxy:z1 * nxy])
                names = [own] if own else R.VIEW_NAMES
                vs = [R.views(grid)[vn] for vn in names]
                for vn, v, g in zip(names, vs, dev.RenderHullSlab(vs, iso, hits=True, **KW)):
                    want = R.want(grid, vn, sn, own, (z0, z1))
                    ctx = "%s %s %s slab [%d, %d) rayskip %d" % (grid, sn, vn, z0, z1, rayskip)
                    assert_images_equal(g, want, ctx)
                    assert np.array_equal(g["hits"], S.pack_hits(want[1], v)), "%s: hit bits differ" % ctx
                    parts.setdefault((vn, sn), []).append(g)
        dev.close()
    hits = 0
    for (vn, sn), p in parts.items():
        merged = vc.render_merge_host(R.views(grid)[vn], p)
        assert_images_equal(merged, R.want(grid, vn, sn), "%s %s %s merged over %s rayskip %d" % (grid, sn, vn, cut, rayskip))
        hits += int((merged["voxel"] >= 0).sum())
    assert len(parts) == len(slab_scenes()) and hits > 5000


# ---- 3. agreement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rayskip", [1, 0])
@pytest.mark.parametrize("grid", R.GRID_NAMES)
def test_agreement_equals_restatement(grid, rayskip):
    dims = R.dims_of(grid)
    dev = make_dev(R.option(grid), dims)
    dev.set_param("rayskip", rayskip)
    names = R.VIEW_NAMES
    vs = [R.views(grid)[vn] for vn in names]
    rng = np.random.RandomState(51)
    masks = [(rng.randint(0, 256, (R.H, R.W)) * (rng.rand(R.H, R.W) < 0.5)).astype(np.uint8) for _ in vs]
    both = 0
    for sn in ("random_0.3", "random_0.03", "random_0.004"):
        sdf, cnt, iso = R.state(grid, sn)
        dev.upload(sdf, cnt)
        counts = dev.HullAgreement(vs, masks, iso)
        for vn, v, m, k in zip(names, vs, masks, counts):
            assert k.tolist() == RR.agreement(v, R.want(grid, vn, sn)[1], m), (grid, sn, vn, rayskip)
            both += int(k[0])
    for vn, v, m in zip(names, vs, masks):
        sdf, cnt, iso = R.corner_cut(grid, vn)
        dev.upload(sdf, cnt)
        k = dev.HullAgreement([v], [m], iso)[0]
        assert k.tolist() == RR.agreement(v, R.want(grid, vn, "corner_cut")[1], m), (grid, vn, rayskip)
    assert both > 1000


# ---- 4. the colouring's internal depth render ------------------------------------------------------------------------

@pytest.mark.parametrize("rayskip", [1, 0])
@pytest.mark.parametrize("grid", R.GRID_NAMES)
def test_colour_through_the_internal_render(grid, rayskip):
    dims = R.dims_of(grid)
    dev = make_dev(R.option(grid), dims)
    dev.set_param("rayskip", rayskip)
    names = R.VIEW_NAMES
    vs = [R.views(grid)[vn] for vn in names]
    ph = CC.photos(vs, 52)
    rng = np.random.RandomState(53)
    half = np.array(dims) / 2.0 * 1.2
    p = ((rng.rand(400, 3) * 2.0 - 1.0) * half).astype(F)
    p[:100] = np.round(p[:100])                       # lattice points: they project onto the tied rays' pixels
    nr = rng.randn(400, 3)
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F)
    for sn in ("random_0.03", "random_0.3"):
        sdf, cnt, iso = R.state(grid, sn)
        dev.upload(sdf, cnt)
        depth = [R.want(grid, vn, sn)[0] for vn in names]      # the restatement's depth images
        for mode, interp in ((CR.WEIGHTED, CR.BILINEAR), (CR.BEST, CR.NN)):
            a = dev.ColorVertices(p, vs, ph, nr, None, mode, interp, 0.6, 0.05, (9.0, 8.0, 7.0), iso_level=iso)
            b = dev.ColorVertices(p, vs, ph, nr, depth, mode, interp, 0.6, 0.05, (9.0, 8.0, 7.0))
            CC.assert_equal(a, (b["rgb"], b["n_used"], b["best_view"]), "%s %s rayskip %d mode %d" % (grid, sn, rayskip, mode))
        seen = dev.ColorVertices(p, vs, ph, None, None, CR.MEAN, CR.NN, 0.6, iso_level=iso)
        free = dev.ColorVertices(p, vs, ph, None, [np.full_like(d, np.inf) for d in depth], CR.MEAN, CR.NN, 0.6)
        assert (seen["n_used"] < free["n_used"]).sum() > 20, "the hull occludes nothing: the test shows nothing"
