"""Connected components of a grid cut into z-slabs: vcy_label_components_slab on every slab's device, the seam pairs
kernel on the upper slab of every seam, the host merge, and the per-slab filter (components.hip), through
ShardedVoxelCarver.LabelComponents / KeepComponents and through the slab-level calls.  All slabs sit on device 0.  The
yardsticks are tests/components_ref.py on the WHOLE state and the whole-grid context's LabelComponents / KeepComponents
(held to that reference by tests/test_gpu_components.py); everything is integer arithmetic, so every assertion is equality."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import components_ref as R
import slab_components_cases as S
from test_gpu_components import (CARVE_PATHS, KEEP_RULES, assert_mesh_equal, bits, box_option, bunny_inputs, make_dev,
                                 random_state, serpentine, state_from_mask, two_blocks_state)
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist
from vacancy_amd import sharded
from vacancy_amd import synth
from vacancy_amd.capi import UpdateOption

pytestmark = pytest.mark.gpu


def make_sharded(option, z_bounds):
    sh = sharded.ShardedVoxelCarver(option, devices=[0], slabs_per_device=len(z_bounds) - 1, z_bounds=list(z_bounds))
    assert sh.Init(), vc.last_error()
    assert sh.z_ranges == list(zip(z_bounds[:-1], z_bounds[1:]))
    return sh


def upload_slabs(sh, sdf, cnt):
    s = sh.dims[0] * sh.dims[1]
    for c, (z0, z1) in zip(sh.slabs, sh.z_ranges):
        c.upload(sdf[z0 * s:z1 * s], cnt[z0 * s:z1 * s])


def download_slabs(sh):
    parts = [c.download() for c in sh.slabs]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def check_sharded_labels(sh, sdf, cnt, iso, want, want_lab, ctx):
    """The merged list and the concatenated labels against the reference of the whole state; every slab's own report
    and every seam's pairs against the numpy restatement of a slab (tests/slab_components_cases.py)."""
    got = sh.LabelComponents(iso, labels=True)
    assert set(got) == {"label", "n_voxels", "bb_min", "bb_max", "labels", "device_ms"}
    R.assert_components_equal(got, want, ctx)
    bad = int((got["labels"] != want_lab).sum())
    assert bad == 0, "%s: the merged labels of %d voxels differ from the reference" % (ctx, bad)
    assert got["device_ms"] >= 0.0
    # the slab level once more, by hand
    solid = R.solid_mask(sdf, cnt, iso)
    bounds = [z0 for z0, _ in sh.z_ranges] + [sh.z_ranges[-1][1]]
    lists, pairs, labs = S.cut_volume(solid, sh.dims, bounds)
    planes = []
    for s, c in enumerate(sh.slabs):
        part = c.LabelComponentsSlab(iso, labels=True)
        R.assert_components_equal(part, lists[s], "%s slab %d" % (ctx, s))
        assert np.array_equal(part["labels"], labs[s]), "%s slab %d: provisional labels" % (ctx, s)
        planes.append(c.component_top_plane())
        assert np.array_equal(planes[s], labs[s][-sh.dims[0] * sh.dims[1]:]), "%s slab %d: top plane" % (ctx, s)
        if s > 0:
            got_pairs = c.component_seam_pairs(planes[s - 1])
            want_pairs = np.unique(pairs[s - 1], axis=0) if len(pairs[s - 1]) else np.zeros((0, 2), np.int64)
            assert np.array_equal(got_pairs, want_pairs), "%s seam below slab %d: pairs" % (ctx, s)
    return got


# ---- 1. random states ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", S.DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_random_states(dims):
    opt = box_option(dims)
    states = []
    for k, (density, iso) in enumerate(itertools.product(S.DENSITIES, (0.0, 0.0125, -0.05))):
        sdf, cnt = random_state(dims, density, iso, 100 + k)
        want, want_lab = R.reference(sdf, cnt, dims, iso)
        assert len(want["label"]) > 0
        states.append((density, iso, sdf, cnt, want, want_lab))
    cuts = S.cuts_for(dims[2])
    assert [0, 2, dims[2]] in cuts and [0, dims[2] - 2, dims[2]] in cuts
    for bounds in cuts:
        sh = make_sharded(opt, bounds)
        assert sh.dims == tuple(dims)
        for density, iso, sdf, cnt, want, want_lab in states:
            upload_slabs(sh, sdf, cnt)
            check_sharded_labels(sh, sdf, cnt, iso, want, want_lab, "%s density %g iso %g cuts %s" % (dims, density, iso, bounds))
            s2, c2 = download_slabs(sh)
            assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt), "labelling changed the state"
        sh.close()


# ---- 2. serpentine: one component through every seam ---------------------------------------------------------------

@pytest.mark.parametrize("slabs", [2, 3, 12])
@pytest.mark.parametrize("complement", [False, True])
def test_serpentine(complement, slabs):
    n = 24
    solid = serpentine(n)
    path_len = int(solid.sum())
    if complement:
        solid = ~solid
    sdf, cnt = state_from_mask(solid)
    want, want_lab = R.reference(sdf, cnt, (n, n, n), 0.0)
    sh = make_sharded(box_option((n, n, n)), S.equal_cuts(n, slabs))
    upload_slabs(sh, sdf, cnt)
    got = check_sharded_labels(sh, sdf, cnt, 0.0, want, want_lab, "serpentine in %d slabs" % slabs)
    if not complement:
        assert got["label"].tolist() == [0] and got["n_voxels"].tolist() == [path_len]
        assert got["bb_min"].tolist() == [[0, 0, 0]] and got["bb_max"].tolist() == [[n - 1, n - 2, n - 2]]
    else:
        assert got["label"][0] == int(np.flatnonzero(solid)[0]) and got["n_voxels"].sum() == n ** 3 - path_len


# ---- 3. seam edge cases ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bounds", [[0, 5, 10], [0, 2, 4, 6, 8, 10]])
def test_checkerboard_joins_nothing(bounds):
    dims = (17, 9, 10)
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    solid = ((x + y + z) % 2 == 0).reshape(-1)
    sdf, cnt = state_from_mask(solid)
    want, want_lab = R.reference(sdf, cnt, dims, 0.0)
    assert np.array_equal(want["label"], np.flatnonzero(solid)) and (want["n_voxels"] == 1).all()
    sh = make_sharded(box_option(dims), bounds)
    upload_slabs(sh, sdf, cnt)
    check_sharded_labels(sh, sdf, cnt, 0.0, want, want_lab, "checkerboard")
    for c, below in zip(sh.slabs[1:], sh.slabs[:-1]):  # diagonal contact across a seam is no contact
        assert len(c.component_seam_pairs(below.component_top_plane())) == 0


def test_seam_stretches_across_a_64_voxel_word():
    """nx = 130: three words per row.  Stretches of the seam in which both sides are solid: x = 60 .. 70 (goes on from
    the first word into the second: the carry), and ones that start at x = 0, 63, 64 and 129 -- in rows of their own, so
    that every stretch joins its own two pieces."""
    dims = (130, 9, 4)
    lower, upper = np.zeros(dims[::-1], bool), np.zeros(dims[::-1], bool)
    lower[1, 0, 55:76], upper[2, 0, 60:71] = True, True     # both: 60 .. 70
    lower[1, 2, 0:3], upper[2, 2, 0:2] = True, True         # starts at 0
    lower[1, 4, 61:64], upper[2, 4, 63:66] = True, True     # 63 alone: the last voxel of a word
    lower[1, 6, 64:70], upper[2, 6, 62:67] = True, True     # starts at 64: the first voxel of a word, its left neighbour one-sided
    lower[1, 8, 120:130], upper[2, 8, 129] = True, True     # 129: the last voxel of the row
    lower[0, 6, 64:70] = True                               # (a piece whose smallest id is not in the seam plane)
    solid = (lower | upper).reshape(-1)
    sdf, cnt = state_from_mask(solid)
    want, want_lab = R.reference(sdf, cnt, dims, 0.0)
    assert len(want["label"]) == 5
    sh = make_sharded(box_option(dims), [0, 2, 4])
    upload_slabs(sh, sdf, cnt)
    check_sharded_labels(sh, sdf, cnt, 0.0, want, want_lab, "nx 130")
    sh.slabs[1].LabelComponentsSlab(0.0)
    pairs = sh.slabs[1].component_seam_pairs(sh.slabs[0].component_top_plane())
    s = dims[0] * dims[1]
    # (sorted by the lower label: the piece that reaches down into slice 0 comes first)
    assert pairs.tolist() == [[6 * 130 + 64, 2 * s + 6 * 130 + 62], [s + 55, 2 * s + 60], [s + 2 * 130, 2 * s + 2 * 130],
                              [s + 4 * 130 + 61, 2 * s + 4 * 130 + 63], [s + 8 * 130 + 120, 2 * s + 8 * 130 + 129]]


def test_tie_with_the_cut_between_the_blocks():
    dims, (sdf, cnt) = two_blocks_state()
    want, want_lab = R.reference(sdf, cnt, dims, 0.0)
    assert want["n_voxels"].tolist() == [27, 27]
    assert want["bb_max"][0][2] < 5 <= want["bb_min"][1][2], "the cut does not lie between the blocks"
    sh = make_sharded(box_option(dims), [0, 5, 10])
    upload_slabs(sh, sdf, cnt)
    got = check_sharded_labels(sh, sdf, cnt, 0.0, want, want_lab, "two blocks")
    assert got["label"][0] < got["label"][1]


# ---- 4. the slab call on a whole-grid context ----------------------------------------------------------------------

def test_slab_call_on_a_whole_grid():
    dims = (70, 23, 19)
    dev = make_dev(dims)
    sdf, cnt = random_state(dims, 0.31, 0.0125, 7)
    dev.upload(sdf, cnt)
    want = dev.LabelComponents(0.0125, labels=True)
    got = dev.LabelComponentsSlab(0.0125, labels=True)
    R.assert_components_equal(got, want, "whole grid through the slab call")
    assert np.array_equal(got["labels"], want["labels"]) and len(want["label"]) > 1
    # ... and the rest of the sequence is a no-op merge of one slab
    merged, maps = vdist.merge_components([got], [])
    R.assert_components_equal(merged, want, "one slab merged")
    dev.resolve_components(got["label"], maps[0])
    assert np.array_equal(dev.download_labels(), want["labels"])


# ---- 5. global ids above 2^32 ----------------------------------------------------------------------------------------

def test_global_ids_above_2_to_32():
    """A tall narrow grid, 4096 x 64 x 16400: a slice is 2^18 voxels, so every id from slice 16384 on is above 2^32.  Only
    the two top slabs of 2 slices exist; the rest of the grid is never allocated."""
    dims = (4096, 64, 16400)
    nx, ny, nz = dims
    opt = box_option(dims)
    lo, hi = vc.VoxelCarver(opt, z_range=(nz - 4, nz - 2)), vc.VoxelCarver(opt, z_range=(nz - 2, nz))
    assert lo.Init() and hi.Init(), vc.last_error()
    assert lo.dims == dims and hi.z_range == (nz - 2, nz)
    s = nx * ny
    vol = np.zeros((4, ny, nx), bool)                      # the four slices nz - 4 .. nz - 1
    vol[0:2, 2:5, 10:21] = True                            # a box in the lower slab alone: 2 * 3 * 11
    vol[1:3, 10:13, 4000:4096] = True                      # one that crosses the seam: 2 * 3 * 96
    vol[3, 60:64, 0:6] = True                              # one in the upper slab alone: 4 * 6
    sdf, cnt = state_from_mask(vol.reshape(-1))
    lo.upload(sdf[:2 * s], cnt[:2 * s])
    hi.upload(sdf[2 * s:], cnt[2 * s:])
    base = (nz - 4) * s
    assert base > 2 ** 32
    a, b, c = base + 2 * nx + 10, base + s + 10 * nx + 4000, base + 3 * s + 60 * nx
    la, lb = lo.LabelComponentsSlab(0.0), hi.LabelComponentsSlab(0.0)
    assert la["label"].tolist() == [b, a] and la["n_voxels"].tolist() == [288, 66]
    assert lb["label"].tolist() == [b + s, c] and lb["n_voxels"].tolist() == [288, 24]
    assert la["bb_min"].tolist() == [[4000, 10, nz - 3], [10, 2, nz - 4]] and la["bb_max"].tolist() == [[4095, 12, nz - 3], [20, 4, nz - 3]]
    assert lb["bb_min"].tolist() == [[4000, 10, nz - 2], [0, 60, nz - 1]] and lb["bb_max"].tolist() == [[4095, 12, nz - 2], [5, 63, nz - 1]]
    pairs = hi.component_seam_pairs(lo.component_top_plane())
    assert pairs.tolist() == [[b, b + s]]
    merged, maps = vdist.merge_components([la, lb], [pairs])
    assert merged["label"].tolist() == [b, a, c] and merged["n_voxels"].tolist() == [576, 66, 24]
    assert merged["bb_min"].tolist() == [[4000, 10, nz - 3], [10, 2, nz - 4], [0, 60, nz - 1]]
    assert merged["bb_max"].tolist() == [[4095, 12, nz - 2], [20, 4, nz - 3], [5, 63, nz - 1]]
    assert maps[0].tolist() == [b, a] and maps[1].tolist() == [b, c]
    lo.resolve_components(la["label"], maps[0])
    hi.resolve_components(lb["label"], maps[1])
    want = np.full(4 * s, -1, np.int64).reshape(4, ny, nx)
    want[0:2, 2:5, 10:21], want[1:3, 10:13, 4000:4096], want[3, 60:64, 0:6] = a, b, c
    assert np.array_equal(np.concatenate([lo.download_labels(), hi.download_labels()]), want.reshape(-1))
    # the filter with such labels: the crossing box goes, from both slabs
    assert lo.KeepComponentsSlab([b], 1.0)["removed_voxels"] == 288 and hi.KeepComponentsSlab([b + s], 1.0)["removed_voxels"] == 288
    s2 = np.concatenate([lo.download()[0], hi.download()[0]])
    assert np.array_equal(s2 < 0, ((want >= 0) & (want != b)).reshape(-1))


# ---- 6. the filter ------------------------------------------------------------------------------------------------------

def check_sharded_filter(dev, sh, iso, rule, views, masks, rot, full_voxel_mesh, fill=1.0):
    """`dev` (whole grid) and `sh` (slabs) hold the same state.  Both filter; everything that reads the state afterwards
    has to agree, the state itself bit for bit."""
    valid = [c.get_param("brick_min_valid") for c in sh.slabs]
    before = {k: v for k, v in dev.LabelComponents(iso).items() if k != "device_ms"}
    want = dev.KeepComponents(iso, fill_sdf=fill, **rule)
    got = sh.KeepComponents(iso, fill_sdf=fill, **rule)
    assert set(got) == {"removed_components", "removed_voxels", "device_ms"}
    assert (got["removed_components"], got["removed_voxels"]) == (want["removed_components"], want["removed_voxels"])
    assert [c.get_param("brick_min_valid") for c in sh.slabs] == valid
    s1, c1 = dev.download()
    s2, c2 = download_slabs(sh)
    assert np.array_equal(c2, c1), "update_num differs"
    assert np.array_equal(bits(s2), bits(s1)), "%d voxels differ from the whole context's filtered state" % int((bits(s2) != bits(s1)).sum())
    # the labels from before the removal, merged
    assert np.array_equal(np.concatenate([c.download_labels() for c in sh.slabs]), dev.download_labels())
    after = sh.LabelComponents(iso, labels=True)
    R.assert_components_equal(after, R.subset(before, R.kept(before, **rule)), "labelling after the filter")
    after_whole = dev.LabelComponents(iso, labels=True)
    assert np.array_equal(after["labels"], after_whole["labels"])
    for skip in (0, 2):
        dev.set_param("mcskip", skip)
        sh.set_param("mcskip", skip)
        for normals in (False, True):
            assert_mesh_equal(sh.ExtractIsoSurface(iso, True, normals=normals), dev.ExtractIsoSurface(iso, True, normals=normals),
                              "mcskip %d normals %s" % (skip, normals))
    for inside_empty in (True, False):
        if inside_empty or full_voxel_mesh:
            a, b = sh.ExtractVoxel(inside_empty), dev.ExtractVoxel(inside_empty)
            assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(bits(a["vertices"]), bits(b["vertices"]))
    for k in range(4):
        fused, cull = CARVE_PATHS[(k + rot) % 4]
        for d in [dev] + sh.slabs:
            d.set_param("fused", fused)
            d.set_param("cull", cull)
            assert d.CarveSilhouette(views[k % len(views)], masks[k % len(views)]), vc.last_error()
            d.sync()
        s1, c1 = dev.download()
        s2, c2 = download_slabs(sh)
        assert np.array_equal(bits(s2), bits(s1)) and np.array_equal(c2, c1), "fused %d cull %d" % (fused, cull)


@pytest.mark.parametrize("rule", range(3))
def test_filter_random(rule):
    dims, iso = (70, 23, 19), 0.0125
    sdf, cnt = random_state(dims, 0.31, iso, 7)
    views, masks = synth.sphere_views(max(dims), 2, 160, 120)
    for bounds in S.cuts_for(dims[2]):
        dev = make_dev(dims)
        dev.upload(sdf, cnt)
        sh = make_sharded(box_option(dims), bounds)
        upload_slabs(sh, sdf, cnt)
        check_sharded_filter(dev, sh, iso, KEEP_RULES[rule], views, masks, rule, True, fill=0.75)
        sh.close()


@pytest.mark.parametrize("rule", range(3))
def test_filter_ties(rule):
    dims, (sdf, cnt) = two_blocks_state()
    views, masks = synth.sphere_views(max(dims), 2, 160, 120)
    dev = make_dev(dims)
    dev.upload(sdf, cnt)
    sh = make_sharded(box_option(dims), [0, 5, 10])
    upload_slabs(sh, sdf, cnt)
    check_sharded_filter(dev, sh, 0.0, KEEP_RULES[rule], views, masks, rule, True)


@pytest.mark.parametrize("rule", range(3))
@pytest.mark.parametrize("slabs", [2, 3])
@pytest.mark.parametrize("mode,nv", list(itertools.product(("default", "tsdf"), (2, 6))))
def test_filter_bunny(mode, nv, slabs, rule):
    views, masks = bunny_inputs()
    opt = B.bunny_option(10.0, UpdateOption(**B.MODES[mode]))
    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=slabs)
    assert sh.Init(), vc.last_error()
    for i in range(nv):
        for d in [dev] + sh.slabs:
            assert d.CarveSilhouette(views[i], masks[i]), vc.last_error()
    for d in [dev] + sh.slabs:
        d.sync()
    # a carved scene: the brick minima are valid on every slab, and have to stay so (the brick-skipping extraction and the
    # carve inside check_sharded_filter are the proof that they are also right)
    assert all(c.get_param("brick_min_valid") == 1 for c in sh.slabs)
    if nv == 2 and rule == 0:
        assert len(dev.LabelComponents(0.0)["label"]) >= 2, "the scene has no floater to remove"
    check_sharded_filter(dev, sh, 0.0, KEEP_RULES[rule], views[2:4], masks[2:4], rule, True)


# ---- 7. untouched slab contexts -------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["init", "reset"])
def test_untouched_slab_context(how):
    n, nv = 24, 2
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, nv, 160, 120)
    dev, plain = vc.VoxelCarver(opt, z_range=(8, 24)), vc.VoxelCarver(opt, z_range=(8, 24))
    assert dev.Init() and plain.Init(), vc.last_error()
    if how == "reset":
        for d in (dev, plain):
            assert d.CarveSilhouette(views[0], masks[0]), vc.last_error()
            d.sync()
            d.reset()
    got = dev.LabelComponentsSlab(0.0, labels=True)
    assert len(got["label"]) == 0 and (got["labels"] == -1).all() and got["device_ms"] == 0.0
    assert (dev.component_top_plane() == -1).all()
    assert len(dev.component_seam_pairs(np.zeros(dev.dims[0] * dev.dims[1], np.int64))) == 0
    dev.resolve_components([], [])
    assert dev.KeepComponentsSlab([], 1.0)["removed_voxels"] == 0
    assert dev.get_param("brick_min_valid") == plain.get_param("brick_min_valid") == 0
    for d in (dev, plain):
        assert d.CarveSilhouette(views[1], masks[1]), vc.last_error()
        d.sync()
    assert dev.get_param("brick_min_valid") == plain.get_param("brick_min_valid") == 1
    assert dev.state_diff(plain) == 0


# ---- 8. errors, each with the state untouched ------------------------------------------------------------------------

def test_slab_call_errors():
    dims, (sdf, cnt) = two_blocks_state()
    s = dims[0] * dims[1]
    opt = box_option(dims)
    lo, hi = vc.VoxelCarver(opt, z_range=(0, 5)), vc.VoxelCarver(opt, z_range=(5, 10))
    assert lo.Init() and hi.Init(), vc.last_error()
    lo.upload(sdf[:5 * s], cnt[:5 * s])
    hi.upload(sdf[5 * s:], cnt[5 * s:])
    lib = capi.load()
    one = np.zeros(1, np.int64)
    plane = np.full(s, -1, np.int64)
    gone = C.c_int64(7)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    def unchanged():
        a, b = lo.download(), hi.download()
        return np.array_equal(bits(np.concatenate([a[0], b[0]])), bits(sdf)) and np.array_equal(np.concatenate([a[1], b[1]]), cnt)

    # before any labelling
    p, n = C.POINTER(C.c_int64)(), C.c_int64(5)
    assert lib.vcy_component_top_plane(hi.ctx, ptr(plane)) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_component_seam_pairs(hi.ctx, ptr(plane), C.byref(p), C.byref(n)) == capi.VCY_ERR_INVALID_ARG and n.value == 0
    assert lib.vcy_resolve_components_slab(hi.ctx, 0, None, None) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_keep_components_slab(hi.ctx, 1.0, 0, None, C.byref(gone)) == capi.VCY_ERR_INVALID_ARG and gone.value == 0
    assert "vcy_label_components_slab" in vc.last_error()
    # a whole-grid labelling is not a slab labelling either, and the old entries still refuse a slab
    with pytest.raises(RuntimeError):
        hi.LabelComponents(0.0)
    assert "whole grid" in vc.last_error()
    la, lb = lo.LabelComponentsSlab(0.0), hi.LabelComponentsSlab(0.0)
    assert len(la["label"]) == len(lb["label"]) == 1
    # a map, and a removal list, naming a label the slab did not report
    one[0] = la["label"][0]
    assert lib.vcy_resolve_components_slab(hi.ctx, 1, ptr(one), ptr(one)) == capi.VCY_ERR_INVALID_ARG
    assert "reported no component" in vc.last_error()
    assert lib.vcy_keep_components_slab(hi.ctx, 1.0, 1, ptr(one), C.byref(gone)) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_resolve_components_slab(hi.ctx, 2, ptr(np.zeros(2, np.int64)), ptr(np.zeros(2, np.int64))) == capi.VCY_ERR_INVALID_ARG
    assert np.array_equal(hi.download_labels(), np.where(R.solid_mask(sdf, cnt, 0.0)[5 * s:], lb["label"][0], -1))
    # the seam-pair call on the slab that starts at slice 0
    assert lib.vcy_component_seam_pairs(lo.ctx, ptr(plane), C.byref(p), C.byref(n)) == capi.VCY_ERR_INVALID_ARG
    assert "slice 0" in vc.last_error()
    # fill_sdf: finite and not below the iso level of the labelling
    one[0] = lb["label"][0]
    for fill in (-0.25, float("nan"), float("inf"), float("-inf")):
        assert lib.vcy_keep_components_slab(hi.ctx, fill, 1, ptr(one), C.byref(gone)) == capi.VCY_ERR_INVALID_ARG, fill
    sh = make_sharded(opt, [0, 5, 10])
    upload_slabs(sh, sdf, cnt)
    with pytest.raises(RuntimeError):
        sh.KeepComponents(0.5, fill_sdf=0.25)
    s2, c2 = download_slabs(sh)
    assert np.array_equal(bits(s2), bits(sdf)) and np.array_equal(c2, cnt)
    assert unchanged()
    # a state that changed under the labels: the seam calls ask for a new labelling
    hi.upload(sdf[5 * s:], cnt[5 * s:])
    assert lib.vcy_keep_components_slab(hi.ctx, 1.0, 1, ptr(one), C.byref(gone)) == capi.VCY_ERR_INVALID_ARG
    assert unchanged()
    # ... and with one, fill_sdf == iso_level is allowed and the piece goes
    hi.LabelComponentsSlab(0.0)
    assert hi.KeepComponentsSlab(one, 0.0)["removed_voxels"] == 27


# ---- 9. the C++ facade ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slabs", [2, 3])
def test_cpp_sharded_carver(slabs):
    """vacancy::ShardedVoxelCarver::LabelComponents / KeepLargestComponents next to a single vacancy::VoxelCarver, through
    host_selftest: equal lists before and after the filter, and the same kept mesh."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([os.path.join(root, "vacancy_amd", "host", "host_selftest"), B.BUNNY, "shardcomponents", "10",
                          str(slabs)], check=True, capture_output=True, text=True).stdout
    row = [l for l in out.splitlines() if l.startswith("SHARDCOMPONENTS")][0].split()
    # slabs, components before, lists equal, components after (largest = 1 keeps one), lists equal, meshes identical
    assert row[1] == str(slabs) and int(row[2]) >= 1 and row[3:] == ["1", "1", "1", "1"], row
