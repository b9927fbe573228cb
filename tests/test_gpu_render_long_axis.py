"""The ray-cast of the hull with its plane tables on either side of what the kernel keeps in LDS (render.hip:
rn_cast_kernel<LDS, ...> holds the three tables in LDS when nx + ny + nz + 3 <= kLdsPlanes and reads them from global
memory otherwise).  Two grids of resolution 1, two voxels high:

  (12281, 2, 2)   12288 table entries: the last LDS case, with the 48 KiB dynamic allocation
  (12282, 2, 4)   12291 entries: tables in global memory, the y and z tables begin beyond index 12282

against the numpy restatement (tests/render_ref.py), whole grid with "rayskip" on and off, the agreement counts, and on
the second grid the z-slabs [0, 2) and [2, 4) with their merge.  The images are 16 x 12, so that the restatement's
[pixels, planes] tables stay small; its answers are computed once.  render_ref.render takes one round per crossing of
the longest path, about a millisecond each, and follows a miss through every plane ahead of it, 6 000 to 12 000 rounds
in every view here: the expected images are those of ray_lattice_scenes.render_by_sorting, the same definition read as
one sort per pixel, which is held against render_ref.render on one view here and on the tie scenes in
test_ray_lattice_cpu.py."""
import os
import re

import numpy as np
import pytest

import ray_lattice_scenes as R
import render_ref as RR
import slab_render_cases as S
import test_gpu_render as T
from vacancy_amd import carver as vc
from vacancy_amd.capi import CarverOption, make_view

pytestmark = pytest.mark.gpu

F = np.float32
LDS_PLANES = 12288   # rn::kLdsPlanes
GRIDS = [(12281, 2, 2), (12282, 2, 4)]
W, H = 16, 12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def option(dims):
    h = [n / 2.0 for n in dims]   # (12281 / 2 is exact in float: the box is dims voxels of 1)
    return CarverOption(bb_min=[-x for x in h], bb_max=h, resolution=1.0)


def pinhole(rot, centre, f):
    r = np.array(rot, np.float64)
    w2c = np.zeros((3, 4), F)
    w2c[:, :3] = r
    w2c[:, 3] = 0.0 - r @ np.array(centre, np.float64)
    return make_view(w2c, f, f, W / 2.0, H / 2.0, W, H)


def views_for(dims):
    """name -> view.  The grid spans x in [-h, h] with h about 6141 and y, z in [-1, 1] or [-2, 2]."""
    h = dims[0] / 2.0
    across = np.zeros((3, 4), F)
    across[:, :3] = np.eye(3)
    across[:, 3] = (-(h - 12.25), 5.625, 5.0)          # ortho: x = u + h - 12.25, y = v - 5.625, from z = -5 along +z
    return {
        # from outside the low end along +x, f = 2^17: the outermost rays drift 0.75 over the whole length and leave
        # through y or z just before the far end, the others walk all 12 28x cells
        "along_px": pinhole(((0, 1, 0), (0, 0, 1), (1, 0, 0)), (-h - 3.0, 0.25, -0.25), 131072.0),
        # from inside, 20 cells before the far end, along -x
        "along_nx_inside": pinhole(((0, 1, 0), (0, 0, -1), (-1, 0, 0)), (h - 20.25, 0.375, 0.125), 64.0),
        "oblique_middle": T.look((3.0, 5.0, -7.0), (0.0, 0.0, 0.0), 20.0, w=W, h=H),
        "oblique_far_end": T.look((h - 10.0, 6.0, -5.0), (h - 30.0, 0.0, 0.0), 20.0, w=W, h=H),
        "ortho_across": make_view(across, 1.0, 1.0, 0.0, 0.0, W, H, is_ortho=True),
    }


def sparse_state(dims):
    """A fifth of the last 64 columns solid -- the far end of the x table and the last words of the bit rows are read --,
    and a dozen voxels elsewhere, four of them round the middle, all in ONE row of cells (y = 1, z = nz / 2) so that the
    rays of the view along x that run in the other rows reach the far end; most bricks hold nothing."""
    nx, ny, nz = dims
    rng = np.random.RandomState(7)
    solid = np.zeros((nz, ny, nx), bool)
    solid[:, :, nx - 64:] = rng.rand(nz, ny, 64) < 0.2
    solid[:, :, nx - 1] |= rng.rand(nz, ny) < 0.5
    solid[nz // 2, 1, rng.randint(0, nx - 64, 8)] = True
    solid[nz // 2, 1, nx // 2 - 3:nx // 2 + 4:2] = True
    solid = solid.reshape(-1)
    return np.where(solid, F(-0.5), F(0.5)).astype(F), np.ones(len(solid), np.int32), 0.0


_cache = {}


def case(dims):
    if dims not in _cache:
        opt = option(dims)
        planes = RR.option_planes(opt)
        views = views_for(dims)
        sdf, cnt, iso = sparse_state(dims)
        solid = RR.solid_mask(sdf, cnt, iso)
        slabs = [(0, dims[2])] + ([(0, 2), (2, 4)] if dims[2] == 4 else [])
        want = {}
        for vn, v in views.items():
            for z in slabs:
                part = S.slab_solid(solid, dims, *z)
                want[vn, z] = R.render_by_sorting(v, planes, dims, part)
        flat = RR.render(views["oblique_far_end"], planes, dims, solid)
        for a, b in zip(R.render_by_sorting(views["oblique_far_end"], planes, dims, solid), flat):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        _cache[dims] = dict(opt=opt, planes=planes, views=views, state=(sdf, cnt, iso), solid=solid, want=want)
    return _cache[dims]


def all_misses(g):
    return np.all(np.isposinf(g["depth"])) and np.all(g["voxel"] == -1) and np.all(g["axis"] == 255)


def test_the_grids_sit_on_either_side_of_the_lds_limit():
    with open(os.path.join(ROOT, "vacancy_amd", "csrc", "render.hip")) as f:
        found = re.findall(r"constexpr int kLdsPlanes = (\d+);", f.read())
    assert found == [str(LDS_PLANES)], "kLdsPlanes has moved: choose the grids of this file anew"
    totals = []
    for dims in GRIDS:
        dev = T.make_dev(option(dims), dims)
        totals.append(sum(dev.dims) + 3)
        dev.close()
    assert totals[0] == LDS_PLANES and totals[1] > LDS_PLANES 
    assert GRIDS[1][0] + 1 > 12282   # where the y table begins


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "%dx%dx%d" % d)
def test_whole_grid_and_agreement(dims):
    c = case(dims)
    dev = T.make_dev(c["opt"], dims)
    assert (sum(dev.dims) + 3 <= LDS_PLANES) == (dims == GRIDS[0])
    names = list(c["views"])
    vs = [c["views"][vn] for vn in names]
    sdf, cnt, iso = c["state"]
    whole = (0, dims[2])
    rng = np.random.RandomState(8)
    masks = [(rng.randint(0, 256, (H, W)) * (rng.rand(H, W) < 0.5)).astype(np.uint8) for _ in vs]
    far = dims[0] - 64
    for rayskip in (1, 0):
        dev.set_param("rayskip", rayskip)
        dev.upload(sdf, cnt)
        got = dev.RenderHull(vs, iso, voxel_ids=True, axes=True)
        for vn, g in zip(names, got):
            T.assert_images_equal(g, c["want"][vn, whole], "%s %s rayskip %d" % (dims, vn, rayskip))
        counts = dev.HullAgreement(vs, masks, iso)
        for vn, v, m, k in zip(names, vs, masks, counts):
            assert k.tolist() == RR.agreement(v, c["want"][vn, whole][1], m), (dims, vn, rayskip)
        dev.upload(np.full_like(sdf, 0.5), cnt)                  # an empty hull: every path is walked to its end
        for g in dev.RenderHull(vs, iso, voxel_ids=True, axes=True):
            assert all_misses(g)
        assert dev.HullAgreement(vs, masks, iso).tolist() == [[0, int((m != 0).sum()), 0] for m in masks]
    # the cases are not vacuous: the view along x hits in the last 64 columns, and every view hits something
    vox = c["want"]["along_px", whole][1]
    assert ((vox >= 0) & (vox % dims[0] >= far)).sum() >= 20
    for vn in names:
        assert (c["want"][vn, whole][1] >= 0).sum() >= 4, vn
    vox = np.concatenate([c["want"][vn, whole][1].reshape(-1) for vn in ("along_nx_inside", "oblique_far_end", "ortho_across")])
    assert (vox[vox >= 0] % dims[0] >= far).sum() >= 20


def test_slabs_beyond_lds_and_their_merge():
    dims = GRIDS[1]
    c = case(dims)
    names = list(c["views"])
    vs = [c["views"][vn] for vn in names]
    sdf, cnt, iso = c["state"]
    s = dims[0] * dims[1]
    for rayskip in (1, 0):
        parts = [[] for _ in vs]
        for z0, z1 in ((0, 2), (2, 4)):
            dev = T.make_dev(c["opt"], dims, z_range=(z0, z1))
            dev.set_param("rayskip", rayskip)
            dev.upload(sdf[z0 * s:z1 * s], cnt[z0 * s:z1 * s])
            got = dev.RenderHullSlab(vs, iso, voxel_ids=True, axes=True, hits=True)
            for j, (vn, v, g) in enumerate(zip(names, vs, got)):
                want = c["want"][vn, (z0, z1)]
                T.assert_images_equal(g, want, "%s slab [%d, %d) rayskip %d" % (vn, z0, z1, rayskip))
                assert np.array_equal(g["hits"], S.pack_hits(want[1], v)), (vn, z0, z1, rayskip)
                parts[j].append(g)
            dev.close()
        for vn, v, p in zip(names, vs, parts):
            T.assert_images_equal(vc.render_merge_host(v, p), c["want"][vn, (0, 4)], "%s merged, rayskip %d" % (vn, rayskip))
    for z in ((0, 2), (2, 4)):
        assert sum(int((c["want"][vn, z][1] >= 0).sum()) for vn in names) >= 20, z
