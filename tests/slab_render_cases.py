"""Shared by tests/test_slab_render_merge.py (host merge, no GPU), tests/test_gpu_slab_render.py and
tests/test_dist_render.py: the boxes, views and states of tests/test_gpu_render.py, where the grids are cut, the
restatement's image of a slab -- tests/render_ref.py on the solid mask restricted to the slab's slices, which is the
definition of a slab image as it stands --, the packing of hit bits, and the views of the tie case."""
import numpy as np

import render_ref as RR
from test_gpu_render import F, H, W, assert_images_equal, bits, case, grid_option, look, make_dev  # noqa: F401
from vacancy_amd.capi import make_view

DIMS = [(9, 8, 7), (65, 9, 17), (24, 20, 17)]


def cut_sets(nz):
    """name -> z bounds: one slab, a cut at every z, {1}, {nz - 1}, and for nz = 17 {8}, {9} and {3, 11}."""
    out = {"one": [0, nz], "every_z": list(range(nz + 1)), "at_1": [0, 1, nz], "at_nz-1": [0, nz - 1, nz]}
    if nz == 17:
        out.update({"at_8": [0, 8, nz], "at_9": [0, 9, nz], "at_3_11": [0, 3, 11, nz]})
    return out


def slabs_of(bounds):
    return list(zip(bounds[:-1], bounds[1:]))


def slab_solid(solid, dims, z0, z1):
    """`solid` with every voxel outside the slices [z0, z1) cleared."""
    z = np.arange(dims[0] * dims[1] * dims[2]) // (dims[0] * dims[1])
    return np.asarray(solid, bool) & (z >= z0) & (z < z1)


_solid, _slab = {}, {}


def solid_of(dims, sn):
    if (dims, sn) not in _solid:
        sdf, cnt, iso = case(dims)["states"][sn]
        _solid[dims, sn] = RR.solid_mask(sdf, cnt, iso)
    return _solid[dims, sn]


def slab_image(dims, sn, vn, z0, z1):
    """(depth, voxel, axis) of the slab [z0, z1) of state `sn` in view `vn` of case(dims): computed once."""
    key = (dims, sn, vn, z0, z1)
    if key not in _slab:
        c = case(dims)
        _slab[key] = c["want"][sn, vn] if (z0, z1) == (0, dims[2]) else \
            RR.render(c["views"][vn], c["planes"], dims, slab_solid(solid_of(dims, sn), dims, z0, z1))
    return _slab[key]


def pack_hits(voxel, view):
    """uint64 [height, (width + 63) // 64]: bit u & 63 of word u >> 6 set where the pixel lies in the ROI and voxel >= 0."""
    h, w = voxel.shape
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    roi = (uu >= view.roi_min[0]) & (uu <= view.roi_max[0]) & (vv >= view.roi_min[1]) & (vv <= view.roi_max[1])
    wide = np.zeros((h, (w + 63) // 64 * 64), bool)
    wide[:, :w] = (voxel >= 0) & roi
    return np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")).view("<u8").astype(np.uint64)


# ---- the tie case ----------------------------------------------------------------------------------------------------
# The (65, 9, 17) box of pitch 1 is centred on the origin: planes at x = -32.5 + k, z = -8.5 + k.  A pinhole with axis-
# aligned rotation stands at x = -52.5, outside the x range, 20 below (looking up z) or above (looking down z) plane 8 of
# z.  The pixels of the column with d_c0 = 1 have rays d = (1, d_y, +-1): they reach x = -32.5, where x comes into range,
# at t = 20 exactly, and plane 8 of z at the same t.  The x crossing sorts first: the ray enters the grid in the slice
# on the near side of plane 8 (depth 20, axis 0) and crosses into the slice on the far side at the same t (depth 20, axis
# 2).  With every voxel solid and a cut at z = 8 both slabs hit at bit-equal depth.
TIE_DIMS = (65, 9, 17)
TIE_CUTS = ("at_8", "every_z")


def tie_views():
    """name -> (view, the sign of s_z of every ray)"""
    out = {}
    for name, sz in (("up", 1), ("down", -1)):
        r = np.diag([1.0, float(sz), float(sz)])     # (down: half a turn about x)
        centre = np.array([-52.5, 0.0, -0.5 - 20.0 * sz])
        w2c = np.zeros((3, 4), F)
        w2c[:, :3] = r
        w2c[:, 3] = -r @ centre
        out[name] = (make_view(w2c, 8.0, 40.0, float(W // 2 - 8), float(H // 2), W, H), sz)
    return out


def tied_pixels(slab_images, merged_voxel):
    """Pixels where two different slabs hit at bit-equal depth: bool [height, width]."""
    depth = np.stack([bits(d) for d, _, _ in slab_images])
    hit = np.stack([v >= 0 for _, v, _ in slab_images])
    tied = np.zeros(merged_voxel.shape, bool)
    for a in range(len(slab_images)):
        for b in range(a + 1, len(slab_images)):
            tied |= hit[a] & hit[b] & (depth[a] == depth[b])
    return tied
