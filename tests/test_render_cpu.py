"""CPU-only checks of the ray-cast of the hull: vcy_cell_planes against numpy, the numpy restatement (tests/render_ref.py)
on hand-made cases whose answers are written out, and the new C-ABI symbols with the argument errors that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import render_ref as RR
from vacancy_amd import capi, carver
from vacancy_amd.capi import CarverOption, make_view

F = np.float32
INF = np.inf

# bb_min, bb_max, resolution: uneven boxes -- n = 1, n = 2, and boxes whose diff / resolution truncates (pitch != resolution)
BOXES = [
    ((-0.5, -1.0, 0.25), (0.75, 1.5, 1.0), 1.0),          # dims (1, 2, 0): refused (an empty axis)
    ((-0.5, -1.0, 0.25), (0.75, 1.5, 1.5), 1.0),          # dims (1, 2, 1)
    ((-4.75, -4.15, -3.95), (4.75, 4.15, 3.95), 1.0),     # dims (9, 8, 7), pitches 9.5 / 9, 8.3 / 8, 7.9 / 7
    ((-270.0, -364.586151, -149.982697), (270.0, 170.542343, 277.329224), 10.0),  # the bunny's box: (54, 53, 42)
    ((0.1, 0.2, 0.3), (6.45, 2.35, 1.31), 0.1),           # (63, 21, 10) with inexact everything
]


def planes_of(bb_min, bb_max, res, axis, n):
    out = np.full(n + 1, np.nan, F)
    rc = capi.load().vcy_cell_planes((C.c_float * 3)(*bb_min), (C.c_float * 3)(*bb_max), res, axis,
                                     out.ctypes.data_as(C.c_void_p))
    return rc, out


@pytest.mark.parametrize("box", BOXES[1:], ids=lambda b: "res%g_%g" % (b[2], b[1][0]))
def test_cell_planes_equal_numpy(box):
    bb_min, bb_max, res = box
    dims = RR.grid_dims(bb_min, bb_max, res)
    lib = capi.load()
    got_dims = (C.c_int32 * 3)()
    assert lib.vcy_compute_dims((C.c_float * 3)(*bb_min), (C.c_float * 3)(*bb_max), res, got_dims) == 0
    assert tuple(got_dims) == dims
    for axis in range(3):
        rc, got = planes_of(bb_min, bb_max, res, axis, dims[axis])
        assert rc == 0, carver.last_error()
        want = RR.cell_planes(bb_min, bb_max, res, axis)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (axis, got, want)
        assert np.all(np.diff(got) > 0)
        # every voxel centre lies strictly inside its cell
        p = RR.axis_positions(bb_min, bb_max, res, axis, dims[axis])
        assert np.all(got[:-1] < p) and np.all(p < got[1:])
    if dims == (1, 2, 1):  # n == 1: half of `resolution` to either side of the centre
        _, px = planes_of(bb_min, bb_max, res, 0, 1)
        c = float(RR.axis_positions(bb_min, bb_max, res, 0, 1)[0])
        assert px[0] == F(c - 0.5) and px[1] == F(c + 0.5)


def test_cell_planes_refusals():
    bb_min, bb_max, res = BOXES[0]
    rc, _ = planes_of(bb_min, bb_max, res, 0, 1)
    assert rc == capi.VCY_ERR_INVALID_ARG and "empty axis" in carver.last_error()
    bb_min, bb_max, res = BOXES[2]
    assert planes_of(bb_min, bb_max, res, 3, 9)[0] == capi.VCY_ERR_INVALID_ARG
    assert planes_of(bb_min, bb_max, res, -1, 9)[0] == capi.VCY_ERR_INVALID_ARG
    lib = capi.load()
    assert lib.vcy_cell_planes(None, (C.c_float * 3)(*bb_max), res, 0, None) == capi.VCY_ERR_INVALID_ARG
    # centres that collide in float: 48 voxels of 1e-5 at 1000 (ulp 6e-5) give a table that does not increase
    bb_min, bb_max, res = (1000.0, 0.0, 0.0), (1000.0005, 0.0005, 0.0005), 1e-5
    dims = RR.grid_dims(bb_min, bb_max, res)
    assert dims[0] > 8 and len(np.unique(RR.axis_positions(bb_min, bb_max, res, 0, dims[0]))) < dims[0]
    rc, _ = planes_of(bb_min, bb_max, res, 0, dims[0])
    assert rc == capi.VCY_ERR_INVALID_ARG and "not increasing" in carver.last_error(), carver.last_error()
    assert planes_of(bb_min, bb_max, res, 1, dims[1])[0] == 0


# ---- the restatement on cases with written-out answers ---------------------------------------------------------------

DIMS = (4, 4, 4)  # unit voxels on [-2, 2]^3: centres -1.5 .. 1.5, planes -2 .. 2


def unit_planes():
    planes = [RR.cell_planes((-2, -2, -2), (2, 2, 2), 1.0, a) for a in range(3)]
    for p in planes:
        assert np.array_equal(p, np.array([-2, -1, 0, 1, 2], F))
    return planes


def solid_of(*voxels):
    s = np.zeros(64, bool)
    for x, y, z in voxels:
        s[z * 16 + y * 4 + x] = True
    return s


def w2c_translate(t):
    m = np.zeros((3, 4), F)
    m[:, :3] = np.eye(3)
    m[:, 3] = t
    return m


def test_ref_single_voxel_axis_aligned_ortho():
    # camera x = world x + 1.5, so pixel u looks down the column of voxel centres x = u; the camera plane is z = -5
    view = make_view(w2c_translate((1.5, 1.5, 5.0)), 1.0, 1.0, 0.0, 0.0, 4, 4, is_ortho=True)
    depth, voxel, axis = RR.render(view, unit_planes(), DIMS, solid_of((1, 2, 3)))
    want_d = np.full((4, 4), INF, F)
    want_v = np.full((4, 4), -1, np.int64)
    want_a = np.full((4, 4), 255, np.uint8)
    want_d[2, 1], want_v[2, 1], want_a[2, 1] = 6.0, 57, 2   # enters z cell 3 through the plane z = 1: t = 1 - (-5)
    assert np.array_equal(depth, want_d) and np.array_equal(voxel, want_v) and np.array_equal(axis, want_a)
    # a second voxel in front of it on the same column wins: z cell 1 begins at the plane z = -1, t = 4
    depth, voxel, axis = RR.render(view, unit_planes(), DIMS, solid_of((1, 2, 3), (1, 2, 1), (0, 0, 0)))
    assert (depth[2, 1], voxel[2, 1], axis[2, 1]) == (4.0, 25, 2)
    assert (depth[0, 0], voxel[0, 0], axis[0, 0]) == (3.0, 0, 2)       # the grid's first plane z = -2
    assert int((voxel >= 0).sum()) == 2
    # the ROI: pixels outside it are misses
    view = make_view(w2c_translate((1.5, 1.5, 5.0)), 1.0, 1.0, 0.0, 0.0, 4, 4, roi_min=(1, 1), roi_max=(3, 3), is_ortho=True)
    depth, voxel, axis = RR.render(view, unit_planes(), DIMS, solid_of((1, 2, 3), (0, 0, 0)))
    assert voxel[2, 1] == 57 and voxel[0, 0] == -1 and depth[0, 0] == INF and axis[0, 0] == 255


def test_ref_camera_inside_a_solid_voxel():
    centre = np.array([-0.5, 0.5, 1.5], F)  # of voxel (1, 2, 3)
    view = make_view(w2c_translate(-centre), 2.0, 2.0, 2.0, 1.5, 5, 4)
    depth, voxel, axis = RR.render(view, unit_planes(), DIMS, solid_of((1, 2, 3)))
    assert np.array_equal(depth, np.zeros((4, 5), F)) and not np.signbit(depth).any()
    assert np.all(voxel == 57) and np.all(axis == 3)
    # the same camera in an empty voxel next to a solid one: straight ahead (u = cx) the ray enters (1, 2, 3) from z
    # cell 2 ... which it is not in: put the camera one voxel lower and look up the column
    view = make_view(w2c_translate(-(centre - np.array([0, 0, 1], F))), 2.0, 2.0, 2.0, 1.0, 5, 3)
    depth, voxel, axis = RR.render(view, unit_planes(), DIMS, solid_of((1, 2, 3)))
    assert (depth[1, 2], voxel[1, 2], axis[1, 2]) == (0.5, 57, 2)     # from z = 0.5 to the plane z = 1


def test_ref_ray_parallel_to_two_axes():
    # a pinhole at (-0.5, 0.5, -5) looking along +z: the central pixel's ray has d = (0, 0, 1), no crossings on x and y
    view = make_view(w2c_translate((0.5, -0.5, 5.0)), 1.0, 1.0, 1.0, 1.0, 3, 3)
    o, d, roi = RR.rays(view)
    assert np.array_equal(d[:, 4], np.array([0, 0, 1], F)) and np.array_equal(o[:, 4], np.array([-0.5, 0.5, -5], F))
    depth, voxel, axis = RR.render(view, unit_planes(), DIMS, solid_of((1, 2, 3), (3, 2, 0)))
    assert (depth[1, 1], voxel[1, 1], axis[1, 1]) == (6.0, 57, 2)
    # its neighbours (d = (+-1, 0, 1) ...) leave the grid's x or y range at t <= 2.5, before z = -2 comes at t = 3
    miss = np.ones((3, 3), bool)
    miss[1, 1] = False
    assert np.all(voxel[miss] == -1) and np.all(depth[miss] == INF) and np.all(axis[miss] == 255)
    # with the voxel the central ray passes moved aside by one cell it is a miss as well: the cell is found by position
    _, voxel, _ = RR.render(view, unit_planes(), DIMS, solid_of((2, 2, 3), (1, 1, 3)))
    assert voxel[1, 1] == -1


# ---- symbols and argument errors that need no GPU --------------------------------------------------------------------

def good_view():
    return make_view(w2c_translate((0.0, 0.0, 5.0)), 10.0, 10.0, 3.5, 2.5, 8, 6)


def test_symbols_are_exported_and_bound():
    lib = capi.load()
    for name in ("vcy_render_hull", "vcy_hull_agreement", "vcy_last_render_ms", "vcy_cell_planes"):
        assert hasattr(lib, name) and name in lib._vcy_symbols
    for name in ("RenderHull", "HullAgreement", "last_render_ms"):
        assert callable(getattr(carver.VoxelCarver, name))
    opt = CarverOption(bb_min=BOXES[2][0], bb_max=BOXES[2][1], resolution=BOXES[2][2])
    assert np.array_equal(carver.cell_planes(opt, 1), RR.cell_planes(*BOXES[2], 1))


def render_rc(view, n=1, ctx=None):
    lib = capi.load()
    arr = (capi.View * 1)(view)
    return lib.vcy_render_hull(ctx, 0.0, n, arr, None, None, None)


def test_argument_errors_without_a_gpu():
    lib = capi.load()
    assert C.sizeof(capi.View) == 92
    assert render_rc(good_view()) == capi.VCY_ERR_NOT_INITIALIZED      # the view is fine, the context is missing
    assert render_rc(good_view(), n=0) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_render_hull(None, 0.0, 1, None, None, None, None) == capi.VCY_ERR_INVALID_ARG
    bad = []
    v = good_view(); v.w2c[7] = float("nan"); bad.append(v)
    v = good_view(); v.w2c[0] = float("inf"); bad.append(v)
    v = good_view(); v.fx = 0.0; bad.append(v)
    v = good_view(); v.fy = -0.0; bad.append(v)
    v = good_view(); v.width = 0; bad.append(v)
    v = good_view(); v.height = -3; bad.append(v)
    v = good_view(); v.roi_max[0] = 8; bad.append(v)
    v = good_view(); v.roi_min[1] = -1; bad.append(v)
    v = good_view(); v.roi_min[0], v.roi_max[0] = 5, 4; bad.append(v)
    for k, v in enumerate(bad):
        assert render_rc(v) == capi.VCY_ERR_INVALID_ARG, k
        mask = np.zeros((6, 8), np.uint8)
        counts = np.zeros(3, np.int64)
        mp = (C.c_void_p * 1)(mask.ctypes.data)
        assert lib.vcy_hull_agreement(None, 0.0, 1, (capi.View * 1)(v), mp, counts.ctypes.data_as(C.c_void_p)) == \
            capi.VCY_ERR_INVALID_ARG, k
    v = good_view(); v.is_ortho = 1; v.fx = 0.0       # an ortho view does not read fx
    assert render_rc(v) == capi.VCY_ERR_NOT_INITIALIZED
    mask = np.zeros((6, 8), np.uint8)
    mp = (C.c_void_p * 1)(mask.ctypes.data)
    arr = (capi.View * 1)(good_view())
    assert lib.vcy_hull_agreement(None, 0.0, 1, arr, mp, None) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_hull_agreement(None, 0.0, 1, arr, None, None) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_hull_agreement(None, 0.0, 1, arr, (C.c_void_p * 1)(None), mask.ctypes.data_as(C.c_void_p)) == \
        capi.VCY_ERR_INVALID_ARG
    ms = C.c_float(-1.0)
    assert lib.vcy_last_render_ms(None, C.byref(ms)) == capi.VCY_ERR_INVALID_ARG
