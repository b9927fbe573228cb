"""Scenes whose voxels project EXACTLY onto the decision edges of the carve kernels' samplers -- shared by
test_lattice_scenes_cpu.py (which shows from the oracle alone that the edges are reached) and test_gpu_lattice.py (which
compares the device with the oracle on them).  No GPU is needed here.

The grids have resolution 1 and half-integer voxel centres, the cameras have identity rotation and translations that are
multiples of 1/4, and the focal lengths are powers of two (or 48 over a depth of 96): on the slice whose camera depth is a
power of two the quotient f / pc.z is exact and a voxel lands on

  * a coordinate with fraction exactly .5 (the tie of the nearest-neighbour rounding),
  * an exact integer (lu == 0; a tap exactly on the last column of a staged tile),
  * exactly roi_min or roi_max (the inclusive ROI test),
  * the float just below .5 (where floor(u + 0.5f) is not round(u)),
  * a negative coordinate next to a ROI that starts above 0,

while the neighbouring slices (pc.z = 57 .. 72) give inexact quotients in the same bricks.  The images hold pixels of
exactly -1 and of the float just below it where voxels with integer coordinates read them (lu == lv == 0: the sample IS the
pixel, so the `dist < -1` equality of the truncation is reached through the geometry), and the ROI views hold +inf and
NaN in the columns and rows just outside the ROI, which the reference never reads.

sample_np restates the reference's two samplers and its ROI test in numpy, float32 operation for float32 operation, with
named mutants: what a kernel would compute if it rounded half to even, tested the ROI exclusively, and so on."""
import functools

import numpy as np

import oracle_lib as O
from color_ref import round_half_away
from vacancy_amd.capi import CarverOption, UpdateOption, make_view

F = np.float32
LOWEST = np.finfo(np.float32).min
W, H = 48, 40
BELOW_HALF = np.nextafter(F(0.5), F(0))
MINUS_ONE = F(-1.0)
BELOW_MINUS_ONE = np.nextafter(F(-1.0), F(-np.inf))
MARGIN = 0.125  # footprint_of (carve_fused_device.h): what a brick's corner hull keeps clear of the ROI to be `sure`

# name -> nx: bb = (-nx / 2, -8, -8) .. (nx / 2, 8, 8); rows of 20 voxels are no multiple of a brick's 8
GRIDS = {"24x16x16": 24, "20x16x16": 20}

# name -> (t, fx, fy, cx, cy, roi_min, roi_max, ortho).  On the slice pc.z == 64 (96 for pin_div3):
#   pin_ties        u = x + 20, v = y + 16 with half-integer x, y: every coordinate ties, floors of both parities
#   pin_int_roi     u = (x + .5) + 20: integers, among them roi_min and roi_max in u and in v
#   pin_half        u = (x + .5) / 2 + 20: every second one ties; v: integers
#   ortho_ties      u = x + 12, v = y + 8 on EVERY slice; pc.z = z + 6.5 is 0 on one slice and -1 on another
#   ortho_int_roi   u = x + 12.5: integers on every slice, among them roi_min and roi_max
#   pin_big         2 pixels per voxel, u = 2 (x - .25) + 24 = 2 k + .5 + 24: ties whose floor is even
#   pin_below_half  cx = cy = nextbelow(.5), roi_min = 0, pc.x == 0 on the plane x = -5.5, pc.y == 0 on y = .5: u == cx
#                   there, and floor(u + .5f) = 1 where round(u) = 0; pc.x < 0 gives u < 0 inside the same brick
#   pin_neg         integers again, a ROI from (3, 2) and voxels down to u = -7, v = -3
#   pin_fxfy        fx = 32, fy = 16: half a pixel per voxel and less (raw tiles by the host's own rule)
#   pin_div3        fx = 48, pc.z = 96 = 3 * 2^5 on one slice: an exact quotient of operands that are no powers of two
# The pinhole views come first: a fused launch holds one projection model (fused_eligible), so the tests launch the
# pinhole views together and the orthographic ones together.  The host's tile rule ("tile" 0) picks raw tiles for
# pin_fxfy and pin_div3 (about half a pixel per voxel) and big tiles for every other view -- pin_half too: its fy = 64
# over a depth of 64.5 is 0.99 pixels per voxel, and the rule takes the larger focal length.
VIEWS = {
    "pin_ties": ((0.0, 0.0, 64.5), 64.0, 64.0, 20.0, 16.0, None, None, False),
    "pin_int_roi": ((0.5, 0.5, 64.5), 64.0, 64.0, 20.0, 16.0, (12, 10), (30, 22), False),
    "pin_half": ((0.5, 0.5, 64.5), 32.0, 64.0, 20.0, 16.0, None, None, False),
    "pin_big": ((-0.25, -0.25, 64.5), 128.0, 128.0, 24.0, 20.0, None, None, False),
    "pin_below_half": ((5.5, -0.5, 64.5), 64.0, 64.0, float(BELOW_HALF), float(BELOW_HALF), None, None, False),
    "pin_neg": ((0.5, 0.5, 64.5), 64.0, 64.0, 4.0, 4.0, (3, 2), (40, 30), False),
    "pin_fxfy": ((0.5, 0.5, 64.5), 32.0, 16.0, 20.0, 16.0, None, None, False),
    "pin_div3": ((0.5, 0.5, 96.5), 48.0, 48.0, 20.0, 16.0, None, None, False),
    "ortho_ties": ((12.0, 8.0, 6.5), 1.0, 1.0, 0.0, 0.0, None, None, True),
    "ortho_int_roi": ((12.5, 8.5, 6.5), 1.0, 1.0, 0.0, 0.0, (5, 3), (20, 14), True),
}
VIEW_NAMES = list(VIEWS)
ROI_VIEWS = [n for n in VIEW_NAMES if VIEWS[n][5] is not None]
CLASSES = ("half", "integer", "roi_min", "roi_max", "below_half", "negative", "z_zero", "z_negative")


def grid_option(grid, **uo):
    nx = GRIDS[grid]
    return CarverOption(bb_min=(-nx / 2.0, -8.0, -8.0), bb_max=(nx / 2.0, 8.0, 8.0), resolution=1.0,
                        update_option=UpdateOption(**uo))


def make(name):
    t, fx, fy, cx, cy, rmin, rmax, ortho = VIEWS[name]
    m = np.array([[1, 0, 0, t[0]], [0, 1, 0, t[1]], [0, 0, 1, t[2]]], np.float32)
    return make_view(m, fx, fy, cx, cy, W, H, roi_min=rmin, roi_max=rmax, is_ortho=ortho)


@functools.lru_cache(maxsize=None)
def positions(grid):
    """The oracle's voxel positions (read-only), x fastest."""
    orc = O.OracleGrid(grid_option(grid))
    assert orc.dims == (GRIDS[grid], 16, 16)
    pos = orc.positions()
    orc.close()
    pos.setflags(write=False)
    return pos


def project(pos, view):
    """(pc.z, in front and inside the ROI, u, v): the oracle's projection of its voxel positions (orc_carve: the
    reference's operations in fp32, in its order), pinhole and orthographic."""
    m = np.array(list(view.w2c), np.float32).reshape(3, 4)
    p = pos.astype(np.float32)
    with np.errstate(all="ignore"):
        pc = [m[i, 3] + (m[i, 0] * p[:, 0] + (m[i, 1] * p[:, 1] + m[i, 2] * p[:, 2])) for i in range(3)]
        if view.is_ortho:
            u, v = pc[0], pc[1]
        else:
            u = np.float32(view.fx) / pc[2] * pc[0] + np.float32(view.cx)
            v = np.float32(view.fy) / pc[2] * pc[1] + np.float32(view.cy)
        assert u.dtype == np.float32 and v.dtype == np.float32
        inside = (u >= view.roi_min[0]) & (v >= view.roi_min[1]) & (u <= view.roi_max[0]) & (v <= view.roi_max[1])
    return pc[2], inside & ~(pc[2] < 0), u, v


def classify(view, pos):
    """{class: bool per voxel} from the fp32 projection.  The coordinate classes count a voxel the reference SAMPLES (in
    front of the camera, inside the ROI) whose u or v is of the class; "negative": in front with u or v below 0;
    "tie_even": a tie whose floor is even (round half to even sends it the other way)."""
    z, ins, u, v = project(pos, view)
    fu, fv = np.floor(u), np.floor(v)
    with np.errstate(invalid="ignore"):
        tie_u, tie_v = u - fu == F(0.5), v - fv == F(0.5)
        out = {
            "half": ins & (tie_u | tie_v),
            "tie_even": ins & ((tie_u & (fu % 2 == 0)) | (tie_v & (fv % 2 == 0))),
            "integer": ins & ((u == fu) | (v == fv)),
            "integer_both": ins & (u == fu) & (v == fv),
            "roi_min": ins & ((u == view.roi_min[0]) | (v == view.roi_min[1])),
            "roi_max": ins & ((u == view.roi_max[0]) | (v == view.roi_max[1])),
            "below_half": ins & ((u == BELOW_HALF) | (v == BELOW_HALF)),
            "negative": ~(z < 0) & ((u < 0) | (v < 0)),
            "z_zero": z == 0,
            "z_negative": z < 0,
        }
    return out


# ---- the images ------------------------------------------------------------------------------------------------------

def _poison_ring(view, img):
    """+inf and NaN, alternating, in the column and the row just outside the ROI on all four sides (corners included)."""
    x0, y0, x1, y1 = view.roi_min[0] - 1, view.roi_min[1] - 1, view.roi_max[0] + 1, view.roi_max[1] + 1
    ring = [(x, y) for x in range(x0, x1 + 1) for y in (y0, y1)] + [(x, y) for y in range(y0 + 1, y1) for x in (x0, x1)]
    for k, (x, y) in enumerate(sorted(ring)):
        if 0 <= x < view.width and 0 <= y < view.height:
            img[y, x] = np.inf if k % 2 == 0 else np.nan


@functools.lru_cache(maxsize=None)
def image(name):
    """The SDF image of a view (read-only): noise in (-0.9, 0.9); -1 and the float below it on a fifth each of the pixels
    that a voxel (of either grid) with integer u AND v samples; in the ROI views the poisoned ring around the ROI."""
    view = make(name)
    rng = np.random.default_rng(1000 + VIEW_NAMES.index(name))
    img = rng.uniform(-0.9, 0.9, (H, W)).astype(np.float32)
    for grid in GRIDS:
        pos = positions(grid)
        both = classify(view, pos)["integer_both"]
        _, _, u, v = project(pos, view)
        for x, y in set(zip(u[both].astype(int).tolist(), v[both].astype(int).tolist())):
            k = (3 * x + 2 * y) % 5
            if k < 2:
                img[y, x] = MINUS_ONE if k == 0 else BELOW_MINUS_ONE
    if name in ROI_VIEWS:
        _poison_ring(view, img)
    # (std::max_element keeps a NaN only from the first pixel; no scene HERE relies on that -- float_class_scenes.py does)
    assert not np.isnan(img[0, 0])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def depth_image(name):
    """A depth image for the depth carve: finite depths around the grid's camera depth everywhere, and +inf / NaN / 0
    (miss, garbage, invalid) cycling over the ring just outside the ROI of the ROI views."""
    view = make(name)
    rng = np.random.default_rng(2000 + VIEW_NAMES.index(name))
    tz = VIEWS[name][0][2]
    img = (tz + rng.uniform(-9.0, 9.0, (H, W))).astype(np.float32)
    if name in ROI_VIEWS:
        ring = np.full((H, W), 1.0, np.float32)
        _poison_ring(view, ring)
        ys, xs = np.nonzero(~(ring == 1.0))
        for k, (y, x) in enumerate(zip(ys, xs)):
            img[y, x] = (np.inf, np.nan, 0.0)[k % 3]
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def photo(name):
    rng = np.random.default_rng(3000 + VIEW_NAMES.index(name))
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


def scene():
    """[(name, view, image)] in the order of VIEWS."""
    return [(n, make(n), image(n)) for n in VIEW_NAMES]


# ---- the samplers, restated ---------------------------------------------------------------------------------------------

RULES = ("ref", "half_even", "floor_half", "strict_max", "strict_min", "no_clamp", "le_trunc")


def sample_np(view, img, u, v, nn, rule="ref"):
    """(inside, dist): the reference's ROI test (voxel_carver.cc:464-465, as its complement: orc_carve says why) and its
    sampler -- SdfInterpolationNn (:16-38) when `nn`, else SdfInterpolationBiliner (:40-76) -- on float32 coordinates;
    dist is only meaningful where inside.  rule: "ref", or a mutant --
      half_even   nearest neighbour with np.rint;          floor_half  with floor(u + 0.5f);
      strict_max  u < roi_max instead of <=;               strict_min  u > roi_min instead of >=;
      no_clamp    the tap x0 + 1 / y0 + 1 not clamped to roi_max (to the image only: this is numpy);
      le_trunc    nothing here: one_view_state drops dist <= -1 instead of dist < -1."""
    assert rule in RULES and u.dtype == F and v.dtype == F
    img = np.asarray(img, F).reshape(view.height, view.width)
    rx0, ry0, rx1, ry1 = view.roi_min[0], view.roi_min[1], view.roi_max[0], view.roi_max[1]
    with np.errstate(all="ignore"):
        lo_u, lo_v = ((u > F(rx0)), (v > F(ry0))) if rule == "strict_min" else ((u >= F(rx0)), (v >= F(ry0)))
        hi_u, hi_v = ((u < F(rx1)), (v < F(ry1))) if rule == "strict_max" else ((u <= F(rx1)), (v <= F(ry1)))
        inside = lo_u & lo_v & hi_u & hi_v
        us, vs = np.where(inside, u, F(rx0)), np.where(inside, v, F(ry0))  # (the others take no further part)
        if nn:
            if rule == "half_even":
                xr, yr = np.rint(us), np.rint(vs)
            elif rule == "floor_half":
                xr, yr = np.floor(us + F(0.5)), np.floor(vs + F(0.5))
            else:
                xr, yr = round_half_away(us), round_half_away(vs)
            assert xr.dtype == F
            xi = np.clip(xr.astype(np.int64), rx0, rx1)
            yi = np.clip(yr.astype(np.int64), ry0, ry1)
            return inside, img[yi, xi]
        x0, y0 = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
        x1, y1 = x0 + 1, y0 + 1
        x0, y0 = np.maximum(x0, rx0), np.maximum(y0, ry0)
        if rule == "no_clamp":
            x1, y1 = np.minimum(x1, view.width - 1), np.minimum(y1, view.height - 1)
        else:
            x1, y1 = np.minimum(x1, rx1), np.minimum(y1, ry1)
        lu, lv = us - x0.astype(F), vs - y0.astype(F)
        one = F(1.0)
        a = (one - lu) * (one - lv) * img[y0, x0]
        b = lu * (one - lv) * img[y0, x1]
        c = (one - lu) * lv * img[y1, x0]
        d = lu * lv * img[y1, x1]
        dist = ((a + b) + c) + d
        assert dist.dtype == F
    return inside, dist


def one_view_state(view, img, pos, nn, rule="ref", outside_max=False, truncation=False):
    """(sdf, update_num) of a fresh grid after this ONE view (orc_carve's first touch), sampled by sample_np."""
    z, _, u, v = project(pos, view)
    inside, dist = sample_np(view, img, u, v, nn, rule)
    front = ~(z < 0)
    with np.errstate(invalid="ignore"):
        max_sdf = F(np.max(np.where(np.isnan(img), -np.inf, img)))  # (std::max_element: a NaN that is not first never wins)
        dist = np.where(inside, dist, max_sdf).astype(F)
        take = front & (inside | outside_max)
        if truncation:
            take &= ~((dist <= F(-1.0)) if rule == "le_trunc" else (dist < F(-1.0)))
    sdf = np.where(take, dist, F(LOWEST)).astype(F)
    return sdf, take.astype(np.int32)


def oracle_one_view(grid, view, img, **uo):
    orc = O.OracleGrid(grid_option(grid, **uo))
    orc.carve(view, img)
    out = orc.download()
    orc.close()
    return out


# ---- bricks ----------------------------------------------------------------------------------------------------------------

def brick_of(grid):
    """(brick index per voxel, number of bricks): the 8 x 8 x 8 wave bricks, as test_scene_takes_the_paths numbers them."""
    nx = GRIDS[grid]
    i = np.arange(nx * 16 * 16)
    brick = ((i // (nx * 16)) // 8 * 2 + (i // nx) % 16 // 8) * ((nx + 7) // 8) + (i % nx) // 8
    return brick, int(brick.max()) + 1


def brick_report(grid, view):
    """{"sure", "sure_raw", "cut": bool per brick} from the oracle's projection of the brick's corner hull.
    sure: what footprint_of documents -- every corner in front of the camera, and the hull, widened by the margin of 0.125,
    has floor(min) >= roi_min and floor(max) < roi_max in u and in v (the device adds guards on its own rounding errors
    that these small exact scenes are far from); sure_raw: its tap rectangle also fits the raw tile's 15 x 15 pixels.
    cut: the ROI test (or the camera plane) separates voxels of the brick."""
    pos = positions(grid)
    brick, nb = brick_of(grid)
    z, ins, _, _ = project(pos, view)
    sure, sure_raw, cut = np.zeros(nb, bool), np.zeros(nb, bool), np.zeros(nb, bool)
    for b in range(nb):
        sel = brick == b
        p = pos[sel]
        lo, hi = p.min(axis=0), p.max(axis=0)
        corners = np.array([[(lo, hi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)], np.float32)
        cz, _, cu, cv = project(corners, view)
        ok, fits = bool((cz > 0).all()), True
        for c, r0, r1 in ((cu, view.roi_min[0], view.roi_max[0]), (cv, view.roi_min[1], view.roi_max[1])):
            a, e = int(np.floor(float(c.min()) - MARGIN)), int(np.floor(float(c.max()) + MARGIN))
            ok &= a >= r0 and e < r1
            fits &= e - a + 1 <= 15
        sure[b], sure_raw[b] = ok, ok and fits
        n_in = int(ins[sel].sum())
        cut[b] = 0 < n_in < int(sel.sum())
        assert not (ok and cut[b]), "a brick the rule calls sure has a voxel outside the ROI"
    return {"sure": sure, "sure_raw": sure_raw, "cut": cut}


def host_picks_big_tile(views):
    """test_gpu_view_loop_paths.host_picks_big_tile with the orthographic branch of launch_carve_fused: one pixel per
    world unit."""
    worst = np.float32(0)
    for v in views:
        pz = np.float32(v.w2c[11])  # t.z + R[2] . (0, 0, 0): the grids are centred on the origin
        ppv = np.float32(1.0) if v.is_ortho else (np.float32(max(v.fx, v.fy)) / pz if pz > 0 else np.float32(np.inf))
        worst = max(worst, ppv)
    return bool(np.float32(8.0) * np.float32(1.7320508) * worst + np.float32(3.0) > np.float32(15.0))
