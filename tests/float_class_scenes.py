"""Scenes whose SAMPLE and STATE values lie at the edges of float -- shared by test_float_class_scenes_cpu.py (which shows
from the oracle alone that every class is reached and that every named defect would be seen) and test_gpu_float_classes.py
(which compares the device with the oracle on them).  Pure numpy and the CPU oracle; nothing of the device path.

The geometry is ordinary.  Two grids of resolution 1 -- (24, 20, 17): rows that are no multiple of a brick's 8;
(64, 16, 18): rows of one whole 64-voxel word -- and eight views of 48 x 40 pixels around them: six pinhole views in
three pairs at about 0.7, 2 and 5 pixels per voxel (the raw 16 x 16 tile, the 2048-pixel tile and sample_generic by the
host's rule side = 8 sqrt(3) ppv + 3 against 15, carve_fused_plan.h) and two orthographic ones, one of them axis-aligned
with a translation that puts one column of voxels EXACTLY on a pixel column (lu == 0: a tap of weight exactly 0).  Every
view has a ROI without pixel [0, 0], so only max_sdf reads that pixel; the even views' ROIs cut the grid's projection
(ROIS).  A fused launch holds one projection model and picks its tile for its worst view, so the views are
carved in the four BATCHES, pair by pair.

What changes is the values.  An image set is a smooth base per view with values PLANTED in a fixed pattern around the
centre of the grid's footprint: per value one full 2 x 2 tap neighbourhood and one isolated pixel, in cells of 5 x 5 pixels.

  zeros     +0 and -0; four images whose maximum is zero, with -0 first and with +0 first
  denormals +-1e-45, +-1e-39, +-FLT_MIN; three images that are the base scaled by 1e-38
  huge      lowest() (the state's own sentinel) planted and as whole images, +-3e38, FLT_MAX; a flat 3e38 image three times
            (the weighted average overflows to +inf) and a -inf after it (inf + -inf)
  inf       +-inf; +inf next to a pixel whose bilinear weight is exactly 0 (0 * inf)
  nan       NaN at pixel [0, 0] only, elsewhere only, both, an all-NaN image, NaN inside the ROI
  max_sdf   the resolution of max_sdf on its own: pixel [0, 0] NaN, +inf, the first of two zeros of either sign, the
            first of tied maxima; an image of -inf everywhere

special_state puts the same classes straight into sdf with counts 0 .. 3 (a count of 0 over a valid value among them),
depth_image into a depth image (-0.0 is "no measurement", as 0 is).  DEFECTS are transformations of the INPUTS that
stand for what a wrong kernel would compute (samples flushed to zero, the sign of zero lost, ...)."""
import functools

import numpy as np

import oracle_lib as O
from vacancy_amd import synth
from vacancy_amd.capi import CarverOption, UpdateOption, make_view

F = np.float32
LOWEST = F(np.finfo(np.float32).min)
FLT_MAX = F(np.finfo(np.float32).max)
FLT_MIN = F(np.finfo(np.float32).tiny)
W, H = 48, 40

# dims -> extent of the box (robust_cases.option_for: diff / resolution truncates, the pitch is not the resolution)
EXTENT = {(24, 20, 17): (24.4, 20.2, 17.3), (64, 16, 18): (64.3, 16.3, 18.3)}
GRIDS = list(EXTENT)

# The eight option sets: between them every value of every switch.
OPTIONS = {
    "kmax": dict(),
    "kmax_trunc": dict(use_truncation=True, truncation_band=0.2),
    "kmax_outside": dict(update_outside=1),
    "kmax_trunc_nn": dict(use_truncation=True, truncation_band=0.2, sdf_interp=0),
    "wa_w1": dict(voxel_update=1, voxel_update_weight=1.0),
    "wa_w1_trunc": dict(voxel_update=1, voxel_update_weight=1.0, use_truncation=True, truncation_band=0.2),
    "wa_w05_outside": dict(voxel_update=1, voxel_update_weight=0.5, update_outside=1),
    "kmax_gate2": dict(voxel_max_update_num=2),
}
KMAX_OPTIONS = [k for k, v in OPTIONS.items() if v.get("voxel_update", 0) == 0]
OUTSIDE_OPTIONS = [k for k, v in OPTIONS.items() if v.get("update_outside", 0) == 1]

SETS = ("zeros", "denormals", "huge", "inf", "nan", "max_sdf")
N_VIEWS = 8
BATCHES = {"ppv07": (0, 1), "ppv2": (2, 3), "ppv5": (4, 5), "ortho": (6, 7)}
UPLOAD_FOLLOW = ("ppv07", "ppv5")  # what is carved on an uploaded special_state: a fused batch, then a per-view one
ROI_WIDE = ((1, 1), (W - 2, H - 2))
ROI_CUT = ((14, 10), (34, 30))
ROI_TIGHT = ((18, 14), (30, 26))  # (at 0.7 pixels per voxel the small grid's whole footprint fits ROI_CUT)
ROIS = (ROI_TIGHT, ROI_WIDE, ROI_CUT, ROI_WIDE, ROI_CUT, ROI_WIDE, ROI_CUT, ROI_WIDE)
AXIS_COLUMN = 24  # the pixel column one column of voxels lands on exactly in view 6


def option_for(dims, name="kmax"):
    h = [e / 2.0 for e in EXTENT[tuple(dims)]]
    return CarverOption(bb_min=[-x for x in h], bb_max=h, resolution=1.0, update_option=UpdateOption(**OPTIONS[name]))


@functools.lru_cache(maxsize=None)
def positions(dims):
    """The oracle's voxel positions [n, 3] (read-only), x fastest."""
    orc = O.OracleGrid(option_for(dims))
    assert orc.dims == tuple(dims), (orc.dims, dims)
    pos = orc.positions()
    orc.close()
    pos.setflags(write=False)
    return pos


# ---- the views -------------------------------------------------------------------------------------------------------

DIST = 90.0
# (direction the camera sits in, pixels per voxel at the grid's centre)
PINHOLES = [((0.5, 0.4, -1.0), 0.7), ((-0.7, 0.3, -0.8), 0.7), ((0.2, -0.5, -1.0), 2.0), ((1.0, 0.2, 0.4), 2.0),
            ((-0.3, 0.6, 1.0), 5.0), ((0.1, -0.2, -1.0), 5.0)]


def _axis_translation(dims):
    """t.x of the axis-aligned orthographic view: the voxel column nx / 2 lands on AXIS_COLUMN in float32, exactly."""
    px = positions(dims)[:dims[0], 0]
    x = px[dims[0] // 2]
    t = F(AXIS_COLUMN) - x
    assert t.dtype == F and F(t + x) == F(AXIS_COLUMN), (t, x)
    return t


@functools.lru_cache(maxsize=None)
def views(dims):
    """The eight views of a grid: pinhole pairs at 0.7, 2 and 5 pixels per voxel, axis-aligned and oblique orthographic."""
    out = []
    for i, (d, ppv) in enumerate(PINHOLES):
        d = np.array(d, np.float64)
        w2c = synth.affine_inverse(synth.lookat_c2w(DIST * d / np.linalg.norm(d), (0.0, 0.0, 0.0), (0.0, 1.0, 0.1)))
        f = F(ppv * DIST)
        fy = f if i % 4 < 2 else F(f * 1.07)  # (fx == fy selects a kernel instance: both)
        rmin, rmax = ROIS[i]
        out.append(make_view(w2c.astype(F), f, fy, F(W / 2.0 - 0.3), F(H / 2.0 + 0.2), W, H, rmin, rmax))
    e = float(max(dims))
    ident = np.zeros((3, 4), F)
    ident[:, :3] = np.eye(3)
    ident[:, 3] = (_axis_translation(tuple(dims)), F(H // 2) + F(0.25), F(e + 3.0))
    out.append(make_view(ident, 1.0, 1.0, 0.0, 0.0, W, H, ROIS[6][0], ROIS[6][1], is_ortho=True))
    w2c = synth.affine_inverse(synth.lookat_c2w(np.array([1.0, 0.7, -1.2]) * e, (0.0, 0.0, 0.0), (0.0, 1.0, 0.1)))
    w2c[0, 3] += W / 2.0
    w2c[1, 3] += H / 2.0
    out.append(make_view(w2c.astype(F), 1.0, 1.0, 0.0, 0.0, W, H, ROIS[7][0], ROIS[7][1], is_ortho=True))
    assert len(out) == N_VIEWS
    return tuple(out)


def project(pos, view):
    """(pc.z, in front and inside the ROI, u, v): the oracle's projection in fp32 (lattice_scenes.project)."""
    m = np.array(list(view.w2c), F).reshape(3, 4)
    p = pos.astype(F)
    with np.errstate(all="ignore"):
        pc = [m[i, 3] + (m[i, 0] * p[:, 0] + (m[i, 1] * p[:, 1] + m[i, 2] * p[:, 2])) for i in range(3)]
        if view.is_ortho:
            u, v = pc[0], pc[1]
        else:
            u = F(view.fx) / pc[2] * pc[0] + F(view.cx)
            v = F(view.fy) / pc[2] * pc[1] + F(view.cy)
        assert u.dtype == F and v.dtype == F
        inside = (u >= view.roi_min[0]) & (v >= view.roi_min[1]) & (u <= view.roi_max[0]) & (v <= view.roi_max[1])
    return pc[2], inside & ~(pc[2] < 0), u, v


def pixels_per_voxel(dims, view):
    """The host's figure for its tile rule (carve_fused_plan.h pixels_per_voxel): at the grid's centre, the origin."""
    return 1.0 if view.is_ortho else float(max(view.fx, view.fy)) / float(view.w2c[11])


# ---- the images ------------------------------------------------------------------------------------------------------

# cells of 5 x 5 pixels from (14, 10): the 2 x 2 block at the cell's origin, the isolated pixel at (+3, +3); the four
# cells around the image centre first -- the grid's footprint at 0.7 pixels per voxel holds little more
CELL_ORDER = (5, 6, 9, 10, 1, 2, 4, 7, 8, 11, 13, 14, 0, 3, 12, 15)


def planted_pixels(k):
    """(block origin x, y), (isolated pixel x, y) of the k-th planted value."""
    c = CELL_ORDER[k % 16]
    bx, by = ROI_CUT[0][0] + 5 * (c % 4), ROI_CUT[0][1] + 5 * (c // 4)
    return (bx, by), (bx + 3, by + 3)


def base_image(i):
    """A smooth image in about +-1.5 (below -1 too: the truncation test)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (1.2 * np.sin(0.21 * xx + 0.7 * i) * np.cos(0.17 * yy - 0.4 * i) + 0.15 * ((i % 3) - 1)).astype(F)


def plant(img, values, shift=0):
    img = np.array(img, F)
    for k, val in enumerate(values):
        (bx, by), (ix, iy) = planted_pixels(k + shift)
        img[by:by + 2, bx:bx + 2] = val
        img[iy, ix] = val
    return img


def max_element(img):
    """(*std::max_element, its flat index): the first pixel if that is a NaN, else the first of the greatest pixels that
    are no NaN -- written as the loop it is (voxel_carver.cc:436)."""
    flat = np.asarray(img, F).reshape(-1)
    best = 0
    for i in range(1, len(flat)):
        if flat[best] < flat[i]:
            best = i
    return flat[best], best


def _max_zero_image(i, first, values):
    """An image below zero everywhere but for planted zeros: its maximum is zero, and the first maximal zero is `first`."""
    img = plant(-(np.abs(base_image(i)) + F(0.25)), values, shift=i)
    idx = int(np.flatnonzero(img.reshape(-1) == 0)[0])
    img.reshape(-1)[idx] = first
    return img


PZ, NZ = F(0.0), F(-0.0)
ZEROS = [PZ, NZ, NZ, PZ, NZ, PZ, PZ, NZ]
DENORMALS = [F(1e-45), F(-1e-45), F(1e-39), F(-1e-39), FLT_MIN, -FLT_MIN]
HUGE = [LOWEST, F(3e38), F(-3e38), FLT_MAX]
INFS = [F(np.inf), F(-np.inf)]
NAN = F(np.nan)


@functools.lru_cache(maxsize=None)
def image_set(name):
    """The eight images of a set (read-only), one per view."""
    b = base_image
    if name == "zeros":
        out = [_max_zero_image(0, NZ, ZEROS), plant(b(1), ZEROS), _max_zero_image(2, PZ, ZEROS), plant(b(3), ZEROS, 2),
               plant(b(4), ZEROS, 1), _max_zero_image(5, PZ, ZEROS[1:]), plant(b(6), ZEROS, 3), _max_zero_image(7, NZ, ZEROS[2:])]
    elif name == "denormals":
        tiny = F(1e-38)
        out = [plant(b(0), DENORMALS), b(1) * tiny, plant(b(2), DENORMALS, 2), plant(b(3), DENORMALS, 4), b(4) * tiny,
               plant(b(5), DENORMALS, 1), plant(b(6), DENORMALS, 3), b(7) * tiny]
    elif name == "huge":
        # (views 1 and 7 see every voxel: a flat lowest() there is a first touch that kMax then keeps -- lowest() > lowest()
        # is false -- wherever no other view looks; the weighted average of two of them overflows to -inf)
        flat, low = np.full((H, W), 3e38, F), np.full((H, W), LOWEST, F)
        out = [plant(b(0), HUGE), low, flat, flat.copy(), flat.copy(), plant(b(5), [F(-np.inf)] * 4), plant(b(6), HUGE, 2),
               low.copy()]
    elif name == "inf":
        out = [plant(b(0), INFS), plant(b(1), INFS, 1), plant(b(2), INFS[:1]), plant(b(3), INFS[1:]), plant(b(4), INFS, 2),
               plant(b(5), INFS, 3), zero_weight_image(), plant(b(7), INFS)]
    elif name == "nan":
        first = [b(i) for i in range(N_VIEWS)]
        for i in (0, 2, 5, 7):
            first[i][0, 0] = NAN
        out = [first[0], plant(first[1], [NAN] * 6), plant(first[2], [NAN] * 2, 1), plant(first[3], [NAN] * 3),
               np.full((H, W), NAN, F), first[5], plant(first[6], [NAN] * 4, 2), plant(first[7], [NAN], 3)]
    elif name == "max_sdf":
        # (the NaNs come late: a NaN state stays one under both update rules and would hide what follows)
        out = [b(i) for i in range(N_VIEWS)]
        for i, (first, later) in ((0, (NZ, PZ)), (1, (PZ, NZ))):  # column 0 lies outside every ROI
            out[i] = -(np.abs(out[i]) + F(0.25))
            out[i][0, 0], out[i][5, 0] = first, later
        out[2] = plant(out[2], [F(7.0)])
        out[2][0, 0] = out[2][3, 0] = F(7.0)
        out[3][0, 0] = np.inf
        out[4][0, 0] = NAN
        out[5][:] = -np.inf
        out[6] = plant(out[6], [NAN])
        out[6][0, 0] = NAN
        out[7][0, 0] = NAN
    else:
        raise KeyError(name)
    out = [np.ascontiguousarray(im, F) for im in out]
    for im in out:
        assert im.shape == (H, W)
        im.setflags(write=False)
    return tuple(out)


def zero_weight_image():
    """View 6's image of the `inf` set: +inf in the column right of AXIS_COLUMN and nothing else that is not finite.  The
    voxels that land on AXIS_COLUMN exactly read it with lu == 0: 0 * inf, a NaN out of an image without one."""
    img = base_image(6)
    img[12:28:2, AXIS_COLUMN + 1] = np.inf
    img[13, AXIS_COLUMN + 1] = np.inf  # (two rows running: lv does not matter either)
    return img


def special_state(dims):
    """(sdf, update_num) to upload: every class as a state value under every count 0 .. 3."""
    n = int(np.prod(dims))
    vals = np.array([1e-45, -1e-45, 1e-39, -FLT_MIN, 0.0, -0.0, 3e38, -3e38, FLT_MAX, LOWEST, np.inf, -np.inf, np.nan,
                     0.5, -0.5, 0.25, -2.0], F)
    i = np.arange(n)
    return vals[i % len(vals)].copy(), (i % 4).astype(np.int32)  # (17 values against 4 counts: every pair)


def depth_image(view, i):
    """The poisoned depth kind: depths around the grid's own camera depth, and -0.0, +-1e-45, +-1e-39, FLT_MAX, +inf on a
    fixed pattern of single pixels (the depth carve reads the nearest pixel)."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = (float(view.w2c[11]) + 8.0 * np.sin(0.19 * xx + i) * np.cos(0.23 * yy - i)).astype(F)
    vals = np.array([-0.0, 1e-45, -1e-45, 1e-39, -1e-39, FLT_MAX, np.inf], F)
    k = (3 * xx + 5 * yy) % 16
    img = np.where(k < len(vals), vals[np.minimum(k, len(vals) - 1)], img).astype(F)
    return np.ascontiguousarray(img)


# ---- the defects, as transformations of the inputs ------------------------------------------------------------------------

def flush_denormals(img):
    img = np.asarray(img, F)
    return np.where(np.abs(img) < FLT_MIN, np.copysign(F(0), img), img).astype(F)


def lose_sign_of_zero(img):
    img = np.asarray(img, F)
    return np.where(img == 0, F(0.0), img).astype(F)


def ignore_nan_in_maximum(img):
    """What a maximum that skips every NaN makes of the image, for max_sdf alone: pixel [0, 0] lies outside every ROI."""
    img = np.array(img, F)
    if np.isnan(img[0, 0]):
        img[0, 0] = LOWEST
    return img


def wrong_zero_of_maximum(img):
    img = np.array(img, F)
    m, idx = max_element(img)
    if m == 0:
        img.reshape(-1)[idx] = -m
    return img


def saturate(img):
    img = np.asarray(img, F)
    with np.errstate(invalid="ignore"):
        return np.where(np.isinf(img), np.copysign(FLT_MAX, img), img).astype(F)


def minus_zero_is_a_measurement(depth):
    depth = np.asarray(depth, F)
    return np.where((depth == 0) & np.signbit(depth), F(1e-45), depth).astype(F)


DEFECTS = {
    "denormal_flush": flush_denormals,
    "lost_sign_of_zero": lose_sign_of_zero,
    "nan_ignoring_maximum": ignore_nan_in_maximum,
    "wrong_zero_of_maximum": wrong_zero_of_maximum,
    "saturation": saturate,
}


# ---- the oracle's results ----------------------------------------------------------------------------------------------

def oracle_carve(dims, option, images, which=range(N_VIEWS), state=None):
    """(sdf, update_num) after the views `which`, in that order, from the fill state or from `state`."""
    prev = O.set_num_threads(1)
    try:
        g = O.OracleGrid(option_for(dims, option))
        if state is not None:
            g.upload(*state)
        vs = views(tuple(dims))
        for i in which:
            g.carve(vs[i], images[i])
        out = g.download()
        g.close()
    finally:
        O.set_num_threads(prev)
    return out


@functools.lru_cache(maxsize=None)
def oracle_states(dims, option, set_name, defect=None):
    """The states (read-only) after each of the four BATCHES of a set, carved one after the other -- with `defect`, of
    the transformed images.  The comparisons look at every one of them: a later view may cover what an earlier one did."""
    images = image_set(set_name)
    if defect is not None:
        images = [DEFECTS[defect](im) for im in images]
    prev = O.set_num_threads(1)
    try:
        g = O.OracleGrid(option_for(dims, option))
        vs, out = views(tuple(dims)), []
        for idx in BATCHES.values():
            for i in idx:
                g.carve(vs[i], images[i])
            sdf, cnt = g.download()
            sdf.setflags(write=False)
            cnt.setflags(write=False)
            out.append((sdf, cnt))
        g.close()
    finally:
        O.set_num_threads(prev)
    return tuple(out)


def oracle_final(dims, option, set_name, defect=None):
    return oracle_states(dims, option, set_name, defect)[-1]


def differ(a, b):
    """Voxels at which two states differ: update_num, NaN-ness, or the bits of a value that is no NaN."""
    (sa, ua), (sb, ub) = a, b
    na, nb = np.isnan(sa), np.isnan(sb)
    bits_a, bits_b = np.where(na, 0, sa.view(np.uint32)), np.where(nb, 0, sb.view(np.uint32))
    return int(((ua != ub) | (na != nb) | (bits_a != bits_b)).sum())
