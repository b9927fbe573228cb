"""The silhouettes at the hand-made edges of the device SDF builder (vacancy_amd/csrc/sdf2d.hip), shared by
test_silhouette_cases_cpu.py (the oracle against the definition, the host restatement against the oracle) and
test_gpu_silhouette_edges.py (every device path against the oracle).  No test in here.

A case is (name, mask uint8 [h][w], roi_min (x, y), roi_max (x, y)), ROI bounds inclusive.  Everything is deterministic:
random masks come from a RandomState seeded by the case's name.  The pixels outside a ROI are, wherever the pattern
leaves the choice, SEEDS of the set under test -- the transform is restricted to the ROI (voxel_carver.cc:107-166) and
has to ignore them.

  row-chunk shapes    3 rows; widths and left edges around the 64-pixel chunk of sdf_rows_kernel; single seeds at the
                      ROI's first / last pixel (carries over every chunk), at lanes 63 and 0 of adjacent chunks, no seed
                      inside while the margin is full of them (raw distance +-FLT_MAX), noise
  column-unroll shapes  5 columns; heights around the 8-row unroll of sdf_cols_kernel; seeds in the first, the last or
                      one middle row only (every other row is kInf after the row pass), noise
  degenerate shapes   1x1, 1xN, Nx1, one-pixel / one-row / one-column ROIs
  truncation equality 7x7 block in 11x11: normalised values are multiples of 1/4, so d == -band exists for the bands
                      0.25, 0.5, 0.75 (MakeSignedDistanceField invalidates on `-band >= d`, equality included)
  scratch-reuse pair  an all-255 image (max |v| = FLT_MAX) and a small blob of the same size
"""
import ctypes as C
import functools
import zlib

import numpy as np

import oracle_lib as O
from vacancy_amd.capi import View

VALUES = np.array([0, 1, 128, 254, 255], np.uint8)
ROW_WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 193)
ROW_LEFT_EDGES = (0, 1, 63, 64)
COL_HEIGHTS = (1, 2, 7, 8, 9, 15, 16, 17, 25)
COL_TOP_EDGES = (0, 1, 5)
BANDS = (0.1, 1.0)
EQUALITY_NAME = "equality/block7_in_11"
EQUALITY_BANDS = (0.25, 0.5, 0.75)
SCRATCH_SHAPE = (18, 24)  # h, w


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _frame(w, h, rmin, rmax, inside, outside):
    m = np.full((h, w), outside, np.uint8)
    m[rmin[1]:rmax[1] + 1, rmin[0]:rmax[0] + 1] = inside
    return m


def _noise(name, w, h, density):
    """255 everywhere, a fraction `density` of the pixels redrawn from VALUES -- over the whole image, margin included."""
    rng = _rng(name)
    m = np.full((h, w), 255, np.uint8)
    sel = rng.rand(h, w) < density
    m[sel] = VALUES[rng.randint(0, len(VALUES), int(sel.sum()))]
    return m


# the two seed sets of MakeSignedDistanceField: "n" -- pixels != 255 are the seeds of the inside distance (background 255),
# "s" -- pixels == 255 are the seeds of the outside distance (background 0)
_SETS = (("n", 255, 0), ("s", 0, 255))


def _row_chunk_cases():
    out = []
    for rw in ROW_WIDTHS:
        for rx0 in ROW_LEFT_EDGES:
            for pad in (0, 3):
                top = 2 if pad else 0
                w, h = rx0 + rw + pad, top + 3 + pad
                rmin, rmax = (rx0, top), (rx0 + rw - 1, top + 2)
                tag = "rows/rw%d_x%d_pad%d/" % (rw, rx0, pad)
                for sname, bg, seed in _SETS:
                    for where, (px, py) in (("first", rmin), ("last", rmax)):
                        m = _frame(w, h, rmin, rmax, bg, seed)
                        m[py, px] = seed
                        out.append((tag + "%s_%s" % (sname, where), m, rmin, rmax))
                    # lane 63 of one chunk and lane 0 of the next one, in the middle row
                    lanes = [k for k in (63, 64) if k < rw]
                    for pick in ([k] for k in lanes) if len(lanes) < 2 else ([63], [64], [63, 64]):
                        m = _frame(w, h, rmin, rmax, bg, seed)
                        for k in pick:
                            m[top + 1, rx0 + k] = seed
                        out.append((tag + "%s_lane%s" % (sname, "+".join(str(k) for k in pick)), m, rmin, rmax))
                    # no seed of this set inside the ROI, the whole margin full of them
                    out.append((tag + "%s_only_outside" % sname, _frame(w, h, rmin, rmax, bg, seed), rmin, rmax))
                for density in (0.02, 0.5):
                    name = tag + "noise%g" % density
                    out.append((name, _noise(name, w, h, density), rmin, rmax))
    return out


def _col_unroll_cases():
    out = []
    rw, rx0 = 5, 2
    for rh in COL_HEIGHTS:
        for ry0 in COL_TOP_EDGES:
            w, h = rx0 + rw + 1, ry0 + rh + min(ry0, 3)
            rmin, rmax = (rx0, ry0), (rx0 + rw - 1, ry0 + rh - 1)
            tag = "cols/rh%d_y%d/" % (rh, ry0)
            for sname, bg, seed in _SETS:
                for where, row in (("first", ry0), ("last", ry0 + rh - 1), ("middle", ry0 + rh // 2)):
                    m = _frame(w, h, rmin, rmax, bg, seed)
                    m[row, rx0 + 1] = m[row, rx0 + 4] = seed
                    out.append((tag + "%s_%s_row" % (sname, where), m, rmin, rmax))
            name = tag + "noise0.05"
            out.append((name, _noise(name, w, h, 0.05), rmin, rmax))
    return out


def _degenerate_cases():
    out = [("degenerate/1x1_255", np.full((1, 1), 255, np.uint8), (0, 0), (0, 0)),
           ("degenerate/1x1_0", np.zeros((1, 1), np.uint8), (0, 0), (0, 0))]
    for n in (64, 65):  # (N = 1 is the 1x1 image above)
        for w, h in ((1, n), (n, 1)):
            tag = "degenerate/%dx%d_" % (w, h)
            full = ((0, 0), (w - 1, h - 1))
            out.append((tag + "all255", np.full((h, w), 255, np.uint8)) + full)
            out.append((tag + "all0", np.zeros((h, w), np.uint8)) + full)
            for sname, bg, seed in _SETS:
                m = np.full((h, w), bg, np.uint8)
                m[h - 1, w - 1] = seed
                out.append((tag + "%s_last" % sname, m) + full)
            out.append((tag + "noise0.3", _noise(tag + "noise0.3", w, h, 0.3)) + full)
    w, h = 70, 20
    for rname, rmin, rmax in (("pixel", (66, 7), (66, 7)), ("row", (1, 19), (68, 19)), ("row_full", (0, 0), (69, 0)),
                              ("column", (69, 0), (69, 19)), ("column_inner", (64, 2), (64, 17))):
        for density in (0.3, 0.97):
            name = "degenerate/70x20_%s_roi_noise%g" % (rname, density)
            out.append((name, _noise(name, w, h, density), rmin, rmax))
        for sname, bg, seed in _SETS:
            out.append(("degenerate/70x20_%s_roi_%s_only_outside" % (rname, sname), _frame(w, h, rmin, rmax, bg, seed),
                        rmin, rmax))
    return out


def _equality_case():
    m = np.zeros((11, 11), np.uint8)
    m[2:9, 2:9] = 255
    case = (EQUALITY_NAME, m, (0, 0), (10, 10))
    # the case must keep testing the `>=`: the largest inside and outside distances are both 4, every normalised value
    # is a multiple of 1/4, and each band meets a pixel exactly
    raw = O.make_sdf(m, (0, 0), (10, 10), False, False, 0.1)
    assert raw.min() == -4.0 and raw.max() == 4.0, (raw.min(), raw.max())
    plain = O.make_sdf(m, (0, 0), (10, 10), True, False, 0.1)
    for band in EQUALITY_BANDS:
        assert np.float32(band) == band and int((plain == -np.float32(band)).sum()) >= 1, band
    return case


def scratch_pair():
    """(all-255 image, small blob) of one size: max |v| is FLT_MAX for the first and a few pixels for the second."""
    h, w = SCRATCH_SHAPE
    full = ((0, 0), (w - 1, h - 1))
    blob = np.zeros((h, w), np.uint8)
    blob[7:11, 9:14] = 255
    blob[8, 14] = 255
    return (("scratch/all255", np.full((h, w), 255, np.uint8)) + full, ("scratch/blob", blob) + full)


@functools.lru_cache(maxsize=None)
def cases():
    """The whole table, in a fixed order, names unique, masks read-only."""
    out = _row_chunk_cases() + _col_unroll_cases() + _degenerate_cases() + [_equality_case()] + list(scratch_pair())
    assert len({c[0] for c in out}) == len(out)
    for name, m, rmin, rmax in out:
        h, w = m.shape
        assert m.dtype == np.uint8 and 0 <= rmin[0] <= rmax[0] < w and 0 <= rmin[1] <= rmax[1] < h, name
        m.setflags(write=False)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c[0] == name)


def bands(name):
    """Truncation bands a case is run with."""
    return BANDS + (EQUALITY_BANDS if name == EQUALITY_NAME else ())


def settings(name):
    """(normalize, truncate, band) of every run of a case: normalise x truncate, every band where it is read."""
    return [(norm, False, BANDS[0]) for norm in (True, False)] + \
           [(norm, True, band) for norm in (True, False) for band in bands(name)]


_expected = {}


def oracle_image(c, normalize, truncate, band):
    """orc_make_sdf of a case -- computed once, shared, read-only."""
    key = (c[0], bool(normalize), bool(truncate), float(band))
    img = _expected.get(key)
    if img is None:
        img = O.make_sdf(c[1], c[2], c[3], bool(normalize), bool(truncate), band)
        img.setflags(write=False)
        _expected[key] = img
    return img


def size_view(w, h, roi_min=None, roi_max=None):
    """A vcy_view that carries only width, height and ROI: all that the producer-only entry points read."""
    v = View()
    v.width, v.height = w, h
    v.roi_min = (C.c_int32 * 2)(*(roi_min if roi_min is not None else (0, 0)))
    v.roi_max = (C.c_int32 * 2)(*(roi_max if roi_max is not None else (w - 1, h - 1)))
    return v


def view_of(c):
    return size_view(c[1].shape[1], c[1].shape[0], c[2], c[3])
