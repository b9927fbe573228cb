"""Meshes for the tests of the quadric representatives: every case of the decimation tests at its cells, a case with corner
rows at both edges of the in-register sort, and cases of their own -- a tessellated box (corners, edges, flats), the box far
from the origin, a tilted flat patch (rank-1 quadrics), a shallow wedge (the optimum outside every cell) and zero-area faces
-- each of which asserts here, against the restatement, the property it exists for; and the restatement's results, computed
once."""
import numpy as np

import decimate_cases as DC
import quadric_ref as QR
import smooth_cases as SC

F = np.float32
REGS = (0.0, 1e-3)
BOX_LO, BOX_HI, BOX_N = -3.1, 4.3, 12
FAR = 4096.0

memo = DC.memo
bits = DC.bits


def box(shift=0.0):
    """The surface of the box [-3.1, 4.3]^3, 12 x 12 quads per side, vertices shared along edges, outward faces."""
    n = BOX_N
    ax = np.linspace(BOX_LO, BOX_HI, n + 1)
    ids, v, t = {}, [], []

    def vid(ijk):
        if ijk not in ids:
            ids[ijk] = len(v)
            v.append([ax[ijk[0]], ax[ijk[1]], ax[ijk[2]]])
        return ids[ijk]

    for axis in range(3):
        a, b = [c for c in range(3) if c != axis]
        for side in (0, 1):
            for i in range(n):
                for j in range(n):
                    def at(ii, jj):
                        ijk = [0, 0, 0]
                        ijk[axis], ijk[a], ijk[b] = side * n, ii, jj
                        return vid(tuple(ijk))
                    q = [at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)]
                    if (side == 1) == (axis != 1):
                        q = q[::-1]
                    t += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return (np.array(v, F) + F(shift)).astype(F), np.array(t, np.int32)


def sheet(z_of_x, base=0):
    ax = np.arange(9, dtype=F) * F(0.4) - F(1.0)
    v = [[x, y, z_of_x(x)] for x in ax for y in ax]
    t = []
    for i in range(8):
        for j in range(8):
            a = base + i * 9 + j
            t += [[a, a + 9, a + 10], [a, a + 10, a + 1]]
    return v, t


def flat_patch():
    v, t = sheet(lambda x: 0.3 + 0.25 * x)
    return np.array(v, F), np.array(t, np.int32)


def wedge():
    """Two sheets z = +-0.02 (x - 40): their planes meet at x = 40, far outside the cells the sheets lie in."""
    v0, t0 = sheet(lambda x: 0.02 * (x - 40.0))
    v1, t1 = sheet(lambda x: -0.02 * (x - 40.0), base=81)
    return np.array(v0 + v1, F), np.array(t0 + t1, np.int32)


def slivers():
    """Faces of three points on one axis-parallel line each (the cross product is exactly 0), their points 3 apart so that
    they survive the cells up to 2.0, and two faces that name a vertex twice."""
    v, t = [], []
    for k in range(6):
        y, z = -5.0 + 2.5 * k, 1.0 + 0.5 * k
        t.append([len(v), len(v) + 1, len(v) + 2])
        v += [[-4.0, y, z], [-1.0, y, z], [2.0, y, z]]
    t += [[0, 0, 4], [7, 2, 7]]
    return np.array(v, F), np.array(t, np.int32)


# name -> (maker, cells)
OWN = {"box": (box, (2.0, 3.7)), "box_far": (lambda: box(FAR), (2.0, 3.7)), "flat_patch": (flat_patch, (0.75,)), "wedge": (wedge, (3.7,)),
       "slivers": (slivers, (0.75, 2.0)), "fans_11_14": (lambda: SC.mesh("fans_11_14"), (0.001, 0.75))}
OWN_NAMES = tuple(OWN)
CASE_NAMES = DC.CASE_NAMES + OWN_NAMES


def origin_of(name):
    return DC.origin_of(name)


def cells_of(name):
    return OWN[name][1] if name in OWN else DC.CELLS


def matrix(name):
    return [(cell, reg) for cell in cells_of(name) for reg in REGS]


def mesh(name):
    """(vertices float32 [n, 3], faces int32 [m, 3]), read-only."""
    if name not in OWN:
        return DC.mesh(name)

    def make():
        v, f = OWN[name][0]()
        v = np.array(v, F)
        f = np.array(f, np.int32)
        assert np.isfinite(v).all()
        v.setflags(write=False)
        f.setflags(write=False)
        check_case(name, v, f)
        return v, f
    return memo(("quadric mesh", name), make)


def want(name, cell, reg):
    """The restatement's outputs."""
    def make():
        v, f = mesh(name)
        return QR.decimate(v, f, cell, origin_of(name), reg)
    return memo(("quadric want", name, cell, reg), make)


def box_distance(p, shift=0.0):
    """Distance of every row of p to the surface of the box (moved by `shift`), in float64."""
    p = np.asarray(p, np.float64)
    lo, hi = np.float64(F(BOX_LO) + F(shift)), np.float64(F(BOX_HI) + F(shift))
    q = np.clip(p, lo, hi)
    outside = np.sqrt(((p - q) ** 2).sum(axis=1))
    inside = np.minimum(p - lo, hi - p).min(axis=1)
    return np.where(outside > 0, outside, np.abs(inside))


def check_case(name, v, f):
    """What the case is there for, asserted against the restatement."""
    ref = lambda cell, reg: QR.decimate(v, f, cell, origin_of(name), reg)
    if name == "box":
        assert len(v) == 6 * 12 * 12 + 2 and len(f) == 6 * 12 * 12 * 2
        for cell in (2.0, 3.7):
            r = ref(cell, 1e-3)
            assert r["n_fallback"] == 0 and 20.0 * box_distance(r["vertices"]).max() < box_distance(r["mean"]).max(), cell
    elif name == "box_far":
        r = ref(2.0, 1e-3)
        assert np.abs(v).min() > 4000 and r["n_fallback"] < len(r["vertices"])
    elif name == "flat_patch":
        r0, r1 = ref(0.75, 0.0), ref(0.75, 1e-3)
        assert len(r0["vertices"]) == 25 and r0["n_fallback"] == 25 and r1["n_fallback"] == 0
    elif name == "wedge":
        r = ref(3.7, 1e-3)
        assert len(r["vertices"]) == 4 and r["n_fallback"] == 4
    elif name == "slivers":
        for cell in (0.75, 2.0):
            r = ref(cell, 1e-3)
            assert len(r["vertices"]) >= 18 and r["n_fallback"] == len(r["vertices"]), cell
    elif name == "fans_11_14":
        valence = np.bincount(f.reshape(-1))
        assert {11, 12, 13, 14} <= set(valence.tolist())       # corner rows at both edges of the in-register sort
