"""Small finite meshes for the mesh smoothing tests, each there for a reason, and the restatement's results over the
test matrix, computed once."""
import numpy as np

import oracle_lib as O
import smooth_ref as SR
from vacancy_amd.capi import CarverOption

F = np.float32
ITERATIONS = (0, 1, 2, 7)
FACTORS = ((0.5, -0.53), (0.33, 0.0), (0.0, 0.0))
PINS = (0, 1)

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def mc_sphere():
    """The CPU oracle's marching-cubes mesh of a sphere on a 24^3 grid: a few thousand vertices in cell raster order, more
    than one block of 256, a last block that is not full."""
    opt = CarverOption(bb_min=[-12.0] * 3, bb_max=[12.0] * 3, resolution=1.0)
    grid = O.OracleGrid(opt)
    assert grid.dims == (24, 24, 24)
    pos = grid.positions().astype(np.float64)
    sdf = (8.3 - np.sqrt((pos * pos).sum(axis=1))).astype(F)     # (negative outside, as a carve leaves it)
    grid.upload(sdf, np.ones(grid.n, np.int32))
    m = grid.marching_cubes(0.0, True)
    grid.close()
    return m["vertices"].astype(F), m["faces"].astype(np.int32)


def two_components():
    v, f = octahedron()
    rng = np.random.RandomState(5)
    w = (v * F(0.37) + rng.rand(6, 3).astype(F) * F(0.2) + F(3.0)).astype(F)
    return np.concatenate([v, w]), np.concatenate([f, f[:, ::-1] + 6]).astype(np.int32)


def open_patch():
    """A 9 x 9 triangulated grid over a paraboloid: 32 rim vertices, 49 interior ones, none of which is at rest."""
    y, x = np.mgrid[0:9, 0:9]
    z = 0.05 * (x * x + 0.5 * y * y)
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(F)
    faces = []
    for j in range(8):
        for i in range(8):
            a, b, c, d = 9 * j + i, 9 * j + i + 1, 9 * (j + 1) + i, 9 * (j + 1) + i + 1
            faces += [[a, b, d], [a, d, c]]
    return v, np.array(faces, np.int32)


def open_patch_rim():
    y, x = np.mgrid[0:9, 0:9]
    return ((x == 0) | (x == 8) | (y == 0) | (y == 8)).reshape(-1)


def fan300():
    """One hub vertex in 300 faces: a row longer than a wave, a block and any in-register row."""
    a = 2.0 * np.pi * np.arange(300) / 300.0
    rng = np.random.RandomState(6)
    rim = np.stack([np.cos(a), np.sin(a), 0.1 * rng.rand(300)], axis=-1)
    v = np.concatenate([[[0.03, -0.02, 1.0]], rim]).astype(F)
    f = np.array([[0, 1 + i, 1 + (i + 1) % 300] for i in range(300)], np.int32)
    return v, f[rng.permutation(300)]            # (the hub's row is not in rim order)


FAN_SIZES = (11, 12, 13, 14)


def fans_11_14():
    """Four closed fans whose hubs have 11, 12, 13 and 14 faces: rows on both sides of the 12 corners a row is sorted with
    in registers, and the lengths next to them."""
    rng = np.random.RandomState(10)
    verts, faces, hubs = [], [], []
    for i, k in enumerate(FAN_SIZES):
        hub = len(verts)
        hubs.append(hub)
        a = 2.0 * np.pi * np.arange(k) / k
        verts += [[4.0 * i + 0.03, -0.02, 1.0]] + [[4.0 * i + np.cos(t), np.sin(t), 0.2 * rng.rand()] for t in a]
        faces += [[hub, hub + 1 + j, hub + 1 + (j + 1) % k] for j in range(k)]
    f = np.array(faces, np.int32)[rng.permutation(len(faces))]
    off, corners = SR.rows(len(verts), f)
    assert tuple(off[h + 1] - off[h] for h in hubs) == FAN_SIZES       # corner counts of 12 and 13 occur
    for h in hubs:                                                     # no hub's faces walk its rim in order
        rim = f[(f == h).any(axis=1), 1]
        assert not np.array_equal(np.sort(rim), rim), h
    return np.array(verts, F), f


def degenerate():
    """Faces that name a vertex twice and three times, one face present twice, a non-manifold edge with three faces."""
    rng = np.random.RandomState(7)
    v = (rng.rand(7, 3) * 2.0 - 1.0).astype(F)
    f = np.array([[0, 0, 1], [2, 2, 2], [0, 1, 2], [3, 4, 0], [0, 1, 2], [4, 3, 1], [3, 4, 5], [5, 6, 5], [6, 2, 3]], np.int32)
    return v, f


def isolated():
    """Vertices that no face names: the first index, the last one and one in the middle."""
    v, f = octahedron()
    rng = np.random.RandomState(8)
    extra = (rng.rand(3, 3) * 4.0).astype(F)
    verts = np.concatenate([extra[:1], v[:3], extra[1:2], v[3:], extra[2:]])
    remap = np.array([1, 2, 3, 5, 6, 7])
    return verts, remap[f].astype(np.int32)


ISOLATED_IDS = (0, 4, 8)


def one_vertex():
    return np.array([[0.25, -1.5, 3.0]], F), np.zeros((0, 3), np.int32)


def strip_257():
    """A triangle strip over 257 vertices: one full block and one lane."""
    rng = np.random.RandomState(9)
    i = np.arange(257)
    v = np.stack([0.5 * i, (i % 2) * 1.0, 0.3 * rng.rand(257)], axis=-1).astype(F)
    f = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(255)], np.int32)
    return v, f


MAKERS = {"octahedron": octahedron, "mc_sphere": mc_sphere, "two_components": two_components, "open_patch": open_patch,
          "fan300": fan300, "degenerate": degenerate, "isolated": isolated, "one_vertex": one_vertex,
          "257_vertices": strip_257, "fans_11_14": fans_11_14}
CASE_NAMES = tuple(MAKERS)


def mesh(name):
    """(vertices float32 [n, 3], faces int32 [m, 3]); no coordinate is -0.0 (p + 0 * d would turn it into +0.0)."""
    def make():
        v, f = MAKERS[name]()
        v = np.ascontiguousarray(v + F(0.0), F)
        assert np.isfinite(v).all() and not np.signbit(v[v == 0]).any()
        v.setflags(write=False)
        f = np.ascontiguousarray(f, np.int32)
        f.setflags(write=False)
        return v, f
    return memo(("mesh", name), make)


def want(name, iterations, factors, pin):
    """The restatement's positions."""
    def make():
        v, f = mesh(name)
        return SR.smooth(v, f, max(ITERATIONS), factors[0], factors[1], pin, keep=ITERATIONS)[1]
    return memo(("want", name, factors, pin), make)[iterations]


def matrix():
    return [(it, fc, pin) for it in ITERATIONS for fc in FACTORS for pin in PINS]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits(got, want_, ctx):
    g, w = bits(got), bits(want_)
    assert g.shape == w.shape, (ctx, g.shape, w.shape)
    assert np.array_equal(g, w), "%s: %d of %d words differ" % (ctx, int((g != w).sum()), g.size)


def assert_normals(got, want_, ctx):
    """Bits where the expected value is finite, NaN-ness elsewhere (the sign of 0 / 0 is not part of the contract)."""
    got, want_ = np.asarray(got, F), np.asarray(want_, F)
    assert got.shape == want_.shape, (ctx, got.shape, want_.shape)
    fin = np.isfinite(want_)
    assert np.array_equal(bits(got)[fin], bits(want_)[fin]), "%s: %d finite words differ" % (
        ctx, int((bits(got)[fin] != bits(want_)[fin]).sum()))
    assert np.array_equal(np.isnan(got), np.isnan(want_)), ctx
