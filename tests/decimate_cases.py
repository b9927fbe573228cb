"""Meshes for the mesh decimation tests -- the smoothing tests' meshes plus cases of their own, each of which asserts here,
against the restatement, the property it exists for -- and the restatement's results over the test matrix, computed
once."""
import numpy as np

import decimate_ref as DR
import oracle_lib as O
import smooth_cases as SC
from vacancy_amd.capi import CarverOption

F = np.float32
CELLS = (0.001, 0.75, 2.0, 3.7, 1000.0)
MODES = (DR.MEAN, DR.NEAREST, DR.FIRST)
ORIGIN = (-13.25, -13.25, -13.25)
SMOOTH_NAMES = ("octahedron", "mc_sphere", "two_components", "open_patch", "fan300", "degenerate", "isolated", "one_vertex",
                "257_vertices")
# no vertex without a face, no repeated or degenerate face: cell 0.001 returns these unchanged
CLEAN = ("octahedron", "mc_sphere", "two_components", "open_patch", "fan300", "257_vertices", "mc_sphere_40", "crowd",
         "two_sheets_opposite", "row_tiers")

memo = SC.memo
bits = SC.bits
assert_bits = SC.assert_bits
assert_normals = SC.assert_normals


def crowd():
    """700 vertices inside one cell (at every cell of the matrix from 0.75 up), each in a face with two vertices of a ring
    that lies in other cells: a member row longer than a block."""
    rng = np.random.RandomState(11)
    inner = (1.8 + 0.5 * rng.rand(700, 3)).astype(F)
    a = 2.0 * np.pi * np.arange(16) / 16.0
    ring = np.stack([2.05 + 6.0 * np.cos(a), 2.05 + 6.0 * np.sin(a), 2.05 + 0.0 * a], axis=-1).astype(F)
    f = np.array([[i, 700 + i % 16, 700 + (i + 1) % 16] for i in range(700)], np.int32)
    return np.concatenate([inner, ring]), f[rng.permutation(700)]


TIER_SIZES = (1, 16, 17, 48, 49, 256, 257)


def row_tiers():
    """Clusters of exactly 1, 16, 17, 48, 49, 256 and 257 members at cell 2.0, one cell each, stacked along z below a ring
    whose vertices have a cell each; every point in a face with two ring vertices: member rows at both edges of the
    two in-register sorts and of the row that gets a workgroup of its own."""
    rng = np.random.RandomState(12)
    groups = [np.array([1.8, 1.8, -12.2 + 2.0 * k], F) + (0.5 * rng.rand(m, 3)).astype(F) for k, m in enumerate(TIER_SIZES)]
    inner = np.concatenate(groups).astype(F)
    n = len(inner)
    a = 2.0 * np.pi * np.arange(16) / 16.0
    ring = np.stack([2.05 + 6.0 * np.cos(a), 2.05 + 6.0 * np.sin(a), 2.05 + 0.0 * a], axis=-1).astype(F)
    order = rng.permutation(n)                   # (a cell's members are not neighbours in the vertex array either)
    f = np.array([[i, n + i % 16, n + (i + 1) % 16] for i in range(n)], np.int32)
    rank = np.empty(n, np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    f[:, 0] = rank[f[:, 0]]
    return np.concatenate([inner[order], ring]), f[rng.permutation(n)]


def two_sheets(opposite):
    v, f = SC.mesh("open_patch")
    w = (v + np.array([0.0, 0.0, 0.01], F)).astype(F)
    g = f[:, ::-1] if opposite else f
    return np.concatenate([v, w]), np.concatenate([f, g + len(v)]).astype(np.int32)


def rotations():
    """Three rotations of one face, its mirror image and one more face over four vertices far apart."""
    v = np.array([[-9.0, -9.0, -9.0], [9.5, -8.0, -7.0], [0.5, 9.0, -8.5], [1.0, 0.5, 10.0]], F)
    f = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [0, 1, 3]], np.int32)
    return v, f


BOUNDARY_AXIS = (-7.4, -6.0, -3.0, -1.5, -0.0, 1.5, 3.0, 6.0, 7.4)


def boundary():
    """A 9 x 9 patch whose x and y lie exactly on cell planes of the cells 0.75, 2.0 and 3.7 with origin 0 (t integral),
    at negative t, and at -0.0; z alternates between -0.0 and a plane."""
    ax = np.array(BOUNDARY_AXIS, F)
    y, x = np.mgrid[0:9, 0:9]
    z = np.where((x + y) % 2 == 0, F(-0.0), F(-1.5)).astype(F)
    v = np.stack([ax[x], ax[y], z], axis=-1).reshape(-1, 3).astype(F)
    return v, SC.mesh("open_patch")[1]


def mc_sphere_40():
    """The CPU oracle's marching-cubes mesh of a sphere on a 40^3 grid: many blocks, a table larger than one block's worth."""
    opt = CarverOption(bb_min=[-20.0] * 3, bb_max=[20.0] * 3, resolution=1.0)
    grid = O.OracleGrid(opt)
    assert grid.dims == (40, 40, 40)
    pos = grid.positions().astype(np.float64)
    sdf = (16.3 - np.sqrt((pos * pos).sum(axis=1))).astype(F)
    grid.upload(sdf, np.ones(grid.n, np.int32))
    m = grid.marching_cubes(0.0, True)
    grid.close()
    return m["vertices"].astype(F), m["faces"].astype(np.int32)


OWN = {"crowd": crowd, "row_tiers": row_tiers, "two_sheets_same": lambda: two_sheets(False), "two_sheets_opposite": lambda: two_sheets(True),
       "rotations": rotations, "boundary": boundary, "mc_sphere_40": mc_sphere_40}
CASE_NAMES = SMOOTH_NAMES + tuple(OWN)


def origin_of(name):
    return (0.0, 0.0, 0.0) if name == "boundary" else ORIGIN


def mesh(name):
    """(vertices float32 [n, 3], faces int32 [m, 3]), read-only."""
    if name in SMOOTH_NAMES:
        return SC.mesh(name)

    def make():
        v, f = OWN[name]()
        v = np.ascontiguousarray(v, F)
        assert np.isfinite(v).all()
        v.setflags(write=False)
        f = np.ascontiguousarray(f, np.int32)
        f.setflags(write=False)
        check_case(name, v, f)
        return v, f
    return memo(("decimate mesh", name), make)


def want(name, cell, mode):
    """The restatement's outputs."""
    def make():
        v, f = mesh(name)
        return DR.decimate(v, f, cell, origin_of(name), mode)
    return memo(("decimate want", name, cell, mode), make)


def matrix():
    return [(cell, mode) for cell in CELLS for mode in MODES]


def canonical_rows(faces):
    return [tuple(r) for r in DR.canonical(faces)]


def check_case(name, v, f):
    """What the case is there for, asserted against the restatement."""
    ref = lambda cell: DR.decimate(v, f, cell, origin_of(name), DR.FIRST)
    if name == "crowd":
        for cell in CELLS[1:]:
            r = ref(cell)
            assert r["members"].max() >= 700 and (len(r["faces"]) >= 1 or cell == 1000.0), cell
    elif name == "row_tiers":
        sizes = sorted(ref(2.0)["members"])
        assert sizes == sorted(TIER_SIZES + (1,) * 16), sizes              # (the ring: sixteen cells of one vertex)
    elif name == "two_sheets_same":
        r = ref(2.0)
        assert 0 < len(r["faces"]) < r["n_noncollapsed"]
    elif name == "two_sheets_opposite":
        r = ref(2.0)
        rows = set(map(tuple, DR.canonical(r["faces"])))
        assert any((a, c, b) in rows for a, b, c in rows)
    elif name == "rotations":
        for cell in CELLS[:-1]:
            r = ref(cell)
            assert list(r["face_source"]) == [0, 3, 4], (cell, r["face_source"])
    elif name == "boundary":
        ax = np.array(BOUNDARY_AXIS, F)
        assert np.signbit(ax[4]) and np.signbit(v[0, 2]) and v[0, 2] == 0
        for cell, k in ((0.75, [-10, -8, -4, -2, 0, 2, 4, 8, 9]), (2.0, [-4, -3, -2, -1, 0, 0, 1, 3, 3]),
                        (3.7, [-2, -2, -1, -1, 0, 0, 0, 1, 2])):
            keys, ok = DR.cell_keys(np.stack([ax, ax, ax], axis=-1), (0.0, 0.0, 0.0), cell)
            assert ok.all() and list(keys[:, 0]) == k, (cell, list(keys[:, 0]))
        t = ax / F(2.0)
        assert (t[[1, 4, 7]] == np.floor(t[[1, 4, 7]])).all() and (ax[:4] < 0).all()   # on a plane; negative t
        assert (ax[[0, 8]] / F(3.7) == np.array([-2, 2], F)).all()
    elif name == "mc_sphere_40":
        assert len(v) > 4096 and len(v) % 256 != 0 and len(f) == 2 * len(v) - 4
