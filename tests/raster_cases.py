"""The cases the CPU and the GPU tests of the mesh rasteriser share (tests/test_raster_cpu.py, tests/test_gpu_raster.py):
name -> (vertices float32 [n, 3], faces int32 [m, 3], list of views), and the numpy restatement's answer for each
(tests/raster_ref.py), computed once.  Images are 48 x 40; one case is 130 wide, so that its rows cross two hit words."""
import numpy as np

import raster_ref as RF
from vacancy_amd import synth
from vacancy_amd.capi import make_view

F = np.float32
W, H = 48, 40

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def ortho_identity(roi=None, w=W, h=H, tz=0.0):
    """u = x, w = y, depth = z + tz: vertices sit on exact pixel coordinates."""
    m = np.zeros((3, 4), F)
    m[:, :3] = np.eye(3)
    m[2, 3] = tz
    rmin, rmax = roi if roi else (None, None)
    return make_view(m, 1.0, 1.0, 0.0, 0.0, w, h, rmin, rmax, True)


def pinhole_identity(roi=None, f=32.0, w=W, h=H, tz=0.0):
    """u = f / z * x + w / 2, w = f / z * y + h / 2 with the camera at the origin looking along +z."""
    m = np.zeros((3, 4), F)
    m[:, :3] = np.eye(3)
    m[2, 3] = tz
    rmin, rmax = roi if roi else (None, None)
    return make_view(m, F(f), F(f), F(w / 2), F(h / 2), w, h, rmin, rmax, False)


def look(pos, target, f=30.0, ortho=False, roi=None, up=(0.0, 1.0, 0.1), w=W, h=H):
    w2c = synth.affine_inverse(synth.lookat_c2w(pos, target, up))
    if ortho:
        w2c[0, 3] += w / 2.0
        w2c[1, 3] += h / 2.0
    rmin, rmax = roi if roi else (None, None)
    return make_view(w2c.astype(F), F(f), F(f * 1.07), F(w / 2.0 - 0.3), F(h / 2.0 + 0.2), w, h, rmin, rmax, ortho)


# the tilted quad of the lattice scenes: z = 4 + (x - 2) / 2 + (y - 2) / 4 over [2, 10]^2, doubled areas 64
QUAD_V = [(2, 2, 4), (10, 2, 8), (2, 10, 6), (10, 10, 10)]
QUAD_F = [(0, 1, 2), (1, 3, 2)]
# the triangle of the pinhole literal: at depth 4, projected to (8, 4), (40, 4), (8, 36) by pinhole_identity
FRONTO_V = [(-2, -2, 4), (2, -2, 4), (-2, 2, 4)]


def box_mesh(levels):
    """A box of 12 triangles, each split `levels` times at its edge midpoints (12 * 4 ** levels faces), vertices shared."""
    c = np.array([(x, y, z) for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64) * (3.0, 2.5, 2.0)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    verts = [tuple(p) for p in c]
    index = {p: i for i, p in enumerate(verts)}
    faces = [t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))]

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for _ in range(levels):
        nxt = []
        for a, b, cc in faces:
            pa, pb, pc = (np.array(verts[k]) for k in (a, b, cc))
            ab, bc, ca = vid(tuple((pa + pb) / 2)), vid(tuple((pb + pc) / 2)), vid(tuple((pc + pa) / 2))
            nxt += [(a, ab, ca), (ab, b, bc), (ca, bc, cc), (ab, bc, ca)]
        faces = nxt
    return np.array(verts, F), np.array(faces, np.int32)


def box_views():
    return [look((9.0, 6.0, -11.0), (0.0, 0.0, 0.0), 70.0), look((-7.0, 9.5, 8.0), (0.3, -0.2, 0.1), 62.0),
            look((2.0, -12.0, 5.0), (0.0, 0.0, 0.0), 66.0, w=130, h=H)]


def many_views(n):
    """n pinhole views on a circle around the origin; every one of them sees the box."""
    out = []
    for i in range(n):
        a = 2.0 * np.pi * i / n
        out.append(look((14.0 * np.cos(a), 3.0 + (i % 5), 14.0 * np.sin(a)), (0.0, 0.0, 0.0), 60.0 + (i % 7)))
    return out


def cases():
    def make():
        A = lambda x, t: np.array(x, t)  # noqa: E731
        inf, nan = np.inf, np.nan
        c = {}
        ortho, pin = ortho_identity(), pinhole_identity()
        # literals: the tilted quad in the identity ortho view (shared diagonal through pixel centres: ties), the
        # fronto-parallel triangle in the pinhole
        c["lattice_ortho"] = (A(QUAD_V, F), A(QUAD_F, np.int32), [ortho])
        c["lattice_pinhole"] = (A(FRONTO_V, F), A([(0, 1, 2)], np.int32), [pin])
        # both windings, coincident faces (0 and 2, 1 and 3), and the same quad behind the first one
        c["coincident"] = (A(QUAD_V + [(x, y, z + 3) for x, y, z in QUAD_V], F),
                           A(QUAD_F + [(0, 2, 1), (1, 2, 3)] + [(4, 5, 6), (5, 7, 6)], np.int32), [ortho])
        # the quad's edges exactly on roi_min / roi_max, a ROI inside it, a one-pixel ROI on its diagonal, one beside it
        c["roi_edges"] = (A(QUAD_V, F), A(QUAD_F, np.int32),
                          [ortho_identity(((2, 2), (10, 10))), ortho_identity(((3, 4), (8, 6))), ortho_identity(((6, 6), (6, 6))),
                           ortho_identity(((11, 2), (11, 2))), ortho_identity(((10, 10), (47, 39)))])
        # a tilted triangle in the pinhole: perspective depth differs from affine depth
        c["tilted_pinhole"] = (A([(-2, -2, 4), (2, -1.5, 8), (-1, 2, 5)], F), A([(0, 1, 2)], np.int32), [pin, pinhole_identity(((5, 4), (40, 33)))])
        # needles without a pixel centre in their box, a sliver with some, fractional corners
        c["needles"] = (A([(5.2, 3.1, 1), (5.4, 30.2, 1), (5.3, 3.4, 1), (20.25, 7.5, 2), (20.75, 7.5, 2), (20.5, 7.9, 2),
                           (30.1, 2.2, 3), (33.9, 37.7, 3), (30.6, 2.1, 3), (12.5, 12.5, 2), (17.25, 13.75, 3), (13.5, 18.125, 4)], F),
                        A([(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11)], np.int32), [ortho])
        # class 1: collinear corners, a repeated index (a NaN vertex named twice is still class 0: the vertex comes first)
        c["degenerate"] = (A(QUAD_V + [(4, 4, 5), (6, 6, 5), (20, 20, nan)], F),
                           A([(0, 4, 5), (0, 1, 1), (2, 2, 2), (0, 1, 2), (6, 6, 1), (3, 3, 6)], np.int32), [ortho, pin])
        # class 0: a vertex behind the pinhole camera, at camera depth 0 (ortho keeps it, the pinhole drops it), NaN, inf
        c["unusable"] = (A([(-2, -2, 4), (2, -2, 4), (-2, 2, -1), (-2, 2, 0), (nan, 0, 4), (0, inf, 4), (1, 1, -inf),
                            (2, 2, 0), (10, 2, 0), (2, 10, 3), (2, 10, -0.5)], F),
                         A([(0, 1, 2), (0, 1, 3), (0, 1, 4), (0, 1, 5), (0, 1, 6), (7, 8, 9), (7, 8, 10)], np.int32), [pin, ortho])
        # a far vertex: the edges anchored at it vanish at every pixel in double, the third decides -- and the candidate
        # box, not the coverage test, is what keeps the column left of min u out (vertex 0 is the far one: the anchor)
        c["far_vertex"] = (A([(2.0 ** 70, 2.0 ** 70, 5), (20.5, 19.5, 2), (5.5, 20.5, 3), (20.5, 25.5, 1)], F),
                           A([(1, 2, 0), (0, 3, 1)], np.int32), [ortho])
        # one triangle over the whole image and beyond it; with the small faces of the box in front of it: both kinds
        bv, bf = box_mesh(1)
        big = A([(-400, -300, 9), (500, -300, 14), (-400, 600, 20)], F)
        c["whole_image"] = (big, A([(0, 1, 2)], np.int32), [ortho, pinhole_identity(tz=0.0), ortho_identity(((5, 4), (40, 33)))])
        bview = [look((9.0, 6.0, -11.0), (0.0, 0.0, 0.0), 30.0), look((0.0, 0.0, -30.0), (0.0, 0.0, 0.0), ortho=True, f=1.0),
                 look((9.0, 6.0, -11.0), (0.0, 0.0, 0.0), 30.0, roi=((24, 20), (24, 20)))]
        wall = A([(-60, -50, 6), (70, -50, 6), (-60, 80, 6), (0.1, 0.1, 0.1), (0.2, 0.1, 0.1), (0.1, 0.2, 0.1)], F)
        c["mixed"] = (np.concatenate([bv, wall]), np.concatenate([bf, A([(0, 1, 2), (3, 4, 5)], np.int32) + len(bv)]), bview)
        # the convex box, coarse and fine, in three pinhole views (one 130 wide)
        c["box_12"] = box_mesh(0) + (box_views(),)
        c["box_192"] = box_mesh(2) + (box_views(),)
        # 65 views: a second chunk on the device
        c["views_65"] = box_mesh(1) + (many_views(65),)
        return c
    return memo("cases", make)


def want(name, rules=frozenset()):
    """The restatement's answer for a case (the definition, or a mutant of it)."""
    rules = frozenset(rules)
    v, f, views = cases()[name]
    return memo(("want", name, rules), lambda: RF.raster(v, f, views, rules))
