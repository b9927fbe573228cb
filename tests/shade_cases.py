"""The cases the CPU and the GPU tests of the shading pass share (tests/test_shade_cpu.py, tests/test_gpu_shade.py):
name -> (vertices float32 [n, 3], faces int32 [m, 3], attributes float32 [n, channels], list of views, background), and the
numpy restatement's answer for each (tests/shade_ref.py), computed once.  The meshes and views of tests/raster_cases.py are
reused and given attributes in [64, 255] from a seeded generator; the cases added here are the ones the shading rules need.
The photometric cases: name -> (vertices, faces, colors float32 [n, 3], views, photos, masks)."""
import zlib

import numpy as np

import raster_cases as RC
import shade_ref as SF

F = np.float32
W, H = RC.W, RC.H
BG = (7.25, 300.0, -3.0, 0.49)   # the background goes through q as well: 7, 255, 0, 0

memo = RC.memo


def attrs(n, channels, seed):
    """n x channels float32 in [64, 255]."""
    return np.random.RandomState(seed).uniform(64.0, 255.0, (n, channels)).astype(F)


def seed_of(name):
    return zlib.crc32(name.encode()) & 0xffff


def affine_attr(v):
    """An affine function of the world position, in [64, 255] on the slanted quad."""
    v = np.asarray(v, np.float64)
    return np.stack([100.0 + 10.0 * v[:, 0] + 7.0 * v[:, 1] + 9.0 * v[:, 2], 200.0 - 12.0 * v[:, 0] + 5.0 * v[:, 1] - 4.0 * v[:, 2],
                     80.0 + 3.0 * v[:, 0] - 6.0 * v[:, 1] + 11.0 * v[:, 2]], axis=1).astype(F)


# a slanted quad in the identity pinhole: camera depth 3 to 10.5 across it
SLANT_V = [(-1, -1, 3), (2.5, -1.2, 10), (-1, 1, 3.2), (2.5, 1.5, 10.5)]
SLANT_F = [(0, 1, 2), (1, 3, 2)]
# corners that the identity pinhole projects exactly onto the pixel centres (8, 4), (32, 16), (16, 36), (40, 36), at depths
# 4 and 8: the shared edge from (32, 16) to (16, 36) passes through the centres (28, 21), (24, 26), (20, 31)
ONVERTEX_V = [(-2, -2, 4), (2, -1, 8), (-1, 2, 4), (4, 4, 8)]
ONVERTEX_F = [(0, 1, 2), (1, 3, 2)]
ONVERTEX_PX = [(8, 4), (32, 16), (16, 36), (40, 36)]
ONEDGE_PX = [(28, 21), (24, 26), (20, 31)]


def sized_views():
    """Three views of different sizes in one call: 48 x 40, one hit word per row exactly (64 x 33), and three words with the
    last one partial (130 x 37)."""
    return [RC.look((9.0, 6.0, -11.0), (0.0, 0.0, 0.0), 70.0), RC.look((-7.0, 9.5, 8.0), (0.3, -0.2, 0.1), 62.0, w=64, h=33),
            RC.look((2.0, -12.0, 5.0), (0.0, 0.0, 0.0), 66.0, w=130, h=37)]


def cases():
    def make():
        A = lambda x, t: np.array(x, t)  # noqa: E731
        c = {}
        for name, (v, f, views) in RC.cases().items():
            if name != "views_65":
                c[name] = (v, f, attrs(len(v), 3, seed_of(name)), views, BG)
        c["slanted_quad"] = (A(SLANT_V, F), A(SLANT_F, np.int32), affine_attr(SLANT_V), [RC.pinhole_identity()], BG)
        # two coplanar faces at equal depth with distinct vertex ids and different attributes (face 1 repeats face 0), and
        # the other half of the quad with ids of its own again: ties over the whole of face 0 and along the diagonal
        tri = [RC.QUAD_V[0], RC.QUAD_V[1], RC.QUAD_V[2]]
        split_v = A(tri + tri + [RC.QUAD_V[1], RC.QUAD_V[3], RC.QUAD_V[2]], F)
        split_a = np.concatenate([np.full((3, 3), 100.0, F), np.full((3, 3), 200.0, F), np.full((3, 3), 150.0, F)])
        split_a += A([[0, 1, 2], [3, 4, 5], [6, 7, 8]] * 3, F)
        c["coincident_split"] = (split_v, A([(0, 1, 2), (3, 4, 5), (6, 7, 8)], np.int32), split_a, [RC.ortho_identity()], BG)
        c["on_vertex"] = (A(ONVERTEX_V, F), A(ONVERTEX_F, np.int32), attrs(4, 3, 11), [RC.pinhole_identity()], BG)
        # every channel count: mixed sizes, 65 views, a one-pixel ROI (raster_cases' roi_edges has one), no faces
        bv, bf = RC.box_mesh(1)
        v65, f65, views65 = RC.cases()["views_65"]
        qv, qf, roi_views = RC.cases()["roi_edges"]
        for ch in (1, 2, 3, 4):
            c["sizes_c%d" % ch] = (bv, bf, attrs(len(bv), ch, 20 + ch), sized_views(), BG)
            c["views_65_c%d" % ch] = (v65, f65, attrs(len(v65), ch, 30 + ch), views65, BG)
            c["roi_c%d" % ch] = (qv, qf, attrs(len(qv), ch, 40 + ch), roi_views, BG)
            c["no_faces_c%d" % ch] = (qv, np.zeros((0, 3), np.int32), attrs(len(qv), ch, 50 + ch), roi_views[:2], BG)
        # q at its edges: NaN, both infinities, negative values, values above 255 and halves
        odd = attrs(len(bv), 4, 60)
        odd[0] = (np.nan, np.inf, -np.inf, -20.0)
        odd[5] = (300.0, -0.0, 254.5, 255.5)
        odd[9] = (0.5, 0.49999997, 1e30, -1e30)
        odd[13:20, 1] = np.linspace(-40.0, 400.0, 7)
        c["odd_values"] = (bv, bf, odd, sized_views()[:2], (np.nan, -np.inf, np.inf, 254.5))
        return c
    return memo("shade cases", make)


def faces_of(name):
    """The definition's face images of a case, shared between its channel counts and with raster_cases where it has them."""
    v, f, a, views, bg = cases()[name]
    if name in RC.cases():
        return [w["face"] for w in RC.want(name)]
    for stem in ("sizes", "views_65", "roi", "no_faces"):
        if name.startswith(stem + "_c"):
            if stem == "views_65":
                return [w["face"] for w in RC.want("views_65")]
            return memo(("shade faces", stem), lambda: [SF.face_image(v, f, view) for view in views])
    if name == "odd_values":
        return faces_of("sizes_c4")[:2]
    return memo(("shade faces", name), lambda: [SF.face_image(v, f, view) for view in views])


def want(name, rules=frozenset()):
    """The restatement's answer for a case (the definition, or a mutant of it)."""
    rules = frozenset(rules)
    v, f, a, views, bg = cases()[name]
    return memo(("shade want", name, rules), lambda: SF.shade(v, f, a, views, bg, rules, faces_of(name)))


def photo_cases():
    def make():
        c = {}
        bv, bf = RC.box_mesh(1)
        for name, views in (("photo_sizes", sized_views()), ("photo_65", RC.cases()["views_65"][2])):
            rng = np.random.RandomState(seed_of(name))
            faces = faces_of("sizes_c3" if name == "photo_sizes" else "views_65_c3")
            photos = [rng.randint(0, 256, (w.height, w.width, 3)).astype(np.uint8) for w in views]
            masks = []
            for i, (w, fi) in enumerate(zip(views, faces)):
                ys, xs = np.nonzero(fi >= 0)
                m = np.zeros((w.height, w.width), np.uint8)
                # left of the middle column of the mesh's image: the silhouette cuts through it (values other than 1 too)
                m[:, :int(np.median(xs)) + 1] = 1 + 100 * (i % 3)
                m[::7] = 0
                masks.append(m)
            masks[1][:] = 0   # a view whose silhouette is empty
            c[name] = (bv, bf, attrs(len(bv), 3, seed_of(name) + 1), views, photos, masks)
        # every hit pixel differs by 255 in the red channel: a constant 255 rendered over a photograph whose red is 0
        views = sized_views()[:1]
        col = attrs(len(bv), 3, 77)
        col[:, 0] = 255.0
        photo = np.random.RandomState(78).randint(0, 256, (views[0].height, views[0].width, 3)).astype(np.uint8)
        photo[:, :, 0] = 0
        c["photo_255"] = (bv, bf, col, views, [photo], None)
        return c
    return memo("photo cases", make)


def photo_faces(name):
    return faces_of({"photo_sizes": "sizes_c3", "photo_65": "views_65_c3", "photo_255": "sizes_c3"}[name])[:len(photo_cases()[name][3])]


def photo_want(name, masked=True, rules=frozenset()):
    rules = frozenset(rules)
    v, f, col, views, photos, masks = photo_cases()[name]
    return memo(("photo want", name, masked, rules),
                lambda: SF.photo_error(v, f, col, views, photos, masks if masked else None, rules, photo_faces(name)))
