"""The colouring of vertices on the device (vcy_color_vertices, color.hip): bit equality with the serial host function and
the numpy restatement (tests/color_ref.py) on supplied depth, on a whole-grid and on a z-slab context; the internal
ray-cast against supplied depth; an occlusion scene whose answer does not share the restatement's arithmetic; the order
of the views; the C++ facade; queued views."""
import os
import subprocess

import numpy as np
import pytest

import color_cases as CC
import color_ref as CR
import test_gpu_render as TR
from vacancy_amd import capi
from vacancy_amd import carver as vc

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(m, i) for m in CC.MODES for i in CC.INTERPS]


def as_tuple(d):
    return d["rgb"], d["n_used"], d["best_view"]


# ---- 1. bit equality with supplied depth -----------------------------------------------------------------------------

@pytest.mark.parametrize("z_range", [None, (5, 11)], ids=["whole", "slab"])
@pytest.mark.parametrize("case", CC.CASE_NAMES)
def test_device_equals_host_and_restatement(case, z_range):
    c = CC.cases()[case]
    dev = TR.make_dev(CC.option(), CC.DIMS, z_range=z_range)   # (a slab is accepted: the depth is supplied)
    for mode, interp in COMBOS:
        ctx = "%s mode %d interp %d" % (case, mode, interp)
        got = dev.ColorVertices(CC.points(), c["views"], c["photos"], CC.normals(), c["depth"], mode, interp, c["tol"],
                                c["min_cos"], c["fallback"])
        host = vc.color_vertices_host(CC.points(), c["views"], c["photos"], c["depth"], CC.normals(), mode, interp, c["tol"],
                                      c["min_cos"], c["fallback"])
        CC.assert_equal(got, as_tuple(host), ctx + " (host function)")
        CC.assert_equal(got, CC.want(case, mode, interp), ctx + " (restatement)")
        assert got["device_ms"] > 0.0
    # more than one block, a last block that is not full, and a single vertex
    p, n = CC.points(), CC.normals()
    for count in (1, 257):
        got = dev.ColorVertices(p[:count], c["views"], c["photos"], n[:count], c["depth"], CR.WEIGHTED, CR.BILINEAR, c["tol"],
                                c["min_cos"], c["fallback"])
        rgb, used, best = CC.want(case, CR.WEIGHTED, CR.BILINEAR)
        CC.assert_equal(got, (rgb[:count], used[:count], best[:count]), "%s first %d" % (case, count))


def test_null_outputs_empty_input_and_refusals_on_the_device():
    lib = capi.load()
    c = CC.cases()["render_depth"]
    dev = TR.make_dev(CC.option(), CC.DIMS)
    keep, args, out = vc._color_args(CC.points(), c["views"], c["photos"], None, c["depth"], CR.MEAN, CR.NN, 0.5, 0.0,
                                     (1.0, 2.0, 3.0))
    full = dev.ColorVertices(CC.points(), c["views"], c["photos"], None, c["depth"], CR.MEAN, CR.NN, 0.5, 0.0, (1.0, 2.0, 3.0))
    for o in out.values():
        o[...] = 77
    a = list(args)
    a[9] = a[10] = None    # n_used_out, best_view_out
    assert lib.vcy_color_vertices(dev.ctx, 0.0, *a) == 0, vc.last_error()
    assert np.array_equal(CC.bits(out["rgb"]), CC.bits(full["rgb"]))
    assert np.all(out["n_used"] == 77) and np.all(out["best_view"] == 77)
    out["rgb"][...] = 77
    a = list(args)
    a[0] = 0
    assert lib.vcy_color_vertices(dev.ctx, 0.0, *a) == 0
    assert np.all(out["rgb"] == 77)
    for change in ("mode", "interp", "tol", "min_cos", "normals", "n_views", "fx", "photo"):
        keep, args, out = vc._color_args(CC.points()[:40], [capi.View.from_buffer_copy(v) for v in c["views"][:2]],
                                         c["photos"][:2], CC.normals()[:40], c["depth"][:2], CR.WEIGHTED, CR.NN, 0.5, 0.0,
                                         (1.0, 2.0, 3.0))
        for o in out.values():
            o[...] = 77
        a, opt = list(args), keep[4]
        if change == "mode":
            opt.mode = 3
        elif change == "interp":
            opt.interp = -1
        elif change == "tol":
            opt.depth_tolerance = float("nan")
        elif change == "min_cos":
            opt.min_cos = -1.0
        elif change == "normals":
            a[2] = None
        elif change == "n_views":
            a[3] = 0
        elif change == "fx":
            keep[5][0].fx = 0.0
        else:
            keep[6][1] = None
        assert lib.vcy_color_vertices(dev.ctx, 0.0, *a) == capi.VCY_ERR_INVALID_ARG, change
        assert all(np.all(o == 77) for o in out.values()), change


# ---- 2. the internal ray-cast equals supplied depth --------------------------------------------------------------------

@pytest.mark.parametrize("rayskip", [1, 0])
@pytest.mark.parametrize("dims", [(24, 20, 17), (65, 9, 17)], ids=lambda d: "%dx%dx%d" % d)
def test_internal_render_equals_supplied_depth(dims, rayskip):
    c = TR.case(dims)
    dev = TR.make_dev(c["opt"], dims)
    dev.set_param("rayskip", rayskip)
    sdf, cnt, iso = c["states"]["random"]
    dev.upload(sdf, cnt)
    vs = list(c["views"].values())
    ph = CC.photos(vs, 31)
    rng = np.random.RandomState(32)
    half = np.array(TR.BOX[dims]) / 2.0 * 1.2
    p = ((rng.rand(1500, 3) * 2.0 - 1.0) * half).astype(F)
    nr = rng.randn(1500, 3)
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F)
    depth = [g["depth"] for g in dev.RenderHull(vs, iso)]
    assert sum(int(np.isfinite(d).sum()) for d in depth) > 500
    for mode, interp in COMBOS:
        a = dev.ColorVertices(p, vs, ph, nr, None, mode, interp, 0.6, 0.05, (9.0, 8.0, 7.0), iso_level=iso)
        assert dev.last_render_ms() > 0.0
        b = dev.ColorVertices(p, vs, ph, nr, depth, mode, interp, 0.6, 0.05, (9.0, 8.0, 7.0))
        CC.assert_equal(a, as_tuple(b), "%s rayskip %d mode %d interp %d" % (dims, rayskip, mode, interp))
    seen = dev.ColorVertices(p, vs, ph, None, None, CR.MEAN, CR.NN, 0.6, iso_level=iso)
    free = dev.ColorVertices(p, vs, ph, None, [np.full_like(d, np.inf) for d in depth], CR.MEAN, CR.NN, 0.6)
    assert (seen["n_used"] < free["n_used"]).sum() > 100, "the hull occludes nothing: the test shows nothing"
    s2, c2 = dev.download()
    assert np.array_equal(CC.bits(s2), CC.bits(sdf)) and np.array_equal(c2, cnt), "colouring changed the state"


def test_more_than_one_chunk_of_views_through_the_internal_render():
    dims = (24, 20, 17)
    c = TR.case(dims)
    dev = TR.make_dev(c["opt"], dims)
    sdf, cnt, iso = c["states"]["random"]
    dev.upload(sdf, cnt)
    vs = CC.tiny_views(70)
    ph = CC.photos(vs, 33)
    depth = [g["depth"] for g in dev.RenderHull(vs, iso)]
    for mode, interp in ((CR.WEIGHTED, CR.BILINEAR), (CR.BEST, CR.NN)):
        a = dev.ColorVertices(CC.points(), vs, ph, CC.normals(), None, mode, interp, 0.6, iso_level=iso)
        b = vc.color_vertices_host(CC.points(), vs, ph, depth, CC.normals(), mode, interp, 0.6)
        CC.assert_equal(a, as_tuple(b), "70 views, mode %d" % mode)
    assert a["best_view"].max() >= 64


def test_slab_without_depth_is_refused_and_a_fresh_context_stays_lazy():
    dims = CC.DIMS
    c = CC.cases()["render_depth"]
    slab = TR.make_dev(CC.option(), dims, z_range=(5, 11))
    with pytest.raises(RuntimeError, match="whole grid"):
        slab.ColorVertices(CC.points(), c["views"], c["photos"], CC.normals())
    lib = capi.load()
    keep, args, out = vc._color_args(CC.points(), c["views"], c["photos"], CC.normals(), None, CR.WEIGHTED, CR.NN, 0.5, 0.0,
                                     (1.0, 2.0, 3.0))
    for o in out.values():
        o[...] = 77
    assert lib.vcy_color_vertices(slab.ctx, 0.0, *args) == capi.VCY_ERR_UNSUPPORTED
    assert all(np.all(o == 77) for o in out.values())
    # nothing carved: every ray is a miss, every view a vertex projects into contributes
    fresh, other = TR.make_dev(CC.option(), dims), TR.make_dev(CC.option(), dims)
    for mode, interp in COMBOS:
        got = fresh.ColorVertices(CC.points(), c["views"], c["photos"], CC.normals(), None, mode, interp, 0.0, 0.0, c["fallback"])
        all_miss = [np.full((v.height, v.width), np.inf, F) for v in c["views"]]
        ref = CR.color_vertices(CC.points(), CC.normals(), c["views"], c["photos"], all_miss, mode, interp, 0.0, 0.0, c["fallback"])
        CC.assert_equal(got, ref, "fresh mode %d interp %d" % (mode, interp))
    assert fresh.state_diff(other) == 0


# ---- 3. occlusion, without the restatement -----------------------------------------------------------------------------

def test_occlusion_between_two_plates():
    dims = CC.DIMS
    nx, ny, nz = dims
    opt = CC.option()
    dev = TR.make_dev(opt, dims)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    solid = ((x >= 4) & (x < 6)) | ((x >= 16) & (x < 18))
    dev.upload(np.where(solid, F(-0.5), F(0.5)).astype(F).reshape(-1), np.ones(nx * ny * nz, np.int32))
    mesh = dev.ExtractIsoSurface(0.0, True)
    v = mesh["vertices"]
    assert len(v) > 1000
    e = float(max(dims))
    view_a = TR.look((e + 2.0, 0.0, 0.0), (0.0, 0.0, 0.0), ortho=True, up=(0.0, 0.0, 1.0))      # from +x
    view_b = TR.look((-(e + 2.0), 0.0, 0.0), (0.0, 0.0, 0.0), ortho=True, up=(0.0, 0.0, 1.0))   # from -x
    red, blue, green = (255.0, 0.0, 0.0), (0.0, 0.0, 255.0), (0.0, 255.0, 0.0)
    photos = [np.broadcast_to(np.array(col, np.uint8), (TR.H, TR.W, 3)).copy() for col in (red, blue)]
    pitch = TR.BOX[dims][0] / nx
    # (the NN sampler: the four bilinear weights do not sum to exactly 1 in float, so a constant photograph samples to
    # 254.99998 at some positions; "exactly" below is a statement about visibility, not about the sampler)
    got = dev.ColorVertices(v, [view_a, view_b], photos, None, None, CR.MEAN, CR.NN, pitch, 0.0, green)
    rgb = got["rgb"]
    px = dev.positions()[:nx, 0].astype(np.float64)      # the voxel centres along x
    xi = (v[:, 0].astype(np.float64) - px[0]) / (px[1] - px[0])   # vertex x in voxel-index units
    assert not np.any(rgb[xi < 10, 0] != 0), "red on the low plate: view A sees through the high plate"
    assert not np.any(rgb[xi > 12, 2] != 0), "blue on the high plate: view B sees through the low plate"
    low_face, high_face = np.abs(xi - 3.5) < 0.01, np.abs(xi - 17.5) < 0.01
    assert low_face.sum() > 200 and high_face.sum() > 200
    assert np.all(rgb[low_face] == np.array(blue, F)) and np.all(got["n_used"][low_face] == 1)
    assert np.all(rgb[high_face] == np.array(red, F)) and np.all(got["best_view"][high_face] == 0)
    is_col = [np.all(rgb == np.array(col, F), axis=1) for col in (red, blue, green)]
    assert np.all(is_col[0] | is_col[1] | is_col[2])
    inner = (np.abs(xi - 5.5) < 0.01) | (np.abs(xi - 15.5) < 0.01)      # the faces between the plates: no view sees them
    assert inner.sum() > 200 and np.all(is_col[2][inner]) and np.all(got["best_view"][inner] == -1)


# ---- 4. the order of the views -----------------------------------------------------------------------------------------

def test_view_order():
    full = CC.cases()["render_depth"]
    # views that share a rotation tie in weight, and a tie goes to the lower index whatever the order: one view per camera
    names = [k for k in CC.views() if k not in ("roi_shrunk", "roi_one_pixel", "ortho_axis_roi", "pinhole_axis")]
    keep = [list(CC.views()).index(k) for k in names]
    c = {k: [full[k][i] for i in keep] for k in ("views", "photos", "depth")}
    c["tol"] = full["tol"]
    dev = TR.make_dev(CC.option(), CC.DIMS)
    n = len(c["views"])
    perm = np.random.RandomState(41).permutation(n)
    assert not np.array_equal(perm, np.arange(n))
    pick = lambda seq: [seq[k] for k in perm]   # noqa: E731
    p, nr = CC.points(), CC.normals()
    base = dev.ColorVertices(p, c["views"], c["photos"], nr, c["depth"], CR.BEST, CR.NN, c["tol"])
    perm_best = dev.ColorVertices(p, pick(c["views"]), pick(c["photos"]), nr, pick(c["depth"]), CR.BEST, CR.NN, c["tol"])
    seen = perm_best["best_view"] >= 0
    assert seen.sum() > 500
    assert np.array_equal(perm[perm_best["best_view"][seen]], base["best_view"][seen])
    assert np.array_equal(perm_best["best_view"] < 0, base["best_view"] < 0)
    assert np.array_equal(CC.bits(perm_best["rgb"]), CC.bits(base["rgb"]))
    # MEAN over constant photographs: sums of small integers are exact in any order
    rng = np.random.RandomState(42)
    const = [np.broadcast_to(rng.randint(0, 256, 3).astype(np.uint8), (v.height, v.width, 3)).copy() for v in c["views"]]
    a = dev.ColorVertices(p, c["views"], const, None, c["depth"], CR.MEAN, CR.BILINEAR, c["tol"])
    b = dev.ColorVertices(p, pick(c["views"]), pick(const), None, pick(c["depth"]), CR.MEAN, CR.NN, c["tol"])
    b2 = dev.ColorVertices(p, pick(c["views"]), pick(const), None, pick(c["depth"]), CR.MEAN, CR.BILINEAR, c["tol"])
    a_nn = dev.ColorVertices(p, c["views"], const, None, c["depth"], CR.MEAN, CR.NN, c["tol"])
    assert np.array_equal(CC.bits(a_nn["rgb"]), CC.bits(b["rgb"])) and np.array_equal(a_nn["n_used"], b["n_used"])
    assert np.array_equal(a["n_used"], b2["n_used"])
    # with random photographs the order is part of the definition: the device follows the host function on the permuted input
    for mode, interp in COMBOS:
        got = dev.ColorVertices(p, pick(c["views"]), pick(c["photos"]), nr, pick(c["depth"]), mode, interp, c["tol"])
        host = vc.color_vertices_host(p, pick(c["views"]), pick(c["photos"]), pick(c["depth"]), nr, mode, interp, c["tol"])
        CC.assert_equal(got, as_tuple(host), "permuted, mode %d interp %d" % (mode, interp))


# ---- 5. the C++ facade -------------------------------------------------------------------------------------------------

def test_cpp_color_mesh_writes_a_coloured_ply(tmp_path):
    r = subprocess.run([os.path.join(ROOT, "vacancy_amd", "host", "host_selftest"), ".", "colormesh", str(tmp_path)],
                       check=True, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    cols = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("VIEWCOLOR") or l.startswith("FALLBACK")])
    assert len(cols) == 9
    row = [l.split() for l in lines if l.startswith("COLORMESH")][0]
    ok, nv, nc, foreign, refused = (int(x) for x in row[1:])
    assert ok == 1 and nv > 500 and nc == nv, row        # vertex_colors().size() == vertices().size()
    assert foreign == 0 and refused == 5, row
    text = open(os.path.join(str(tmp_path), "colored.ply")).read().split("end_header\n")
    header, body = text[0], text[1].splitlines()
    for name in ("red", "green", "blue", "alpha"):
        assert "property uchar %s\n" % name in header
    assert "element vertex %d\n" % nv in header
    rows = np.array([[float(x) for x in l.split()] for l in body[:nv]])
    assert rows.shape == (nv, 7) and np.all(rows[:, 6] == 255)
    rgb = rows[:, 3:6]
    # a weighted mean of the views' colours, or the fallback: inside their range channel by channel ...
    assert np.all(rgb >= cols.min(axis=0)) and np.all(rgb <= cols.max(axis=0))
    # ... and most of the sphere is seen by some view, from more than one side
    assert len(np.unique(rgb, axis=0)) > 20
    assert np.all(rgb == cols[8], axis=1).sum() < nv // 4


# ---- 6. queued views ---------------------------------------------------------------------------------------------------

def test_queued_views_are_applied_first():
    n, opt, views, masks = TR.sphere_scene(6)
    lazy, eager = TR.make_dev(opt, (n, n, n)), TR.make_dev(opt, (n, n, n))
    eager.set_param("defer", 0)
    for v, m in zip(views, masks):
        assert eager.CarveSilhouette(v, m), vc.last_error()
    mesh = eager.ExtractIsoSurface(0.0, True, normals=True)
    assert len(mesh["vertices"]) > 500
    for v, m in zip(views, masks):
        assert lazy.CarveSilhouette(v, m), vc.last_error()      # (queued)
    ph = CC.photos(views, 51)
    a = lazy.ColorVertices(mesh["vertices"], views, ph, mesh["normals"])
    b = eager.ColorVertices(mesh["vertices"], views, ph, mesh["normals"])
    CC.assert_equal(a, as_tuple(b), "queued against eager")
    assert (b["n_used"] > 0).mean() > 0.9 and 0 < (b["n_used"] < len(views)).sum()   # seen, and not from everywhere
    assert lazy.state_diff(eager) == 0
