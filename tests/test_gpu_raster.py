"""The mesh rasteriser on the device (vcy_raster_mesh / vcy_mesh_agreement, raster.hip) against the serial host function
(vcy_raster_mesh_host, which tests/test_raster_cpu.py holds against the numpy restatement): depth BITS, face ids, hit words
and drop counts are compared for equality, with the wide-face threshold on both sides of every box, on the CPU cases, on
an extracted, smoothed and decimated mesh, from a z-slab context, and through MeshAgreement and ColorVertices."""
import numpy as np
import pytest

import oracle_lib as O
import raster_cases as RC
import raster_ref as RF
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import CarverOption

pytestmark = pytest.mark.gpu

F = np.float32
DIMS = (24, 20, 17)
BOX = (24.4, 20.2, 17.3)
WIDE = (None, 0, 1, 1 << 30)   # "rasterwide": the default, every face by its wave, all but one-pixel boxes, every face by its lane
DEFAULT_WIDE = 64
NAMES = list(RC.cases())

_memo = {}


def option():
    h = [e / 2.0 for e in BOX]
    return CarverOption(bb_min=[-x for x in h], bb_max=h, resolution=1.0)


def make_dev(z_range=None):
    dev = vc.VoxelCarver(option(), z_range=z_range)
    assert dev.Init(), vc.last_error()
    assert dev.dims == DIMS and dev.get_param("rasterwide") == DEFAULT_WIDE
    return dev


@pytest.fixture(scope="module")
def dev():
    return make_dev()


def set_wide(dev, wide):
    dev.set_param("rasterwide", DEFAULT_WIDE if wide is None else wide)


def host(v, f, views):
    return vc.raster_mesh_host(v, f, views)


def assert_same(got, want, ctx):
    assert len(got) == len(want), ctx
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["depth"].view(np.uint32), w["depth"].view(np.uint32)), (ctx, i, "depth")
        assert np.array_equal(g["face"], w["face"]), (ctx, i, "face")
        assert np.array_equal(g["hits"], w["hits"]), (ctx, i, "hits")
        assert np.array_equal(g["n_dropped"], w["n_dropped"]), (ctx, i, "n_dropped")


def carved_meshes(dev):
    """The oracle's extraction from an 8-view carve of the 24 x 20 x 17 grid (a sphere of radius 5.6), raw, after SmoothMesh
    and after DecimateMesh, and the views they are drawn in: sub-pixel, pixel-sized and larger faces."""
    if "meshes" not in _memo:
        views, masks = synth.sphere_views(16, 8, 160, 120)
        orc = O.OracleGrid(option())
        for view, mask in zip(views, masks):
            orc.carve(view, O.make_sdf(mask))
        raw = orc.marching_cubes(0.0, True)
        v, f = raw["vertices"], raw["faces"]
        assert len(f) > 500
        smooth = dev.SmoothMesh(v, f, 5)
        dec = dev.DecimateMesh(smooth["vertices"], f, 3.0)
        draw = [RC.look((30.0, 21.0, -39.0), (0.5, -0.3, 0.2), 120.0),                    # a face is about a pixel
                RC.look((30.0, 21.0, -39.0), (0.5, -0.3, 0.2), 420.0),                    # closer: faces of 3 - 4 pixels, cut by the image
                RC.look((9.0, 6.0, -11.0), (0.0, 0.0, 0.0), 30.0),                        # sub-pixel faces
                RC.look((-20.0, 14.0, 17.0), (0.0, 0.0, 0.0), ortho=True),
                RC.look((30.0, 21.0, -39.0), (0.5, -0.3, 0.2), 120.0, roi=((5, 4), (40, 33))),
                RC.look((30.0, 21.0, -39.0), (0.5, -0.3, 0.2), 120.0, roi=((24, 20), (24, 20))),
                RC.look((0.0, 1.0, 2.0), (0.0, 9.0, 2.0), 20.0)]                          # from inside: vertices behind the camera
        _memo["meshes"] = ({"raw": (v, f), "smoothed": (smooth["vertices"], f), "decimated": (dec["vertices"], dec["faces"])}, draw)
    return _memo["meshes"]


@pytest.mark.parametrize("wide", WIDE)
@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host_on_the_cpu_cases(dev, name, wide):
    v, f, views = RC.cases()[name]
    set_wide(dev, wide)
    try:
        got = dev.RenderMesh(v, f, views, depth=True, face=True, hits=True)
    finally:
        set_wide(dev, None)
    assert_same(got, host(v, f, views), "%s wide %s" % (name, wide))
    assert all(g["raster_ms"] > 0.0 and g["resolve_ms"] > 0.0 for g in got)


@pytest.mark.parametrize("wide", WIDE)
@pytest.mark.parametrize("which", ["raw", "smoothed", "decimated"])
def test_device_equals_host_on_an_extracted_mesh(dev, which, wide):
    meshes, views = carved_meshes(dev)
    v, f = meshes[which]
    want = host(v, f, views)
    if which == "raw" and wide is None:
        # not vacuous, from the restatement: hits in every view, boxes without a pixel, of a few and of many pixels, and
        # faces dropped for a vertex behind the camera
        assert all((w["face"] >= 0).sum() > 20 for w in want[:5]) and (want[5]["face"] >= 0).sum() == 1
        boxes = []
        for view in views[:3]:
            s = {}
            RF.raster_view(v, f[::5], view, stats=s)
            boxes += s["boxes"]
        assert any(b == 0 for b in boxes) and any(1 <= b <= 4 for b in boxes) and any(b > 9 for b in boxes)
        assert want[6]["n_dropped"][0] > 0 and (want[6]["face"] >= 0).any()
    set_wide(dev, wide)
    try:
        got = dev.RenderMesh(v, f, views, depth=True, face=True, hits=True)
    finally:
        set_wide(dev, None)
    assert_same(got, want, "%s wide %s" % (which, wide))


@pytest.mark.parametrize("n_views", [1, 3, 65])
def test_view_counts_and_chunks(dev, n_views):
    v, f, views = RC.cases()["views_65"]
    views = views[:n_views] if n_views > 1 else views[64:]
    got = dev.RenderMesh(v, f, views, depth=True, face=True, hits=True)
    want = host(v, f, views)
    assert_same(got, want, "%d views" % n_views)
    assert all((w["face"] >= 0).any() for w in want)
    if n_views == 1:   # a single view passed as such returns its dict
        one = dev.RenderMesh(v, f, views[0], depth=True, face=True, hits=True)
        assert_same([one], want, "single view")


def test_two_calls_return_identical_images(dev):
    for name in ("mixed", "coincident", "whole_image"):
        v, f, views = RC.cases()[name]
        a = dev.RenderMesh(v, f, views, depth=True, face=True, hits=True)
        b = dev.RenderMesh(v, f, views, depth=True, face=True, hits=True)
        assert_same(a, b, name)


def test_slab_context_returns_the_same_bits_and_keeps_its_state():
    slab = make_dev(z_range=(5, 11))
    views, masks = synth.sphere_views(16, 2, 160, 120)
    for view, mask in zip(views, masks):
        assert slab.CarveSilhouette(view, mask)
    before = slab.download()
    for name in ("mixed", "box_12", "unusable"):
        v, f, vs = RC.cases()[name]
        assert_same(slab.RenderMesh(v, f, vs, depth=True, face=True, hits=True), host(v, f, vs), "slab " + name)
    after = slab.download()
    assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])


def test_null_outputs_on_the_device(dev):
    v, f, views = RC.cases()["roi_edges"]
    want = host(v, f, views)
    for keys in (("depth",), ("face",), ("hits",), ()):
        got = dev.RenderMesh(v, f, views, depth="depth" in keys, face="face" in keys, hits="hits" in keys)
        for g, w in zip(got, want):
            assert set(g) == set(keys) | {"n_dropped", "raster_ms", "resolve_ms"}
            for k in keys:
                assert np.array_equal(g[k].view(np.uint32) if k == "depth" else g[k], w[k].view(np.uint32) if k == "depth" else w[k])
            assert np.array_equal(g["n_dropped"], w["n_dropped"])
    got = dev.RenderMesh(v, np.zeros((0, 3), np.int32), views, depth=True, face=True, hits=True)   # no faces: no raster launch
    assert all(np.isinf(g["depth"]).all() and (g["face"] == -1).all() and not g["hits"].any() for g in got)
    with pytest.raises(RuntimeError) as e:
        dev.RenderMesh(v, np.array([[0, 1, 4]], np.int32), views)
    assert e.value.rc == capi.VCY_ERR_INVALID_ARG


def test_mesh_agreement_equals_the_host_count_over_the_host_hit_bits(dev):
    rng = np.random.RandomState(5)
    meshes, draw = carved_meshes(dev)
    for v, f, views in (RC.cases()["mixed"], RC.cases()["box_12"], RC.cases()["views_65"], meshes["smoothed"] + (draw,)):
        masks = [(rng.rand(w.height, w.width) < 0.5).astype(np.uint8) * (1 + (i % 3) * 100) for i, w in enumerate(views)]
        want = np.array([vc.hull_agreement_host(w, [h["hits"]], m) for w, h, m in zip(views, host(v, f, views), masks)])
        for wide in (None, 0):
            set_wide(dev, wide)
            try:
                got = dev.MeshAgreement(v, f, views, masks)
            finally:
                set_wide(dev, None)
            assert np.array_equal(got, want), wide
        assert want[:, 0].sum() > 0 and want[:, 1].sum() > 0 and want[:, 2].sum() > 0


def test_color_vertices_takes_its_occlusion_from_the_mesh(dev):
    meshes, draw = carved_meshes(dev)
    v, f = meshes["smoothed"]
    views = draw[:5]
    rng = np.random.RandomState(9)
    photos = [rng.randint(0, 256, (w.height, w.width, 3)).astype(np.uint8) for w in views]
    depth = [h["depth"] for h in vc.raster_mesh_host(v, f, views, face=False, hits=False)]
    for mode in (capi.VCY_COLOR_MEAN, capi.VCY_COLOR_BEST):
        normals = vc.mesh_normals_host(v, f)[0]
        want = vc.color_vertices_host(v, views, photos, depth, normals=normals, mode=mode, depth_tolerance=0.25)
        got = dev.ColorVertices(v, views, photos, normals=normals, mode=mode, depth_tolerance=0.25, mesh_faces=f)
        assert np.array_equal(got["rgb"].view(np.uint32), want["rgb"].view(np.uint32))
        assert np.array_equal(got["n_used"], want["n_used"]) and np.array_equal(got["best_view"], want["best_view"])
        assert 0 < (want["n_used"] > 0).sum() and (want["n_used"] < len(views)).any()   # some views see, the mesh hides
    with pytest.raises(ValueError):
        dev.ColorVertices(v, views, photos, depth=depth, mesh_faces=f)
