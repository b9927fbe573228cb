"""The shading pass on the device (vcy_shade_mesh / vcy_mesh_photo_error, raster_shade.hip) against the serial host
functions (vcy_shade_mesh_host / vcy_mesh_photo_error_host, which tests/test_shade_cpu.py holds against the numpy
restatement): float BITS of value and bary, bytes of value8 and the seven sums are compared for equality, for one to four
channels, with each output alone and all together, from a z-slab context, on both sides of the wide-face threshold; the
rasteriser's own calls, the voxel state and queued views must not notice the pass."""
import numpy as np
import pytest

import raster_cases as RC
import shade_cases as SC
import shade_ref as SF
from hashing import fnv1a64
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import CarverOption

pytestmark = pytest.mark.gpu

F = np.float32
BOX = (24.4, 20.2, 17.3)
DEFAULT_WIDE = 64
NAMES = list(SC.cases())
PHOTO = list(SC.photo_cases())

_host = {}


def option():
    h = [e / 2.0 for e in BOX]
    return CarverOption(bb_min=[-x for x in h], bb_max=h, resolution=1.0)


def make_dev(z_range=None):
    dev = vc.VoxelCarver(option(), z_range=z_range)
    assert dev.Init(), vc.last_error()
    return dev


@pytest.fixture(scope="module")
def dev():
    return make_dev()


def host(name):
    """The host function's answer for a case, computed once and shared."""
    if name not in _host:
        v, f, a, views, bg = SC.cases()[name]
        _host[name] = vc.shade_mesh_host(v, f, a, views, background=bg, value=True, value8=True, bary=True)
    return _host[name]


def host_error(name, masked):
    if (name, masked) not in _host:
        v, f, col, views, photos, masks = SC.photo_cases()[name]
        _host[(name, masked)] = vc.mesh_photo_error_host(v, f, col, views, photos, masks if masked else None)
    return _host[(name, masked)]


def device(dev, name, **kw):
    v, f, a, views, bg = SC.cases()[name]
    return dev.ShadeMesh(v, f, a, views, background=bg, **kw)


def assert_same(got, want, name, keys=("value", "value8", "bary")):
    same = SF.same_but_nan if name == "odd_values" else SF.same
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for k in keys:
            assert same([g], [w], (k,)), (name, i, k)


@pytest.mark.parametrize("wide", [None, 0])
@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host(dev, name, wide):
    """"rasterwide" 0 and the default: the winner does not depend on who draws a face."""
    dev.set_param("rasterwide", DEFAULT_WIDE if wide is None else wide)
    try:
        got = device(dev, name, value=True, value8=True, bary=True)
    finally:
        dev.set_param("rasterwide", DEFAULT_WIDE)
    assert_same(got, host(name), name)
    v, f, a, views, bg = SC.cases()[name]
    assert all(g["shade_ms"] > 0.0 and (g["raster_ms"] > 0.0) for g in got)
    assert all(g["value"].shape == (w.height, w.width, a.shape[1]) for g, w in zip(got, views))


@pytest.mark.parametrize("only", ["value", "value8", "bary"])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_each_output_alone(dev, ch, only):
    for name in ("sizes_c%d" % ch, "roi_c%d" % ch, "no_faces_c%d" % ch):
        got = device(dev, name, value=only == "value", value8=only == "value8", bary=only == "bary")
        assert all(set(g) == {only, "raster_ms", "shade_ms"} for g in got)
        assert_same(got, host(name), name, (only,))


def test_slab_context_returns_the_same_bits_and_keeps_its_state():
    slab = make_dev(z_range=(5, 11))
    views, masks = synth.sphere_views(16, 2, 160, 120)
    for view, mask in zip(views, masks):
        assert slab.CarveSilhouette(view, mask)
    before = [fnv1a64(x) for x in slab.download()]
    for name in ("mixed", "sizes_c3", "odd_values"):
        assert_same(device(slab, name, value=True, value8=True, bary=True), host(name), "slab " + name)
    v, f, col, vs, photos, masks = SC.photo_cases()["photo_sizes"]
    assert np.array_equal(slab.MeshPhotoError(v, f, col, vs, photos, masks), host_error("photo_sizes", True))
    assert [fnv1a64(x) for x in slab.download()] == before


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("name", PHOTO)
def test_photo_error_equals_host(dev, name, masked):
    v, f, col, views, photos, masks = SC.photo_cases()[name]
    masked = masked and masks is not None
    for wide in (DEFAULT_WIDE, 0):
        dev.set_param("rasterwide", wide)
        try:
            got = dev.MeshPhotoError(v, f, col, views, photos, masks if masked else None)
        finally:
            dev.set_param("rasterwide", DEFAULT_WIDE)
        assert got.dtype == np.int64 and got.shape == (len(views), 7)
        assert np.array_equal(got, host_error(name, masked)), (name, masked, wide)
    ms = dev.last_shade_ms()
    assert ms[0] > 0.0 and ms[1] > 0.0


def test_photo_error_largest_term(dev):
    v, f, col, views, photos, masks = SC.photo_cases()["photo_255"]
    got = dev.MeshPhotoError(v, f, col, views, photos)[0]
    n = int((SC.photo_faces("photo_255")[0] >= 0).sum())
    assert got[0] == n and got[1] == n * 255 and got[4] == n * 65025


@pytest.mark.parametrize("name", ["photo_sizes", "photo_65"])
def test_counted_pixels_are_mesh_agreements(dev, name):
    """n is MeshAgreement's `both` under the same silhouettes, and both + mesh only without."""
    v, f, col, views, photos, masks = SC.photo_cases()[name]
    agree = dev.MeshAgreement(v, f, views, masks)
    assert np.array_equal(dev.MeshPhotoError(v, f, col, views, photos, masks)[:, 0], agree[:, 0])
    assert np.array_equal(dev.MeshPhotoError(v, f, col, views, photos)[:, 0], agree[:, 0] + agree[:, 2])
    assert (agree[:, 0] > 0).any() and (agree[:, 2] > 0).any()


def raster_bits(dev, name):
    v, f, views = RC.cases()[name]
    out = dev.RenderMesh(v, f, views, depth=True, face=True, hits=True)
    return [(o["depth"].view(np.uint32).copy(), o["face"].copy(), o["hits"].copy(), o["n_dropped"].copy()) for o in out]


def test_the_rasterisers_calls_do_not_notice_the_pass(dev):
    """The pool is shared: RenderMesh and MeshAgreement before and after a ShadeMesh and a MeshPhotoError."""
    v, f, views = RC.cases()["mixed"]
    masks = [(np.random.RandomState(3 + i).rand(w.height, w.width) < 0.5).astype(np.uint8) for i, w in enumerate(views)]
    before = raster_bits(dev, "mixed"), dev.MeshAgreement(v, f, views, masks)
    ms = dev.last_raster_ms()
    device(dev, "views_65_c4", value=True, value8=True, bary=True)
    pv, pf, col, pviews, photos, pmasks = SC.photo_cases()["photo_sizes"]
    dev.MeshPhotoError(pv, pf, col, pviews, photos, pmasks)
    assert dev.last_raster_ms() == ms   # (the pass keeps times of its own)
    after = raster_bits(dev, "mixed"), dev.MeshAgreement(v, f, views, masks)
    for a, b in zip(before[0], after[0]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(before[1], after[1])
    assert_same(device(dev, "mixed", value=True, value8=True, bary=True), host("mixed"), "mixed")


@pytest.mark.parametrize("defer", [1, 0])
def test_voxel_state_and_queued_views_are_untouched(defer):
    """Two contexts carve the same three views; one shades and measures in between, with views still queued ("defer" 1)."""
    views, masks = synth.sphere_views(16, 3, 160, 120)
    v, f, col, pviews, photos, pmasks = SC.photo_cases()["photo_sizes"]
    hashes = []
    for shade in (False, True):
        d = make_dev()
        d.set_param("defer", defer)
        if shade:
            assert_same(device(d, "sizes_c2", value=True, value8=True, bary=True), host("sizes_c2"), "fresh")
            assert d.get_param("fresh") == 1   # the lazy fill has not been written for it
        for i in range(2):
            assert d.CarveSilhouette(views[i], masks[i])
        if shade:
            assert_same(device(d, "sizes_c3", value=True, value8=True, bary=True), host("sizes_c3"), "queued")
            assert np.array_equal(d.MeshPhotoError(v, f, col, pviews, photos, pmasks), host_error("photo_sizes", True))
        assert d.CarveSilhouette(views[2], masks[2])
        hashes.append([fnv1a64(x) for x in d.download()])
    assert hashes[0] == hashes[1]


def test_a_larger_then_a_smaller_mesh(dev):
    """The pool is grow-only: nothing stale of the larger call is read by the smaller one, in either flavour."""
    for big, small in (("box_192", "lattice_ortho"), ("views_65_c4", "no_faces_c1"), ("whole_image", "needles")):
        assert_same(device(dev, big, value=True, value8=True, bary=True), host(big), big)
        assert_same(device(dev, small, value=True, value8=True, bary=True), host(small), small)
    for name in ("photo_65", "photo_255", "photo_sizes"):
        v, f, col, views, photos, masks = SC.photo_cases()[name]
        assert np.array_equal(dev.MeshPhotoError(v, f, col, views, photos, masks), host_error(name, masks is not None)), name


def test_refusals_on_the_device(dev):
    v, f, a, views, bg = SC.cases()["lattice_ortho"]
    with pytest.raises(RuntimeError) as e:
        dev.ShadeMesh(v, np.array([[0, 1, 4]], np.int32), a, views)
    assert e.value.rc == vc.capi.VCY_ERR_INVALID_ARG
    with pytest.raises(RuntimeError) as e:
        dev.ShadeMesh(v, f, np.zeros((len(v), 5), F), views)
    assert e.value.rc == vc.capi.VCY_ERR_INVALID_ARG
    one = dev.ShadeMesh(v, f, a, views[0], background=bg, value8=True, bary=True)   # a single view returns its dict
    assert_same([one], host("lattice_ortho"), "single view")
