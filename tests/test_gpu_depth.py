"""The depth carve on the device (vcy_carve_depth_device / vcy_carve_depth, carve_depth.hip) against the numpy restatement of
its definition (tests/depth_ref.py) and against the serial host function: sdf bits and update_num are compared for
equality.  Then what does not go through the restatement alone: splitting and order among silhouette carves, queued views,
the state's bookkeeping, z-slabs, a concavity no silhouette sees, the round trip of the bunny's rendered depth, the
refusals and the example.  (A NaN only has to be a NaN: robust_ref.assert_sdf_equal says why.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import components_ref as CR
import depth_cases as DC
import depth_ref as DR
import oracle_lib as O
import render_ref as RR
import robust_cases as RC
import robust_ref as R
import test_gpu_render as TR
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.sharded import ShardedVoxelCarver

pytestmark = pytest.mark.gpu

F = np.float32
LOWEST = np.finfo(np.float32).min
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")
ids3 = lambda d: "%dx%dx%d" % d  # noqa: E731


def make_dev(opt, dims=None, z_range=None):
    dev = vc.VoxelCarver(opt, z_range=z_range)
    assert dev.Init(), vc.last_error()
    if dims is not None:
        assert dev.dims == tuple(dims), (dev.dims, dims)
    return dev


def assert_state(dev, want, ctx):
    ds, du = dev.download()
    assert np.array_equal(du, want[1]), "%s: %d update_num differ" % (ctx, int((du != want[1]).sum()))
    R.assert_sdf_equal(ds, want[0], ctx)


def carve_base(dev, dims):
    """The two silhouette views of depth_cases.base_state, on the device."""
    views, sdfs = RC.scene(dims, "mixed", 2)
    ptrs = [dev.upload_sdf(s) for s in sdfs]
    assert dev.CarveBatchDevice(views, ptrs), vc.last_error()
    dev.sync()
    for p in ptrs:
        dev.free_device(p)


# ---- 1. equality with the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(DC.MODES))
@pytest.mark.parametrize("dims", DC.DIMS, ids=ids3)
def test_equals_restatement(dims, mode):
    opt = DC.option_for(dims, mode)
    for call in DC.CALLS:
        views, depths = DC.scene(dims, *call)
        band = call[2]
        for on_base in (False, True):
            want = DC.want(dims, mode, call, on_base)
            dev = make_dev(opt, dims)
            if on_base:
                carve_base(dev, dims)
            ptrs = [dev.upload_sdf(d) for d in depths]
            got = dev.CarveDepthDevice(views, ptrs, band)
            assert got["device_ms"] > 0.0
            assert_state(dev, want, (dims, mode, call, on_base, "device images"))
            for p in ptrs:
                dev.free_device(p)
            other = make_dev(opt, dims)
            if on_base:
                carve_base(other, dims)
            assert other.CarveDepth(views, depths, band)["device_ms"] > 0.0
            assert_state(other, want, (dims, mode, call, on_base, "host images"))


# ---- 2. the device against the host function --------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(DC.MODES))
@pytest.mark.parametrize("dims", [(257, 3, 2), (65, 9, 17)], ids=ids3)
def test_equals_host_function(dims, mode):
    opt = DC.option_for(dims, mode)
    for call in DC.CALLS:
        views, depths = DC.scene(dims, *call)
        s, u = DC.base_state(dims, mode)
        vc.carve_depth_host(opt, views, depths, call[2], s, u)
        dev = make_dev(opt, dims)
        carve_base(dev, dims)
        dev.CarveDepth(views, depths, call[2])
        assert_state(dev, (s, u), (dims, mode, call))


# ---- 3. counter widths ---------------------------------------------------------------------------------------------------

def test_counters_pass_255():
    """Constant images and a band wider than the scene, so that every view that sees a voxel contributes, in
    weighted-average mode, where every contribution counts.  The views cycle through the pinhole set, of which
    pinhole_away sees nothing and roi_one_pixel next to nothing: 260 views give a voxel at most 3 x 52 + 52 = 208 samples,
    short of the premise.  520 views are used, so that the counts do pass 255; the premise is asserted."""
    dims, n = (24, 20, 17), 520
    opt = DC.option_for(dims, "average_w07")
    opt.update_option.voxel_max_update_num = 1000
    table = TR.views_for(dims)
    names = DC.VIEW_SETS["pinhole"]
    views = [table[names[i % len(names)]] for i in range(n)]
    depths = [np.full((DC.H, DC.W), 30.0 + 0.1 * i, F) for i in range(n)]
    band = 200.0
    want = DR.carve_depth(opt, views, depths, band)
    assert want[1].max() > 255
    dev = make_dev(opt, dims)
    assert dev.get_param("count_bytes") == 1
    dev.CarveDepth(views, depths, band)
    assert dev.get_param("count_bytes") == 2
    assert_state(dev, want, "u16")


def test_four_byte_counters():
    dims, call = (65, 9, 17), DC.CALLS[3]
    opt = DC.option_for(dims, "average_w1")
    opt.update_option.voxel_max_update_num = 70000
    views, depths = DC.scene(dims, *call)
    dev = make_dev(opt, dims)
    dev.set_param("lazycount", 0)
    assert dev.get_param("count_bytes") == 4
    dev.CarveDepth(views, depths, call[2])
    assert dev.get_param("count_bytes") == 4
    assert_state(dev, DR.carve_depth(opt, views, depths, call[2]), "u32")


# ---- 4. splitting and order ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["max", "average_w07"])
def test_splitting_a_call_changes_nothing(mode):
    dims, call = (65, 9, 17), DC.CALLS[3]
    opt = DC.option_for(dims, mode)
    views, depths = DC.scene(dims, *call)
    want = DC.want(dims, mode, call, False)
    for cut in (64, 35):
        dev = make_dev(opt, dims)
        dev.CarveDepth(views[:cut], depths[:cut], call[2])
        dev.CarveDepth(views[cut:], depths[cut:], call[2])
        assert_state(dev, want, (mode, cut))


@pytest.mark.parametrize("fused", [1, 0])
def test_interleaved_with_silhouette_views(fused):
    dims, call = (24, 20, 17), DC.CALLS[1]
    opt = DC.option_for(dims, "max")
    sviews, sdfs = RC.scene(dims, "pinhole", 4)
    dviews, depths = DC.scene(dims, *call)
    # oracle, restatement, oracle -- in the order of the calls
    g = O.OracleGrid(opt)
    for v, s in zip(sviews[:2], sdfs[:2]):
        g.carve(v, s)
    mid = DR.carve_depth(opt, dviews, depths, call[2], *g.download())
    g.upload(*mid)
    for v, s in zip(sviews[2:], sdfs[2:]):
        g.carve(v, s)
    want = g.download()
    g.close()
    dev = make_dev(opt, dims)
    dev.set_param("fused", fused)
    sp = [dev.upload_sdf(s) for s in sdfs]
    dp = [dev.upload_sdf(d) for d in depths]
    assert dev.CarveBatchDevice(sviews[:2], sp[:2]), vc.last_error()
    dev.CarveDepthDevice(dviews, dp, call[2])
    assert dev.CarveBatchDevice(sviews[2:], sp[2:]), vc.last_error()  # (stale brick minima would show here)
    assert_state(dev, want, fused)
    assert not np.array_equal(mid[0].view(np.uint32), want[0].view(np.uint32))
    for p in sp + dp:
        dev.free_device(p)


# ---- 5. queued views ---------------------------------------------------------------------------------------------------------

def test_queued_views_are_applied_first():
    dims, call = (24, 20, 17), DC.CALLS[1]
    opt = DC.option_for(dims, "max")
    sviews, sdfs = RC.scene(dims, "pinhole", 2)
    dviews, depths = DC.scene(dims, *call)
    states = []
    for defer in (1, 0):
        dev = make_dev(opt, dims)
        dev.set_param("defer", defer)
        for v, s in zip(sviews, sdfs):
            assert dev.Carve(v, s), vc.last_error()
        dev.CarveDepth(dviews, depths, call[2])
        states.append(dev.download())
    assert np.array_equal(states[0][1], states[1][1])
    R.assert_sdf_equal(states[0][0], states[1][0], "defer")
    g = O.OracleGrid(opt)
    for v, s in zip(sviews, sdfs):
        g.carve(v, s)
    want = DR.carve_depth(opt, dviews, depths, call[2], *g.download())
    g.close()
    assert np.array_equal(states[0][1], want[1])
    R.assert_sdf_equal(states[0][0], want[0], "restatement")


# ---- 6. the state's bookkeeping ------------------------------------------------------------------------------------------------

def test_later_calls_see_the_state_as_after_an_upload():
    c = DC.concavity_scene()  # (a state with a surface: a mesh, a hull to render, components)
    opt = c["opt"]("max")
    a, b = make_dev(opt), make_dev(opt)
    # a context that has extracted, rendered and labelled before: everything it kept must be rebuilt
    a.CarveDepth(c["views"][:1], c["depths"][:1], 3.0)
    a.ExtractIsoSurface(0.0)
    a.RenderHull(c["views"][:1], 0.0)
    a.LabelComponents(0.0)
    a.CarveDepth(c["views"][1:], c["depths"][1:], 3.0)
    sdf, cnt = a.download()
    b.upload(sdf, cnt)
    ma, mb = a.ExtractIsoSurface(0.0), b.ExtractIsoSurface(0.0)
    assert len(ma["faces"]) > 0 and np.array_equal(ma["faces"], mb["faces"]) and np.array_equal(ma["keys"], mb["keys"])
    assert np.array_equal(ma["vertices"].view(np.uint32), mb["vertices"].view(np.uint32))
    planes, solid = RR.option_planes(opt), RR.solid_mask(sdf, cnt, 0.0)
    for v in (c["views"][0], c["views"][5]):
        got = a.RenderHull(v, 0.0, voxel_ids=True, axes=True)
        TR.assert_images_equal(got, RR.render(v, planes, a.dims, solid), "render")
        assert np.isfinite(got["depth"]).any()
    got = a.LabelComponents(0.0, labels=True)
    want, lab = CR.reference(sdf, cnt, a.dims, 0.0)
    CR.assert_components_equal(got, want, "components")
    assert np.array_equal(got["labels"], lab) and len(want["label"]) > 0


# ---- 7. z-slabs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 8, 9])
def test_z_slabs_concatenate_to_the_whole_grid(k):
    dims, mode, call = (65, 9, 17), "average_w07", DC.CALLS[3]
    opt = DC.option_for(dims, mode)
    views, depths = DC.scene(dims, *call)
    want = DC.want(dims, mode, call, False)
    nxy = dims[0] * dims[1]
    for z0, z1 in ((0, k), (k, dims[2])):
        if z0 == 1:  # (no context can own [1, nz): a slab above the first starts at z >= 2 for its halo; the host
            refused = vc.VoxelCarver(opt, z_range=(z0, z1))  # function's test covers that cut)
            assert not refused.Init() and "z >= 2" in vc.last_error()
            continue
        slab = make_dev(opt, dims, z_range=(z0, z1))
        slab.CarveDepth(views, depths, call[2])
        assert_state(slab, (want[0][z0 * nxy:z1 * nxy], want[1][z0 * nxy:z1 * nxy]), (k, z0, z1))


@pytest.mark.parametrize("n_slabs", [2, 3])
def test_sharded_carver_equals_one_context(n_slabs):
    dims, mode, call = (24, 20, 17), "max", DC.CALLS[1]
    opt = DC.option_for(dims, mode)
    views, depths = DC.scene(dims, *call)
    sh = ShardedVoxelCarver(opt, [0], slabs_per_device=n_slabs)
    assert sh.Init(), vc.last_error()
    assert sh.CarveDepth(views, depths, call[2])["device_ms"] > 0.0
    parts = [c.download() for c in sh.slabs]
    want = DC.want(dims, mode, call, False)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want[1])
    R.assert_sdf_equal(np.concatenate([p[0] for p in parts]), want[0], n_slabs)
    sh.close()


# ---- 8. a concavity no silhouette sees -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["max", "average_w1"])
def test_depth_carves_the_dent(mode):
    c = DC.concavity_scene()
    opt = c["opt"](mode)
    want = DR.carve_depth(opt, c["views"], c["depths"], 3.0)
    DC.assert_concavity(want[0], want[1], touched_only=mode != "max")  # the claim, on the restatement first
    dev = make_dev(opt)
    dev.CarveDepth(c["views"], c["depths"], 3.0)
    sdf, cnt = dev.download()
    DC.assert_concavity(sdf, cnt, touched_only=mode != "max")
    assert_state(dev, want, mode)


# ---- 9. round trip on the bunny -------------------------------------------------------------------------------------------------

def test_bunny_round_trip():
    res = 10.0
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    hull = make_dev(B.bunny_option(res))
    assert hull.CarveBatchSilhouettes(views, B.load_masks()), vc.last_error()
    hs, hu = hull.download()
    depths = [r["depth"] for r in hull.RenderHull(views, 0.0)]
    assert all(np.isfinite(d).any() for d in depths)
    opt = B.bunny_option(res)
    want = DR.carve_depth(opt, views, depths, 3.0 * res)
    dev = make_dev(opt)
    dev.CarveDepth(views, depths, 3.0 * res)
    assert_state(dev, want, "bunny")
    # The clause "no voxel the hull carved (sdf > 0) is left solid with update_num >= 1 and sdf < -0.5" is not asserted: the
    # restatement itself breaks it on 8 of the 91 729 carved voxels (voxels at the hull's rim whose nearest pixel holds the
    # depth of a surface in front of them), so it is no property of the definition.
    assert (hs > 0).sum() > 1000 and (want[1] >= 1).sum() > 1000


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_state_untouched():
    dims, call = (24, 20, 17), DC.CALLS[1]
    opt = DC.option_for(dims, "max")
    views, depths = DC.scene(dims, *call)
    dev, twin = make_dev(opt, dims), make_dev(opt, dims)
    carve_base(dev, dims)
    carve_base(twin, dims)
    dptr = [dev.upload_sdf(d).value for d in depths]
    hptr = [d.ctypes.data for d in depths]
    bad_roi = capi.View.from_buffer_copy(views[1])
    bad_roi.roi_max[0] = DC.W
    denormal = float(np.float32(1e-40))
    for entry, pp in (("vcy_carve_depth_device", dptr), ("vcy_carve_depth", hptr)):
        cases = [("band 0", views, pp, 0.0, "band"), ("band negative", views, pp, -2.0, "band"),
                 ("band NaN", views, pp, float("nan"), "band"), ("band inf", views, pp, float("inf"), "band"),
                 ("band denormal", views, pp, denormal, "band"), ("no views", [], [], 2.0, "views"),
                 ("null image in the middle", views, pp[:2] + [None] + pp[3:], 2.0, "null image of view 2"),
                 ("ROI outside the image", [views[0], bad_roi] + views[2:], pp, 2.0, "ROI")]
        for name, vs, ps, band, text in cases:
            arr = (capi.View * max(len(vs), 1))(*vs)
            ptrs = (C.c_void_p * max(len(ps), 1))(*ps)
            assert getattr(dev._lib, entry)(dev.ctx, len(vs), arr, ptrs, band) == capi.VCY_ERR_INVALID_ARG, (entry, name)
            assert text in vc.last_error(), (entry, name, vc.last_error())
            assert dev.state_diff(twin) == 0, (entry, name)
    with pytest.raises(RuntimeError, match="band"):
        dev.CarveDepth(views, depths, 0.0)
    assert dev.state_diff(twin) == 0
    ms = C.c_float(-1.0)
    assert dev._lib.vcy_last_depth_ms(None, C.byref(ms)) == capi.VCY_ERR_INVALID_ARG and ms.value == -1.0
    dev.CarveDepthDevice(views, dptr, call[2])
    assert dev.state_diff(twin) > 0
    assert_state(dev, DC.want(dims, "max", call, True), "after the refusals")
    for p in dptr:
        dev.free_device(p)


# ---- 11. the example -------------------------------------------------------------------------------------------------------------

def read_ply_counts(path):
    """(vertices, faces) of a PLY header."""
    counts = {}
    with open(path, "rb") as f:
        for line in f:
            words = line.decode("ascii", "replace").split()
            if words[:1] == ["element"]:
                counts[words[1]] = int(words[2])
            if words[:1] == ["end_header"]:
                break
    return counts.get("vertex", 0), counts.get("face", 0)


def test_bunny_example_fuses_the_rendered_depth(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "--fuse-depth"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = [l.split() for l in run.stdout.splitlines() if l.startswith("DEPTH fused")]
    assert len(rows) == 1, run.stdout
    # DEPTH fused verts <n> faces <m> device_ms <x>
    r = rows[0]
    assert [r[2], r[4], r[6]] == ["verts", "faces", "device_ms"] and float(r[7]) > 0.0, r
    nv, nf = read_ply_counts(str(tmp_path / "depth_fused.ply"))
    assert nf >= 1 and (nv, nf) == (int(r[3]), int(r[5]))
