"""The carve kernels and the extractions at the edges of the float range: the scenes of tests/float_class_scenes.py --
denormals, signed zeros, values near FLT_MAX, an average that overflows, +-inf, 0 * inf, NaN, and max_sdf resolved from an
image whose first pixel is a NaN, a zero of either sign or one of tied maxima -- through every carve path, against the CPU
oracle.  update_num equal, NaN voxels NaN on both sides, every other word equal as bits (test_gpu_parity.
assert_state_equal_nan); no tolerance anywhere.  The state is compared after each of the four batches, and the final state
goes through ExtractIsoSurface (iso 0 and the denormal 1e-40) and ExtractVoxel.  test_float_class_scenes_cpu.py shows from
the oracle alone what these scenes reach and which defects they would expose."""
import numpy as np
import pytest

import depth_ref as DR
import float_class_scenes as S
import oracle_lib as O
import robust_ref as R
from test_gpu_parity import assert_state_equal_nan
from vacancy_amd import carver as vc

pytestmark = pytest.mark.gpu

F = np.float32
ISOS = (0.0, 1e-40)
ids3 = lambda d: "%dx%dx%d" % d  # noqa: E731


def make_dev(dims, option, params=(), z_range=None):
    dev = vc.VoxelCarver(S.option_for(dims, option), z_range=z_range)
    assert dev.Init(), vc.last_error()
    assert dev.dims == tuple(dims), (dev.dims, dims)
    for k, v in params:
        dev.set_param(k, v)
    return dev


def assert_mesh_equal_nan(dm, om, ctx):
    """test_gpu_parity.assert_mesh_equal, but a NaN coordinate only has to be a NaN (a vertex between non-finite values)."""
    assert dm["vertices"].shape == om["vertices"].shape, (ctx, dm["vertices"].shape, om["vertices"].shape)
    assert dm["faces"].shape == om["faces"].shape, (ctx, dm["faces"].shape, om["faces"].shape)
    if "keys" in om:
        assert np.array_equal(dm["keys"], om["keys"]), (ctx, "edge keys / vertex order differ")
    assert np.array_equal(dm["faces"], om["faces"]), (ctx, "faces differ")
    nd, no = np.isnan(dm["vertices"]), np.isnan(om["vertices"])
    assert np.array_equal(nd, no), (ctx, "NaN coordinates differ")
    bd, bo = np.where(nd, 0, dm["vertices"].view(np.uint32)), np.where(no, 0, om["vertices"].view(np.uint32))
    assert np.array_equal(bd, bo), (ctx, "%d vertex words differ" % int((bd != bo).sum()))


_meshes = {}


def oracle_meshes(key, dims, option, state):
    """The oracle's extractions of `state` (computed once per key): iso-surfaces at ISOS and the voxel mesh."""
    if key not in _meshes:
        g = O.OracleGrid(S.option_for(dims, option))
        g.upload(*state)
        _meshes[key] = ([g.marching_cubes(iso, True) for iso in ISOS], g.extract_voxel(False))
        g.close()
    return _meshes[key]


def check_extractions(dev, key, dims, option, state, ctx):
    iso_meshes, voxel_mesh = oracle_meshes(key, dims, option, state)
    for iso, want in zip(ISOS, iso_meshes):
        assert_mesh_equal_nan(dev.ExtractIsoSurface(iso, True), want, (ctx, "iso", iso))
    assert_mesh_equal_nan(dev.ExtractVoxel(False), voxel_mesh, (ctx, "voxels"))


class Images:
    """The images of a set resident on a context's device."""

    def __init__(self, dev, images):
        self.dev, self.ptrs = dev, [dev.upload_sdf(im) for im in images]

    def free(self):
        for p in self.ptrs:
            self.dev.free_device(p)


def carve_batch(dev, views, ptrs, idx):
    assert dev.CarveBatchDevice([views[i] for i in idx], [ptrs[i] for i in idx]), vc.last_error()


# name -> (knobs, how the views of a batch are applied)
PATHS = {
    "perview": ((("fused", 0),), "batch"),
    "fused_cull1": ((("cull", 1),), "batch"),
    "fused_cull0": ((("cull", 0),), "batch"),
    "oneview": ((("oneview", 1),), "single"),
    "rowkernel": ((("rowkernel", -1),), "batch"),
    "tile1": ((("tile", 1),), "batch"),
    "tile2": ((("tile", 2),), "batch"),
    "prologue1": ((("prologue", 1),), "batch"),
    "recordcache": ((("recordcache", 1),), "twice"),
    "host_queue": ((), "host"),
}
# the row flavour needs rows of whole bricks: on the 24-wide grid "rowkernel" -1 selects the general flavour after all
CASES = [(d, p) for d in S.GRIDS for p in PATHS if p != "rowkernel" or d[0] % 8 == 0]


@pytest.mark.parametrize("set_name", S.SETS)
@pytest.mark.parametrize("dims,path", CASES, ids=lambda v: ids3(v) if isinstance(v, tuple) else v)
def test_every_path_equals_the_oracle(dims, path, set_name):
    knobs, how = PATHS[path]
    views, images = S.views(dims), S.image_set(set_name)
    for option in S.OPTIONS:
        want = S.oracle_states(dims, option, set_name)
        dev = make_dev(dims, option, knobs)
        imgs = Images(dev, images) if how != "host" else None
        for b, (name, idx) in enumerate(S.BATCHES.items()):
            ctx = (ids3(dims), path, set_name, option, name)
            if how == "batch":
                carve_batch(dev, views, imgs.ptrs, idx)
            elif how == "single":  # one launch per view: the instance compiled for one view
                for i in idx:
                    carve_batch(dev, views, imgs.ptrs, (i,))
            elif how == "host":    # host images are queued; the download flushes the queue as one batch
                for i in idx:
                    assert dev.Carve(views[i], images[i]), vc.last_error()
            elif how == "twice" and b == 0:
                # the first batch (raw tiles, the general flavour), a reset, and the same batch again: a kMax launch
                # finds its records kept and bounds its footprints in the kernel
                carve_batch(dev, views, imgs.ptrs, idx)
                assert_state_equal_nan(dev.download(), want[b], ctx + ("first call",))
                hits = dev.get_param("recordcache_hits")
                dev.reset()
                carve_batch(dev, views, imgs.ptrs, idx)
                if option in S.KMAX_OPTIONS:
                    assert dev.get_param("recordcache_hits") == hits + 1, ctx
            else:
                carve_batch(dev, views, imgs.ptrs, idx)
            assert_state_equal_nan(dev.download(), want[b], ctx)
        check_extractions(dev, (dims, option, set_name), dims, option, want[-1], (ids3(dims), path, set_name, option))
        if imgs:
            imgs.free()
        dev.close()


@pytest.mark.parametrize("set_name", S.SETS)
@pytest.mark.parametrize("cut", ["on_a_brick_layer", "inside_a_brick_layer"])
@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_two_z_slabs_concatenate_to_the_oracle(dims, cut, set_name):
    z = 8 if cut == "on_a_brick_layer" else 5
    views, images = S.views(dims), S.image_set(set_name)
    for option in S.OPTIONS:
        want = S.oracle_states(dims, option, set_name)
        slabs = [make_dev(dims, option, z_range=zr) for zr in ((0, z), (z, dims[2]))]
        imgs = [Images(dev, images) for dev in slabs]
        for b, (name, idx) in enumerate(S.BATCHES.items()):
            parts = []
            for dev, im in zip(slabs, imgs):
                carve_batch(dev, views, im.ptrs, idx)
                parts.append(dev.download())
            got = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
            assert_state_equal_nan(got, want[b], (ids3(dims), cut, set_name, option, name))
        for dev, im in zip(slabs, imgs):
            im.free()
            dev.close()


@pytest.mark.parametrize("set_name", S.SETS)
@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_carve_on_an_uploaded_special_state(dims, set_name):
    """Every value class straight into sdf under counts 0 .. 3, then a fused batch and a per-view batch on top.  The
    context has carved the fused batch's cameras before: after the upload the brick minima are off and update_num is no
    longer implied by sdf, and a kMax launch reuses its kept records over a state that is not fresh."""
    views, images = S.views(dims), S.image_set(set_name)
    state = S.special_state(dims)
    fused_idx, perview_idx = (S.BATCHES[b] for b in S.UPLOAD_FOLLOW)
    for option in S.OPTIONS:
        ctx = (ids3(dims), set_name, option)
        dev = make_dev(dims, option)
        imgs = Images(dev, images)
        carve_batch(dev, views, imgs.ptrs, fused_idx)
        dev.upload(*state)
        assert_state_equal_nan(dev.download(), state, ctx + ("upload",))
        carve_batch(dev, views, imgs.ptrs, fused_idx)
        mid = S.oracle_carve(dims, option, images, fused_idx, state=state)
        assert_state_equal_nan(dev.download(), mid, ctx + ("fused batch",))
        dev.set_param("fused", 0)
        carve_batch(dev, views, imgs.ptrs, perview_idx)
        end = S.oracle_carve(dims, option, images, perview_idx, state=mid)
        assert_state_equal_nan(dev.download(), end, ctx + ("per-view batch",))
        check_extractions(dev, (dims, option, set_name, "uploaded"), dims, option, end, ctx)
        imgs.free()
        dev.close()


def test_extractions_of_the_special_state_itself():
    for dims in S.GRIDS:
        state = S.special_state(dims)
        dev = make_dev(dims, "kmax")
        dev.upload(*state)
        check_extractions(dev, (dims, "special"), dims, "kmax", state, (ids3(dims), "special state"))
        dev.close()


# ---- the robust carve ----------------------------------------------------------------------------------------------------

ROBUST_OPTIONS = ["kmax", "kmax_trunc", "kmax_outside", "kmax_trunc_nn"]  # (an order statistic needs kMax)


@pytest.mark.parametrize("set_name", S.SETS)
@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_robust_carve_equals_the_restatement(dims, set_name):
    views, images = list(S.views(dims)), list(S.image_set(set_name))
    for option in ROBUST_OPTIONS:
        has, val = R.samples(S.option_for(dims, option), views, images)
        dev = make_dev(dims, option)
        imgs = Images(dev, images)
        for m in (0, 1):
            got = dev.CarveRobustDevice(views, imgs.ptrs, m, 0.0)
            sdf, cnt, over = R.robust_from_samples(has, val, m, 0.0)
            ctx = (ids3(dims), set_name, option, m)
            assert_state_equal_nan(dev.download(), (sdf, cnt), ctx)
            assert np.array_equal(got["overruled"], over), (ctx, got["overruled"], over)
        imgs.free()
        dev.close()


# ---- the depth carve -----------------------------------------------------------------------------------------------------

DEPTH_OPTIONS = ["kmax", "wa_w1", "wa_w05_outside", "kmax_gate2"]


@pytest.mark.parametrize("band", [2.0, 200.0])
@pytest.mark.parametrize("dims", S.GRIDS, ids=ids3)
def test_depth_carve_equals_the_restatement(dims, band):
    views = list(S.views(dims))
    depths = [S.depth_image(v, i) for i, v in enumerate(views)]
    for option in DEPTH_OPTIONS:
        opt = S.option_for(dims, option)
        want = DR.carve_depth(opt, views, depths, band)
        ctx = (ids3(dims), band, option)
        dev = make_dev(dims, option)
        imgs = Images(dev, depths)
        dev.CarveDepthDevice(views, imgs.ptrs, band)
        assert_state_equal_nan(dev.download(), want, ctx + ("device images",))
        imgs.free()
        dev.close()
        sdf, cnt = np.full(len(want[0]), S.LOWEST, F), np.zeros(len(want[0]), np.int32)
        vc.carve_depth_host(opt, views, depths, band, sdf, cnt)
        assert_state_equal_nan((sdf, cnt), want, ctx + ("host function",))
