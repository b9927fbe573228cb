"""The paths of the extraction's host driver (mc_extract.hip) WITHOUT normals, one after the other on one context: the
exact-sizes path of a first extraction, the guessed path with the mesh written straight into host memory ("mcdirect"),
a guess that was too small (direct buffers released, the chain run again), a guess followed by an empty mesh, and the
edge keys switched off and on.  The normals tests reach the rerun too, but normals force the staged path; here the
rerun follows a direct enqueue.  Every mesh equals the oracle's marching cubes array for array."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_normals import snap_band_state
from test_gpu_parity import assert_mesh_equal
from vacancy_amd import carver as vc
from vacancy_amd import synth

pytestmark = pytest.mark.gpu

N = 24            # 24^3: seed 1 of snap_band_state already exceeds the guess with headroom (checked with the oracle)
NOISE_SEED = 1
ISO = 0.0


def ball_state(dims):
    """The small ball of test_gpu_normals.py: a smooth mesh of a few hundred vertices."""
    zz, yy, xx = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    ball = (np.sqrt((xx - 12.0) ** 2 + (yy - 12.0) ** 2 + (zz - 12.0) ** 2) - 3.0).astype(np.float32).reshape(-1)
    return ball, np.ones(ball.size, np.int32)


def assert_empty(m, ctx):
    assert len(m["vertices"]) == 0 and len(m["faces"]) == 0 and len(m["keys"]) == 0, ctx
    assert m["n_foreign"] == 0, ctx


@pytest.mark.parametrize("mcdirect", [None, 0])
def test_driver_paths_on_one_context(mcdirect):
    opt = synth.sphere_option(N)
    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    if mcdirect is not None:
        dev.set_param("mcdirect", mcdirect)
    orc = O.OracleGrid(opt)
    dims = dev.dims
    n = dims[0] * dims[1] * dims[2]

    def put(state):
        dev.upload(*state)
        orc.upload(*state)

    def check(ctx, interp=True):
        om = orc.marching_cubes(ISO, interp)
        assert_mesh_equal(dev.ExtractIsoSurface(ISO, interp), om, ctx)
        return om

    # 1. a fresh grid: no valid cell, an empty mesh without arrays
    assert_empty(dev.ExtractIsoSurface(ISO, True), "fresh grid")
    # 2. the hint is 0: the counts first, then buffers of the exact sizes
    ball = ball_state(dims)
    put(ball)
    small = check("ball, exact sizes")
    assert len(small["vertices"]) > 0
    # 3. the sizes of step 2 as the guess: one enqueue, one wait
    check("ball, guessed sizes")
    # 4. a guess that is too small: the direct buffers go back, the chain runs again with the exact sizes
    noise = snap_band_state(dims, NOISE_SEED, ISO)
    put(noise)
    big = orc.marching_cubes(ISO, True)
    assert len(big["vertices"]) > len(small["vertices"]) * 5 // 4 + 4096  # (beyond the guess and its headroom)
    check("noise after the ball: rerun")
    check("noise, guessed sizes", interp=False)
    # 5. a hint above 0 and no active cell: an empty mesh, the direct buffers released
    put((np.full(n, 1.0, np.float32), np.ones(n, np.int32)))
    assert len(orc.marching_cubes(ISO, True)["vertices"]) == 0
    assert_empty(dev.ExtractIsoSurface(ISO, True), "all outside")
    # 6. the empty mesh reset the hint: the exact path again
    put(ball)
    check("ball after the empty mesh")
    # 7. without the edge keys, then with them
    dev.set_param("meshkeys", 0)
    bare = dev.ExtractIsoSurface(ISO, True)
    assert len(bare["keys"]) == 0
    assert np.array_equal(bare["faces"], small["faces"])
    assert np.array_equal(bare["vertices"].view(np.uint32), small["vertices"].view(np.uint32))
    dev.set_param("meshkeys", 1)
    check("ball, keys back on")


def test_driver_paths_on_the_upper_of_two_slabs():
    """24 x 24 x 24 split at z = 12: the upper slab's ghost layer (has_ghost, the foreign vertices) through the exact, the
    guessed and the rerun path."""
    opt = synth.sphere_option(N)
    slabs = []
    for z_range in ((0, N // 2), (N // 2, N)):
        c = vc.VoxelCarver(opt, z_range=z_range)
        assert c.Init(), vc.last_error()
        slabs.append(c)
    upper = slabs[1]
    orc = O.OracleGrid(opt)
    dims = upper.dims
    per_slab = dims[0] * dims[1] * (N // 2)

    def put(state):
        orc.upload(*state)
        for r, c in enumerate(slabs):
            c.upload(state[0][r * per_slab:(r + 1) * per_slab], state[1][r * per_slab:(r + 1) * per_slab])
        gathered = np.concatenate([c.halo_pack_host() for c in slabs])
        for r, c in enumerate(slabs):
            c.halo_unpack_host(gathered, r, 2)

    def check(ctx):
        ref = O.marching_cubes_slab(orc, upper.z_range[0], upper.z_range[1], ISO, True)
        m = upper.ExtractIsoSurface(ISO, True)
        assert m["n_foreign"] == ref["n_foreign"], ctx
        assert_mesh_equal(m, ref, ctx)
        return ref

    put(ball_state(dims))
    small = check("upper slab, ball, exact sizes")
    assert small["n_foreign"] > 0  # (the ball is cut by the seam: the ghost layer owns vertices)
    check("upper slab, ball, guessed sizes")
    put(snap_band_state(dims, NOISE_SEED, ISO))
    big = O.marching_cubes_slab(orc, upper.z_range[0], upper.z_range[1], ISO, True)
    assert len(big["vertices"]) > len(small["vertices"]) * 5 // 4 + 4096
    assert big["n_foreign"] > 0
    check("upper slab, noise after the ball: rerun")
