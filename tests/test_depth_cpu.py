"""The depth carve's host function (vcy_carve_depth_host, the definition run serially) against the numpy restatement
(tests/depth_ref.py) -- sdf bits and update_num compared for equality --, its splitting into calls and z-slabs, a property
that does not share the restatement's arithmetic (a concavity no silhouette sees is carved), the refusals, and the
stand-alone sanitizer build.  No GPU.  (A NaN only has to be a NaN: robust_ref.assert_sdf_equal says why.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_cases as DC
import depth_ref as DR
import oracle_lib as O
import robust_ref as R
from vacancy_amd import capi
from vacancy_amd import carver as vc

F = np.float32
LOWEST = np.finfo(np.float32).min
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fill_state(opt, z_range=None):
    n = len(DR.positions(opt, z_range)[0])
    return np.full(n, LOWEST, F), np.zeros(n, np.int32)


def host(opt, views, depths, band, state=None, z_range=None):
    s, u = state if state is not None else fill_state(opt, z_range)
    s, u = np.array(s, F), np.array(u, np.int32)
    return vc.carve_depth_host(opt, views, depths, band, s, u, z_range)


def assert_state_equal(got, want, ctx):
    assert np.array_equal(got[1], want[1]), "%s: %d update_num differ" % (ctx, int((got[1] != want[1]).sum()))
    R.assert_sdf_equal(got[0], want[0], ctx)


# ---- 1. the host function equals the restatement; 2. every outcome of a sample occurs -----------------------------------

@pytest.mark.parametrize("mode", list(DC.MODES))
def test_host_equals_restatement_and_every_outcome_occurs(mode):
    total = {}
    for dims in DC.DIMS:
        opt = DC.option_for(dims, mode)
        for call in DC.CALLS:
            views, depths = DC.scene(dims, *call)
            for on_base in (False, True):
                want = DC.want(dims, mode, call, on_base)
                got = host(opt, views, depths, call[2], DC.base_state(dims, mode) if on_base else None)
                assert_state_equal(got, want, (dims, mode, call, on_base))
                for k, v in want[2].items():
                    total[k] = total.get(k, 0) + v
    for key in ("clamped", "dropped", "invalid", "between", "exactly_plus_one", "exactly_minus_one"):
        assert total.get(key, 0) > 0, (mode, key, total)
    if mode == "max_gate2":  # the gate acts: the counts stop at voxel_max_update_num + 1 and some voxel gets there
        top = max(int(DC.want(d, mode, DC.CALLS[3], True)[1].max()) for d in DC.DIMS)
        assert top == 3


# ---- 3. one call of n views is n calls of one -----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(DC.MODES))
def test_splitting_a_call_changes_nothing(mode):
    dims, call = (24, 20, 17), DC.CALLS[1]
    opt = DC.option_for(dims, mode)
    views, depths = DC.scene(dims, *call)
    band = call[2]
    want = DC.want(dims, mode, call, False)
    state = host(opt, views[:2], depths[:2], band)
    assert_state_equal(host(opt, views[2:], depths[2:], band, state), want, "2 + 3")
    state = None
    for v, d in zip(views, depths):
        state = host(opt, [v], [d], band, state)
    assert_state_equal(state, want, "5 x 1")


# ---- 4. z-slabs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 8, 9])
def test_slabs_concatenate_to_the_whole_grid(k):
    dims, mode, call = (65, 9, 17), "average_w07", DC.CALLS[3]
    opt = DC.option_for(dims, mode)
    views, depths = DC.scene(dims, *call)
    want = DC.want(dims, mode, call, False)
    lo, hi = host(opt, views, depths, call[2], z_range=(0, k)), host(opt, views, depths, call[2], z_range=(k, dims[2]))
    assert len(lo[0]) == k * dims[0] * dims[1]
    assert_state_equal((np.concatenate([lo[0], hi[0]]), np.concatenate([lo[1], hi[1]])), want, k)


# ---- 5. a concavity no silhouette sees -------------------------------------------------------------------------------------

def test_depth_carves_the_dent_a_visual_hull_keeps():
    c = DC.concavity_scene()
    opt = c["opt"]("max")
    sdf, cnt = host(opt, c["views"], c["depths"], 3.0)
    DC.assert_concavity(sdf, cnt)
    # for contrast, the silhouettes of the same six views: the dent stays filled
    prev = O.set_num_threads(1)
    try:
        g = O.OracleGrid(opt)
        for v, d in zip(c["views"], c["depths"]):
            g.carve(v, O.make_sdf(np.where(d < np.inf, 255, 0).astype(np.uint8)))
        hs, hu = g.download()
        g.close()
    finally:
        O.set_num_threads(prev)
    # The issue's claim, "the dent voxels are all still solid there", does not hold for its scene: the dent opens at the pole,
    # so the side views look through its upper part, and the hull of these six silhouettes carves 276 of the 464 dent voxels.
    # What holds, and is asserted: the dent voxels no silhouette can reach (depth_cases.concavity_scene: 100 of them) all
    # stay solid in the visual hull, and the depth carve has carved every one of them (assert_concavity above).
    hidden = c["hidden"]
    assert hidden.sum() >= 50 and (hidden <= c["dent"]).all()
    still = (hu[hidden] >= 1) & (hs[hidden] < 0)
    assert still.all(), "%d hidden dent voxels are not solid in the visual hull" % int((~still).sum())
    assert (sdf[hidden] > 0).all()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_arrays_untouched():
    dims, mode, call = (24, 20, 17), "max", DC.CALLS[1]
    opt = DC.option_for(dims, mode)
    views, depths = DC.scene(dims, *call)
    lib = capi.load()
    s0, u0 = DC.base_state(dims, mode)
    s, u = s0.copy(), u0.copy()
    n = len(views)
    arr = (capi.View * n)(*views)
    ptrs = [d.ctypes.data for d in depths]

    def call_raw(nv, pointers, band):
        pp = (C.c_void_p * n)(*pointers)
        return lib.vcy_carve_depth_host(C.byref(opt), 0, dims[2], nv, arr, pp, band, s.ctypes.data_as(C.c_void_p),
                                        u.ctypes.data_as(C.c_void_p))

    denormal = float(np.float32(1e-40))
    with np.errstate(over="ignore"):
        assert denormal > 0.0 and np.isinf(F(1.0) / F(denormal))
    for name, nv, pointers, band, text in [("band 0", n, ptrs, 0.0, "band"), ("band negative", n, ptrs, -1.0, "band"),
                                           ("band NaN", n, ptrs, float("nan"), "band"), ("band inf", n, ptrs, float("inf"), "band"),
                                           ("band denormal", n, ptrs, denormal, "band"), ("no views", 0, ptrs, 2.0, "views"),
                                           ("null image", n, ptrs[:2] + [None] + ptrs[3:], 2.0, "null image of view 2")]:
        assert call_raw(nv, pointers, band) == capi.VCY_ERR_INVALID_ARG, name
        assert text in vc.last_error(), (name, vc.last_error())
        assert np.array_equal(u, u0) and np.array_equal(s.view(np.uint32), s0.view(np.uint32)), name
    assert call_raw(n, ptrs, 2.3) == 0, vc.last_error()
    assert not np.array_equal(s.view(np.uint32), s0.view(np.uint32))


# ---- 7. the host function under AddressSanitizer and UBSan, as a program of its own ------------------------------------------

def test_host_function_is_clean_under_host_sanitizers():
    run = subprocess.run(["make", "-C", os.path.join(ROOT, "vacancy_amd", "csrc"), "-s", "depth_host_check"], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "depth_host_check: ok" in run.stdout
