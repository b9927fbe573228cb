"""The restatement of the robust carve (tests/robust_ref.py) checked on the CPU: for m = 0 it must be the oracle's own
sequential kMax carve; hand-made sample tables pin NaN handling, n <= m and ties; and the library exports the entry points
and refuses, without a GPU, what it can refuse without one."""
import ctypes as C

import numpy as np
import pytest

import bunny_data as B
import oracle_lib as O
import robust_cases as RC
import robust_ref as R
from vacancy_amd import capi
from vacancy_amd import synth

F = np.float32
LOWEST = np.finfo(np.float32).min
NAN = np.nan


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def oracle_sequential(opt, views, sdfs):
    g = O.OracleGrid(opt)
    for v, s in zip(views, sdfs):
        g.carve(v, s)
    out = g.download()
    g.close()
    return out


def assert_m0_is_the_ordinary_carve(opt, views, sdfs, ctx):
    assert len(views) < 256  # (voxel_max_update_num = 255 then never stops a voxel)
    sdf, cnt, overruled = R.robust(opt, views, sdfs, 0)
    os_, ou = oracle_sequential(opt, views, sdfs)
    assert np.array_equal(bits(sdf), bits(os_)), (ctx, int((bits(sdf) != bits(os_)).sum()))
    assert np.array_equal(cnt > 0, ou > 0) and (cnt >= ou).all(), ctx  # (the oracle counts changes, the robust carve samples)
    assert not overruled.any(), ctx                                     # (K = 1 discards nothing)
    return cnt


def test_m0_equals_the_oracle_on_the_bunny():
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    sdfs = [O.make_sdf(m) for m in B.load_masks()]
    cnt = assert_m0_is_the_ordinary_carve(B.bunny_option(20.0), views, sdfs, "bunny")
    assert cnt.max() == 6 and cnt.min() < 6  # (views that see the voxel, not changes of its value)


@pytest.mark.parametrize("mode", list(RC.MODES))
def test_m0_equals_the_oracle_on_a_synthetic_scene(mode):
    opt = RC.option_for((24, 20, 17), mode)
    views, sdfs = RC.scene((24, 20, 17), "mixed", 16)
    cnt = assert_m0_is_the_ordinary_carve(opt, views, sdfs, mode)
    assert cnt.max() > 4


def table(rows):
    """rows[voxel] = samples in view order, None where the view gives none -> (has, val) of robust_ref."""
    nv = max(len(r) for r in rows)
    has = np.zeros((nv, len(rows)), bool)
    val = np.zeros((nv, len(rows)), F)
    for x, r in enumerate(rows):
        for i, d in enumerate(r):
            if d is not None:
                has[i, x], val[i, x] = True, d
    return has, val


def test_hand_made_tables():
    rows = [
        [NAN, 1.0, 2.0],            # 0: a NaN that came first stays first: never displaced, never passed
        [1.0, NAN, 5.0],            # 1: at K = 2 the NaN in the last place blocks d > t[K-1]: 5 is dropped
        [None, 0.25, None],         # 2: one sample
        [None, None, None],         # 3: none
        [0.5, 0.5, 0.5],            # 4: ties: the later equal sample is dropped
        [0.2, -0.3, 0.2, -0.5],     # 5
        [-0.1, -0.2, -0.3, -0.4],   # 6: all inside
        [0.0, -1.0, 0.0, -2.0],     # 7: exactly the iso level counts as outside
    ]
    has, val = table(rows)
    # K = 2
    sdf, cnt, over = R.robust_from_samples(has, val, 1, 0.0)
    assert cnt.tolist() == [3, 3, 1, 0, 3, 4, 4, 4]
    want = [2.0, NAN, 0.25, LOWEST, 0.5, 0.2, -0.2, 0.0]
    assert np.array_equal(np.isnan(sdf), np.isnan(F(want))) and np.array_equal(np.nan_to_num(sdf), np.nan_to_num(F(want)))
    assert over.tolist() == [0, 0, 0, 0]  # no voxel is solid with a discarded sample >= 0: voxel 6 discards -0.1 only
    t, ix, _ = R.top_list(has, val, 2)
    assert ix[0].tolist() == [0, 2] and ix[1].tolist() == [0, 1] and ix[4].tolist() == [0, 1] and ix[5].tolist() == [0, 2]
    assert ix[2].tolist() == [1, -1] and ix[3].tolist() == [-1, -1]
    # K = 3
    sdf, cnt, over = R.robust_from_samples(has, val, 2, 0.0)
    want = [1.0, 5.0, 0.25, LOWEST, 0.5, -0.3, -0.3, -1.0]  # (voxel 1: 5 is appended behind the NaN and stays there)
    assert np.array_equal(np.isnan(sdf), np.isnan(F(want))) and np.array_equal(np.nan_to_num(sdf), np.nan_to_num(F(want)))
    # voxel 5 keeps -0.3 over the 0.2 of views 0 and 2; voxel 7 keeps -1 over the 0.0 of views 0 and 2 (0.0 >= iso)
    assert over.tolist() == [2, 0, 2, 0]
    # ... a discarded NaN blames nobody
    sdf, cnt, over = R.robust_from_samples(has, val, 2, 1.5)
    # iso = 1.5: voxel 0 keeps 1.0 (solid) over NaN (view 0) and 2.0 (view 2); no other discarded entry is >= 1.5
    assert over.tolist() == [0, 0, 1, 0]
    # K = 4, n <= m everywhere but voxels 5 .. 7: the smallest of fewer than K samples
    sdf, cnt, over = R.robust_from_samples(has, val, 3, 0.0)
    assert sdf[2] == F(0.25) and sdf[4] == F(0.5) and sdf[5] == F(-0.5) and sdf[6] == F(-0.4) and sdf[7] == F(-2.0)
    assert sdf[0] == F(1.0) and sdf[1] == F(5.0) and sdf[3] == F(LOWEST)
    assert over.tolist() == [2, 0, 2, 0]
    # K = 1 is first touch followed by UpdateVoxelMax
    sdf, cnt, over = R.robust_from_samples(has, val, 0, 0.0)
    want = [NAN, 5.0, 0.25, LOWEST, 0.5, 0.2, -0.1, 0.0]
    assert np.array_equal(np.isnan(sdf), np.isnan(F(want))) and np.array_equal(np.nan_to_num(sdf), np.nan_to_num(F(want)))
    assert not over.any()


def test_entry_points_are_exported_and_refuse_without_a_gpu():
    lib = capi.load()
    for name in ("vcy_carve_robust_device", "vcy_carve_robust_silhouettes", "vcy_last_robust_ms"):
        assert hasattr(lib, name) and name in lib._vcy_symbols
    view = synth.sphere_views(8, 1, 16, 12)[0][0]
    arr = (capi.View * 1)(view)
    ptr = (C.c_void_p * 1)(1)  # (never read: every call below is refused first)
    over = np.full(1, -7, np.int64)
    po = over.ctypes.data_as(C.c_void_p)
    for entry in (lib.vcy_carve_robust_device, lib.vcy_carve_robust_silhouettes):
        assert entry(None, 1, arr, ptr, 4, 0.0, po) == capi.VCY_ERR_INVALID_ARG and b"tolerate" in lib.vcy_last_error()
        assert entry(None, 1, arr, ptr, -1, 0.0, po) == capi.VCY_ERR_INVALID_ARG
        assert entry(None, 0, arr, ptr, 1, 0.0, po) == capi.VCY_ERR_INVALID_ARG and b"views" in lib.vcy_last_error()
        assert entry(None, 1025, arr, ptr, 1, 0.0, po) == capi.VCY_ERR_INVALID_ARG
        assert entry(None, 1, arr, ptr, 1, 0.0, po) == capi.VCY_ERR_NOT_INITIALIZED
    assert over[0] == -7
    ms = C.c_float(-1.0)
    assert lib.vcy_last_robust_ms(None, C.byref(ms)) == capi.VCY_ERR_INVALID_ARG and ms.value == -1.0
