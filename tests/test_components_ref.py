"""The numpy reference of the component labelling (components_ref.py) on cases small enough to write the answers out,
and the host-visible part of the feature: the struct's layout and the exported, bound symbols.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import components_ref as R
from vacancy_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWEST = np.finfo(np.float32).min


def vol(dims, voxels):
    nx, ny, nz = dims
    s = np.zeros(nx * ny * nz, bool)
    for x, y, z in voxels:
        s[(z * ny + y) * nx + x] = True
    return s


def test_solid_mask_follows_marching_cubes():
    iso = 0.0125  # not a float: the comparison is made in double
    f = np.float32
    sdf = np.array([f(iso), np.nextafter(f(iso), f(-1)), -1.0, LOWEST, LOWEST, np.nan, 0.5, -0.5], np.float32)
    cnt = np.array([1, 1, 1, 0, 3, 1, 1, 0], np.int32)
    #  float32(0.0125) = 0.012500000186... is NOT below 0.0125; its predecessor is; an untouched voxel is not solid though
    #  lowest() < iso; a touched voxel holding lowest() is; a NaN is not; update_num 0 never is
    assert float(np.float32(iso)) > iso
    assert R.solid_mask(sdf, cnt, iso).tolist() == [False, True, True, False, True, False, False, False]
    assert R.solid_mask(sdf, cnt, -0.05).tolist() == [False, False, True, False, True, False, False, False]


def test_3x3x3_by_hand():
    dims = (3, 3, 3)
    # a 2 x 2 square in the plane z = 0 (ids 0, 1, 3, 4); (2,2,1) = id 17 and (2,2,2) = id 26 share a face;
    # (0,0,2) = id 18 is two steps above (0,0,0) and touches nothing
    s = vol(dims, [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (2, 2, 2), (0, 0, 2), (2, 2, 1)])
    lab = R.label_volume(s, dims)
    want = np.full(27, -1, np.int64)
    want[[0, 1, 3, 4]] = 0
    want[[17, 26]] = 17
    want[18] = 18
    assert lab.tolist() == want.tolist()
    c = R.components(lab, dims)
    assert c["label"].tolist() == [0, 17, 18]
    assert c["n_voxels"].tolist() == [4, 2, 1]
    assert c["bb_min"].tolist() == [[0, 0, 0], [2, 2, 1], [0, 0, 2]]
    assert c["bb_max"].tolist() == [[1, 1, 0], [2, 2, 2], [0, 0, 2]]


def test_3x3x3_edge_and_corner_contact_do_not_join():
    dims = (3, 3, 3)
    s = vol(dims, [(0, 0, 0), (1, 1, 0), (2, 2, 1), (1, 1, 1)])  # 0-4 edge, 4-13 face, 13-17 edge, 0-13 corner
    lab = R.label_volume(s, dims)
    assert lab[[0, 4, 13, 17]].tolist() == [0, 4, 4, 17]
    c = R.components(lab, dims)
    assert c["label"].tolist() == [4, 0, 17] and c["n_voxels"].tolist() == [2, 1, 1]  # ties: the lower label first


def test_4x4x4_by_hand():
    dims = (4, 4, 4)
    # a U: two bars along x at y = 0 and y = 2 of the plane z = 1, joined by a post at x = 3 -- the label of the upper
    # bar (first id 24) has to come down to the lower bar's first id 16 through the post
    bars = [(x, 0, 1) for x in range(4)] + [(x, 2, 1) for x in range(4)] + [(3, 1, 1)]
    # a second body: (1, 3, 2) and (1, 3, 3), ids 45 and 61 -- (1, 3, 1) and (1, 2, 2) are empty, so it touches the U
    # at the edge between (1, 2, 1) and (1, 3, 2) only
    col = [(1, 3, 2), (1, 3, 3)]
    s = vol(dims, bars + col)
    lab = R.label_volume(s, dims)
    c = R.components(lab, dims)
    assert c["label"].tolist() == [16, 45]
    assert c["n_voxels"].tolist() == [9, 2]
    assert c["bb_min"].tolist() == [[0, 0, 1], [1, 3, 2]]
    assert c["bb_max"].tolist() == [[3, 2, 1], [1, 3, 3]]
    assert set(lab[lab >= 0].tolist()) == {16, 45}
    assert int((lab == 16).sum()) == 9
    # all solid / none solid
    c = R.components(R.label_volume(np.ones(64, bool), dims), dims)
    assert c["label"].tolist() == [0] and c["n_voxels"].tolist() == [64]
    assert c["bb_min"].tolist() == [[0, 0, 0]] and c["bb_max"].tolist() == [[3, 3, 3]]
    c = R.components(R.label_volume(np.zeros(64, bool), dims), dims)
    assert len(c["label"]) == 0 and c["bb_min"].shape == (0, 3)


def test_keep_rule_and_filter():
    dims = (4, 4, 4)
    s = vol(dims, [(x, 0, 0) for x in range(4)] + [(0, 2, 0), (1, 2, 0)] + [(0, 0, 2), (1, 0, 2)] + [(3, 3, 3)])
    sdf = np.where(s, -1.0, 0.5).astype(np.float32)
    cnt = np.ones(64, np.int32)
    comps, lab = R.reference(sdf, cnt, dims, 0.0)
    assert comps["label"].tolist() == [0, 8, 32, 63] and comps["n_voxels"].tolist() == [4, 2, 2, 1]
    assert R.kept(comps, 1, 0).tolist() == [True, False, False, False]
    assert R.kept(comps, 0, 2).tolist() == [True, True, True, False]
    assert R.kept(comps, 2, 3).tolist() == [True, False, False, False]
    assert R.kept(comps, 2, 0).tolist() == [True, True, False, False]  # of the tie the lower label is "larger"
    out, gone, nc, nv = R.filter_state(sdf, lab, comps, 2, 0, 1.0)
    assert (nc, nv) == (2, 3)
    assert np.flatnonzero(gone).tolist() == [32, 33, 63]
    assert out[gone].tolist() == [1.0, 1.0, 1.0] and np.array_equal(out[~gone], sdf[~gone])


def test_random_volumes_against_flood_fill():
    """The vectorised labelling against a plain breadth-first flood fill (and scipy, where there is one)."""
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    rng = np.random.RandomState(5)
    for dims, density in (((5, 4, 3), 0.5), ((9, 10, 7), 0.31), ((13, 3, 5), 0.7)):
        nx, ny, nz = dims
        s = rng.rand(nx * ny * nz) < density
        lab = R.label_volume(s, dims)
        want = np.full(s.size, -1, np.int64)
        for v in np.flatnonzero(s):  # ascending: the seed is the component's smallest id
            if want[v] >= 0:
                continue
            want[v] = v
            todo = [int(v)]
            while todo:
                u = todo.pop()
                x, y, z = u % nx, (u // nx) % ny, u // (nx * ny)
                for ok, w in ((x > 0, u - 1), (x < nx - 1, u + 1), (y > 0, u - nx), (y < ny - 1, u + nx),
                              (z > 0, u - nx * ny), (z < nz - 1, u + nx * ny)):
                    if ok and s[w] and want[w] < 0:
                        want[w] = v
                        todo.append(w)
        assert np.array_equal(lab, want), dims
        if ndimage is not None:
            _, k = ndimage.label(s.reshape(nz, ny, nx))
            assert k == len(R.components(lab, dims)["label"])


def test_component_struct_is_40_bytes():
    assert C.sizeof(capi.Component) == 40
    assert capi.Component.label.offset == 0 and capi.Component.n_voxels.offset == 8
    assert capi.Component.bb_min.offset == 16 and capi.Component.bb_max.offset == 28


NEW_SYMBOLS = ("vcy_label_components", "vcy_components_free", "vcy_download_labels", "vcy_keep_components",
               "vcy_last_components_ms")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vacancy_hip.h")).read()
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in vacancy_hip.h"
        assert name in lib._vcy_symbols, name + " is not bound in capi.py"
        fn = getattr(lib, name)
        assert fn.argtypes is not None
    assert lib.vcy_keep_components.argtypes[4] is C.c_float
    # argument checks that need no device
    ms = C.c_float(-1.0)
    assert lib.vcy_last_components_ms(None, C.byref(ms)) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_download_labels(None, None) == capi.VCY_ERR_NOT_INITIALIZED
    n = C.c_int64(7)
    p = C.POINTER(capi.Component)()
    assert lib.vcy_label_components(None, 0.0, C.byref(p), C.byref(n)) == capi.VCY_ERR_NOT_INITIALIZED
    lib.vcy_components_free(None)
