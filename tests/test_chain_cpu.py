"""vcy_extract_iso_chain without a GPU: the symbols, the struct layouts, and the checks that need no context -- option
refusals come first, with the separate calls' codes, and a NULL context is reported behind them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vacancy_amd import capi, carver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def option(**kw):
    o = capi.ChainOption()
    o.smooth, o.smooth_option = 1, capi.SmoothOption(2, 0.5, -0.53, 0)
    o.decimate, o.decimate_option, o.regularize = 1, capi.DecimateOption(2.0, (0.0, 0.0, 0.0), capi.VCY_DECIMATE_MEAN), 1e-3
    o.which, o.maps = capi.VCY_NORMALS_VERTEX | capi.VCY_NORMALS_FACE, 1
    for key, value in kw.items():
        target, _, field = key.rpartition("__")
        setattr(getattr(o, target) if target else o, field, value)
    return o


def call(o, mesh=True, normals=True):
    m, mn, rep = capi.Mesh(), capi.MeshNormals(), capi.ChainReport()
    return capi.load().vcy_extract_iso_chain(None, 0.0, 1, C.byref(o) if o is not None else None, C.byref(m) if mesh else None,
                                             C.byref(mn) if normals else None, C.byref(rep))


def test_symbols_exist():
    lib = capi.load()
    for name in ("vcy_extract_iso_chain", "vcy_chain_report_free", "vcy_last_chain_ms", "vcy_mesh_index_limits"):
        assert hasattr(lib, name), name


def test_struct_layouts_match_the_header():
    assert C.sizeof(capi.ChainOption) == 56 and C.sizeof(capi.ChainReport) == 40
    assert capi.ChainOption.decimate_option.offset == 24 and capi.ChainOption.maps.offset == 52
    assert capi.ChainReport.vertex_map.offset == 24
    header = open(os.path.join(ROOT, "include", "vacancy_hip.h")).read()
    body = re.search(r"typedef struct vcy_chain_option \{(.*?)\} vcy_chain_option;\s*/\* 56 bytes \*/", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [name for name, _ in capi.ChainOption._fields_]
    body = re.search(r"typedef struct vcy_chain_report \{(.*?)\} vcy_chain_report;\s*/\* 40 bytes", header, re.S).group(1)
    assert re.findall(r"(\w+)[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [name for name, _ in capi.ChainReport._fields_]


def test_null_context_is_reported_behind_the_argument_checks():
    assert call(option()) == capi.VCY_ERR_NOT_INITIALIZED
    assert call(option(smooth=0, decimate=0, which=0), normals=False) == capi.VCY_ERR_NOT_INITIALIZED
    assert call(None) == capi.VCY_ERR_INVALID_ARG
    assert call(option(), mesh=False) == capi.VCY_ERR_INVALID_ARG
    assert call(option(), normals=False) == capi.VCY_ERR_INVALID_ARG
    assert capi.load().vcy_last_chain_ms(None, *([None] * 8)) == capi.VCY_ERR_INVALID_ARG
    capi.load().vcy_chain_report_free(None)
    rep = capi.ChainReport()
    capi.load().vcy_chain_report_free(C.byref(rep))


BAD = {
    "smooth 2": dict(smooth=2), "decimate 3": dict(decimate=3), "decimate -1": dict(decimate=-1), "which 4": dict(which=4),
    "maps 2": dict(maps=2),
    "iterations -1": dict(smooth_option__iterations=-1), "iterations 10001": dict(smooth_option__iterations=10001),
    "lambda nan": dict(smooth_option__lam=float("nan")), "mu -inf": dict(smooth_option__mu=float("-inf")),
    "pin 2": dict(smooth_option__pin_boundary=2),
    "cell 0": dict(decimate_option__cell=0.0), "cell nan": dict(decimate_option__cell=float("nan")),
    "mode 3": dict(decimate_option__mode=3), "mode -1": dict(decimate_option__mode=-1),
    "quadric from NEAREST": dict(decimate=2, decimate_option__mode=capi.VCY_DECIMATE_NEAREST),
    "regularize nan": dict(decimate=2, regularize=float("nan")), "regularize 2": dict(decimate=2, regularize=2.0),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_option_refusals_need_no_context(name):
    assert call(option(**BAD[name])) == capi.VCY_ERR_INVALID_ARG
    assert capi.load().vcy_last_error()


def test_a_stage_that_is_off_is_not_checked():
    assert call(option(smooth=0, smooth_option__iterations=-1)) == capi.VCY_ERR_NOT_INITIALIZED
    assert call(option(decimate=0, decimate_option__cell=0.0)) == capi.VCY_ERR_NOT_INITIALIZED
    assert call(option(decimate=1, regularize=float("nan"))) == capi.VCY_ERR_NOT_INITIALIZED


def test_mesh_size_refusal_is_the_separate_calls_at_the_same_sizes():
    """The chain applies vcy_mesh_index_limits to the mesh it has extracted; it is the bound of the separate calls' own
    checks: 3 * n_faces + 2 and n_vertices must fit 31 bits."""
    lib = capi.load()
    max_faces, max_vertices = (2 ** 31 - 3) // 3, 2 ** 31 - 1
    assert 3 * (max_faces - 1) + 2 <= max_vertices < 3 * (max_faces + 1) + 2   # (the last corner id 3 f + 2 that fits an int)
    for nv, nf, rc in ((0, 0, 0), (max_vertices, max_faces, 0), (1, max_faces + 1, capi.VCY_ERR_UNSUPPORTED),
                       (max_vertices + 1, 1, capi.VCY_ERR_UNSUPPORTED), (2 ** 32, 2 ** 32 - 1, capi.VCY_ERR_UNSUPPORTED),
                       (-1, 0, capi.VCY_ERR_INVALID_ARG), (0, -1, capi.VCY_ERR_INVALID_ARG)):
        assert lib.vcy_mesh_index_limits(nv, nf) == rc, (nv, nf)
    # the separate calls at the edge: refused before an array is read (the arrays here hold one face)
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    keep, args, out = carver._smooth_args(v, f, 1, 0.5, -0.53, 0, False)
    for nv, nf in ((3, max_faces + 1), (max_vertices + 1, 1)):
        a = (nv, nf) + tuple(args[2:])
        assert lib.vcy_smooth_mesh_host(*a) == lib.vcy_mesh_index_limits(nv, nf) == capi.VCY_ERR_UNSUPPORTED
        msg = lib.vcy_last_error().decode()
        assert "32 bits wide" in msg and str(nf) in msg
    keep, args, out = carver._decimate_args(v, f, 1.0, (0.0, 0.0, 0.0), 0, False)
    for nv, nf in ((3, max_faces + 1), (max_vertices + 1, 1)):
        a = (nv, nf) + tuple(args[2:])
        assert lib.vcy_decimate_mesh_host(*a) == capi.VCY_ERR_UNSUPPORTED
        assert "32 bits wide" in lib.vcy_last_error().decode()
