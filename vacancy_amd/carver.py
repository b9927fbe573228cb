"""Python host-side mirror of vacancy::VoxelCarver over the C-ABI (include/vacancy_hip.h).

Method names and argument meaning follow the reference class
(include/vacancy/voxel_carver.h:95-118 in unclearness/vacancy); errors that the reference
reports as `return false` + LOGE surface here as `False` returns with the message in
`last_error()`.  Every call goes to libvacancy_hip.so; there is no CPU path.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import CarverOption, ColorOption, DecimateOption, Mesh, SmoothOption, UpdateOption, View, make_view  # noqa: F401


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _mesh_array(ptr, count, width, dtype):
    """Copy of `count` rows of `width` from a library-owned mesh array (NULL when the mesh is empty)."""
    if count == 0 or not ptr:
        return np.zeros((0, width), dtype)
    return np.ctypeslib.as_array(ptr, shape=(count * width,)).reshape(count, width).copy()


def last_error():
    return capi.load().vcy_last_error().decode()


def mesh_normals_host(vertices, faces):
    """vcy_mesh_normals_host: Mesh::CalcFaceNormal + Mesh::CalcNormal (reference mesh.cc:197-240) of a mesh in host
    arrays, serial, no GPU needed.  Returns (vertex normals [n_vertices, 3], face normals [n_faces, 3]), float32."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    vn = np.zeros((len(v), 3), np.float32)
    fn = np.zeros((len(f), 3), np.float32)
    rc = capi.load().vcy_mesh_normals_host(len(v), len(f), _p(v), _p(f), _p(vn), _p(fn))
    if rc != 0:
        raise RuntimeError(last_error())
    return vn, fn


def mesh_normals_host_seam(vertices, faces, face_begin, face_end, seam_vertex_ids, vertex_normals):
    """vcy_mesh_normals_host_seam: finishes, IN PLACE in `vertex_normals` (C-contiguous float32 [n_vertices, 3]), the
    normals of the listed vertices of a merged mesh from the faces [face_begin, face_end) -- the reference's sum in
    ascending face index, division, normalisation; every other row stays as it is.  Serial, no GPU needed."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    ids = np.ascontiguousarray(seam_vertex_ids, np.int64).reshape(-1)
    vn = vertex_normals
    if not (isinstance(vn, np.ndarray) and vn.dtype == np.float32 and vn.flags.c_contiguous and vn.flags.writeable
            and vn.shape == v.shape):
        raise ValueError("vertex_normals must be a writeable C-contiguous float32 array of the vertices' shape")
    if face_end > len(f):
        raise ValueError("faces [%d, %d) of %d" % (face_begin, face_end, len(f)))
    rc = capi.load().vcy_mesh_normals_host_seam(len(v), _p(v), _p(f), int(face_begin), int(face_end), len(ids), _p(ids), _p(vn))
    if rc != 0:
        raise RuntimeError(last_error())
    return vn


def mesh_normals_seam_sum(n_vertices, faces, face_normals, face_begin, face_end, seam_vertex_ids, vertex_normals):
    """vcy_mesh_normals_seam_sum: the seam finish from the merged mesh's face normals (the devices' own) instead of the
    positions, IN PLACE in `vertex_normals` like mesh_normals_host_seam; of two NaN terms the later one's, as on the
    device.  Serial, no GPU needed."""
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    fn = np.ascontiguousarray(face_normals, np.float32).reshape(-1, 3)
    ids = np.ascontiguousarray(seam_vertex_ids, np.int64).reshape(-1)
    vn = vertex_normals
    if not (isinstance(vn, np.ndarray) and vn.dtype == np.float32 and vn.flags.c_contiguous and vn.flags.writeable
            and vn.shape == (int(n_vertices), 3)):
        raise ValueError("vertex_normals must be a writeable C-contiguous float32 array of the vertices' shape")
    if face_end > len(f) or len(fn) != len(f):
        raise ValueError("faces [%d, %d) of %d, %d face normals" % (face_begin, face_end, len(f), len(fn)))
    rc = capi.load().vcy_mesh_normals_seam_sum(int(n_vertices), _p(f), _p(fn), int(face_begin), int(face_end), len(ids),
                                               _p(ids), _p(vn))
    if rc != 0:
        raise RuntimeError(last_error())
    return vn


def merge_meshes_host(vertices, faces, keys, n_foreign, normals=None, face_normals=None, layer_faces=None):
    """vcy_merge_meshes_host: the meshes of z-slabs stitched by edge key into the mesh of the whole grid (rule and errors:
    include/vacancy_hip.h).  Every argument is a list with one entry per slab, in z order; the last three are given
    together (ExtractIsoSurfaceSlab's) or not at all.  Returns {"vertices" float32 [n, 3], "keys" int64 [n, 2], "faces"
    int32 [m, 3]} plus, with normals, {"normals", "face_normals"}.  Serial, no GPU needed."""
    n = len(vertices)
    given = [x for x in (normals, face_normals, layer_faces) if x is not None]
    with_normals = len(given) == 3
    if len(given) not in (0, 3) or any(len(x) != n for x in [faces, keys, n_foreign] + given):
        raise ValueError("one entry per slab in every list, and normals, face_normals and layer_faces together")
    rows = lambda col, t, w: [np.ascontiguousarray(a, t).reshape(-1, w) for a in col]  # noqa: E731
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if len(a) else None  # noqa: E731
    v, f, k = rows(vertices, np.float32, 3), rows(faces, np.int32, 3), rows(keys, np.int64, 2)
    vn, fn = (rows(normals, np.float32, 3), rows(face_normals, np.float32, 3)) if with_normals else (v, f)
    slabs = (Mesh * max(n, 1))()
    extra = (capi.MeshNormals * max(n, 1))()
    for s in range(n):
        if len(k[s]) not in (0, len(v[s])) or len(vn[s]) != len(v[s]) or len(fn[s]) != len(f[s]):
            raise ValueError("slab %d: one edge key and one normal per vertex, one face normal per face" % s)
        slabs[s] = Mesh(len(v[s]), len(f[s]), ptr(v[s], C.c_float), ptr(f[s], C.c_int32), ptr(k[s], C.c_int64), int(n_foreign[s]))
        if with_normals:
            extra[s] = capi.MeshNormals(ptr(vn[s], C.c_float), ptr(fn[s], C.c_float))
    lf = (C.c_int64 * max(2 * n, 1))(*[int(x) for pair in layer_faces for x in pair]) if with_normals else None
    nv = max(0, sum(len(a) - int(nfo) for a, nfo in zip(v, n_foreign)))
    nf = sum(len(a) for a in f)
    out = {"vertices": np.empty((nv, 3), np.float32), "keys": np.empty((nv, 2), np.int64), "faces": np.empty((nf, 3), np.int32)}
    if with_normals:
        out["normals"], out["face_normals"] = np.empty((nv, 3), np.float32), np.empty((nf, 3), np.float32)
    rc = capi.load().vcy_merge_meshes_host(n, slabs, extra if with_normals else None, lf, _p(out["vertices"]), _p(out["faces"]),
                                           _p(out["keys"]), _p(out["normals"]) if with_normals else None,
                                           _p(out["face_normals"]) if with_normals else None)
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def _color_args(vertices, views, photos, normals, depth, mode, interp, depth_tolerance, min_cos, fallback):
    """The arrays and ctypes arguments vcy_color_vertices and vcy_color_vertices_host share; the first element keeps every
    array alive for the call."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    vs = list(views)
    n = len(vs)
    ph = [np.ascontiguousarray(p, np.uint8) for p in photos]
    if len(ph) != n or any(p.shape != (w.height, w.width, 3) for p, w in zip(ph, vs)):
        raise ValueError("one height x width x 3 uint8 photograph per view")
    nr = None
    if normals is not None:
        nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if nr.shape != v.shape:
            raise ValueError("one normal per vertex")
    dp = None
    if depth is not None:
        dp = [np.ascontiguousarray(d, np.float32) for d in depth]
        if len(dp) != n or any(d.shape != (w.height, w.width) for d, w in zip(dp, vs)):
            raise ValueError("one height x width float32 depth image per view")
    opt = ColorOption(mode, interp, depth_tolerance, min_cos, fallback)
    out = {"rgb": np.zeros((len(v), 3), np.float32), "n_used": np.zeros(len(v), np.int32),
           "best_view": np.zeros(len(v), np.int32)}
    arr = (View * max(n, 1))(*vs)
    pp = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in ph])
    dpp = (C.c_void_p * n)(*[d.ctypes.data for d in dp]) if dp is not None else None
    args = (len(v), _p(v), _p(nr) if nr is not None else None, n, arr, pp, dpp, C.byref(opt), _p(out["rgb"]),
            _p(out["n_used"]), _p(out["best_view"]))
    return (v, nr, ph, dp, opt, arr, pp, dpp), args, out


def color_vertices_host(vertices, views, photos, depth, normals=None, mode=capi.VCY_COLOR_WEIGHTED,
                        interp=capi.VCY_INTERP_BILINEAR, depth_tolerance=0.0, min_cos=0.0, fallback=(128, 128, 128)):
    """vcy_color_vertices_host: the colour of every vertex from the photographs of the views that see it (definition:
    include/vacancy_hip.h), serial, no GPU needed.  `depth`: one float32 depth image per view with RenderHull's meaning.
    Returns {"rgb": float32 [n, 3] in 0 .. 255, "n_used": int32 [n], "best_view": int32 [n], -1 where no view contributes}."""
    keep, args, out = _color_args(vertices, views, photos, normals, depth, mode, interp, depth_tolerance, min_cos, fallback)
    if capi.load().vcy_color_vertices_host(*args) != 0:
        raise RuntimeError(last_error())
    return out


def _raster_args(vertices, faces, views, depth=True, face=False, hits=False):
    """The arrays and ctypes arguments vcy_raster_mesh and vcy_raster_mesh_host share (everything behind the context); the
    first element keeps every array alive for the call.  The result: one dict per view and the int64 [n_views, 2] drops."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    vs = list(views)
    n = len(vs)
    out = [{} for _ in vs]
    for o, w in zip(out, vs):
        if depth:
            o["depth"] = np.empty((w.height, w.width), np.float32)
        if face:
            o["face"] = np.empty((w.height, w.width), np.int32)
        if hits:
            o["hits"] = np.empty((w.height, (w.width + 63) // 64), np.uint64)
    dropped = np.zeros((n, 2), np.int64)
    arr = (View * max(n, 1))(*vs)
    ptrs = [(C.c_void_p * max(n, 1))(*[o[k].ctypes.data for o in out]) if on else None
            for k, on in (("depth", depth), ("face", face), ("hits", hits))]
    args = (len(v), len(f), _p(v), _p(f), n, arr, ptrs[0], ptrs[1], ptrs[2], _p(dropped))
    return (v, f, arr, ptrs), args, out, dropped


def _raster_result(rc, single, out, dropped):
    if rc != 0:
        e = RuntimeError(last_error())
        e.rc = rc
        raise e
    for o, d in zip(out, dropped):
        o["n_dropped"] = d
    return out[0] if single else out


def raster_mesh_host(vertices, faces, views, depth=True, face=True, hits=True):
    """vcy_raster_mesh_host: the indexed mesh rasterised into `views` (one vcy_view or a list), serial, no GPU needed
    (definition: include/vacancy_hip.h, "rasterising an indexed mesh").  Per view a dict: "depth" (float32 [height, width],
    camera depth, +inf on a miss), "face" (int32, the winning face, -1 on a miss), "hits" (uint64 [height, (width + 63) //
    64], RenderHullSlab's hit bits), each when asked for, and "n_dropped" (int64 [2]: faces with an unusable vertex, faces
    without area).  A single view returns its dict, a list a list.  RuntimeError (with .rc) on a refusal."""
    single = isinstance(views, View)
    keep, args, out, dropped = _raster_args(vertices, faces, [views] if single else views, depth, face, hits)
    return _raster_result(capi.load().vcy_raster_mesh_host(*args), single, out, dropped)


def _shade_args(vertices, faces, attributes, views, background, value, value8, bary):
    """The arrays and ctypes arguments vcy_shade_mesh and vcy_shade_mesh_host share (everything behind the context); the
    first element keeps every array alive for the call.  The result: one dict per view."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    a = np.ascontiguousarray(attributes, np.float32)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or len(a) != len(v):
        raise ValueError("one row of attributes per vertex")
    ch = a.shape[1]
    vs = list(views)
    n = len(vs)
    opt = capi.ShadeOption(ch, background if background is not None else (0.0,) * 4)
    out = [{} for _ in vs]
    for o, w in zip(out, vs):
        if value:
            o["value"] = np.empty((w.height, w.width, ch), np.float32)
        if value8:
            o["value8"] = np.empty((w.height, w.width, ch), np.uint8)
        if bary:
            o["bary"] = np.empty((w.height, w.width, 3), np.float32)
    arr = (View * max(n, 1))(*vs)
    ptrs = [(C.c_void_p * max(n, 1))(*[o[k].ctypes.data for o in out]) if on else None
            for k, on in (("value", value), ("value8", value8), ("bary", bary))]
    args = (len(v), len(f), _p(v), _p(f), _p(a), n, arr, C.byref(opt), ptrs[0], ptrs[1], ptrs[2])
    return (v, f, a, opt, arr, ptrs), args, out


def _shade_result(rc, single, out):
    if rc != 0:
        e = RuntimeError(last_error())
        e.rc = rc
        raise e
    return out[0] if single else out


def shade_mesh_host(vertices, faces, attributes, views, background=None, value=True, value8=False, bary=False):
    """vcy_shade_mesh_host: per-vertex `attributes` (float32 [n_vertices, channels], channels 1 .. 4) interpolated,
    perspective-correct, at the winning face of every pixel of `views` (one vcy_view or a list), serial, no GPU needed
    (definition: include/vacancy_hip.h, "shading a rasterised mesh").  Per view a dict: "value" (float32 [height, width,
    channels]), "value8" (uint8, rounded half up and clamped to 0 .. 255), "bary" (float32 [height, width, 3], zeros on a
    miss), each when asked for.  Pixels without a winner hold `background` (default zeros).  A single view returns its
    dict, a list a list.  RuntimeError (with .rc) on a refusal."""
    single = isinstance(views, View)
    keep, args, out = _shade_args(vertices, faces, attributes, [views] if single else views, background, value, value8, bary)
    return _shade_result(capi.load().vcy_shade_mesh_host(*args), single, out)


def _photo_error_args(vertices, faces, colors, views, photos, masks):
    """The arrays and ctypes arguments vcy_mesh_photo_error and vcy_mesh_photo_error_host share; the first element keeps
    every array alive for the call.  The result: int64 [n_views, 7]."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    col = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    if col.shape != v.shape:
        raise ValueError("one colour per vertex")
    vs = list(views)
    n = len(vs)
    ph = [np.ascontiguousarray(p, np.uint8) for p in photos]
    if len(ph) != n or any(p.shape != (w.height, w.width, 3) for p, w in zip(ph, vs)):
        raise ValueError("one height x width x 3 uint8 photograph per view")
    ms = None
    if masks is not None:
        ms = [np.ascontiguousarray(m, np.uint8) for m in masks]
        if len(ms) != n or any(m.shape != (w.height, w.width) for m, w in zip(ms, vs)):
            raise ValueError("one height x width silhouette per view")
    arr = (View * max(n, 1))(*vs)
    pp = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in ph])
    mp = (C.c_void_p * max(n, 1))(*[m.ctypes.data for m in ms]) if ms is not None else None
    sums = np.zeros((n, 7), np.int64)
    args = (len(v), len(f), _p(v), _p(f), _p(col), n, arr, pp, mp, _p(sums))
    return (v, f, col, ph, ms, arr, pp, mp), args, sums


def mesh_photo_error_host(vertices, faces, colors, views, photos, masks=None):
    """vcy_mesh_photo_error_host: the mesh with per-vertex `colors` (float32 [n_vertices, 3], 0 .. 255) rendered into `views`
    and compared, as uint8, with the photographs (uint8 [height, width, 3] per view), serial, no GPU needed.  int64
    [n_views, 7]: per view {n, sad r g b, ssd r g b} over the pixels the mesh covers -- and, with `masks`, whose silhouette
    is non-zero.  photo_error_stats turns them into MAE and PSNR."""
    keep, args, sums = _photo_error_args(vertices, faces, colors, views, photos, masks)
    if capi.load().vcy_mesh_photo_error_host(*args) != 0:
        raise RuntimeError(last_error())
    return sums


def photo_error_stats(sums):
    """MAE and PSNR from the seven sums of mesh_photo_error_host / MeshPhotoError (int64 [..., 7]), in float64:
    {"n": int64 [...], "mae": [..., 3] = sad / n, "mse": [..., 3] = ssd / n, "psnr": [..., 3] = 10 log10(255^2 / mse) in
    dB -- +inf for mse == 0 --, "mae_all", "psnr_all": over the three channels together}.  A view with n == 0 has no
    error to speak of: NaN everywhere."""
    s = np.asarray(sums, np.int64)
    n = s[..., 0]
    nf = n.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mae = s[..., 1:4] / nf[..., None]
        mse = s[..., 4:7] / nf[..., None]
        mse_all = s[..., 4:7].sum(axis=-1) / (3.0 * nf)
        psnr = 10.0 * np.log10(65025.0 / mse)
        psnr_all = 10.0 * np.log10(65025.0 / mse_all)
        mae_all = s[..., 1:4].sum(axis=-1) / (3.0 * nf)
    return {"n": n, "mae": mae, "mse": mse, "psnr": psnr, "mae_all": mae_all, "psnr_all": psnr_all}


def _smooth_args(vertices, faces, iterations, lam, mu, pin_boundary, normals):
    """The arrays and ctypes arguments vcy_smooth_mesh and vcy_smooth_mesh_host share; the first element keeps every array
    alive for the call."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    opt = SmoothOption(int(iterations), float(lam), float(mu), int(pin_boundary))
    out = {"vertices": np.zeros((len(v), 3), np.float32)}
    if normals:
        out["normals"] = np.zeros((len(v), 3), np.float32)
        out["face_normals"] = np.zeros((len(f), 3), np.float32)
    args = (len(v), len(f), _p(v), _p(f), C.byref(opt), _p(out["vertices"]),
            _p(out["normals"]) if normals else None, _p(out["face_normals"]) if normals else None)
    return (v, f, opt), args, out


def smooth_mesh_host(vertices, faces, iterations, lam, mu, pin_boundary=False, normals=False):
    """vcy_smooth_mesh_host: `iterations` Taubin iterations (a pass with factor `lam`, then one with `mu`; mu = 0: plain
    Laplacian smoothing) over an indexed mesh, serial, no GPU needed (definition: include/vacancy_hip.h, "mesh
    smoothing").  pin_boundary: vertices of an edge that one face uses stay.  Returns {"vertices": float32 [n, 3]} and, with
    normals=True, "normals" / "face_normals" = mesh_normals_host of the result.  RuntimeError (with .rc) on a refusal."""
    keep, args, out = _smooth_args(vertices, faces, iterations, lam, mu, pin_boundary, normals)
    rc = capi.load().vcy_smooth_mesh_host(*args)
    if rc != 0:
        e = RuntimeError(last_error())
        e.rc = rc
        raise e
    return out


def _decimate_args(vertices, faces, cell, origin, mode, normals):
    """The arrays and ctypes arguments vcy_decimate_mesh and vcy_decimate_mesh_host share; the first element keeps every array
    alive for the call."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    opt = DecimateOption(float(cell), [float(x) for x in origin], int(mode))
    out = {"vertices": np.zeros((len(v), 3), np.float32), "faces": np.zeros((len(f), 3), np.int32),
           "vertex_map": np.zeros(len(v), np.int32), "face_source": np.zeros(len(f), np.int32)}
    if normals:
        out["normals"] = np.zeros((len(v), 3), np.float32)
        out["face_normals"] = np.zeros((len(f), 3), np.float32)
    counts = (C.c_int64(-1), C.c_int64(-1))
    args = (len(v), len(f), _p(v), _p(f), C.byref(opt), _p(out["vertices"]), _p(out["faces"]), C.byref(counts[0]),
            C.byref(counts[1]), _p(out["vertex_map"]), _p(out["face_source"]),
            _p(out["normals"]) if normals else None, _p(out["face_normals"]) if normals else None)
    return (v, f, opt, counts), args, out


def _decimate_result(rc, keep, out):
    """The outputs cut to the counts the call returned."""
    if rc != 0:
        e = RuntimeError(last_error())
        e.rc = rc
        raise e
    nv, nf = keep[3][0].value, keep[3][1].value
    if len(keep[0]) == 0 or len(keep[1]) == 0:
        out["vertex_map"][...] = -1      # (an empty call writes no array: no vertex has an output)
    for key in ("vertices", "normals"):
        if key in out:
            out[key] = out[key][:nv]
    for key in ("faces", "face_source", "face_normals"):
        if key in out:
            out[key] = out[key][:nf]
    return out


def decimate_mesh_host(vertices, faces, cell, origin=(0.0, 0.0, 0.0), mode=capi.VCY_DECIMATE_MEAN, normals=False):
    """vcy_decimate_mesh_host: vertex clustering of an indexed mesh over a lattice of cubes of edge `cell` with a corner at
    `origin`, serial, no GPU needed (definition: include/vacancy_hip.h, "mesh decimation").  mode: the representative of a
    cluster, VCY_DECIMATE_MEAN / _NEAREST / _FIRST.  Returns {"vertices", "faces", "vertex_map" (output index of every input
    vertex, or -1), "face_source" (input index of every output face)} and, with normals=True, "normals" / "face_normals" =
    mesh_normals_host of the result.  RuntimeError (with .rc) on a refusal."""
    keep, args, out = _decimate_args(vertices, faces, cell, origin, mode, normals)
    return _decimate_result(capi.load().vcy_decimate_mesh_host(*args), keep, out)


def _quadric_args(vertices, faces, cell, origin, regularize, normals):
    """_decimate_args for vcy_decimate_mesh_quadric and its host function: MEAN, `regularize` behind the option, the fallback
    count (keep[4]) at the end."""
    keep, args, out = _decimate_args(vertices, faces, cell, origin, capi.VCY_DECIMATE_MEAN, normals)
    n_fallback = C.c_int64(-1)
    return keep + (n_fallback,), args[:5] + (C.c_float(regularize),) + args[5:] + (C.byref(n_fallback),), out


def _quadric_result(rc, keep, out):
    out = _decimate_result(rc, keep, out)
    out["n_fallback"] = keep[4].value
    return out


def decimate_mesh_quadric_host(vertices, faces, cell, origin=(0.0, 0.0, 0.0), regularize=1e-3, normals=False):
    """vcy_decimate_mesh_quadric_host: decimate_mesh_host with MEAN clusters whose representative is the quadric-error
    optimum of the input faces around the cluster (definition: include/vacancy_hip.h, "mesh decimation, quadric
    representatives"), serial, no GPU needed.  Returns decimate_mesh_host's dict plus "n_fallback", the output vertices that
    kept the mean.  RuntimeError (with .rc) on a refusal."""
    keep, args, out = _quadric_args(vertices, faces, cell, origin, regularize, normals)
    return _quadric_result(capi.load().vcy_decimate_mesh_quadric_host(*args), keep, out)


def carve_depth_host(option, views, depths, band, sdf, update_num, z_range=None):
    """vcy_carve_depth_host: the depth carve (definition: include/vacancy_hip.h, "carve from depth images") serially on the
    host, no GPU needed, IN PLACE on `sdf` (float32) and `update_num` (int32), C-contiguous arrays in download()'s layout
    for the slices z_range = (z_begin, z_end) of the grid of `option` (default: the whole grid).  `depths`: one float32
    height x width image per view.  RuntimeError (with .rc) on a refusal; the arrays are then untouched."""
    lib = capi.load()
    n = len(views)
    dp = [np.ascontiguousarray(d, np.float32) for d in depths]
    if len(dp) != n or any(d.shape != (v.height, v.width) for d, v in zip(dp, views)):
        raise ValueError("one height x width float32 depth image per view")
    for a, t in ((sdf, np.float32), (update_num, np.int32)):
        if not (isinstance(a, np.ndarray) and a.dtype == t and a.flags.c_contiguous and a.flags.writeable):
            raise ValueError("sdf and update_num must be writeable C-contiguous float32 / int32 arrays")
    dims = (C.c_int32 * 3)()
    if lib.vcy_compute_dims(option.bb_min, option.bb_max, option.resolution, dims) != 0:
        raise RuntimeError(last_error())
    z0, z1 = z_range if z_range is not None else (0, int(dims[2]))
    if sdf.size != update_num.size or sdf.size != int(dims[0]) * int(dims[1]) * max(z1 - z0, 0):
        raise ValueError("sdf and update_num hold one entry per voxel of the slices [%d, %d)" % (z0, z1))
    arr = (View * max(n, 1))(*views)
    ptrs = (C.c_void_p * max(n, 1))(*[d.ctypes.data for d in dp])
    rc = lib.vcy_carve_depth_host(C.byref(option), int(z0), int(z1), n, arr, ptrs, float(band), _p(sdf), _p(update_num))
    if rc != 0:
        e = RuntimeError(last_error())
        e.rc = rc
        raise e
    return sdf, update_num


def distance_field_host(option, sdf, update_num, iso_level=0.0, radius=8):
    """vcy_distance_field_host: the distance field of the hull (definition: include/vacancy_hip.h, "distance field of the
    hull") serially on the host, no GPU needed.  `sdf` (float32) and `update_num` (int32) in download()'s layout for the
    whole grid of `option`.  Returns (d2, sdf_out): the signed int32 field and the sdf Redistance would leave.
    RuntimeError (with .rc) on a refusal."""
    lib = capi.load()
    s = np.ascontiguousarray(sdf, np.float32).reshape(-1)
    u = np.ascontiguousarray(update_num, np.int32).reshape(-1)
    dims = (C.c_int32 * 3)()
    if lib.vcy_compute_dims(option.bb_min, option.bb_max, option.resolution, dims) != 0:
        raise RuntimeError(last_error())
    if s.size != u.size or s.size != int(dims[0]) * int(dims[1]) * int(dims[2]):
        raise ValueError("sdf and update_num hold one entry per voxel of the grid")
    d2, out = np.empty(s.size, np.int32), np.empty(s.size, np.float32)
    rc = lib.vcy_distance_field_host(C.byref(option), _p(s), _p(u), float(iso_level), int(radius), _p(d2), _p(out))
    if rc != 0:
        e = RuntimeError(last_error())
        e.rc = rc
        raise e
    return d2, out


def _raise_rc(rc):
    e = RuntimeError(last_error())
    e.rc = rc
    raise e


def _slab_slice(option, z_range):
    """(voxels of an xy slice, slices of the slab) of the slab z_range of the grid of `option`"""
    dims = (C.c_int32 * 3)()
    if capi.load().vcy_compute_dims(option.bb_min, option.bb_max, option.resolution, dims) != 0:
        raise RuntimeError(last_error())
    return int(dims[0]) * int(dims[1]), max(int(z_range[1]) - int(z_range[0]), 0)


def _planes_arg(planes, slice_voxels):
    """(array to keep alive, pointer or None, count) of a stack of uint16 planes (None: no planes)"""
    if planes is None:
        return None, None, 0
    a = np.ascontiguousarray(planes, np.uint16).reshape(-1)
    if a.size % slice_voxels:
        raise ValueError("planes hold nx * ny uint16 each")
    return a, (_p(a) if a.size else None), a.size // slice_voxels


def distance_slab_planes_host(option, z_range, sdf, update_num, iso_level=0.0, radius=8):
    """vcy_distance_slab_planes_host: the first half of the distance field of a z-slab on the host, no GPU needed -- the x
    and the y pass over the slices z_range = (z_begin, z_end) of the grid of `option`, `sdf` / `update_num` in download()'s
    layout for those slices.  Returns the planes, uint16 [slices, nx * ny]: class in bit 15, the capped squared 2-D
    distance below it.  RuntimeError (with .rc) on a refusal."""
    sl, nzl = _slab_slice(option, z_range)
    s = np.ascontiguousarray(sdf, np.float32).reshape(-1)
    u = np.ascontiguousarray(update_num, np.int32).reshape(-1)
    if s.size != u.size or s.size != sl * nzl:
        raise ValueError("sdf and update_num hold one entry per voxel of the slices [%d, %d)" % tuple(z_range))
    h = np.empty((nzl, sl), np.uint16)
    rc = capi.load().vcy_distance_slab_planes_host(C.byref(option), int(z_range[0]), int(z_range[1]), _p(s), _p(u),
                                                   float(iso_level), int(radius), _p(h))
    if rc != 0:
        _raise_rc(rc)
    return h


def distance_slab_finish_host(option, z_range, h, below, above, radius, sdf, update_num):
    """vcy_distance_slab_finish_host: the second half -- the z pass over the slab's planes `h` with the planes of the
    global slices [z_begin - n, z_begin) in `below` and [z_end, z_end + m) in `above` (None: none), n = min(radius,
    z_begin), m = min(radius, nz - z_end).  Returns (d2, sdf_out) of the slab as distance_field_host does of the grid.
    RuntimeError (with .rc) on a refusal."""
    sl, nzl = _slab_slice(option, z_range)
    hh = np.ascontiguousarray(h, np.uint16).reshape(-1)
    s = np.ascontiguousarray(sdf, np.float32).reshape(-1)
    u = np.ascontiguousarray(update_num, np.int32).reshape(-1)
    if not (hh.size == s.size == u.size == sl * nzl):
        raise ValueError("h, sdf and update_num hold one entry per voxel of the slices [%d, %d)" % tuple(z_range))
    kb, pb, nb = _planes_arg(below, sl)
    ka, pa, na = _planes_arg(above, sl)
    d2, out = np.empty(s.size, np.int32), np.empty(s.size, np.float32)
    rc = capi.load().vcy_distance_slab_finish_host(C.byref(option), int(z_range[0]), int(z_range[1]), _p(hh), pb, nb, pa, na,
                                                   int(radius), _p(u), _p(s), _p(d2), _p(out))
    del kb, ka
    if rc != 0:
        _raise_rc(rc)
    return d2, out


def close_hull_plan(radius_voxels, resolution):
    """(r, R) of CloseHull by vcy_close_hull_plan (no GPU): r = radius_voxels * resolution in world units and the
    transform's radius R = ceil(radius_voxels) + 2.  ValueError, with the library's text, for a radius out of range or one
    on which the closing ties (include/vacancy_hip.h, the tie rule) -- pick 1.3, 2.3, ..."""
    r, big_r = C.c_double(0.0), C.c_int(0)
    if capi.load().vcy_close_hull_plan(float(radius_voxels), float(resolution), C.byref(r), C.byref(big_r)) != 0:
        raise ValueError(last_error())
    return r.value, big_r.value


class VoxelCarver:
    def __init__(self, option=None, device_id=0, z_range=None):
        self._lib = capi.load()
        self._ctx = C.c_void_p()
        self._device = device_id
        self._z_range = z_range
        self.option = option
        self.dims = None

    # -- VoxelCarver::set_option / Init (voxel_carver.cc:373-392)
    def set_option(self, option):
        self.option = option

    def Init(self):
        self.close()
        z0, z1 = self._z_range if self._z_range else (0, -1)
        rc = self._lib.vcy_create(C.byref(self.option), self._device, z0, z1, C.byref(self._ctx))
        if rc != 0:
            self._ctx = C.c_void_p()
            return False
        d = (C.c_int32 * 3)()
        self._lib.vcy_grid_dims(self._ctx, d)
        self.dims = tuple(d)
        zr = (C.c_int32 * 2)()
        self._lib.vcy_slab_range(self._ctx, zr)
        self.z_range = tuple(zr)
        return True

    def close(self):
        if self._ctx:
            self._lib.vcy_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx(self):
        return self._ctx

    @property
    def slab_voxels(self):
        return self.dims[0] * self.dims[1] * (self.z_range[1] - self.z_range[0])

    # -- Carve(camera, roi_min, roi_max, sdf)  (voxel_carver.cc:415-496)
    def Carve(self, view, sdf):
        if not self._ctx:
            return False
        sdf = np.ascontiguousarray(sdf, dtype=np.float32)
        assert sdf.shape == (view.height, view.width)
        return self._lib.vcy_carve(self._ctx, C.byref(view), _p(sdf)) == 0

    # -- Carve(camera, silhouette, roi_min, roi_max, &sdf)  (voxel_carver.cc:394-413)
    def CarveSilhouette(self, view, silhouette, return_sdf=False):
        if not self._ctx:
            return False
        mask = np.ascontiguousarray(silhouette, dtype=np.uint8)
        sdf = np.empty(mask.shape, np.float32) if return_sdf else None
        rc = self._lib.vcy_carve_silhouette(self._ctx, C.byref(view), _p(mask),
                                            _p(sdf) if return_sdf else None)
        return (rc == 0, sdf) if return_sdf else rc == 0

    # -- Carve(vector<Camera>, vector<Image1b>) (voxel_carver.cc:516-528), streamed + fused
    def CarveBatchSilhouettes(self, views, silhouettes):
        n = len(views)
        arr = (View * n)(*views)
        masks = [np.ascontiguousarray(m, np.uint8) for m in silhouettes]
        ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in masks])
        return self._lib.vcy_carve_batch_silhouettes(self._ctx, n, arr, ptrs) == 0

    def make_sdf_batch_into(self, views, silhouettes, out_ptrs):
        """vcy_make_sdf_batch_device: SDF images of `silhouettes` (host) into caller-owned device images."""
        n = len(views)
        arr = (View * n)(*views)
        masks = [np.ascontiguousarray(m, np.uint8) for m in silhouettes]
        mptr = (C.c_void_p * n)(*[m.ctypes.data for m in masks])
        optr = (C.c_void_p * n)(*[p.value if isinstance(p, C.c_void_p) else int(p) for p in out_ptrs])
        return self._lib.vcy_make_sdf_batch_device(self._ctx, n, arr, mptr, optr) == 0

    def last_stream_ms(self):
        """(producer ms, carve ms, wall ms) of the last CarveBatchSilhouettes (vcy_last_stream_ms)."""
        a, b, w = C.c_float(), C.c_float(), C.c_float()
        assert self._lib.vcy_last_stream_ms(self._ctx, C.byref(a), C.byref(b), C.byref(w)) == 0, last_error()
        return a.value, b.value, w.value

    # -- the robust visual hull (no reference counterpart; definition: include/vacancy_hip.h, "robust carve")
    def _carve_robust(self, entry, views, pointers, keep, tolerate, iso_level):
        n = len(views)
        arr = (View * max(n, 1))(*views)
        ptrs = (C.c_void_p * max(n, 1))(*pointers)
        overruled = np.zeros(n, np.int64)
        rc = entry(self._ctx, n, arr, ptrs, int(tolerate), float(iso_level), _p(overruled))
        del keep
        if rc != 0:
            e = RuntimeError(last_error())
            e.rc = rc
            raise e
        ms = C.c_float()
        self._lib.vcy_last_robust_ms(self._ctx, C.byref(ms))
        return {"overruled": overruled, "device_ms": ms.value}

    def CarveRobustDevice(self, views, sdf_devs, tolerate, iso_level=0.0):
        """vcy_carve_robust_device: REPLACES the state by the robust hull of `views` (SDF images resident on the device):
        per voxel the (tolerate + 1)-th largest sample instead of the largest, so a voxel is carved only when more than
        `tolerate` views say outside.  {"overruled": int64 [n], the voxels kept solid although view i says outside;
        "device_ms"}.  RuntimeError (with .rc) on a refusal; the state is then untouched."""
        ptrs = [p.value if isinstance(p, C.c_void_p) else p for p in sdf_devs]
        if len(ptrs) != len(views):
            raise ValueError("one SDF image per view")
        return self._carve_robust(self._lib.vcy_carve_robust_device, views, ptrs, None, tolerate, iso_level)

    def CarveRobustSilhouettes(self, views, silhouettes, tolerate, iso_level=0.0):
        """vcy_carve_robust_silhouettes: the same from silhouettes in host memory; every SDF is built on the device."""
        masks = [np.ascontiguousarray(m, np.uint8) for m in silhouettes]
        if len(masks) != len(views):
            raise ValueError("one silhouette per view")
        return self._carve_robust(self._lib.vcy_carve_robust_silhouettes, views, [m.ctypes.data for m in masks], masks,
                                  tolerate, iso_level)

    # -- carve from depth images (no reference counterpart; definition: include/vacancy_hip.h, "carve from depth images")
    def _carve_depth(self, entry, views, pointers, keep, band):
        n = len(views)
        arr = (View * max(n, 1))(*views)
        ptrs = (C.c_void_p * max(n, 1))(*pointers)
        rc = entry(self._ctx, n, arr, ptrs, float(band))
        del keep
        if rc != 0:
            e = RuntimeError(last_error())
            e.rc = rc
            raise e
        ms = C.c_float()
        self._lib.vcy_last_depth_ms(self._ctx, C.byref(ms))
        return {"device_ms": ms.value}

    def CarveDepthDevice(self, views, depth_devs, band):
        """vcy_carve_depth_device: fuses the depth images of `views` (resident on the device; RenderHull's meaning: camera
        depth, +inf on a miss) into the state -- per voxel and view the sample (depth(pixel) - z_c) / band, clamped to 1
        and dropped below -1, through the context's update rule.  {"device_ms"}.  RuntimeError (with .rc) on a refusal;
        the state is then untouched."""
        ptrs = [p.value if isinstance(p, C.c_void_p) else p for p in depth_devs]
        if len(ptrs) != len(views):
            raise ValueError("one depth image per view")
        return self._carve_depth(self._lib.vcy_carve_depth_device, views, ptrs, None, band)

    def CarveDepth(self, views, depths, band):
        """vcy_carve_depth: the same from numpy images (float32 height x width per view), uploaded by the call."""
        dp = [np.ascontiguousarray(d, np.float32) for d in depths]
        if len(dp) != len(views) or any(d.shape != (v.height, v.width) for d, v in zip(dp, views)):
            raise ValueError("one height x width float32 depth image per view")
        return self._carve_depth(self._lib.vcy_carve_depth, views, [d.ctypes.data for d in dp], dp, band)

    def download_voxels(self, ids):
        ids = np.ascontiguousarray(ids, np.int64)
        s = np.empty(len(ids), np.float32)
        u = np.empty(len(ids), np.int32)
        rc = self._lib.vcy_download_voxels(self._ctx, len(ids), _p(ids), _p(s), _p(u))
        if rc != 0:
            raise RuntimeError(last_error())
        return s, u

    # -- device-resident SDF images (bench / streaming)
    def upload_sdf(self, sdf):
        sdf = np.ascontiguousarray(sdf, dtype=np.float32)
        out = C.c_void_p()
        rc = self._lib.vcy_sdf_upload(self._ctx, _p(sdf), sdf.shape[1], sdf.shape[0], C.byref(out))
        if rc != 0:
            raise RuntimeError(last_error())
        return out

    def make_sdf_device(self, mask, roi_min=None, roi_max=None, normalize=True, use_truncation=False, band=0.1):
        """MakeSignedDistanceField on the device; returns a device pointer (free_device it)."""
        mask = np.ascontiguousarray(mask, np.uint8)
        h, w = mask.shape
        rmin = (C.c_int32 * 2)(*(roi_min or (0, 0)))
        rmax = (C.c_int32 * 2)(*(roi_max or (w - 1, h - 1)))
        out = C.c_void_p()
        rc = self._lib.vcy_make_sdf_device(self._ctx, _p(mask), w, h, rmin, rmax, int(normalize),
                                           int(use_truncation), band, C.byref(out))
        if rc != 0:
            raise RuntimeError(last_error())
        return out

    def download_image(self, ptr, shape):
        out = np.empty(shape, np.float32)
        assert self._lib.vcy_memcpy_d2h(self._ctx, _p(out), ptr, out.nbytes) == 0, last_error()
        return out

    def memcpy_h2d(self, ptr, array):
        array = np.ascontiguousarray(array)
        assert self._lib.vcy_memcpy_h2d(self._ctx, ptr, _p(array), array.nbytes) == 0, last_error()

    def free_device(self, ptr):
        self._lib.vcy_device_free(self._ctx, ptr)

    def CarveDevice(self, view, sdf_dev):
        return self._lib.vcy_carve_device(self._ctx, C.byref(view), sdf_dev) == 0

    # -- Carve(vector<Camera>, vector<...>) loop (voxel_carver.cc:516-528), fused on device
    @staticmethod
    def prepare_batch(views, sdf_devs):
        """ctypes arrays for CarveBatchDevice, built once when the same batch is carved repeatedly."""
        n = len(views)
        arr = (View * n)(*views)
        ptrs = (C.c_void_p * n)(*[p.value if isinstance(p, C.c_void_p) else p for p in sdf_devs])
        return n, arr, ptrs

    def CarveBatchDevice(self, views, sdf_devs=None):
        n, arr, ptrs = views if sdf_devs is None else self.prepare_batch(views, sdf_devs)
        return self._lib.vcy_carve_batch_device(self._ctx, n, arr, ptrs) == 0

    # -- ExtractIsoSurface(mesh, iso_level, linear_interp)  (voxel_carver.cc:540-543)
    def ExtractIsoSurface(self, iso_level=0.0, linear_interp=True, normals=False):
        """normals=True: vcy_extract_iso_normals -- the dict gains "normals" (per vertex), "face_normals" and
        "normals_device_ms": Mesh::CalcNormal of the mesh, computed on the device (bit-equal to mesh_normals_host)."""
        m = Mesh()
        mn = capi.MeshNormals()
        if normals:
            rc = self._lib.vcy_extract_iso_normals(self._ctx, iso_level, int(linear_interp),
                                                   capi.VCY_NORMALS_VERTEX | capi.VCY_NORMALS_FACE, C.byref(m),
                                                   C.byref(mn))
        else:
            rc = self._lib.vcy_extract_iso(self._ctx, iso_level, int(linear_interp), C.byref(m))
        if rc != 0:
            self._lib.vcy_mesh_free(C.byref(m))
            self._lib.vcy_mesh_normals_free(C.byref(mn))
            raise RuntimeError(last_error())
        nv, nf = m.n_vertices, m.n_faces
        out = {
            "vertices": _mesh_array(m.vertices, nv, 3, np.float32),
            "faces": _mesh_array(m.faces, nf, 3, np.int32),
            "keys": _mesh_array(m.edge_keys, nv, 2, np.int64),
            "n_foreign": int(m.n_foreign_vertices),
        }
        ms = C.c_float()
        if normals:
            out["normals"] = _mesh_array(mn.vertex_normals, nv, 3, np.float32)
            out["face_normals"] = _mesh_array(mn.face_normals, nf, 3, np.float32)
            self._lib.vcy_mesh_normals_free(C.byref(mn))
            self._lib.vcy_last_normals_ms(self._ctx, C.byref(ms))
            out["normals_device_ms"] = ms.value
        self._lib.vcy_mesh_free(C.byref(m))
        self._lib.vcy_last_extract_ms(self._ctx, C.byref(ms))
        out["device_ms"] = ms.value
        self._lib.vcy_last_extract_wall_ms(self._ctx, C.byref(ms))
        out["wall_ms"] = ms.value  # vcy_extract_iso entry -> mesh arrays in host memory
        return out

    def ExtractIsoSurfaceSlab(self, iso_level=0.0, linear_interp=True, normals=True):
        """vcy_extract_iso_normals_slab: the extraction of a context that owns a z-slab (or the whole grid) as one part
        of a merge.  The dict of ExtractIsoSurface plus "normals", "face_normals", "normals_device_ms" and "layer_faces"
        = (faces of the first, of the last own cell layer): the normals of the seam vertices are zero until
        vacancy_amd.dist.merge_meshes has finished them on the host.  normals=False is ExtractIsoSurface."""
        if not normals:
            return self.ExtractIsoSurface(iso_level, linear_interp)
        m = Mesh()
        mn = capi.MeshNormals()
        lf = (C.c_int64 * 2)()
        rc = self._lib.vcy_extract_iso_normals_slab(self._ctx, iso_level, int(linear_interp),
                                                    capi.VCY_NORMALS_VERTEX | capi.VCY_NORMALS_FACE, C.byref(m),
                                                    C.byref(mn), lf)
        if rc != 0:
            self._lib.vcy_mesh_free(C.byref(m))
            self._lib.vcy_mesh_normals_free(C.byref(mn))
            raise RuntimeError(last_error())
        nv, nf = m.n_vertices, m.n_faces
        out = {
            "vertices": _mesh_array(m.vertices, nv, 3, np.float32),
            "faces": _mesh_array(m.faces, nf, 3, np.int32),
            "keys": _mesh_array(m.edge_keys, nv, 2, np.int64),
            "n_foreign": int(m.n_foreign_vertices),
            "normals": _mesh_array(mn.vertex_normals, nv, 3, np.float32),
            "face_normals": _mesh_array(mn.face_normals, nf, 3, np.float32),
            "layer_faces": (int(lf[0]), int(lf[1])),
        }
        self._lib.vcy_mesh_normals_free(C.byref(mn))
        self._lib.vcy_mesh_free(C.byref(m))
        ms = C.c_float()
        self._lib.vcy_last_normals_ms(self._ctx, C.byref(ms))
        out["normals_device_ms"] = ms.value
        self._lib.vcy_last_extract_ms(self._ctx, C.byref(ms))
        out["device_ms"] = ms.value
        self._lib.vcy_last_extract_wall_ms(self._ctx, C.byref(ms))
        out["wall_ms"] = ms.value
        return out

    # -- ExtractVoxel(mesh, inside_empty)  (voxel_carver.cc:530-538)
    def ExtractVoxel(self, inside_empty=False, arrays=True):
        """arrays=False: only the sizes (bench.py times the library call, not numpy's copy of an 800 MB mesh)."""
        m = Mesh()
        rc = self._lib.vcy_extract_voxel(self._ctx, int(inside_empty), C.byref(m))
        if rc != 0:
            self._lib.vcy_mesh_free(C.byref(m))
            raise RuntimeError(last_error())
        nv, nf = m.n_vertices, m.n_faces
        if not arrays:
            self._lib.vcy_mesh_free(C.byref(m))
            return {"n_vertices": int(nv), "n_faces": int(nf)}
        out = {
            "vertices": _mesh_array(m.vertices, nv, 3, np.float32),
            "faces": _mesh_array(m.faces, nf, 3, np.int32),
        }
        self._lib.vcy_mesh_free(C.byref(m))
        return out

    def ExtractVoxelInto(self, inside_empty=False):
        """vcy_extract_voxel_into: the voxel mesh written by the library into numpy arrays this call allocates once the
        sizes are known (what the C++ class API does with its Mesh's vectors)."""
        got = {"vertices": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int32)}

        def provide(user, nv, nf, pv, pf):
            got["vertices"] = np.empty((nv, 3), np.float32)
            got["faces"] = np.empty((nf, 3), np.int32)
            pv[0] = got["vertices"].ctypes.data_as(C.POINTER(C.c_float))
            pf[0] = got["faces"].ctypes.data_as(C.POINTER(C.c_int32))
            return 0

        cb = capi.MeshArraysFn(provide)
        rc = self._lib.vcy_extract_voxel_into(self._ctx, int(inside_empty), cb, None)
        if rc != 0:
            raise RuntimeError(last_error())
        return got

    def extract_voxel_ids(self, inside_empty=False):
        """vcy_extract_voxel_ids: GLOBAL ids of the voxels of this slab that ExtractVoxel keeps, in scan order."""
        p, n = C.POINTER(C.c_int64)(), C.c_int64(0)
        rc = self._lib.vcy_extract_voxel_ids(self._ctx, int(inside_empty), C.byref(p), C.byref(n))
        if rc != 0:
            raise RuntimeError(last_error())
        if n.value == 0:
            return np.zeros(0, np.int64)
        ids = np.ctypeslib.as_array(p, shape=(n.value,)).copy()
        self._lib.vcy_ids_free(p)
        return ids

    # -- connected components of the hull (no reference counterpart; definitions: include/vacancy_hip.h)
    def LabelComponents(self, iso_level=0.0, labels=False):
        """vcy_label_components: the 6-connected components of the solid voxels (update_num >= 1 and sdf < iso_level),
        labelled on the device.  Dict of numpy arrays, one row per component, n_voxels descending then label ascending:
        "label" (int64, the component's smallest voxel id), "n_voxels" (int64), "bb_min" / "bb_max" (int32 [n, 3],
        inclusive x y z); with labels=True also "labels" (int64 per voxel, -1 where not solid); "device_ms"."""
        return self._label(self._lib.vcy_label_components, iso_level, labels)

    def _label(self, entry, iso_level, labels):
        p, n = C.POINTER(capi.Component)(), C.c_int64(0)
        rc = entry(self._ctx, iso_level, C.byref(p), C.byref(n))
        if rc != 0:
            raise RuntimeError(last_error())
        out = components_to_dict(p, n.value)
        if labels:
            out["labels"] = self.download_labels()
        out["device_ms"] = self.last_components_ms()
        return out

    def KeepComponents(self, iso_level=0.0, largest=1, min_voxels=0, fill_sdf=1.0):
        """vcy_keep_components: keeps the `largest` largest components (<= 0: any number) that have at least
        `min_voxels` voxels; every voxel of every other component gets sdf = fill_sdf (finite, >= iso_level), in
        place, with the brick minima kept current."""
        rc_n, rv_n = C.c_int64(0), C.c_int64(0)
        rc = self._lib.vcy_keep_components(self._ctx, iso_level, int(largest), int(min_voxels), fill_sdf,
                                           C.byref(rc_n), C.byref(rv_n))
        if rc != 0:
            raise RuntimeError(last_error())
        return {"removed_components": int(rc_n.value), "removed_voxels": int(rv_n.value),
                "device_ms": self.last_components_ms()}

    # -- the same for a context that owns a z-slab; the order of the calls is in include/vacancy_hip.h, and
    # vacancy_amd.dist.label_components_slabs / keep_components_slabs go through it
    def LabelComponentsSlab(self, iso_level=0.0, labels=False):
        """vcy_label_components_slab: the pieces of the slices this context owns, as LabelComponents returns them, with
        provisional labels (the piece's smallest global voxel id) and boxes in global z."""
        return self._label(self._lib.vcy_label_components_slab, iso_level, labels)

    def component_top_plane(self):
        """vcy_component_top_plane: provisional labels of the slab's last slice (int64 [nx * ny], -1 where not solid)."""
        plane = np.empty(self.dims[0] * self.dims[1], np.int64)
        if self._lib.vcy_component_top_plane(self._ctx, _p(plane)) != 0:
            raise RuntimeError(last_error())
        return plane

    def component_seam_pairs(self, below_plane):
        """vcy_component_seam_pairs: int64 [n, 2] of (label in the slab below, label in this slab) for the pieces that
        touch across the seam at this slab's first slice; `below_plane` = component_top_plane() of the slab below."""
        below = np.ascontiguousarray(below_plane, np.int64)
        if below.size != self.dims[0] * self.dims[1]:
            raise ValueError("the plane has %d entries, a slice of this grid %d" % (below.size, self.dims[0] * self.dims[1]))
        p, n = C.POINTER(C.c_int64)(), C.c_int64(0)
        if self._lib.vcy_component_seam_pairs(self._ctx, _p(below), C.byref(p), C.byref(n)) != 0:
            raise RuntimeError(last_error())
        if not n.value:
            return np.zeros((0, 2), np.int64)
        pairs = np.ctypeslib.as_array(p, shape=(n.value, 2)).copy()
        self._lib.vcy_seam_pairs_free(p)
        return pairs

    def resolve_components(self, provisional, merged):
        """vcy_resolve_components_slab: installs the merged label of every piece LabelComponentsSlab reported;
        download_labels() then returns merged labels."""
        a, b = np.ascontiguousarray(provisional, np.int64), np.ascontiguousarray(merged, np.int64)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError("one merged label per provisional label")
        if self._lib.vcy_resolve_components_slab(self._ctx, len(a), _p(a), _p(b)) != 0:
            raise RuntimeError(last_error())

    def KeepComponentsSlab(self, remove_provisional, fill_sdf=1.0):
        """vcy_keep_components_slab: the voxels of the listed pieces get sdf = fill_sdf.  {"removed_voxels", "device_ms"}."""
        a = np.ascontiguousarray(remove_provisional, np.int64).reshape(-1)
        gone = C.c_int64(0)
        if self._lib.vcy_keep_components_slab(self._ctx, fill_sdf, len(a), _p(a), C.byref(gone)) != 0:
            raise RuntimeError(last_error())
        return {"removed_voxels": int(gone.value), "device_ms": self.last_components_ms()}

    def download_labels(self):
        """vcy_download_labels: the label of every voxel as of the last LabelComponents / KeepComponents."""
        lab = np.empty(self.slab_voxels, np.int64)
        if self._lib.vcy_download_labels(self._ctx, _p(lab)) != 0:
            raise RuntimeError(last_error())
        return lab

    def last_components_ms(self):
        ms = C.c_float()
        self._lib.vcy_last_components_ms(self._ctx, C.byref(ms))
        return ms.value

    # -- distance field of the hull (no reference counterpart; definitions: include/vacancy_hip.h)
    def DistanceField(self, iso_level=0.0, radius=8):
        """vcy_distance_field: the signed squared Euclidean distance, in voxels, of every voxel to the nearest voxel of
        the other class (solid: update_num >= 1 and sdf < iso_level), built on the device: int32 per voxel, -d2 where
        solid, +d2 elsewhere, exact up to radius * radius, radius * radius + 1 beyond.  The state is not changed."""
        d2 = np.empty(self.slab_voxels, np.int32)
        if self._lib.vcy_distance_field(self._ctx, float(iso_level), int(radius), _p(d2)) != 0:
            raise RuntimeError(last_error())
        return d2

    def Redistance(self, iso_level=0.0, radius=8):
        """vcy_redistance: every touched voxel gets sdf = (sqrt(min(d2, radius^2)) - 0.5) * resolution, negated where
        solid, in place: ExtractIsoSurface(+r) is then the hull grown by r, (-r) the hull shrunk by r, for
        |r| < (radius - 0.5) * resolution.  Returns {"rewritten", "device_ms"}."""
        n = C.c_int64(0)
        if self._lib.vcy_redistance(self._ctx, float(iso_level), int(radius), C.byref(n)) != 0:
            raise RuntimeError(last_error())
        return {"rewritten": int(n.value), "device_ms": self.last_distance_ms()}

    def CloseHull(self, radius_voxels, iso_level=0.0):
        """Morphological closing of the hull by a ball of radius_voxels voxels: three Redistance calls (the metric field,
        the field of the hull grown by r, the field of that shrunk by r).  The state ends as the metric field of the closed
        hull with its surface at iso 0.  ValueError for a radius on which the closing ties (close_hull_plan)."""
        r, big_r = close_hull_plan(radius_voxels, self.option.resolution)
        return [self.Redistance(iso_level, big_r), self.Redistance(r, big_r), self.Redistance(-r, big_r)]

    # ... of a z-slab: DistanceSlabBegin on every slab, the slabs' planes through the host (vacancy_amd.dist.distance_halos),
    # then DistanceFieldSlab or RedistanceSlab on every slab (include/vacancy_hip.h; composed in vacancy_amd.dist)
    def DistanceSlabBegin(self, iso_level=0.0, radius=8):
        """vcy_distance_slab_begin: the x and the y pass over the slab's own slices, kept on the device.  Returns the
        device ms.  RuntimeError (with .rc) on a refusal."""
        rc = self._lib.vcy_distance_slab_begin(self._ctx, float(iso_level), int(radius))
        if rc != 0:
            _raise_rc(rc)
        return self.last_distance_ms()

    def DistanceSlabPlanes(self, z_begin, z_end):
        """vcy_distance_slab_planes: the kept planes of the global slices [z_begin, z_end) of the slab, uint16
        [slices, nx * ny].  RuntimeError (with .rc) without a DistanceSlabBegin or after a write of the state."""
        h = np.empty((max(int(z_end) - int(z_begin), 0), self.dims[0] * self.dims[1]), np.uint16)
        rc = self._lib.vcy_distance_slab_planes(self._ctx, int(z_begin), int(z_end), _p(h))
        if rc != 0:
            _raise_rc(rc)
        return h

    def DistanceFieldSlab(self, below=None, above=None):
        """vcy_distance_field_slab: DistanceField of the slab's slices as the whole grid's context would return them, from
        the planes of its neighbours (None: none).  RuntimeError (with .rc) on a refusal."""
        sl = self.dims[0] * self.dims[1]
        kb, pb, nb = _planes_arg(below, sl)
        ka, pa, na = _planes_arg(above, sl)
        d2 = np.empty(self.slab_voxels, np.int32)
        rc = self._lib.vcy_distance_field_slab(self._ctx, pb, nb, pa, na, _p(d2))
        del kb, ka
        if rc != 0:
            _raise_rc(rc)
        return d2

    def RedistanceSlab(self, below=None, above=None):
        """vcy_redistance_slab: Redistance of the slab's slices as the whole grid's context would leave them.  Returns
        {"rewritten", "device_ms"}.  RuntimeError (with .rc) on a refusal; the state is then untouched."""
        sl = self.dims[0] * self.dims[1]
        kb, pb, nb = _planes_arg(below, sl)
        ka, pa, na = _planes_arg(above, sl)
        n = C.c_int64(0)
        rc = self._lib.vcy_redistance_slab(self._ctx, pb, nb, pa, na, C.byref(n))
        del kb, ka
        if rc != 0:
            _raise_rc(rc)
        return {"rewritten": int(n.value), "device_ms": self.last_distance_ms()}

    def last_distance_ms(self):
        ms = C.c_float()
        self._lib.vcy_last_distance_ms(self._ctx, C.byref(ms))
        return ms.value

    # -- ray-cast of the hull into views (no reference counterpart; definitions: include/vacancy_hip.h)
    def RenderHull(self, views, iso_level=0.0, voxel_ids=False, axes=False):
        """vcy_render_hull: per view, the first solid voxel (update_num >= 1 and sdf < iso_level) on every pixel's ray.
        `views`: one vcy_view or a list (one launch).  Per view a dict: "depth" (float32 [height, width], camera depth of
        the crossing that entered the voxel, +inf on a miss; depth < inf is the hull's silhouette); with voxel_ids=True
        "voxel" (int64, global voxel id, -1 on a miss); with axes=True "axis" (uint8, 0 / 1 / 2 the entry axis, 3 started
        inside, 255 on a miss).  A single view returns its dict, a list a list."""
        single = isinstance(views, View)
        vs = [views] if single else list(views)
        n = len(vs)
        out = [{"depth": np.empty((v.height, v.width), np.float32)} for v in vs]
        for o, v in zip(out, vs):
            if voxel_ids:
                o["voxel"] = np.empty((v.height, v.width), np.int64)
            if axes:
                o["axis"] = np.empty((v.height, v.width), np.uint8)
        arr = (View * n)(*vs)
        dp = (C.c_void_p * n)(*[o["depth"].ctypes.data for o in out])
        vp = (C.c_void_p * n)(*[o["voxel"].ctypes.data for o in out]) if voxel_ids else None
        ap = (C.c_void_p * n)(*[o["axis"].ctypes.data for o in out]) if axes else None
        if self._lib.vcy_render_hull(self._ctx, iso_level, n, arr, dp, vp, ap) != 0:
            raise RuntimeError(last_error())
        return out[0] if single else out

    def HullAgreement(self, views, masks, iso_level=0.0):
        """vcy_hull_agreement: renders the hull into `views` and compares it with the silhouettes `masks` (non-zero =
        object) on the device.  int64 [n_views, 3]: pixels inside the ROI with (mask and hull, mask and not hull, hull
        and not mask)."""
        vs = list(views)
        n = len(vs)
        ms = [np.ascontiguousarray(m, np.uint8) for m in masks]
        if len(ms) != n or any(m.shape != (v.height, v.width) for m, v in zip(ms, vs)):
            raise ValueError("one height x width silhouette per view")
        arr = (View * n)(*vs)
        mp = (C.c_void_p * n)(*[m.ctypes.data for m in ms])
        counts = np.zeros((n, 3), np.int64)
        if self._lib.vcy_hull_agreement(self._ctx, iso_level, n, arr, mp, _p(counts)) != 0:
            raise RuntimeError(last_error())
        return counts

    def RenderHullSlab(self, views, iso_level=0.0, voxel_ids=False, axes=False, hits=False):
        """vcy_render_hull_slab: RenderHull of the slices this context owns -- the whole-grid image of the state in which
        no voxel outside them is solid (global voxel ids, depths and axes of the global path) --, on any context.  With
        hits=True "hits": uint64 [height, (width + 63) // 64], bit u & 63 of word u >> 6 set where the pixel lies in the
        ROI and hits.  The slabs' images are merged by render_merge_host, their hit bits compared by
        hull_agreement_host."""
        single = isinstance(views, View)
        vs = [views] if single else list(views)
        n = len(vs)
        out = [{"depth": np.empty((v.height, v.width), np.float32)} for v in vs]
        for o, v in zip(out, vs):
            if voxel_ids:
                o["voxel"] = np.empty((v.height, v.width), np.int64)
            if axes:
                o["axis"] = np.empty((v.height, v.width), np.uint8)
            if hits:
                o["hits"] = np.empty((v.height, (v.width + 63) // 64), np.uint64)
        arr = (View * n)(*vs)
        ptrs = [(C.c_void_p * n)(*[o[k].ctypes.data for o in out]) if on else None
                for k, on in (("depth", True), ("voxel", voxel_ids), ("axis", axes), ("hits", hits))]
        if self._lib.vcy_render_hull_slab(self._ctx, iso_level, n, arr, *ptrs) != 0:
            raise RuntimeError(last_error())
        return out[0] if single else out

    def last_render_ms(self):
        ms = C.c_float()
        self._lib.vcy_last_render_ms(self._ctx, C.byref(ms))
        return ms.value

    # -- rasteriser of an indexed mesh (no reference counterpart; definition: include/vacancy_hip.h)
    def RenderMesh(self, vertices, faces, views, depth=True, face=False, hits=False):
        """vcy_raster_mesh: raster_mesh_host on this context's device and stream, the same bits.  The context only names the
        device: its voxel state is not touched, and a z-slab will do.  Dicts as raster_mesh_host's (a single view returns
        its dict), each with the call's device times "raster_ms" and "resolve_ms".  RuntimeError (with .rc) on a refusal."""
        single = isinstance(views, View)
        keep, args, out, dropped = _raster_args(vertices, faces, [views] if single else views, depth, face, hits)
        rc = self._lib.vcy_raster_mesh(self._ctx, *args)
        ms = self.last_raster_ms()
        for o in out:
            o["raster_ms"], o["resolve_ms"] = ms
        return _raster_result(rc, single, out, dropped)

    def MeshAgreement(self, vertices, faces, views, masks):
        """vcy_mesh_agreement: rasterises the mesh into `views` and compares it with the silhouettes `masks` (non-zero =
        object) on the device.  int64 [n_views, 3]: pixels inside the ROI with (mask and mesh, mask and not mesh, mesh and
        not mask) -- HullAgreement's triple for the mesh."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        vs = list(views)
        n = len(vs)
        ms = [np.ascontiguousarray(m, np.uint8) for m in masks]
        if len(ms) != n or any(m.shape != (w.height, w.width) for m, w in zip(ms, vs)):
            raise ValueError("one height x width silhouette per view")
        arr = (View * max(n, 1))(*vs)
        mp = (C.c_void_p * max(n, 1))(*[m.ctypes.data for m in ms])
        counts = np.zeros((n, 3), np.int64)
        if self._lib.vcy_mesh_agreement(self._ctx, len(v), len(f), _p(v), _p(f), n, arr, mp, _p(counts)) != 0:
            raise RuntimeError(last_error())
        return counts

    def last_raster_ms(self):
        ms = [C.c_float(), C.c_float()]
        self._lib.vcy_last_raster_ms(self._ctx, *[C.byref(m) for m in ms])
        return ms[0].value, ms[1].value

    # -- the shading pass behind the rasteriser (no reference counterpart; definition: include/vacancy_hip.h)
    def ShadeMesh(self, vertices, faces, attributes, views, background=None, value=True, value8=False, bary=False):
        """vcy_shade_mesh: shade_mesh_host on this context's device and stream, the same bits.  The context only names the
        device: its voxel state is not touched, and a z-slab will do.  Dicts as shade_mesh_host's (a single view returns its
        dict), each with the call's device times "raster_ms" and "shade_ms".  RuntimeError (with .rc) on a refusal."""
        single = isinstance(views, View)
        keep, args, out = _shade_args(vertices, faces, attributes, [views] if single else views, background, value, value8, bary)
        rc = self._lib.vcy_shade_mesh(self._ctx, *args)
        ms = self.last_shade_ms()
        for o in out:
            o["raster_ms"], o["shade_ms"] = ms
        return _shade_result(rc, single, out)

    def MeshPhotoError(self, vertices, faces, colors, views, photos, masks=None):
        """vcy_mesh_photo_error: mesh_photo_error_host on the device, the same sums; no image is downloaded.  int64
        [n_views, 7]."""
        keep, args, sums = _photo_error_args(vertices, faces, colors, views, photos, masks)
        if self._lib.vcy_mesh_photo_error(self._ctx, *args) != 0:
            raise RuntimeError(last_error())
        return sums

    def last_shade_ms(self):
        ms = [C.c_float(), C.c_float()]
        self._lib.vcy_last_shade_ms(self._ctx, *[C.byref(m) for m in ms])
        return ms[0].value, ms[1].value

    # -- colour of vertices from the photographs (no reference counterpart; definition: include/vacancy_hip.h)
    def ColorVertices(self, vertices, views, photos, normals=None, depth=None, mode=capi.VCY_COLOR_WEIGHTED,
                      interp=capi.VCY_INTERP_BILINEAR, depth_tolerance=None, min_cos=0.0, fallback=(128, 128, 128),
                      iso_level=0.0, mesh_faces=None):
        """vcy_color_vertices: per vertex the mean (VCY_COLOR_MEAN), the mean weighted by |cos| between normal and viewing
        ray (VCY_COLOR_WEIGHTED) or the most frontal sample (VCY_COLOR_BEST) of the photographs of the views that see it.
        A view sees a vertex whose camera depth is at most the hull's depth at its pixel + depth_tolerance (default: 1.5
        voxels).  `depth`: one image per view (RenderHull's, a merged slab render, a sensor's) -- any context will do then;
        None: the hull is ray-cast here at `iso_level` and the depth never leaves the device (whole-grid contexts only).
        `mesh_faces` (without `depth`): the vertices are those of this indexed mesh, and the occlusion comes from the mesh
        itself -- RenderMesh's depth images of (vertices, mesh_faces), passed on as `depth`; any context will do.
        Returns {"rgb": float32 [n, 3] in 0 .. 255, "n_used", "best_view" (-1: none): int32 [n], "device_ms"}."""
        if depth_tolerance is None:
            depth_tolerance = 1.5 * self.option.resolution
        if mesh_faces is not None:
            if depth is not None:
                raise ValueError("depth images or mesh_faces, not both")
            depth = [o["depth"] for o in self.RenderMesh(vertices, mesh_faces, list(views))]
        keep, args, out = _color_args(vertices, views, photos, normals, depth, mode, interp, depth_tolerance, min_cos, fallback)
        if self._lib.vcy_color_vertices(self._ctx, iso_level, *args) != 0:
            raise RuntimeError(last_error())
        ms = C.c_float()
        self._lib.vcy_last_color_ms(self._ctx, C.byref(ms))
        out["device_ms"] = ms.value
        return out

    # -- Taubin smoothing of an indexed mesh (no reference counterpart; definition: include/vacancy_hip.h)
    def SmoothMesh(self, vertices, faces, iterations, lam=0.5, mu=-0.53, pin_boundary=False, normals=False):
        """vcy_smooth_mesh: smooth_mesh_host on this context's device and stream, the same bits.  The context only names the
        device: its voxel state is not touched, and a z-slab will do.  Returns {"vertices"}, with normals=True "normals" and
        "face_normals" (Mesh::CalcNormal of the result), and the device times "build_ms" (incidence table), "passes_ms",
        "normals_ms".  RuntimeError (with .rc) on a refusal."""
        keep, args, out = _smooth_args(vertices, faces, iterations, lam, mu, pin_boundary, normals)
        rc = self._lib.vcy_smooth_mesh(self._ctx, *args)
        if rc != 0:
            e = RuntimeError(last_error())
            e.rc = rc
            raise e
        ms = [C.c_float(), C.c_float(), C.c_float()]
        self._lib.vcy_last_smooth_ms(self._ctx, *[C.byref(m) for m in ms])
        out["build_ms"], out["passes_ms"], out["normals_ms"] = (m.value for m in ms)
        return out

    # -- vertex-clustering decimation of an indexed mesh (no reference counterpart; definition: include/vacancy_hip.h)
    def DecimateMesh(self, vertices, faces, cell, origin=None, mode=capi.VCY_DECIMATE_MEAN, normals=False):
        """vcy_decimate_mesh: decimate_mesh_host on this context's device and stream, the same bits.  `origin` defaults to
        the carver's bb_min, so the cells line up with the voxels.  The context only names the device: its voxel state is
        not touched, and a z-slab will do.  Returns decimate_mesh_host's dict plus the device times "cluster_ms",
        "faces_ms", "emit_ms", "normals_ms".  RuntimeError (with .rc) on a refusal."""
        if origin is None:
            origin = tuple(self.option.bb_min)
        keep, args, out = _decimate_args(vertices, faces, cell, origin, mode, normals)
        out = _decimate_result(self._lib.vcy_decimate_mesh(self._ctx, *args), keep, out)
        ms = [C.c_float() for _ in range(4)]
        self._lib.vcy_last_decimate_ms(self._ctx, *[C.byref(m) for m in ms])
        out["cluster_ms"], out["faces_ms"], out["emit_ms"], out["normals_ms"] = (m.value for m in ms)
        return out

    def DecimateMeshQuadric(self, vertices, faces, cell, origin=None, regularize=1e-3, normals=False):
        """vcy_decimate_mesh_quadric: decimate_mesh_quadric_host on this context's device and stream, the same bits, under
        DecimateMesh's terms.  Returns its dict (with "n_fallback") plus DecimateMesh's four device times and "quadric_ms",
        the quadric stage alone (it is part of "cluster_ms")."""
        if origin is None:
            origin = tuple(self.option.bb_min)
        keep, args, out = _quadric_args(vertices, faces, cell, origin, regularize, normals)
        out = _quadric_result(self._lib.vcy_decimate_mesh_quadric(self._ctx, *args), keep, out)
        ms = [C.c_float() for _ in range(5)]
        self._lib.vcy_last_decimate_ms(self._ctx, *[C.byref(m) for m in ms[:4]])
        self._lib.vcy_last_quadric_ms(self._ctx, C.byref(ms[4]))
        out["cluster_ms"], out["faces_ms"], out["emit_ms"], out["normals_ms"], out["quadric_ms"] = (m.value for m in ms)
        return out

    # -- extract, smooth, decimate and normals in one call, the mesh staying on the device (definition: include/vacancy_hip.h)
    CHAIN_MS = ("extract_ms", "table_ms", "passes_ms", "cluster_ms", "quadric_ms", "faces_emit_ms", "normals_ms", "wall_ms")

    def chain_option(self, smooth=None, decimate=None, normals=True, maps=False):
        """The vcy_chain_option of ExtractIsoChain's arguments.  smooth: None or a dict of SmoothMesh's keywords
        (iterations, lam, mu, pin_boundary).  decimate: None or a dict with cell and either mode (DecimateMesh) or
        regularize (DecimateMeshQuadric), and optionally origin (default: the carver's bb_min)."""
        o = capi.ChainOption()
        if smooth is not None:
            o.smooth = 1
            o.smooth_option = SmoothOption(int(smooth["iterations"]), float(smooth.get("lam", 0.5)), float(smooth.get("mu", -0.53)),
                                           int(smooth.get("pin_boundary", False)))
        if decimate is not None:
            quadric = "regularize" in decimate
            o.decimate = 2 if quadric else 1
            origin = decimate.get("origin")
            origin = tuple(self.option.bb_min) if origin is None else origin
            o.decimate_option = DecimateOption(float(decimate["cell"]), [float(x) for x in origin],
                                               int(decimate.get("mode", capi.VCY_DECIMATE_MEAN)))
            o.regularize = float(decimate["regularize"]) if quadric else 0.0
        o.which = (capi.VCY_NORMALS_VERTEX | capi.VCY_NORMALS_FACE) if normals else 0
        o.maps = int(bool(maps))
        return o

    def ExtractIsoChain(self, iso_level=0.0, linear_interp=True, smooth=None, decimate=None, normals=True, maps=False):
        """vcy_extract_iso_chain: the bits of ExtractIsoSurface -> SmoothMesh -> DecimateMesh[Quadric] -> normals of the last
        mesh, without the mesh leaving the device in between (arguments: chain_option).  Needs a whole-grid context with
        "meshkeys" 0.  Returns {"vertices", "faces"}, with normals "normals" and "face_normals", with a decimation and
        maps=True "vertex_map" and "face_source" (numbered by the extracted mesh), with quadric representatives
        "n_fallback", then "extracted": (vertices, faces) of the extracted mesh and the times of CHAIN_MS.  RuntimeError
        (with .rc) on a refusal."""
        o = self.chain_option(smooth, decimate, normals, maps)
        m, mn, rep = Mesh(), capi.MeshNormals(), capi.ChainReport()
        rc = self._lib.vcy_extract_iso_chain(self._ctx, iso_level, int(linear_interp), C.byref(o), C.byref(m), C.byref(mn),
                                             C.byref(rep))
        if rc != 0:
            e = RuntimeError(last_error())
            e.rc = rc
            raise e
        nv, nf = m.n_vertices, m.n_faces
        out = {"vertices": _mesh_array(m.vertices, nv, 3, np.float32), "faces": _mesh_array(m.faces, nf, 3, np.int32)}
        if normals:
            out["normals"] = _mesh_array(mn.vertex_normals, nv, 3, np.float32)
            out["face_normals"] = _mesh_array(mn.face_normals, nf, 3, np.float32)
        out["extracted"] = (int(rep.n_extracted_vertices), int(rep.n_extracted_faces))
        if o.decimate and maps:
            out["vertex_map"] = (_mesh_array(rep.vertex_map, out["extracted"][0], 1, np.int32).reshape(-1)
                                 if rep.vertex_map else np.full(out["extracted"][0], -1, np.int32))
            out["face_source"] = _mesh_array(rep.face_source, nf, 1, np.int32).reshape(-1)
        if o.decimate == 2:
            out["n_fallback"] = int(rep.n_fallback)
        self._lib.vcy_mesh_free(C.byref(m))
        self._lib.vcy_mesh_normals_free(C.byref(mn))
        self._lib.vcy_chain_report_free(C.byref(rep))
        ms = [C.c_float() for _ in self.CHAIN_MS]
        self._lib.vcy_last_chain_ms(self._ctx, *[C.byref(x) for x in ms])
        for key, x in zip(self.CHAIN_MS, ms):
            out[key] = x.value
        return out

    # -- state access
    def download(self):
        n = self.slab_voxels
        s = np.empty(n, np.float32)
        u = np.empty(n, np.int32)
        rc = self._lib.vcy_download(self._ctx, _p(s), _p(u))
        if rc != 0:
            raise RuntimeError(last_error())
        return s, u

    def upload(self, sdf, update_num):
        s = np.ascontiguousarray(sdf, np.float32)
        u = np.ascontiguousarray(update_num, np.int32)
        rc = self._lib.vcy_upload(self._ctx, _p(s), _p(u))
        if rc != 0:
            raise RuntimeError(last_error())

    def positions(self):
        p = np.empty((self.slab_voxels, 3), np.float32)
        rc = self._lib.vcy_download_positions(self._ctx, _p(p))
        if rc != 0:
            raise RuntimeError(last_error())
        return p

    # -- halo staging through the host (gloo path of vacancy_amd.dist)
    def halo_pack_host(self):
        import ctypes as C_
        nbytes = int(self._lib.vcy_halo_bytes(self._ctx))
        dev = C_.c_void_p()
        host = np.empty(nbytes, np.uint8)
        rc = self._lib.vcy_device_alloc(self._ctx, nbytes, C_.byref(dev))
        assert rc == 0, last_error()
        assert self._lib.vcy_halo_pack(self._ctx, dev) == 0, last_error()
        assert self._lib.vcy_memcpy_d2h(self._ctx, _p(host), dev, nbytes) == 0, last_error()
        self._lib.vcy_device_free(self._ctx, dev)
        return host

    def halo_unpack_host(self, gathered, rank, world):
        import ctypes as C_
        gathered = np.ascontiguousarray(gathered, np.uint8)
        dev = C_.c_void_p()
        assert self._lib.vcy_device_alloc(self._ctx, gathered.nbytes, C_.byref(dev)) == 0, last_error()
        assert self._lib.vcy_memcpy_h2d(self._ctx, dev, _p(gathered), gathered.nbytes) == 0, last_error()
        assert self._lib.vcy_halo_unpack(self._ctx, dev, rank, world) == 0, last_error()
        self._lib.vcy_device_free(self._ctx, dev)

    def halo_install_host(self, pack):
        import ctypes as C_
        pack = np.ascontiguousarray(pack, np.uint8)
        dev = C_.c_void_p()
        assert self._lib.vcy_device_alloc(self._ctx, pack.nbytes, C_.byref(dev)) == 0, last_error()
        assert self._lib.vcy_memcpy_h2d(self._ctx, dev, _p(pack), pack.nbytes) == 0, last_error()
        assert self._lib.vcy_halo_install(self._ctx, dev) == 0, last_error()
        self._lib.vcy_device_free(self._ctx, dev)

    def state_diff(self, other):
        """Number of voxels whose (sdf bits, update_num) differ from `other` (same slab, same device);
        compared on the device (vcy_state_equal), nothing is downloaded."""
        n = C.c_int64(-1)
        if self._lib.vcy_state_equal(self._ctx, other._ctx, C.byref(n)) != 0:
            raise RuntimeError(last_error())
        return int(n.value)

    def use_stream_of(self, other):
        """Launch on another context's stream (several slabs of one GPU in sequence)."""
        st = C.c_void_p()
        assert self._lib.vcy_get_stream(other._ctx, C.byref(st)) == 0, last_error()
        assert self._lib.vcy_set_stream(self._ctx, st) == 0, last_error()

    def set_param(self, name, value):
        assert self._lib.vcy_set_param(self._ctx, name.encode(), int(value)) == 0, last_error()

    def get_param(self, name):
        v = C.c_int()
        assert self._lib.vcy_get_param(self._ctx, name.encode(), C.byref(v)) == 0, last_error()
        return v.value

    def reset(self):
        """Back to the state right after Init(): sdf = lowest(), update_num = 0."""
        assert self._lib.vcy_reset(self._ctx) == 0, last_error()

    def sync(self):
        self._lib.vcy_sync(self._ctx)

    def selftest(self):
        """vcy_selftest: device-side identities behind the fast paths; True when all hold."""
        return self._lib.vcy_selftest(self._ctx) == 0

    def last_carve_ms(self):
        """(pre-pass ms, carve kernel ms) of the last fused launch; needs set_param("carvetimer", 1)."""
        a, b = C.c_float(), C.c_float()
        assert self._lib.vcy_last_carve_ms(self._ctx, C.byref(a), C.byref(b)) == 0, last_error()
        return a.value, b.value

    def last_carve_pairs(self):
        """(processed, total, per-layer array) of the last fused launch; needs set_param("paircount", 1)."""
        a, b, n = C.c_int64(), C.c_int64(), C.c_int()
        per = np.zeros(4096, np.int64)
        rc = self._lib.vcy_last_carve_pairs(self._ctx, C.byref(a), C.byref(b), _p(per), len(per), C.byref(n))
        if rc != 0:
            raise RuntimeError(last_error())
        return int(a.value), int(b.value), per[: n.value].copy()

    def plan_z_slabs(self, views, sdf_devs, n_slabs, stride=0, brick_cost=0.0):
        """vcy_plan_z_slabs: (z_bounds [n_slabs + 1], layer_cost [brick layers of the grid]) for a fused carve of these
        views; `views, sdf_devs` as for CarveBatchDevice (or a prepared batch as `views`)."""
        n, arr, ptrs = views if sdf_devs is None else self.prepare_batch(views, sdf_devs)
        bounds = np.zeros(n_slabs + 1, np.int32)
        cost = np.zeros(8192, np.float64)
        nl = C.c_int()
        rc = self._lib.vcy_plan_z_slabs(self._ctx, n, arr, ptrs, int(n_slabs), int(stride), float(brick_cost),
                                        _p(bounds), _p(cost), len(cost), C.byref(nl))
        if rc != 0:
            raise RuntimeError(last_error())
        return [int(z) for z in bounds], cost[: nl.value].copy()

    def carve_log(self, clear=True, max_records=8192):
        """[(begin_ms, prepass_ms, kernel_ms, first_chunk)] of every chunk of every fused launch since "carvetimer" was
        set / the log was cleared (vcy_carve_log); waits for those launches, nothing synchronised in between."""
        b = np.empty(max_records, np.float32)
        p = np.empty(max_records, np.float32)
        k = np.empty(max_records, np.float32)
        f = np.empty(max_records, np.int32)
        n = C.c_int(0)
        rc = self._lib.vcy_carve_log(self._ctx, max_records, _p(b), _p(p), _p(k), _p(f), C.byref(n), int(clear))
        assert rc == 0, last_error()
        return [(float(b[i]), float(p[i]), float(k[i]), int(f[i])) for i in range(n.value)]

    def timer_begin(self):
        self._lib.vcy_timer_begin(self._ctx)

    def timer_end(self):
        ms = C.c_float()
        self._lib.vcy_timer_end(self._ctx, C.byref(ms))
        return ms.value


_COMPONENT_REC = np.dtype([("label", np.int64), ("n_voxels", np.int64), ("bb_min", np.int32, 3), ("bb_max", np.int32, 3)])
assert _COMPONENT_REC.itemsize == C.sizeof(capi.Component)


def cell_planes(option, axis):
    """vcy_cell_planes: the dims[axis] + 1 planes between the cells of one axis (float32), host arithmetic, no GPU."""
    lib = capi.load()
    dims = (C.c_int32 * 3)()
    if lib.vcy_compute_dims(option.bb_min, option.bb_max, option.resolution, dims) != 0:
        raise RuntimeError(last_error())
    out = np.empty(max(int(dims[axis]), 0) + 1, np.float32)
    if lib.vcy_cell_planes(option.bb_min, option.bb_max, option.resolution, int(axis), _p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def components_to_dict(p, n):
    """A library-owned vcy_component list as the dict of arrays LabelComponents returns; frees the list."""
    if n:
        arr = np.frombuffer(C.string_at(p, n * _COMPONENT_REC.itemsize), _COMPONENT_REC)
        capi.load().vcy_components_free(p)
    else:
        arr = np.zeros(0, _COMPONENT_REC)
    return {k: np.ascontiguousarray(arr[k]) for k in ("label", "n_voxels", "bb_min", "bb_max")}


def merge_components_host(lists, pairs):
    """vcy_merge_components_host (no GPU): `lists` = the slabs' LabelComponentsSlab dicts in z order, `pairs` = the seams'
    int64 [n, 2] arrays (one fewer).  Returns (merged dict, [merged label of every piece of slab s])."""
    lib = capi.load()
    ns = len(lists)
    if len(pairs) != max(0, ns - 1):
        raise ValueError("%d slabs have %d seams, not %d" % (ns, max(0, ns - 1), len(pairs)))
    counts = np.array([len(l["label"]) for l in lists], np.int64)
    flat = np.zeros(int(counts.sum()), _COMPONENT_REC)
    at = 0
    for l in lists:
        k = len(l["label"])
        for key in ("label", "n_voxels", "bb_min", "bb_max"):
            flat[key][at:at + k] = l[key]
        at += k
    pr = [np.ascontiguousarray(q, np.int64).reshape(-1, 2) for q in pairs]
    pcounts = np.array([len(q) for q in pr], np.int64)
    pflat = np.ascontiguousarray(np.concatenate(pr).reshape(-1) if pr else np.zeros(0, np.int64))
    glob = np.full(len(flat), -1, np.int64)
    p, n = C.POINTER(capi.Component)(), C.c_int64(0)
    rc = lib.vcy_merge_components_host(ns, _p(flat), _p(counts), _p(pflat), _p(pcounts), C.byref(p), C.byref(n), _p(glob))
    if rc != 0:
        e = RuntimeError(last_error())
        e.rc = rc
        raise e
    ends = np.cumsum(counts)
    return components_to_dict(p, n.value), [glob[e - k:e].copy() for e, k in zip(ends, counts)]


def carve_batch_silhouettes_sharded(carvers, views, silhouettes):
    """vcy_carve_batch_silhouettes_sharded: the slabs of one grid held by THIS process carve `views` from silhouettes
    in host memory; the devices share the producer (device r builds the SDFs of views r, r + R, ... of every chunk, one
    RCCL all-gather per chunk hands every device all of them)."""
    lib = capi.load()
    n = len(views)
    arr = (View * n)(*views)
    masks = [np.ascontiguousarray(m, np.uint8) for m in silhouettes]
    ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in masks])
    ctxs = (C.c_void_p * len(carvers))(*[c.ctx for c in carvers])
    rc = lib.vcy_carve_batch_silhouettes_sharded(ctxs, len(carvers), n, arr, ptrs)
    if rc != 0:
        e = RuntimeError(last_error())
        e.rc = rc
        raise e
    return True


def voxel_cubes(option, ids):
    """vcy_voxel_cubes: the serial half of ExtractVoxel (extract_voxel.cc:290-311) for kept voxel ids in scan order --
    host arithmetic, no GPU."""
    lib = capi.load()
    ids = np.ascontiguousarray(ids, np.int64)
    m = Mesh()
    rc = lib.vcy_voxel_cubes(C.byref(option), len(ids), _p(ids), C.byref(m))
    if rc != 0:
        lib.vcy_mesh_free(C.byref(m))
        raise RuntimeError(last_error())
    out = {"vertices": _mesh_array(m.vertices, m.n_vertices, 3, np.float32),
           "faces": _mesh_array(m.faces, m.n_faces, 3, np.int32)}
    lib.vcy_mesh_free(C.byref(m))
    return out


def voxel_cubes_into(option, ids):
    """vcy_voxel_cubes_into: as voxel_cubes, into numpy arrays allocated by the callback."""
    lib = capi.load()
    ids = np.ascontiguousarray(ids, np.int64)
    got = {"vertices": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int32), "calls": 0}

    def provide(user, nv, nf, pv, pf):
        got["calls"] += 1
        got["vertices"] = np.empty((nv, 3), np.float32)
        got["faces"] = np.empty((nf, 3), np.int32)
        pv[0] = got["vertices"].ctypes.data_as(C.POINTER(C.c_float))
        pf[0] = got["faces"].ctypes.data_as(C.POINTER(C.c_int32))
        return 0

    cb = capi.MeshArraysFn(provide)
    rc = lib.vcy_voxel_cubes_into(C.byref(option), len(ids), _p(ids), cb, None)
    if rc != 0:
        raise RuntimeError(last_error())
    return got


def halo_allgather(carvers):
    """All z-slabs of one grid held by THIS process, in z order: one native RCCL all-gather
    (vcy_halo_allgather) installs every slab's two halo slices."""
    lib = capi.load()
    arr = (C.c_void_p * len(carvers))(*[c.ctx for c in carvers])
    rc = lib.vcy_halo_allgather(arr, len(carvers))
    if rc != 0:
        e = RuntimeError(last_error())
        e.rc = rc
        raise e
    return lib.vcy_last_collective().decode()


def halo_exchange(carvers):
    """halo_allgather, or -- only when the library reports that librccl cannot be loaded at all
    (VCY_ERR_UNSUPPORTED) -- the explicit alternative: peer-to-peer copies slab by slab
    (vcy_halo_copy_from).  Returns what was done as a dict for the benchmark record."""
    lib = capi.load()
    try:
        text = halo_allgather(carvers)
    except RuntimeError as e:
        if getattr(e, "rc", 0) != capi.VCY_ERR_UNSUPPORTED:
            raise
        nbytes = 0
        for below, c in zip([None] + list(carvers[:-1]), carvers):
            if lib.vcy_halo_copy_from(c.ctx, below.ctx if below is not None else None) != 0:
                raise RuntimeError(last_error())
            nbytes += int(lib.vcy_halo_bytes(c.ctx)) if below is not None else 0
        return {"backend": "peer copies (vcy_halo_copy_from): librccl could not be loaded", "op": "hipMemcpyPeerAsync",
                "ranks": len({c._device for c in carvers}), "bytes_total": nbytes, "slabs": len(carvers),
                "note": str(e)[:160]}
    info = dict(kv.split("=", 1) for kv in text.split() if "=" in kv)
    ranks, per = int(info.get("ranks", 0)), int(info.get("bytes_per_rank", 0))
    # an all-gather hands EVERY rank every pack (ranks * bytes_per_rank received per rank) although a slab only needs
    # the pack of the slab below it: what the north star asks for, and small next to the state (10 MiB per slab at 1024^2)
    return {"backend": "rccl (native, vcy_halo_allgather)", "op": info.get("op"), "ranks": ranks,
            "bytes_per_rank": per, "bytes_received_per_rank": per * ranks,
            "bytes_needed_per_slab": int(capi.load().vcy_halo_bytes(carvers[0].ctx)),
            "rccl_version": int(info.get("version", 0)), "slabs": len(carvers)}


class ClockProbe:
    """Shader clock of the device while other work runs on it (vcy_clock_probe_*): one wave on a stream of its own
    samples the clock counter against the 100 MHz reference until stop().  `with ClockProbe(dev) as p: ...; p.result`."""

    def __init__(self, device_id=0, max_samples=1 << 16):
        self._lib = capi.load()
        self._p = C.c_void_p()
        self.result = None
        if self._lib.vcy_clock_probe_start(int(device_id), int(max_samples), C.byref(self._p)) != 0:
            raise RuntimeError("vcy_clock_probe_start: " + last_error())

    def stop(self):
        if self._p:
            mean, settled, lo, hi, cov, n = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int()
            rc = self._lib.vcy_clock_probe_stop(self._p, C.byref(mean), C.byref(settled), C.byref(lo), C.byref(hi), C.byref(n),
                                                C.byref(cov))
            self._p = C.c_void_p()
            if rc != 0:
                raise RuntimeError("vcy_clock_probe_stop: " + last_error())
            self.result = {"mean_hz": mean.value, "settled_hz": settled.value, "min_hz": lo.value, "max_hz": hi.value, "samples": n.value,
                           "covered_ms": cov.value}
        return self.result

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.stop()
        return False

    def __del__(self):  # a probe that is dropped must not keep its wave resident (it also ends by itself after 2 s)
        try:
            self.stop()
        except Exception:
            pass


def measure_bandwidth(device_id=0, nbytes=1 << 31, reps=3):
    """(read GB/s, device-to-device copy GB/s) measured on this GPU (vcy_measure_bandwidth)."""
    lib = capi.load()
    rd, cp = C.c_double(), C.c_double()
    rc = lib.vcy_measure_bandwidth(int(device_id), int(nbytes), int(reps), C.byref(rd), C.byref(cp))
    if rc != 0:
        raise RuntimeError("vcy_measure_bandwidth: " + last_error())
    return rd.value, cp.value


def make_sdf(mask, roi_min=None, roi_max=None, normalize=True, use_truncation=False, band=0.1):
    """MakeSignedDistanceField (voxel_carver.cc:169-237) through the C-ABI."""
    lib = capi.load()
    mask = np.ascontiguousarray(mask, np.uint8)
    h, w = mask.shape
    rmin = (C.c_int32 * 2)(*(roi_min or (0, 0)))
    rmax = (C.c_int32 * 2)(*(roi_max or (w - 1, h - 1)))
    out = np.empty((h, w), np.float32)
    rc = lib.vcy_make_sdf(_p(mask), w, h, rmin, rmax, int(normalize), int(use_truncation), band, _p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def distance_transform_l1(mask, roi_min=None, roi_max=None):
    lib = capi.load()
    mask = np.ascontiguousarray(mask, np.uint8)
    h, w = mask.shape
    rmin = (C.c_int32 * 2)(*(roi_min or (0, 0)))
    rmax = (C.c_int32 * 2)(*(roi_max or (w - 1, h - 1)))
    out = np.empty((h, w), np.float32)
    rc = lib.vcy_distance_transform_l1(_p(mask), w, h, rmin, rmax, _p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def render_merge_host(view, parts):
    """vcy_render_merge_host: the slabs' images of one view (RenderHullSlab dicts in ascending z; "voxel" is required,
    "depth" and "axis" are merged when every slab has them) merged into the whole grid's: the hit of the first slab in
    the ray's direction of travel along z that has one.  No GPU."""
    lib = capi.load()
    n = len(parts)
    if n == 0 or any("voxel" not in p for p in parts):
        raise ValueError("render_merge_host needs the voxel ids of at least one slab")
    shape = (view.height, view.width)
    keep = {k: [np.ascontiguousarray(p[k], t) for p in parts] for k, t in
            (("depth", np.float32), ("voxel", np.int64), ("axis", np.uint8)) if all(k in p for p in parts)}
    if any(a.shape != shape for arrs in keep.values() for a in arrs):
        raise ValueError("every slab image is height x width of the view")
    out = {k: np.empty(shape, arrs[0].dtype) for k, arrs in keep.items()}
    ptr = {k: (C.c_void_p * n)(*[a.ctypes.data for a in arrs]) for k, arrs in keep.items()}
    if lib.vcy_render_merge_host(C.byref(view), n, ptr.get("depth"), ptr["voxel"], ptr.get("axis"),
                                 _p(out["depth"]) if "depth" in out else None, _p(out["voxel"]),
                                 _p(out["axis"]) if "axis" in out else None) != 0:
        raise RuntimeError(last_error())
    return out


def hull_agreement_host(view, hits, mask):
    """vcy_hull_agreement_host: int64 [3] = pixels inside the ROI with (mask and hull, mask and not hull, hull and not
    mask), the hull being the OR of the slabs' hit bits (`hits`: uint64 [height, (width + 63) // 64] per slab).  No GPU."""
    lib = capi.load()
    hs = [np.ascontiguousarray(h, np.uint64) for h in hits]
    m = np.ascontiguousarray(mask, np.uint8)
    if not hs or any(h.shape != (view.height, (view.width + 63) // 64) for h in hs) or m.shape != (view.height, view.width):
        raise ValueError("hit bits of height x (width + 63) // 64 words per slab and a height x width silhouette")
    counts = np.zeros(3, np.int64)
    hp = (C.c_void_p * len(hs))(*[h.ctypes.data for h in hs])
    if lib.vcy_hull_agreement_host(C.byref(view), len(hs), hp, _p(m), _p(counts)) != 0:
        raise RuntimeError(last_error())
    return counts
