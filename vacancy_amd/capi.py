"""ctypes mirror of include/vacancy_hip.h (POD structs + the loader of libvacancy_hip.so).

The product path has no CPU fallback: `load()` raises if the HIP library is missing, and
`vcy_create` fails if no GPU is usable.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VCY_HIP_LIB: another build of the same library (kernel variants under development, profiles/tools/build_variant.sh)
LIB_PATH = os.environ.get("VCY_HIP_LIB") or os.path.join(_HERE, "csrc", "libvacancy_hip.so")

# vcy_status (include/vacancy_hip.h)
VCY_OK, VCY_ERR_INVALID_ARG, VCY_ERR_NOT_INITIALIZED, VCY_ERR_TOO_MANY_VOXELS = 0, -1, -2, -3
VCY_ERR_HIP, VCY_ERR_NO_DEVICE, VCY_ERR_UNSUPPORTED, VCY_ERR_INTERNAL = -4, -5, -6, -7
VCY_UPDATE_MAX, VCY_UPDATE_WEIGHTED_AVERAGE = 0, 1
VCY_INTERP_NN, VCY_INTERP_BILINEAR = 0, 1
VCY_OUTSIDE_NONE, VCY_OUTSIDE_MAX = 0, 1


class UpdateOption(C.Structure):
    """vacancy::VoxelUpdateOption (reference include/vacancy/voxel_carver.h:43-52)."""
    _fields_ = [
        ("voxel_update", C.c_int32),
        ("sdf_interp", C.c_int32),
        ("update_outside", C.c_int32),
        ("voxel_max_update_num", C.c_int32),
        ("voxel_update_weight", C.c_float),
        ("use_truncation", C.c_int32),
        ("truncation_band", C.c_float),
    ]

    def __init__(self, voxel_update=VCY_UPDATE_MAX, sdf_interp=VCY_INTERP_BILINEAR,
                 update_outside=VCY_OUTSIDE_NONE, voxel_max_update_num=255,
                 voxel_update_weight=1.0, use_truncation=False, truncation_band=0.1):
        super().__init__(voxel_update, sdf_interp, update_outside, voxel_max_update_num,
                         voxel_update_weight, int(bool(use_truncation)), truncation_band)


class CarverOption(C.Structure):
    """vacancy::VoxelCarverOption (voxel_carver.h:54-60)."""
    _fields_ = [
        ("bb_max", C.c_float * 3),
        ("bb_min", C.c_float * 3),
        ("resolution", C.c_float),
        ("sdf_minmax_normalize", C.c_int32),
        ("update_option", UpdateOption),
    ]

    def __init__(self, bb_min=(0, 0, 0), bb_max=(1, 1, 1), resolution=0.1,
                 sdf_minmax_normalize=True, update_option=None):
        super().__init__()
        self.bb_max = (C.c_float * 3)(*bb_max)
        self.bb_min = (C.c_float * 3)(*bb_min)
        self.resolution = resolution
        self.sdf_minmax_normalize = int(bool(sdf_minmax_normalize))
        self.update_option = update_option if update_option is not None else UpdateOption()


class View(C.Structure):
    """What Carve() reads from the camera + ROI (see vcy_view in vacancy_hip.h)."""
    _fields_ = [
        ("w2c", C.c_float * 12),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("is_ortho", C.c_int32),
        ("roi_min", C.c_int32 * 2),
        ("roi_max", C.c_int32 * 2),
        ("width", C.c_int32), ("height", C.c_int32),
    ]


class Mesh(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_int64),
        ("n_faces", C.c_int64),
        ("vertices", C.POINTER(C.c_float)),
        ("faces", C.POINTER(C.c_int32)),
        ("edge_keys", C.POINTER(C.c_int64)),
        ("n_foreign_vertices", C.c_int64),
    ]


class MeshNormals(C.Structure):
    """vcy_mesh_normals: what vcy_extract_iso_normals returns next to the Mesh."""
    _fields_ = [
        ("vertex_normals", C.POINTER(C.c_float)),
        ("face_normals", C.POINTER(C.c_float)),
    ]


VCY_NORMALS_VERTEX, VCY_NORMALS_FACE = 1, 2
VCY_COLOR_MEAN, VCY_COLOR_WEIGHTED, VCY_COLOR_BEST = 0, 1, 2


class ColorOption(C.Structure):
    """vcy_color_option: how vcy_color_vertices combines the views that see a vertex."""
    _fields_ = [
        ("mode", C.c_int32),
        ("interp", C.c_int32),
        ("depth_tolerance", C.c_float),
        ("min_cos", C.c_float),
        ("fallback", C.c_float * 3),
    ]

    def __init__(self, mode=VCY_COLOR_WEIGHTED, interp=VCY_INTERP_BILINEAR, depth_tolerance=0.0, min_cos=0.0,
                 fallback=(128.0, 128.0, 128.0)):
        super().__init__(mode, interp, depth_tolerance, min_cos, (C.c_float * 3)(*fallback))


class ShadeOption(C.Structure):
    """vcy_shade_option: floats per vertex and the value of a pixel without a winner (vcy_shade_mesh)."""
    _fields_ = [
        ("channels", C.c_int32),
        ("background", C.c_float * 4),
    ]

    def __init__(self, channels=3, background=(0.0, 0.0, 0.0, 0.0)):
        bg = [float(x) for x in background] + [0.0] * 4
        super().__init__(channels, (C.c_float * 4)(*bg[:4]))


class SmoothOption(C.Structure):
    """vcy_smooth_option: the passes of vcy_smooth_mesh (one iteration = a lambda pass, then a mu pass)."""
    _fields_ = [
        ("iterations", C.c_int32),
        ("lam", C.c_float),
        ("mu", C.c_float),
        ("pin_boundary", C.c_int32),
    ]


VCY_DECIMATE_MEAN, VCY_DECIMATE_NEAREST, VCY_DECIMATE_FIRST = 0, 1, 2


class DecimateOption(C.Structure):
    """vcy_decimate_option: the cell lattice and the representative of vcy_decimate_mesh."""
    _fields_ = [
        ("cell", C.c_float),
        ("origin", C.c_float * 3),
        ("mode", C.c_int32),
    ]

    def __init__(self, cell=1.0, origin=(0.0, 0.0, 0.0), mode=0):
        super().__init__(cell, (C.c_float * 3)(*origin), mode)


class ChainOption(C.Structure):
    """vcy_chain_option: the stages of vcy_extract_iso_chain."""
    _fields_ = [
        ("smooth", C.c_int32),
        ("smooth_option", SmoothOption),
        ("decimate", C.c_int32),
        ("decimate_option", DecimateOption),
        ("regularize", C.c_float),
        ("which", C.c_int32),
        ("maps", C.c_int32),
    ]


class ChainReport(C.Structure):
    """vcy_chain_report: the extracted mesh's counts, the fallbacks and the decimation's maps (vcy_chain_report_free)."""
    _fields_ = [
        ("n_extracted_vertices", C.c_int64),
        ("n_extracted_faces", C.c_int64),
        ("n_fallback", C.c_int64),
        ("vertex_map", C.POINTER(C.c_int32)),
        ("face_source", C.POINTER(C.c_int32)),
    ]


class Component(C.Structure):
    """vcy_component: one 6-connected component of the solid voxels (vcy_label_components)."""
    _fields_ = [
        ("label", C.c_int64),
        ("n_voxels", C.c_int64),
        ("bb_min", C.c_int32 * 3),
        ("bb_max", C.c_int32 * 3),
    ]


# vcy_mesh_arrays_fn: int (*)(void* user, int64 n_vertices, int64 n_faces, float** vertices, int32** faces)
MeshArraysFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.POINTER(C.c_float)),
                           C.POINTER(C.POINTER(C.c_int32)))


def make_view(w2c_f32, fx, fy, cx, cy, width, height, roi_min=None, roi_max=None, is_ortho=False):
    v = View()
    flat = [float(x) for x in list(w2c_f32.reshape(-1))]
    assert len(flat) == 12
    v.w2c = (C.c_float * 12)(*flat)
    v.fx, v.fy, v.cx, v.cy = fx, fy, cx, cy
    v.is_ortho = int(bool(is_ortho))
    rmin = roi_min if roi_min is not None else (0, 0)
    rmax = roi_max if roi_max is not None else (width - 1, height - 1)
    v.roi_min = (C.c_int32 * 2)(*rmin)
    v.roi_max = (C.c_int32 * 2)(*rmax)
    v.width, v.height = width, height
    return v


_lib = None


def load():
    """Load libvacancy_hip.so (built by __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "vacancy_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'`."
            " There is no CPU fallback for the carving path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    P = C.POINTER
    vp = C.c_void_p
    sig = {
        "vcy_create": (C.c_int, [P(CarverOption), C.c_int, C.c_int, C.c_int, P(vp)]),
        "vcy_destroy": (None, [vp]),
        "vcy_grid_dims": (C.c_int, [vp, P(C.c_int32)]),
        "vcy_slab_range": (C.c_int, [vp, P(C.c_int32)]),
        "vcy_compute_dims": (C.c_int, [P(C.c_float), P(C.c_float), C.c_float, P(C.c_int32)]),
        "vcy_axis_positions": (C.c_int, [P(C.c_float), P(C.c_float), C.c_float, C.c_int, vp]),
        "vcy_carve": (C.c_int, [vp, P(View), vp]),
        "vcy_carve_device": (C.c_int, [vp, P(View), vp]),
        "vcy_carve_batch_device": (C.c_int, [vp, C.c_int, P(View), P(vp)]),
        "vcy_carve_silhouette": (C.c_int, [vp, P(View), vp, vp]),
        "vcy_carve_batch_silhouettes": (C.c_int, [vp, C.c_int, P(View), P(vp)]),
        "vcy_carve_batch_silhouettes_sharded": (C.c_int, [P(vp), C.c_int, C.c_int, P(View), P(vp)]),
        "vcy_make_sdf_batch_device": (C.c_int, [vp, C.c_int, P(View), P(vp), P(vp)]),
        "vcy_carve_robust_device": (C.c_int, [vp, C.c_int, P(View), P(vp), C.c_int, C.c_double, vp]),
        "vcy_carve_robust_silhouettes": (C.c_int, [vp, C.c_int, P(View), P(vp), C.c_int, C.c_double, vp]),
        "vcy_last_robust_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_carve_depth_device": (C.c_int, [vp, C.c_int, P(View), P(vp), C.c_float]),
        "vcy_carve_depth": (C.c_int, [vp, C.c_int, P(View), P(vp), C.c_float]),
        "vcy_carve_depth_host": (C.c_int, [P(CarverOption), C.c_int, C.c_int, C.c_int, P(View), P(vp), C.c_float, vp, vp]),
        "vcy_last_depth_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_download_voxels": (C.c_int, [vp, C.c_int64, vp, vp, vp]),
        "vcy_distance_transform_l1": (C.c_int, [vp, C.c_int, C.c_int, P(C.c_int32), P(C.c_int32), vp]),
        "vcy_make_sdf": (C.c_int, [vp, C.c_int, C.c_int, P(C.c_int32), P(C.c_int32),
                                   C.c_int, C.c_int, C.c_float, vp]),
        "vcy_make_sdf_device": (C.c_int, [vp, vp, C.c_int, C.c_int, P(C.c_int32), P(C.c_int32),
                                          C.c_int, C.c_int, C.c_float, P(vp)]),
        "vcy_extract_iso": (C.c_int, [vp, C.c_double, C.c_int, P(Mesh)]),
        "vcy_extract_iso_normals": (C.c_int, [vp, C.c_double, C.c_int, C.c_int, P(Mesh), P(MeshNormals)]),
        "vcy_extract_iso_normals_slab": (C.c_int, [vp, C.c_double, C.c_int, C.c_int, P(Mesh), P(MeshNormals),
                                                   P(C.c_int64)]),
        "vcy_mesh_normals_free": (None, [P(MeshNormals)]),
        "vcy_last_normals_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_label_components": (C.c_int, [vp, C.c_double, P(P(Component)), P(C.c_int64)]),
        "vcy_components_free": (None, [P(Component)]),
        "vcy_download_labels": (C.c_int, [vp, vp]),
        "vcy_keep_components": (C.c_int, [vp, C.c_double, C.c_int, C.c_int64, C.c_float, P(C.c_int64), P(C.c_int64)]),
        "vcy_last_components_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_label_components_slab": (C.c_int, [vp, C.c_double, P(P(Component)), P(C.c_int64)]),
        "vcy_component_top_plane": (C.c_int, [vp, vp]),
        "vcy_component_seam_pairs": (C.c_int, [vp, vp, P(P(C.c_int64)), P(C.c_int64)]),
        "vcy_seam_pairs_free": (None, [P(C.c_int64)]),
        "vcy_merge_components_host": (C.c_int, [C.c_int, vp, vp, vp, vp, P(P(Component)), P(C.c_int64), vp]),
        "vcy_resolve_components_slab": (C.c_int, [vp, C.c_int64, vp, vp]),
        "vcy_keep_components_slab": (C.c_int, [vp, C.c_float, C.c_int64, vp, P(C.c_int64)]),
        "vcy_select_components_host": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int64, vp, P(C.c_int64), P(C.c_int64), vp,
                                                 C.c_int64, vp]),
        "vcy_distance_field": (C.c_int, [vp, C.c_double, C.c_int, vp]),
        "vcy_redistance": (C.c_int, [vp, C.c_double, C.c_int, P(C.c_int64)]),
        "vcy_distance_field_host": (C.c_int, [P(CarverOption), vp, vp, C.c_double, C.c_int, vp, vp]),
        "vcy_last_distance_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_close_hull_plan": (C.c_int, [C.c_double, C.c_float, P(C.c_double), P(C.c_int)]),
        "vcy_distance_slab_begin": (C.c_int, [vp, C.c_double, C.c_int]),
        "vcy_distance_slab_planes": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "vcy_distance_field_slab": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp]),
        "vcy_redistance_slab": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, P(C.c_int64)]),
        "vcy_distance_slab_planes_host": (C.c_int, [P(CarverOption), C.c_int, C.c_int, vp, vp, C.c_double, C.c_int, vp]),
        "vcy_distance_slab_finish_host": (C.c_int, [P(CarverOption), C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int,
                                                    vp, vp, vp, vp]),
        "vcy_distance_halo_host": (C.c_int, [C.c_int, vp, C.c_int, C.c_int64, P(vp), P(vp), C.c_int, vp, vp, P(C.c_int),
                                             P(C.c_int)]),
        "vcy_cell_planes": (C.c_int, [P(C.c_float), P(C.c_float), C.c_float, C.c_int, vp]),
        "vcy_render_hull": (C.c_int, [vp, C.c_double, C.c_int, P(View), P(vp), P(vp), P(vp)]),
        "vcy_hull_agreement": (C.c_int, [vp, C.c_double, C.c_int, P(View), P(vp), vp]),
        "vcy_render_hull_slab": (C.c_int, [vp, C.c_double, C.c_int, P(View), P(vp), P(vp), P(vp), P(vp)]),
        "vcy_render_merge_host": (C.c_int, [P(View), C.c_int, P(vp), P(vp), P(vp), vp, vp, vp]),
        "vcy_hull_agreement_host": (C.c_int, [P(View), C.c_int, P(vp), vp, vp]),
        "vcy_last_render_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_color_vertices_host": (C.c_int, [C.c_int64, vp, vp, C.c_int, P(View), P(vp), P(vp), P(ColorOption), vp, vp, vp]),
        "vcy_color_vertices": (C.c_int, [vp, C.c_double, C.c_int64, vp, vp, C.c_int, P(View), P(vp), P(vp), P(ColorOption),
                                         vp, vp, vp]),
        "vcy_last_color_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_raster_mesh_host": (C.c_int, [C.c_int64, C.c_int64, vp, vp, C.c_int, P(View), P(vp), P(vp), P(vp), vp]),
        "vcy_raster_mesh": (C.c_int, [vp, C.c_int64, C.c_int64, vp, vp, C.c_int, P(View), P(vp), P(vp), P(vp), vp]),
        "vcy_mesh_agreement": (C.c_int, [vp, C.c_int64, C.c_int64, vp, vp, C.c_int, P(View), P(vp), vp]),
        "vcy_last_raster_ms": (C.c_int, [vp, P(C.c_float), P(C.c_float)]),
        "vcy_shade_mesh_host": (C.c_int, [C.c_int64, C.c_int64, vp, vp, vp, C.c_int, P(View), P(ShadeOption), P(vp), P(vp), P(vp)]),
        "vcy_shade_mesh": (C.c_int, [vp, C.c_int64, C.c_int64, vp, vp, vp, C.c_int, P(View), P(ShadeOption), P(vp), P(vp), P(vp)]),
        "vcy_mesh_photo_error_host": (C.c_int, [C.c_int64, C.c_int64, vp, vp, vp, C.c_int, P(View), P(vp), P(vp), vp]),
        "vcy_mesh_photo_error": (C.c_int, [vp, C.c_int64, C.c_int64, vp, vp, vp, C.c_int, P(View), P(vp), P(vp), vp]),
        "vcy_last_shade_ms": (C.c_int, [vp, P(C.c_float), P(C.c_float)]),
        "vcy_smooth_mesh_host": (C.c_int, [C.c_int64, C.c_int64, vp, vp, P(SmoothOption), vp, vp, vp]),
        "vcy_smooth_mesh": (C.c_int, [vp, C.c_int64, C.c_int64, vp, vp, P(SmoothOption), vp, vp, vp]),
        "vcy_last_smooth_ms": (C.c_int, [vp, P(C.c_float), P(C.c_float), P(C.c_float)]),
        "vcy_decimate_mesh_host": (C.c_int, [C.c_int64, C.c_int64, vp, vp, P(DecimateOption), vp, vp, P(C.c_int64), P(C.c_int64),
                                             vp, vp, vp, vp]),
        "vcy_decimate_mesh": (C.c_int, [vp, C.c_int64, C.c_int64, vp, vp, P(DecimateOption), vp, vp, P(C.c_int64), P(C.c_int64),
                                        vp, vp, vp, vp]),
        "vcy_last_decimate_ms": (C.c_int, [vp, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float)]),
        "vcy_decimate_mesh_quadric_host": (C.c_int, [C.c_int64, C.c_int64, vp, vp, P(DecimateOption), C.c_float, vp, vp,
                                                     P(C.c_int64), P(C.c_int64), vp, vp, vp, vp, P(C.c_int64)]),
        "vcy_decimate_mesh_quadric": (C.c_int, [vp, C.c_int64, C.c_int64, vp, vp, P(DecimateOption), C.c_float, vp, vp,
                                                P(C.c_int64), P(C.c_int64), vp, vp, vp, vp, P(C.c_int64)]),
        "vcy_last_quadric_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_extract_iso_chain": (C.c_int, [vp, C.c_double, C.c_int, P(ChainOption), P(Mesh), P(MeshNormals), P(ChainReport)]),
        "vcy_chain_report_free": (None, [P(ChainReport)]),
        "vcy_mesh_index_limits": (C.c_int, [C.c_int64, C.c_int64]),
        "vcy_last_chain_ms": (C.c_int, [vp] + [P(C.c_float)] * 8),
        "vcy_mesh_normals_host": (C.c_int, [C.c_int64, C.c_int64, vp, vp, vp, vp]),
        "vcy_mesh_normals_host_seam": (C.c_int, [C.c_int64, vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, vp]),
        "vcy_mesh_normals_seam_sum": (C.c_int, [C.c_int64, vp, vp, C.c_int64, C.c_int64, C.c_int64, vp, vp]),
        "vcy_merge_meshes_host": (C.c_int, [C.c_int, P(Mesh), P(MeshNormals), P(C.c_int64), vp, vp, vp, vp, vp]),
        "vcy_extract_voxel": (C.c_int, [vp, C.c_int, P(Mesh)]),
        "vcy_extract_voxel_ids": (C.c_int, [vp, C.c_int, P(P(C.c_int64)), P(C.c_int64)]),
        "vcy_ids_free": (None, [P(C.c_int64)]),
        "vcy_voxel_cubes": (C.c_int, [P(CarverOption), C.c_int64, vp, P(Mesh)]),
        "vcy_extract_voxel_into": (C.c_int, [vp, C.c_int, MeshArraysFn, vp]),
        "vcy_voxel_cubes_into": (C.c_int, [P(CarverOption), C.c_int64, vp, MeshArraysFn, vp]),
        "vcy_mesh_free": (None, [P(Mesh)]),
        "vcy_last_extract_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_last_extract_wall_ms": (C.c_int, [vp, P(C.c_float)]),
        "vcy_download": (C.c_int, [vp, vp, vp]),
        "vcy_upload": (C.c_int, [vp, vp, vp]),
        "vcy_download_positions": (C.c_int, [vp, vp]),
        "vcy_halo_bytes": (C.c_int64, [vp]),
        "vcy_halo_pack": (C.c_int, [vp, vp]),
        "vcy_halo_unpack": (C.c_int, [vp, vp, C.c_int, C.c_int]),
        "vcy_halo_install": (C.c_int, [vp, vp]),
        "vcy_halo_copy_from": (C.c_int, [vp, vp]),
        "vcy_halo_allgather": (C.c_int, [P(vp), C.c_int]),
        "vcy_halo_shutdown": (None, []),
        "vcy_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, P(vp)]),
        "vcy_comm_destroy": (None, [vp]),
        "vcy_halo_allgather_ranks": (C.c_int, [vp, P(vp), C.c_int]),
        "vcy_rendezvous_exchange": (C.c_int, [C.c_int, C.c_int, C.c_char_p, vp, C.c_int]),
        "vcy_last_collective": (C.c_char_p, []),
        "vcy_state_equal": (C.c_int, [vp, vp, P(C.c_int64)]),
        "vcy_device_count": (C.c_int, [P(C.c_int)]),
        "vcy_sdf_upload": (C.c_int, [vp, vp, C.c_int, C.c_int, P(vp)]),
        "vcy_device_free": (C.c_int, [vp, vp]),
        "vcy_device_alloc": (C.c_int, [vp, C.c_int64, P(vp)]),
        "vcy_memcpy_h2d": (C.c_int, [vp, vp, vp, C.c_int64]),
        "vcy_memcpy_d2h": (C.c_int, [vp, vp, vp, C.c_int64]),
        "vcy_reset": (C.c_int, [vp]),
        "vcy_set_param": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "vcy_get_param": (C.c_int, [vp, C.c_char_p, P(C.c_int)]),
        "vcy_set_stream": (C.c_int, [vp, vp]),
        "vcy_get_stream": (C.c_int, [vp, P(vp)]),
        "vcy_sync": (C.c_int, [vp]),
        "vcy_timer_begin": (C.c_int, [vp]),
        "vcy_timer_end": (C.c_int, [vp, P(C.c_float)]),
        "vcy_selftest": (C.c_int, [vp]),
        "vcy_last_carve_ms": (C.c_int, [vp, P(C.c_float), P(C.c_float)]),
        "vcy_last_carve_pairs": (C.c_int, [vp, P(C.c_int64), P(C.c_int64), vp, C.c_int, P(C.c_int)]),
        "vcy_plan_z_slabs": (C.c_int, [vp, C.c_int, P(View), P(vp), C.c_int, C.c_int, C.c_float, vp, vp, C.c_int,
                                       P(C.c_int)]),
        "vcy_last_stream_ms": (C.c_int, [vp, P(C.c_float), P(C.c_float), P(C.c_float)]),
        "vcy_partition_layers": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp]),
        "vcy_carve_log": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, P(C.c_int), C.c_int]),
        "vcy_measure_bandwidth": (C.c_int, [C.c_int, C.c_uint64, C.c_int, P(C.c_double), P(C.c_double)]),
        "vcy_clock_probe_start": (C.c_int, [C.c_int, C.c_int, P(vp)]),
        "vcy_clock_probe_stop": (C.c_int, [vp, P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_int),
                                           P(C.c_double)]),
        "vcy_last_error": (C.c_char_p, []),
        "vcy_version": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError if the C-ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    lib._vcy_symbols = sorted(sig)
    _lib = lib
    return lib
