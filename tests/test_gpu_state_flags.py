"""Two rules of "writers declare, caches compare" (vacancy_amd/csrc/state_flags.h) that no sequence of
tests/state_model.py reaches: an upload that is refused has touched nothing, and the seam calls follow the slab labelling for
exactly as long as no voxel of the slab has changed.  The smaller grid of state_model.SHAPES, cut at 8 into two slabs on one
device; the base state is carved, so that the brick minima are valid.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import state_model as SM
from test_gpu_components import assert_mesh_equal
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist

pytestmark = pytest.mark.gpu

DIMS = SM.SHAPES[0]  # 24 x 20 x 17
CUT = 8


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_refused_upload_touches_nothing():
    m = SM.model("max", DIMS)
    cap = m.opt.update_option.voxel_max_update_num + 1
    new = m.upload_arrays(m.state(()))
    with SM.Device(m, CUT) as d:
        d.base()      # (asserts brick_min_valid == 1 on both slabs)
        d.exchange()  # the upper slab holds the lower slab's last two slices
        before = [c.download() for c in d.ctxs]
        upper = d.ctxs[1]
        mesh, ids = upper.ExtractIsoSurface(0.0, True), upper.extract_voxel_ids(True)
        assert len(mesh["faces"]) > 0 and len(ids) > 0
        for bad in (-1, cap + 1):
            for c, (z0, z1), (s0, u0) in zip(d.ctxs, d.ranges, before):
                s, u = m.slab(new, z0, z1)
                assert (bits(s) != bits(s0)).any(), "the refused upload would not have changed the sdf"
                u = u.copy()
                u[-1] = bad  # the LAST counter: everything in front of it is good
                with pytest.raises(RuntimeError, match="update_num"):
                    c.upload(s, u)
                assert c.get_param("brick_min_valid") == 1, "z %d..%d: the brick minima went with a refused upload" % (z0, z1)
        # the upper slab's extractions BEFORE its download: nothing in between that could repair a flag
        got = upper.ExtractIsoSurface(0.0, True)
        assert got["n_foreign"] == mesh["n_foreign"]
        assert_mesh_equal(got, mesh, "the upper slab after refused uploads")
        assert np.array_equal(upper.extract_voxel_ids(True), ids)
        for c, (z0, z1), (s0, u0) in zip(d.ctxs, d.ranges, before):
            s1, u1 = c.download()
            assert np.array_equal(bits(s1), bits(s0)) and np.array_equal(u1, u0), "z %d..%d: the state moved" % (z0, z1)
            assert c.get_param("brick_min_valid") == 1
        # ... and it is still the model's base state, minima included: one more fused carve at "cull" 1, every reader
        d.apply(SM.CLOSE, (SM.CLOSE,))
        d.read_all((SM.CLOSE,))


def test_seam_calls_follow_the_labelling_until_a_voxel_changes():
    m = SM.model("max", DIMS)
    lib = capi.load()
    with SM.Device(m, CUT) as d:
        d.base()
        lower, upper = d.ctxs
        r = vdist.label_components_slabs(d.ctxs, 0, 1, 0.0)
        assert len(r["merged"]["label"]) >= 2, "nothing to remove"
        planes = [c.component_top_plane() for c in d.ctxs]
        pairs = upper.component_seam_pairs(planes[0])
        # a filter that removes nothing, on both slabs: no launch, no write -- the labelling stays and the seam calls answer
        for c in d.ctxs:
            assert c.KeepComponentsSlab([], 1.0) == {"removed_voxels": 0, "device_ms": 0.0}
        for c, plane in zip(d.ctxs, planes):
            assert np.array_equal(c.component_top_plane(), plane)
        assert np.array_equal(upper.component_seam_pairs(planes[0]), pairs)
        for k, c in enumerate(d.ctxs):
            c.resolve_components(r["lists"][k]["label"], r["maps"][k])
            assert c.KeepComponentsSlab([], 1.0)["removed_voxels"] == 0
        # (the halo went all the same: the slab below has run its filter step too)
        d.check_halo_refused("an empty filter")
        # one piece of the lower slab goes: its own write makes its labelling stale, the upper slab's stays
        piece = r["lists"][0]["label"][-1:]
        n_piece = int(r["lists"][0]["n_voxels"][-1])
        assert lower.KeepComponentsSlab(piece, 1.0)["removed_voxels"] == n_piece > 0
        plane = np.empty(DIMS[0] * DIMS[1], np.int64)
        gone = C.c_int64(7)
        assert lib.vcy_component_top_plane(lower.ctx, plane.ctypes.data_as(C.c_void_p)) == capi.VCY_ERR_INVALID_ARG
        assert "vcy_label_components_slab" in vc.last_error()
        assert lib.vcy_resolve_components_slab(lower.ctx, 0, None, None) == capi.VCY_ERR_INVALID_ARG
        assert lib.vcy_keep_components_slab(lower.ctx, 1.0, 0, None, C.byref(gone)) == capi.VCY_ERR_INVALID_ARG
        assert gone.value == 0 and "vcy_label_components_slab" in vc.last_error()
        assert np.array_equal(upper.component_top_plane(), planes[1])
        # the labels from before the removal are still there to be read, and a new labelling sees the piece gone
        same = r["maps"][0] == r["maps"][0][-1]  # (pieces of the lower slab that belong to the removed piece's component)
        assert (lower.download_labels() == r["maps"][0][-1]).sum() == r["lists"][0]["n_voxels"][same].sum()
        again = lower.LabelComponentsSlab(0.0)
        assert again["n_voxels"].sum() == r["lists"][0]["n_voxels"].sum() - n_piece
        assert lower.KeepComponentsSlab([], 1.0)["removed_voxels"] == 0
