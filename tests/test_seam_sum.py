"""vcy_mesh_normals_seam_sum on the host (no GPU): the seam finish of the sharded normals from face normals that exist
already.  For numbers it is vcy_mesh_normals_host_seam to the bit (yardstick: that call, itself held to
vcy_mesh_normals_host by tests/test_seam_normals.py); of two NaN terms it keeps the later one's bits, the choice of the
device's sum, where x86 would keep the earlier one's."""
import numpy as np
import pytest

import normals_ref as NR
from vacancy_amd import carver as vc

POS_NAN, NEG_NAN = np.uint32(0x7FC00000), np.uint32(0xFFC00000)


def random_mesh(seed, nv=40, nf=120):
    rng = np.random.RandomState(seed)
    v = rng.randn(nv, 3).astype(np.float32)
    f = rng.randint(0, nv, (nf, 3)).astype(np.int32)
    f[:nv, 0] = np.arange(nv)  # every vertex is named
    return v, f


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_numbers_equal_the_host_seam(seed):
    v, f = random_mesh(seed)
    fn = NR.face_normals(v, f)
    ids = np.array([3, 17, 4, 39, 0, 17], np.int64)  # (a repeated id: one slot)
    for begin, end in ((0, len(f)), (10, 70), (5, 5)):
        want = np.full(v.shape, -7.25, np.float32)
        got = want.copy()
        vc.mesh_normals_host_seam(v, f, begin, end, ids, want)
        vc.mesh_normals_seam_sum(len(v), f, fn, begin, end, ids, got)
        assert np.array_equal(NR.bits(got), NR.bits(want)), (begin, end)
        rest = np.setdiff1d(np.arange(len(v)), ids)
        assert (got[rest] == np.float32(-7.25)).all()


def test_of_two_nans_the_later_term():
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1]], np.int32)
    one = np.float32(1.0).view(np.uint32)
    for terms, want in (((POS_NAN, NEG_NAN, one), NEG_NAN), ((NEG_NAN, POS_NAN, one), POS_NAN),
                        ((one, NEG_NAN, POS_NAN), POS_NAN), ((one, one, NEG_NAN), NEG_NAN), ((POS_NAN, one, one), POS_NAN)):
        fn = np.zeros((3, 3), np.uint32)
        fn[:, 0] = terms          # x: the terms of vertex 0 in face order
        fn[:, 1] = one            # y: numbers
        vn = np.zeros((4, 3), np.float32)
        vc.mesh_normals_seam_sum(4, f, fn.view(np.float32), 0, 3, [0], vn)
        assert NR.bits(vn)[0, 0] == want, (terms, hex(NR.bits(vn)[0, 0]))
        assert NR.bits(vn)[0, 1] == np.float32(1.0).view(np.uint32)  # 3 / 3, not normalised: n2 is NaN
        assert not NR.bits(vn)[1:].any()


def test_errors():
    v, f = random_mesh(4)
    fn = NR.face_normals(v, f)
    vn = np.zeros(v.shape, np.float32)
    with pytest.raises(RuntimeError):
        vc.mesh_normals_seam_sum(len(v), f, fn, 0, len(f), [len(v)], vn)
    assert "vcy_mesh_normals_seam_sum" in vc.last_error()
    bad = f.copy()
    bad[7, 1] = len(v)
    with pytest.raises(RuntimeError):
        vc.mesh_normals_seam_sum(len(v), bad, fn, 0, len(f), [1], vn)
    with pytest.raises(ValueError):
        vc.mesh_normals_seam_sum(len(v), f, fn[:-1], 0, len(f), [1], vn)
    assert not vn.any()
