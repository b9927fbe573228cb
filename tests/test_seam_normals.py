"""The seam finish of the sharded normals on the host (no GPU): vcy_mesh_normals_host_seam and the merge rule of
vacancy_amd.dist.merge_meshes.  Slab meshes come from the CPU oracle's slab extraction, as in tests/test_dist_cpu.py; the
yardstick is vcy_mesh_normals_host on the merged mesh (itself checked against the numpy restatement of mesh.cc:197-240
in tests/test_mesh_normals.py).  Everything is compared as uint32 bits."""
import ctypes as C

import numpy as np
import pytest

import bunny_data as B
import normals_ref as NR
import oracle_lib as O
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist

SENTINEL = np.float32(-7.25)


@pytest.fixture(scope="module")
def bunny_grid():
    masks = B.load_masks()
    views = B.bunny_views(lambda t, q: O.affine_inverse(O.pose_from_tum(t, q)))
    g = O.OracleGrid(B.bunny_option(10.0))
    for i in range(6):
        g.carve(views[i], O.make_sdf(masks[i]))
    yield g
    g.close()


def layer_face_count(g, z, iso, interp):
    """Faces of the cell layer whose max corners lie in slice z (z >= 1): a slab of that one layer."""
    return len(O.marching_cubes_slab(g, z, z + 1, iso, interp)["faces"])


def slab_parts(g, bounds, iso=0.0, interp=True):
    """The slabs' meshes with "layer_faces" = (faces of the first, of the last own cell layer), from the oracle."""
    parts = []
    for z0, z1 in zip(bounds[:-1], bounds[1:]):
        m = O.marching_cubes_slab(g, z0, z1, iso, interp)
        m["layer_faces"] = (layer_face_count(g, max(z0, 1), iso, interp), layer_face_count(g, z1 - 1, iso, interp))
        parts.append(m)
    return parts


def seams_of(parts):
    """[(face_begin, face_end, merged ids of the seam vertices)] per seam, by the rule of vcy_extract_iso_normals_slab,
    written out independently of merge_meshes: edge keys of the foreign vertices looked up in the merged key array."""
    merged = vdist.merge_meshes([{k: m[k] for k in ("vertices", "faces", "keys", "n_foreign")} for m in parts])
    gid = {(int(a), int(b)): i for i, (a, b) in enumerate(merged["keys"])}
    out, face_offset = [], 0
    for s, m in enumerate(parts):
        if s > 0:
            ids = np.array([gid[(int(a), int(b))] for a, b in m["keys"][:m["n_foreign"]]], np.int64)
            out.append((face_offset - parts[s - 1]["layer_faces"][1], face_offset + m["layer_faces"][0], ids))
        face_offset += len(m["faces"])
    return merged, out


BOUNDS = [[0, 21, 42], [0, 14, 28, 42], [0, 10, 21, 31, 42], [0, 5, 10, 15, 21, 26, 31, 36, 42],
          [0, 2, 42], [0, 40, 42], [0, 18, 20, 22, 42], [0, 2, 4, 6, 8, 42]]


@pytest.mark.parametrize("bounds", BOUNDS)
@pytest.mark.parametrize("iso,interp", [(0.0, True), (0.1, False), (0.1, True)])
def test_seam_finish_restores_the_host_walk(bunny_grid, bounds, iso, interp):
    g = bunny_grid
    assert g.dims[2] == bounds[-1]
    parts = slab_parts(g, bounds, iso, interp)
    merged, seams = seams_of(parts)
    full = g.marching_cubes(iso, interp)
    assert np.array_equal(NR.bits(merged["vertices"]), NR.bits(full["vertices"])) and np.array_equal(merged["faces"], full["faces"])
    want, _ = vc.mesh_normals_host(merged["vertices"], merged["faces"])
    assert not (want == SENTINEL).any()
    got = want.copy()
    n_seam = 0
    for begin, end, ids in seams:
        got[ids] = SENTINEL
        n_seam += len(ids)
    assert n_seam > 0 or bounds[1] == 2  # (a seam at slice 1 or 40 runs through empty space: a case, not a skip)
    for begin, end, ids in seams:
        vc.mesh_normals_host_seam(merged["vertices"], merged["faces"], begin, end, ids, got)
    bad = int((NR.bits(got) != NR.bits(want)).any(axis=1).sum())
    print("bounds %s iso %g interp %s: %d seam vertices of %d, %d rows differ" % (bounds, iso, interp, n_seam, len(want), bad))
    assert bad == 0


def test_a_face_range_one_face_short_is_noticed(bunny_grid):
    """The check above can fail: with the last face of the range left out, or the first, a seam vertex loses a term."""
    parts = slab_parts(bunny_grid, [0, 21, 42])
    merged, seams = seams_of(parts)
    (begin, end, ids), = seams
    assert len(ids) > 0
    want, _ = vc.mesh_normals_host(merged["vertices"], merged["faces"])
    named = np.isin(merged["faces"], ids).any(axis=1)
    first, last = np.nonzero(named)[0][[0, -1]]
    assert begin <= first and last < end
    for b, e in ((begin, last), (first + 1, end)):
        got = want.copy()
        got[ids] = SENTINEL
        vc.mesh_normals_host_seam(merged["vertices"], merged["faces"], b, e, ids, got)
        assert (NR.bits(got) != NR.bits(want)).any()
    # the exact range of the named faces is enough
    got = want.copy()
    got[ids] = SENTINEL
    vc.mesh_normals_host_seam(merged["vertices"], merged["faces"], first, last + 1, ids, got)
    assert np.array_equal(NR.bits(got), NR.bits(want))


def test_seam_finish_arguments():
    lib = capi.load()
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    vn = np.full((4, 3), SENTINEL, np.float32)
    call = lambda nv, faces, b, e, ids: lib.vcy_mesh_normals_host_seam(  # noqa: E731
        nv, v.ctypes.data, faces.ctypes.data, b, e, len(ids), np.asarray(ids, np.int64).ctypes.data, vn.ctypes.data)
    # an empty seam is a no-op, whatever the range
    assert call(4, f, 0, 2, []) == 0 and (vn == SENTINEL).all()
    assert lib.vcy_mesh_normals_host_seam(4, None, None, 0, 0, 0, None, None) == 0
    # ids and ranges
    assert call(4, f, 0, 2, [4]) == capi.VCY_ERR_INVALID_ARG and b"seam vertex" in lib.vcy_last_error()
    assert call(4, f, 0, 2, [-1]) == capi.VCY_ERR_INVALID_ARG
    assert call(4, f, -1, 2, [0]) == capi.VCY_ERR_INVALID_ARG
    assert call(4, f, 2, 1, [0]) == capi.VCY_ERR_INVALID_ARG
    assert call(3, f, 0, 2, [0]) == capi.VCY_ERR_INVALID_ARG and b"names vertex" in lib.vcy_last_error()
    bad = np.array([[0, 1, -2], [0, 2, 3]], np.int32)
    assert call(4, bad, 0, 2, [0]) == capi.VCY_ERR_INVALID_ARG
    assert (vn == SENTINEL).all()  # nothing was written by a refused call
    # only the listed rows change; a repeated id is one vertex; a listed vertex no face of the range names is 0 / 0
    assert call(4, f, 0, 2, [0, 3, 0]) == 0
    want, _ = vc.mesh_normals_host(v, f)
    assert np.array_equal(NR.bits(vn[[0, 3]]), NR.bits(want[[0, 3]])) and (vn[[1, 2]] == SENTINEL).all()
    assert call(4, f, 0, 1, [3]) == 0 and np.isnan(vn[3]).all()
    with pytest.raises(ValueError):
        vc.mesh_normals_host_seam(v, f, 0, 3, [0], vn)
    with pytest.raises(ValueError):
        vc.mesh_normals_host_seam(v, f, 0, 2, [0], vn.astype(np.float64))
    assert C.sizeof(C.c_int64) == 8


@pytest.mark.parametrize("bounds", BOUNDS)
def test_merge_meshes_finishes_the_seams(bunny_grid, bounds):
    """merge_meshes with parts that carry normals: every slab's part holds what its device can finish -- the whole-grid
    normal at own vertices off the seams, zero at its foreign vertices and at those of its top plane the next slab
    names -- and the merge returns Mesh::CalcNormal of the merged mesh.  Without the three keys the result is as before."""
    g = bunny_grid
    parts = slab_parts(g, bounds)
    plain = vdist.merge_meshes([{k: m[k] for k in ("vertices", "faces", "keys", "n_foreign")} for m in parts])
    assert sorted(plain) == ["faces", "keys", "vertices"]
    want_v, want_f = vc.mesh_normals_host(plain["vertices"], plain["faces"])
    gid = {(int(a), int(b)): i for i, (a, b) in enumerate(plain["keys"])}
    face_offset = 0
    for s, m in enumerate(parts):
        ids = np.array([gid[(int(a), int(b))] for a, b in m["keys"]], np.int64)
        n = want_v[ids].copy()
        n[:m["n_foreign"]] = 0
        if s + 1 < len(parts):
            nxt = parts[s + 1]
            above = {(int(a), int(b)) for a, b in nxt["keys"][:nxt["n_foreign"]]}
            n[[i for i, (a, b) in enumerate(m["keys"]) if (int(a), int(b)) in above]] = 0
        m["normals"] = n
        m["face_normals"] = want_f[face_offset:face_offset + len(m["faces"])].copy()
        face_offset += len(m["faces"])
    got = vdist.merge_meshes(parts)
    assert sorted(got) == ["face_normals", "faces", "keys", "normals", "vertices"]
    for k in ("vertices", "faces", "keys"):
        assert np.array_equal(got[k], plain[k]) and got[k].dtype == plain[k].dtype
    assert np.array_equal(NR.bits(got["face_normals"]), NR.bits(want_f))
    assert np.array_equal(NR.bits(got["normals"]), NR.bits(want_v))
    # a part without normals: the merge is the plain one
    del parts[-1]["normals"]
    assert sorted(vdist.merge_meshes(parts)) == ["faces", "keys", "vertices"]
