"""vcy_merge_meshes_host (host only, no GPU): the stitch of z-slab meshes by edge key, with and without the slabs' normals.
The yardstick is tests/merge_ref.py, the numpy statement of the rule that vacancy_amd.dist.merge_meshes was before the
library call existed, and -- for the plain arrays -- the CPU oracle's marching cubes over the whole grid.  Slab meshes
come from the oracle's slab extraction (test_seam_normals.slab_parts) and from hand-made cases of a few vertices.
Floats are compared as uint32 bits."""
import ctypes as C

import numpy as np
import pytest

import merge_ref
import normals_ref as NR
from test_seam_normals import BOUNDS, bunny_grid, slab_parts  # noqa: F401 -- bunny_grid is a fixture
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist

WHO = "vcy_merge_meshes_host"
PLAIN = ("vertices", "faces", "keys", "n_foreign")


def assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        same = np.array_equal(NR.bits(got[k]), NR.bits(want[k])) if got[k].dtype == np.float32 else np.array_equal(got[k], want[k])
        assert same, k


_bunny = {}


def bunny_case(g, bounds, iso, interp):
    """(parts with normals, merge_ref of them with normals, merge_ref of them without, the oracle's whole-grid mesh),
    computed once.  A part's normals are Mesh::CalcNormal of the slab's mesh alone: final away from the seams, and at the
    seam vertices some value for the merge to replace."""
    key = (tuple(bounds), iso, interp)
    if key not in _bunny:
        parts = slab_parts(g, bounds, iso, interp)
        for m in parts:
            m["normals"], m["face_normals"] = vc.mesh_normals_host(m["vertices"], m["faces"])
        _bunny[key] = (parts, merge_ref.merge_meshes(parts), merge_ref.merge_meshes([{k: m[k] for k in PLAIN} for m in parts]),
                       g.marching_cubes(iso, interp))
    return _bunny[key]


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("iso,interp", [(0.0, True), (0.1, False)])
@pytest.mark.parametrize("bounds", BOUNDS)
def test_bunny_slabs_equal_the_numpy_rule_and_the_whole_grid(bunny_grid, bounds, iso, interp, normals):
    parts, want_normals, want_plain, full = bunny_case(bunny_grid, bounds, iso, interp)
    want = want_normals if normals else want_plain
    assert sorted(want) == (["face_normals", "faces", "keys", "normals", "vertices"] if normals else ["faces", "keys", "vertices"])
    got = vdist.merge_meshes(parts if normals else [{k: m[k] for k in PLAIN} for m in parts])
    assert_same(got, want)
    assert len(got["vertices"]) > 0
    assert np.array_equal(NR.bits(got["vertices"]), NR.bits(full["vertices"]))
    assert np.array_equal(got["faces"], full["faces"]) and np.array_equal(got["keys"], full["keys"])
    if normals:  # the seams are finished: Mesh::CalcNormal of the merged mesh
        whole_v, whole_f = vc.mesh_normals_host(got["vertices"], got["faces"])
        assert np.array_equal(NR.bits(got["normals"]), NR.bits(whole_v))
        assert np.array_equal(NR.bits(got["face_normals"]), NR.bits(whole_f))


# ---- hand-made slabs of a few vertices --------------------------------------------------------------------------------

def part(rng, foreign_keys, own_keys, n_faces, layer_faces=None):
    """A slab part: the foreign vertices first, random positions, faces and normals (the merge never looks at them)."""
    keys = np.array(list(foreign_keys) + list(own_keys), np.int64).reshape(-1, 2)
    nv = len(keys)
    assert nv > 0 or n_faces == 0
    return {"vertices": rng.rand(nv, 3).astype(np.float32), "keys": keys, "n_foreign": len(foreign_keys),
            "faces": rng.randint(0, max(nv, 1), (n_faces, 3)).astype(np.int32),
            "normals": rng.rand(nv, 3).astype(np.float32), "face_normals": rng.rand(n_faces, 3).astype(np.float32),
            "layer_faces": layer_faces if layer_faces is not None else (n_faces // 2, n_faces - n_faces // 3)}


def K(*ids):
    """Keys of in-plane edges (id, id + 1)."""
    return [(i, i + 1) for i in ids]


def hand_cases():
    r = np.random.RandomState(7)
    empty = lambda: part(r, [], [], 0)  # noqa: E731
    return {
        "one slab": [part(r, [], K(0, 2, 4, 9), 5)],
        "all slabs empty": [empty(), empty(), empty()],
        "an empty slab between two": [part(r, [], K(0, 2, 4), 4), empty(), part(r, [], K(200, 202), 3)],
        "vertices but nothing foreign": [part(r, [], K(0, 2, 100, 102), 4), part(r, [], K(200, 210, 220), 5)],
        "foreign in another order than the owners": [part(r, [], K(0, 100, 102, 104, 106, 2), 6),
                                                     part(r, K(106, 100, 104), K(200, 202), 7),
                                                     part(r, K(202, 200), K(300), 4)],
        "a slab of foreign vertices only": [part(r, [], K(0, 100, 102), 3), part(r, K(102, 100), [], 4),
                                            part(r, [], K(300, 302), 2)],
        "no faces": [part(r, [], K(0, 100), 0), part(r, K(100), K(200), 0)],
    }


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_made_slabs(name, normals):
    parts = hand_cases()[name]
    if not normals:
        parts = [{k: m[k] for k in PLAIN} for m in parts]
    want = merge_ref.merge_meshes(parts)
    got = vdist.merge_meshes(parts)
    assert_same(got, want)
    if name == "one slab":  # the identity
        m = parts[0]
        assert np.array_equal(got["vertices"], m["vertices"]) and np.array_equal(got["faces"], m["faces"])
        assert np.array_equal(got["keys"], m["keys"])
        assert not normals or (np.array_equal(got["normals"], m["normals"]) and np.array_equal(got["face_normals"], m["face_normals"]))
    if name == "foreign in another order than the owners":  # by hand: slab 1's vertices 0, 1, 2 are slab 0's 4, 1, 3
        f0, f1 = parts[0]["faces"], parts[1]["faces"]
        lut = np.array([4, 1, 3, 6, 7])
        assert np.array_equal(got["faces"][len(f0):len(f0) + len(f1)], lut[f1])
        assert len(got["vertices"]) == 6 + 2 + 1


def test_no_slabs_at_all():
    assert_same(vdist.merge_meshes([]), merge_ref.merge_meshes([]))


# ---- errors -----------------------------------------------------------------------------------------------------------

SENTINEL_F, SENTINEL_I = np.float32(-7.25), -77


def raw_call(parts, normals=False, patch=None, n_slabs=None, null=()):
    """vcy_merge_meshes_host on the parts through ctypes, the five output arrays pre-filled with a sentinel.
    patch(slabs, extra, layer_faces) edits the structs before the call; `null` names arguments passed as NULL.
    Returns (status, message, the outputs untouched?)."""
    lib = capi.load()
    n = len(parts)
    keep = []

    def ptr(a, t):
        if a is None or len(a) == 0:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(t))

    slabs = (capi.Mesh * max(n, 1))()
    extra = (capi.MeshNormals * max(n, 1))()
    lf = (C.c_int64 * max(2 * n, 1))()
    for s, m in enumerate(parts):
        slabs[s] = capi.Mesh(len(m["vertices"]), len(m["faces"]), ptr(m["vertices"], C.c_float), ptr(m["faces"], C.c_int32),
                             ptr(m.get("keys"), C.c_int64), m["n_foreign"])
        if normals:
            extra[s] = capi.MeshNormals(ptr(m.get("normals"), C.c_float), ptr(m.get("face_normals"), C.c_float))
            lf[2 * s], lf[2 * s + 1] = m["layer_faces"]
    if patch:
        patch(slabs, extra, lf)
    rows = 64  # more than any case here merges
    out = {"vertices": np.full((rows, 3), SENTINEL_F), "faces": np.full((rows, 3), SENTINEL_I, np.int32),
           "edge_keys": np.full((rows, 2), SENTINEL_I, np.int64), "vertex_normals": np.full((rows, 3), SENTINEL_F),
           "face_normals": np.full((rows, 3), SENTINEL_F)}
    arg = {k: a.ctypes.data for k, a in out.items()}
    if not normals:
        arg["vertex_normals"] = arg["face_normals"] = None
    arg.update(slabs=slabs, normals=extra if normals else None, layer_faces=lf if normals else None)
    for k in null:
        arg[k] = None
    rc = lib.vcy_merge_meshes_host(n if n_slabs is None else n_slabs, arg["slabs"], arg["normals"], arg["layer_faces"],
                                   arg["vertices"], arg["faces"], arg["edge_keys"], arg["vertex_normals"], arg["face_normals"])
    untouched = all((a == (SENTINEL_F if a.dtype == np.float32 else SENTINEL_I)).all() for a in out.values())
    return rc, vc.last_error(), untouched


def two_slabs():
    r = np.random.RandomState(11)
    return [part(r, [], K(0, 100, 102, 104), 4), part(r, K(104, 100), K(200, 202), 5)]


def set_field(s, name, value):
    return lambda slabs, extra, lf: setattr(slabs[s], name, value)


def test_the_error_cases_start_from_a_merge_that_works():
    for normals in (False, True):
        rc, _, untouched = raw_call(two_slabs(), normals)
        assert rc == 0 and not untouched


def drop_normals(s, field):
    return lambda slabs, extra, lf: setattr(extra[s], field, None)


def set_layer(i, value):
    def patch(slabs, extra, lf):
        lf[i] = value
    return patch


def huge(slabs, extra, lf):  # 2^30 own vertices in each of two slabs: only the structs are looked at before the refusal
    slabs[0].n_vertices = slabs[1].n_vertices = 1 << 30
    slabs[1].n_foreign_vertices = 0


def orphan():
    parts = two_slabs()
    parts[1]["keys"][1] = (102, 104)  # lies within the range of the foreign keys; no vertex of slab 0 has it
    return parts


UP_FRONT = {
    # name: (parts, normals, raw_call's keywords, what the message must hold)
    "negative n_slabs": (two_slabs, False, dict(n_slabs=-1), ""),
    "null slabs": (two_slabs, False, dict(null=("slabs",)), ""),
    "normals without layer_faces": (two_slabs, True, dict(null=("layer_faces",)), ""),
    "layer_faces without normals": (two_slabs, True, dict(null=("normals",)), ""),
    "normals out without normals in": (two_slabs, True, dict(null=("normals", "layer_faces")), ""),
    "null vertices out": (two_slabs, False, dict(null=("vertices",)), "null output"),
    "null faces out": (two_slabs, False, dict(null=("faces",)), "null output"),
    "null normals out": (two_slabs, True, dict(null=("vertex_normals",)), "null output"),
    "null face normals out": (two_slabs, True, dict(null=("face_normals",)), "null output"),
    "null vertices in": (two_slabs, False, dict(patch=set_field(1, "vertices", None)), "slab 1"),
    "null faces in": (two_slabs, False, dict(patch=set_field(0, "faces", None)), "slab 0"),
    "negative n_vertices": (two_slabs, False, dict(patch=set_field(1, "n_vertices", -1)), "slab 1"),
    "negative n_faces": (two_slabs, False, dict(patch=set_field(0, "n_faces", -3)), "slab 0"),
    "negative n_foreign": (two_slabs, False, dict(patch=set_field(1, "n_foreign_vertices", -2)), "slab 1"),
    "more foreign vertices than vertices": (two_slabs, False, dict(patch=set_field(1, "n_foreign_vertices", 5)), "slab 1"),
    "slab 0 with foreign vertices": (two_slabs, False, dict(patch=set_field(0, "n_foreign_vertices", 1)), "slab 0"),
    "foreign vertices without edge keys": (two_slabs, False, dict(patch=set_field(1, "edge_keys", None)), "slab 1 has no edge keys"),
    "keys wanted from a slab without": (two_slabs, False, dict(patch=set_field(0, "edge_keys", None)), "slab 0 has no edge keys"),
    "a foreign key without an owner": (orphan, False, dict(), "slab 1: foreign vertex 1 with edge key (102, 104)"),
    "a foreign key without an owner, normals": (orphan, True, dict(), "(102, 104)"),
    "vertex normals for slab 0 only": (two_slabs, True, dict(patch=drop_normals(1, "vertex_normals")), "slab 1 has no normals"),
    "face normals for slab 1 only": (two_slabs, True, dict(patch=drop_normals(0, "face_normals")), "slab 0 has no normals"),
    "layer_faces below 0": (two_slabs, True, dict(patch=set_layer(1, -1)), "slab 0: layer_faces"),
    "layer_faces above n_faces": (two_slabs, True, dict(patch=set_layer(2, 6)), "slab 1: layer_faces"),
    "more than INT32_MAX merged vertices": (two_slabs, False, dict(patch=huge), "slab 1: the merged mesh has more than 2147483647"),
}


@pytest.mark.parametrize("name", sorted(UP_FRONT))
def test_errors_found_before_the_first_write(name):
    make, normals, kw, text = UP_FRONT[name]
    rc, message, untouched = raw_call(make(), normals, **kw)
    print(name, "->", message)
    assert rc == capi.VCY_ERR_INVALID_ARG
    assert WHO in message and text in message
    assert untouched


@pytest.mark.parametrize("bad", [9, -1])
def test_a_face_outside_the_slabs_vertices(bad):
    """Found while the faces are written: the outputs are unspecified afterwards, the status and the text are not."""
    parts = two_slabs()
    parts[1]["faces"][2, 1] = bad
    rc, message, _ = raw_call(parts)
    assert rc == capi.VCY_ERR_INVALID_ARG
    assert WHO in message and "slab 1: face 2 names vertex %d of 4" % bad in message


def test_the_python_callers_raise():
    with pytest.raises(RuntimeError, match=WHO + ".*no owner"):
        vdist.merge_meshes(orphan())
    parts = two_slabs()
    with pytest.raises(ValueError):
        vc.merge_meshes_host(*[[m[k] for m in parts] for k in PLAIN], normals=[m["normals"] for m in parts])
    parts[0]["normals"] = parts[0]["normals"][:-1]
    with pytest.raises(ValueError):
        vdist.merge_meshes(parts)
