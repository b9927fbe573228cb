"""Mesh normals on the host (no GPU): vcy_mesh_normals_host and the facade's Mesh::CalcNormal against the numpy
restatement of the reference's mesh.cc:197-240 (tests/normals_ref.py), compared as uint32 bits; the binary PLY writer
with and without normals; the C-ABI of the new calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import normals_ref as NR
import oracle_lib as O
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import UpdateOption

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "vacancy_amd", "host", "host_selftest")


def carved_bunny_mesh(res, interp):
    opt = B.bunny_option(res, UpdateOption())
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    orc = O.OracleGrid(opt)
    for view, mask in zip(views, B.load_masks()):
        orc.carve(view, O.make_sdf(mask))
    return orc.marching_cubes(0.0, interp)


def sphere_mesh(n=64, nv=4):
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, nv, 160, 120)
    orc = O.OracleGrid(opt)
    for view, mask in zip(views, masks):
        orc.carve(view, O.make_sdf(mask))
    return orc.marching_cubes(0.0, True)


def assert_host_equals_numpy(vertices, faces):
    rvn, rfn = NR.mesh_normals(vertices, faces)
    hvn, hfn = vc.mesh_normals_host(vertices, faces)
    assert hvn.shape == rvn.shape and hfn.shape == rfn.shape
    assert np.array_equal(NR.bits(hfn), NR.bits(rfn)), "face normals differ"
    assert np.array_equal(NR.bits(hvn), NR.bits(rvn)), "vertex normals differ"
    return rvn, rfn


@pytest.mark.parametrize("res", [10.0, 5.0])
@pytest.mark.parametrize("interp", [True, False])
def test_host_normals_of_the_carved_bunny(res, interp):
    m = carved_bunny_mesh(res, interp)
    assert len(m["vertices"]) > 1000
    vn, fn = assert_host_equals_numpy(m["vertices"], m["faces"])
    if not interp:  # every position is a voxel centre: many zero-area triangles, whose normal is 0
        assert (fn == 0).all(axis=1).any()


def test_host_normals_of_a_sphere_at_64():
    m = sphere_mesh()
    vn, fn = assert_host_equals_numpy(m["vertices"], m["faces"])
    nz = (vn != 0).any(axis=1)
    assert np.abs(np.sqrt((vn[nz].astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() <= 4 * np.finfo(np.float32).eps


def test_host_normals_of_hand_made_meshes():
    # a zero-area face (two corners coincide) next to a proper one
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0.25, 0.5, 3]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [2, 1, 4]], np.int32)
    vn, fn = assert_host_equals_numpy(v, f)
    assert (fn[1] == 0).all() and (fn[0] == np.array([0, 0, 1], np.float32)).all()
    # a vertex shared by two faces whose normals cancel: the sum is 0, 0 / 2 = 0, normalize() leaves 0
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    vn, fn = assert_host_equals_numpy(v, f)
    assert (fn[0] == -fn[1]).all() and (vn == 0).all()
    # the order of the sum is part of the result: three addends that do not associate
    rng = np.random.default_rng(5)
    v = rng.normal(size=(40, 3)).astype(np.float32)
    f = np.array([[0, i, i + 1] for i in range(1, 39)], np.int32)
    assert_host_equals_numpy(v, f)
    # an empty mesh
    vn, fn = vc.mesh_normals_host(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert vn.shape == (0, 3) and fn.shape == (0, 3)
    rvn, rfn = NR.mesh_normals(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert rvn.shape == (0, 3) and rfn.shape == (0, 3)
    # only one of the two outputs, and a face that names a vertex that is not there
    lib = capi.load()
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    only = np.zeros((1, 3), np.float32)
    assert lib.vcy_mesh_normals_host(3, 1, v.ctypes.data, f.ctypes.data, None, only.ctypes.data) == 0
    assert (only == np.array([[0, 0, 1]], np.float32)).all()
    bad = np.array([[0, 1, 3]], np.int32)
    assert lib.vcy_mesh_normals_host(3, 1, v.ctypes.data, bad.ctypes.data, None, only.ctypes.data) == capi.VCY_ERR_INVALID_ARG


def read_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode().splitlines()
    nv = int([l for l in header if l.startswith("element vertex")][0].split()[2])
    nf = int([l for l in header if l.startswith("element face")][0].split()[2])
    props = [l.split()[2] for l in header if l.startswith("property float")]
    body = data[end:]
    vrec = np.frombuffer(body[: 4 * len(props) * nv], np.float32).reshape(nv, len(props))
    rest = body[4 * len(props) * nv:]
    assert len(rest) == 13 * nf
    frec = np.frombuffer(rest, np.uint8).reshape(nf, 13)
    assert (frec[:, 0] == 3).all()
    faces = np.ascontiguousarray(frec[:, 1:]).view(np.int32).reshape(nf, 3)
    return header, props, vrec, faces


def test_facade_calc_normal_and_binary_ply(tmp_path):
    """Mesh::CalcNormal through the C++ facade gives the same bits; Clear() empties the normal vectors; WritePlyBinary
    writes nx ny nz after z (24-byte vertices) when the mesh has normals and today's bytes when it has none."""
    m = carved_bunny_mesh(10.0, True)
    v, f = m["vertices"], m["faces"]
    v.tofile(str(tmp_path / "vertices.f32"))
    f.astype(np.int32).tofile(str(tmp_path / "faces.i32"))
    out = subprocess.run([SELFTEST, B.BUNNY, "normals", str(tmp_path)], check=True, stdout=subprocess.PIPE).stdout.decode()
    row = [l for l in out.splitlines() if l.startswith("NORMALS")][0].split()
    assert row[1:] == ["1", str(len(v)), str(len(f)), str(len(f)), "0", "0", "0"], row
    rvn, rfn = NR.mesh_normals(v, f)
    vn = np.fromfile(str(tmp_path / "normals.f32"), np.float32).reshape(-1, 3)
    fn = np.fromfile(str(tmp_path / "face_normals.f32"), np.float32).reshape(-1, 3)
    ni = np.fromfile(str(tmp_path / "normal_indices.i32"), np.int32).reshape(-1, 3)
    assert np.array_equal(NR.bits(vn), NR.bits(rvn)) and np.array_equal(NR.bits(fn), NR.bits(rfn))
    assert np.array_equal(ni, f)
    header, props, vrec, faces = read_ply(str(tmp_path / "with_normals.ply"))
    assert props == ["x", "y", "z", "nx", "ny", "nz"] and vrec.shape == (len(v), 6)
    assert np.array_equal(NR.bits(vrec[:, :3]), NR.bits(v)) and np.array_equal(NR.bits(vrec[:, 3:]), NR.bits(rvn))
    assert np.array_equal(faces, f)
    # without normals: byte for byte the writer as it was
    want = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f))).encode()
    rec = np.empty((len(f), 13), np.uint8)
    rec[:, 0] = 3
    rec[:, 1:] = np.ascontiguousarray(f.astype(np.int32)).view(np.uint8).reshape(len(f), 12)
    want += np.ascontiguousarray(v, np.float32).tobytes() + rec.tobytes()
    assert open(str(tmp_path / "without_normals.ply"), "rb").read() == want


def test_c_abi_of_the_normals_calls():
    lib = capi.load()
    for name in ("vcy_extract_iso_normals", "vcy_mesh_normals_free", "vcy_last_normals_ms", "vcy_mesh_normals_host"):
        assert hasattr(lib, name) and name in lib._vcy_symbols
    assert C.sizeof(capi.MeshNormals) == 16
    assert C.sizeof(capi.Mesh) == 48
    assert (capi.VCY_NORMALS_VERTEX, capi.VCY_NORMALS_FACE) == (1, 2)
    header = open(os.path.join(ROOT, "include", "vacancy_hip.h")).read()
    assert "#define VCY_NORMALS_VERTEX 1" in header and "#define VCY_NORMALS_FACE   2" in header
    # freeing an empty struct is harmless
    mn = capi.MeshNormals()
    lib.vcy_mesh_normals_free(C.byref(mn))
    assert not mn.vertex_normals and not mn.face_normals
