"""Normals of a grid cut into z-slabs: vcy_extract_iso_normals_slab on every slab's device (the slab instance of the
vertex normals kernel, mc_normals.hip) plus the seam finish on the host (vcy_mesh_normals_host_seam through
vacancy_amd.dist.merge_meshes).  The yardstick is the single whole-grid context's vcy_extract_iso_normals, itself held to
Mesh::CalcNormal by tests/test_gpu_normals.py.  Every comparison of floats is one of uint32 bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import normals_ref as NR
from test_gpu_normals import snap_band_state
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist
from vacancy_amd import sharded
from vacancy_amd import synth
from vacancy_amd.capi import UpdateOption

pytestmark = pytest.mark.gpu

PARAMS = [(iso, interp, mcskip) for iso in (0.0, 0.1) for interp in (True, False) for mcskip in (0, 1)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(NR.bits(a), NR.bits(b))


def check_sharded(whole, sh, iso, interp, ctx):
    """The assertions of every scene: the merged result and every slab's own part against the whole-grid context."""
    want = whole.ExtractIsoSurface(iso, interp, normals=True)
    # the slab call on a whole-grid context is vcy_extract_iso_normals
    alone = whole.ExtractIsoSurfaceSlab(iso, interp)
    for k in ("vertices", "normals", "face_normals"):
        assert same(alone[k], want[k]), "%s: whole grid through the slab call: %s differs" % (ctx, k)
    assert np.array_equal(alone["faces"], want["faces"]) and np.array_equal(alone["keys"], want["keys"]) and alone["n_foreign"] == 0
    assert 0 <= alone["layer_faces"][0] <= len(want["faces"]) and 0 <= alone["layer_faces"][1] <= len(want["faces"])
    # the merged mesh
    got = sh.ExtractIsoSurface(iso, interp, normals=True)
    bad_v = int((NR.bits(got["normals"]) != NR.bits(want["normals"])).any(axis=1).sum()) if same(got["vertices"], want["vertices"]) else -1
    print("%s: %d vertices %d faces, %d merged vertex normals differ, normals_device_ms %.4f"
          % (ctx, len(want["vertices"]), len(want["faces"]), bad_v, got["normals_device_ms"]))
    assert same(got["vertices"], want["vertices"]) and np.array_equal(got["faces"], want["faces"]), ctx + ": merged mesh differs"
    assert np.array_equal(got["keys"], want["keys"]), ctx
    assert same(got["face_normals"], want["face_normals"]), ctx + ": merged face normals differ"
    assert same(got["normals"], want["normals"]), "%s: %d merged vertex normals differ" % (ctx, bad_v)
    # every slab's own part: the mesh bits are vcy_extract_iso's on that context, and its normals off the seams are final
    parts = sh.extract_slabs(iso, interp, normals=True)
    plain = sh.extract_slabs(iso, interp)
    gid = {(int(a), int(b)): i for i, (a, b) in enumerate(want["keys"])}
    face_offset = 0
    for s, (p, q) in enumerate(zip(parts, plain)):
        assert same(p["vertices"], q["vertices"]) and np.array_equal(p["faces"], q["faces"]), "%s slab %d mesh" % (ctx, s)
        assert np.array_equal(p["keys"], q["keys"]) and p["n_foreign"] == q["n_foreign"], "%s slab %d keys" % (ctx, s)
        assert p["normals"].shape == p["vertices"].shape and p["face_normals"].shape == p["faces"].shape
        nf = len(p["faces"])
        assert same(p["face_normals"], want["face_normals"][face_offset:face_offset + nf]), "%s slab %d face normals" % (ctx, s)
        face_offset += nf
        assert 0 <= p["layer_faces"][0] <= nf and 0 <= p["layer_faces"][1] <= nf
        if sh.z_ranges[s][1] - max(sh.z_ranges[s][0], 1) == 1:  # one cell layer: first == last == all
            assert p["layer_faces"] == (nf, nf)
        ids = np.array([gid[(int(a), int(b))] for a, b in p["keys"]], np.int64).reshape(-1)
        seam = np.zeros(len(ids), bool)
        seam[:p["n_foreign"]] = True
        if s + 1 < len(parts):
            nxt = parts[s + 1]
            above = {(int(a), int(b)) for a, b in nxt["keys"][:nxt["n_foreign"]]}
            seam |= np.array([(int(a), int(b)) in above for a, b in p["keys"]], bool).reshape(-1)
        own = ~seam
        assert same(p["normals"][own], want["normals"][ids[own]]), "%s slab %d: own normals off the seams differ" % (ctx, s)
        assert not NR.bits(p["normals"][seam]).any(), "%s slab %d: seam slots are not zero" % (ctx, s)
    if len(want["faces"]) > 0:
        assert got["normals_device_ms"] > 0
    return want


def carved(opt, views, sdfs, z_bounds=None, slabs=None):
    whole = vc.VoxelCarver(opt)
    assert whole.Init(), vc.last_error()
    for v, s in zip(views, sdfs):
        assert whole.Carve(v, s)
    count = slabs if slabs is not None else len(z_bounds) - 1
    sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=count, z_bounds=z_bounds)
    assert sh.Init(), vc.last_error()
    for c in sh.slabs:
        for v, s in zip(views, sdfs):
            assert c.Carve(v, s)
    return whole, sh


def sphere_scene(n=64, nv=5):
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, nv, 160, 120)
    return opt, views, [vc.make_sdf(m) for m in masks]


def run_params(whole, sh, ctx):
    total = 0
    for iso, interp, mcskip in PARAMS:
        whole.set_param("mcskip", mcskip)
        sh.set_param("mcskip", mcskip)
        m = check_sharded(whole, sh, iso, interp, "%s iso %g interp %s mcskip %d" % (ctx, iso, interp, mcskip))
        total += len(m["vertices"])
    return total


@pytest.mark.parametrize("slabs", [2, 3, 4, 8])
def test_sphere_in_equal_slabs(slabs):
    opt, views, sdfs = sphere_scene()
    whole, sh = carved(opt, views, sdfs, slabs=slabs)
    assert run_params(whole, sh, "sphere 64 in %d slabs" % slabs) > 0


# the sphere (radius 22.4 around the centre of 64 slices) spans about slices 10 .. 54
@pytest.mark.parametrize("z_bounds", [[0, 30, 64],              # a seam through the surface
                                      [0, 4, 64], [0, 60, 64],  # a seam in empty space (and a slab with an empty mesh)
                                      [0, 31, 33, 64],          # two seams two slices apart: the thinnest slab there is
                                      [0, 2, 64], [0, 62, 64],  # the thinnest slab at either end of the grid
                                      [0, 10, 12, 14, 40, 42, 54, 56, 64]])
def test_sphere_with_hand_picked_cuts(z_bounds):
    opt, views, sdfs = sphere_scene()
    whole, sh = carved(opt, views, sdfs, z_bounds=z_bounds)
    assert sh.z_ranges == list(zip(z_bounds[:-1], z_bounds[1:]))
    assert run_params(whole, sh, "sphere 64 cut at %s" % z_bounds[1:-1]) > 0


@pytest.mark.parametrize("slabs", [2, 3])
@pytest.mark.parametrize("mode", ["default", "tsdf"])
def test_bunny_after_every_view(slabs, mode):
    opt = B.bunny_option(10.0, UpdateOption(**B.MODES[mode]))
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    masks = B.load_masks()
    whole = vc.VoxelCarver(opt)
    assert whole.Init(), vc.last_error()
    sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=slabs)
    assert sh.Init(), vc.last_error()
    for i in range(6):
        assert whole.CarveSilhouette(views[i], masks[i]), vc.last_error()
        for c in sh.slabs:
            assert c.CarveSilhouette(views[i], masks[i]), vc.last_error()
        assert run_params(whole, sh, "bunny %s view %d in %d slabs" % (mode, i, slabs)) > 0


@pytest.mark.parametrize("seed,iso", [(1, 0.0), (2, 0.0125), (3, -0.05)])
@pytest.mark.parametrize("z_bounds", [[0, 12, 24], [0, 7, 9, 16, 24], [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24]])
def test_uploaded_states_in_the_snap_band(seed, iso, z_bounds):
    """States within 1e-5 of the iso level, equal neighbours and dead voxels, uploaded slab by slab (the halo exchanged by
    the sharded carver): the argument order of VertexInterp at the seams, where a position depends on which cell of the
    slab below owns the edge."""
    n = 24
    opt = synth.sphere_option(n)
    whole = vc.VoxelCarver(opt)
    assert whole.Init(), vc.last_error()
    dims = whole.dims
    assert dims[2] == z_bounds[-1]
    sdf, cnt = snap_band_state(dims, seed, iso)
    whole.upload(sdf, cnt)
    sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=len(z_bounds) - 1, z_bounds=z_bounds)
    assert sh.Init(), vc.last_error()
    s = dims[0] * dims[1]
    for c, (z0, z1) in zip(sh.slabs, sh.z_ranges):
        c.upload(sdf[z0 * s:z1 * s], cnt[z0 * s:z1 * s])
    for level in (iso, 0.0, 0.1):
        for interp in (True, False):
            for mcskip in (0, 1):
                whole.set_param("mcskip", mcskip)
                sh.set_param("mcskip", mcskip)
                m = check_sharded(whole, sh, level, interp, "snap band seed %d cuts %s iso %g interp %s mcskip %d"
                                  % (seed, z_bounds[1:-1], level, interp, mcskip))
                assert len(m["vertices"]) > 1000


def test_slab_call_contract():
    """The old entry still refuses a slab; the new one needs the edge keys on a slab, takes any `which`, and an empty
    slab is a mesh without arrays."""
    opt, views, sdfs = sphere_scene()
    lib = capi.load()
    slab = vc.VoxelCarver(opt, z_range=(32, 64))
    low = vc.VoxelCarver(opt, z_range=(0, 32))
    assert slab.Init() and low.Init(), vc.last_error()
    for c in (slab, low):
        for v, s in zip(views, sdfs):
            assert c.Carve(v, s)
    vc.halo_exchange([low, slab])
    with pytest.raises(RuntimeError):
        slab.ExtractIsoSurface(0.0, True, normals=True)
    assert "whole grid" in vc.last_error()
    m, mn, lf = capi.Mesh(), capi.MeshNormals(), (C.c_int64 * 2)(7, 7)
    slab.set_param("meshkeys", 0)
    rc = lib.vcy_extract_iso_normals_slab(slab.ctx, 0.0, 1, capi.VCY_NORMALS_VERTEX, C.byref(m), C.byref(mn), lf)
    assert rc == capi.VCY_ERR_INVALID_ARG and "meshkeys" in vc.last_error()
    assert not m.vertices and not mn.vertex_normals and tuple(lf) == (0, 0)
    slab.set_param("meshkeys", 1)
    assert lib.vcy_extract_iso_normals_slab(slab.ctx, 0.0, 1, 4, C.byref(m), C.byref(mn), lf) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_extract_iso_normals_slab(slab.ctx, 0.0, 1, 1, C.byref(m), C.byref(mn), None) == capi.VCY_ERR_INVALID_ARG
    full = slab.ExtractIsoSurfaceSlab(0.0, True)
    plain = slab.ExtractIsoSurface(0.0, True)
    assert len(full["faces"]) > 0 and full["n_foreign"] == plain["n_foreign"] > 0 and full["normals_device_ms"] > 0
    for which in (0, capi.VCY_NORMALS_VERTEX, capi.VCY_NORMALS_FACE):
        rc = lib.vcy_extract_iso_normals_slab(slab.ctx, 0.0, 1, which, C.byref(m), C.byref(mn), lf)
        assert rc == 0, vc.last_error()
        assert m.n_vertices == len(full["vertices"]) and m.n_faces == len(full["faces"]) and tuple(lf) == full["layer_faces"]
        assert bool(mn.vertex_normals) == bool(which & 1) and bool(mn.face_normals) == bool(which & 2)
        v = np.ctypeslib.as_array(m.vertices, shape=(m.n_vertices * 3,)).reshape(-1, 3)
        assert same(v, plain["vertices"])
        if which & 1:
            assert same(np.ctypeslib.as_array(mn.vertex_normals, shape=(m.n_vertices * 3,)).reshape(-1, 3), full["normals"])
        if which & 2:
            assert same(np.ctypeslib.as_array(mn.face_normals, shape=(m.n_faces * 3,)).reshape(-1, 3), full["face_normals"])
        lib.vcy_mesh_free(C.byref(m))
        lib.vcy_mesh_normals_free(C.byref(mn))
    # a slab in empty space
    empty = vc.VoxelCarver(opt, z_range=(0, 4))
    assert empty.Init(), vc.last_error()
    for v, s in zip(views, sdfs):
        assert empty.Carve(v, s)
    e = empty.ExtractIsoSurfaceSlab(0.0, True)
    assert len(e["vertices"]) == len(e["faces"]) == len(e["normals"]) == len(e["face_normals"]) == 0 and e["layer_faces"] == (0, 0)
    # merge_meshes takes the two slabs' parts as they come
    merged = vdist.merge_meshes([low.ExtractIsoSurfaceSlab(0.0, True), full])
    whole = vc.VoxelCarver(opt)
    assert whole.Init()
    for v, s in zip(views, sdfs):
        assert whole.Carve(v, s)
    want = whole.ExtractIsoSurface(0.0, True, normals=True)
    assert same(merged["normals"], want["normals"]) and same(merged["face_normals"], want["face_normals"])


@pytest.mark.parametrize("slabs,iso,interp", [(3, 0.0, 1), (2, 0.1, 0), (8, 0.0, 1)])
def test_cpp_sharded_carver_equals_the_python_path(tmp_path, slabs, iso, interp):
    """vacancy::ShardedVoxelCarver::ExtractIsoSurface(mesh, iso, interp, with_normals = true) through host_selftest: the
    merged mesh and its normals equal the Python sharded carver's, which equal the whole-grid context's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([os.path.join(root, "vacancy_amd", "host", "host_selftest"), B.BUNNY, "shardnormals", "10",
                          str(slabs), str(tmp_path), repr(iso), str(interp)], check=True, capture_output=True, text=True).stdout
    opt = B.bunny_option(10.0, UpdateOption())
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    masks = B.load_masks()
    whole = vc.VoxelCarver(opt)
    assert whole.Init(), vc.last_error()
    sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=slabs)
    assert sh.Init(), vc.last_error()
    for v, m in zip(views, masks):
        assert whole.CarveSilhouette(v, m), vc.last_error()
        for c in sh.slabs:
            assert c.CarveSilhouette(v, m), vc.last_error()
    want = check_sharded(whole, sh, iso, bool(interp), "bunny res 10 in %d slabs" % slabs)
    got = sh.ExtractIsoSurface(iso, bool(interp), normals=True)
    nv, nf = len(want["vertices"]), len(want["faces"])
    assert nv > 0
    row = [l for l in out.splitlines() if l.startswith("SHARDNORMALS")][0].split()
    assert row == ["SHARDNORMALS", "1", str(slabs), str(nv), str(nf), str(nv), str(nf), str(nf)], row
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dt).reshape(-1, 3)  # noqa: E731
    assert same(rd("vertices.f32", np.float32), got["vertices"]) and np.array_equal(rd("faces.i32", np.int32), got["faces"])
    assert same(rd("normals.f32", np.float32), got["normals"])
    assert same(rd("face_normals.f32", np.float32), got["face_normals"])
