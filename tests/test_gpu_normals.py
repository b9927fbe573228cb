"""Normals of the iso surface on the device (vcy_extract_iso_normals, mc_normals.hip) against the reference's
Mesh::CalcNormal: every test asserts (a) the mesh arrays are bit-equal to ExtractIsoSurface without normals on the same
context, (b) the device normals are bit-equal to vcy_mesh_normals_host on that mesh, (c) and to the numpy restatement
of mesh.cc:197-240 (tests/normals_ref.py)."""
import threading

import numpy as np
import pytest

import bunny_data as B
import normals_ref as NR
import oracle_lib as O
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import synth
from vacancy_amd.capi import UpdateOption

pytestmark = pytest.mark.gpu


def check_normals(dev, iso, interp, ctx=""):
    plain = dev.ExtractIsoSurface(iso, interp)
    m = dev.ExtractIsoSurface(iso, interp, normals=True)
    assert m["vertices"].shape == plain["vertices"].shape and m["faces"].shape == plain["faces"].shape, ctx
    assert np.array_equal(NR.bits(m["vertices"]), NR.bits(plain["vertices"])), ctx + " vertex bits differ"
    assert np.array_equal(m["faces"], plain["faces"]), ctx + " faces differ"
    assert np.array_equal(m["keys"], plain["keys"]), ctx + " keys differ"
    assert m["n_foreign"] == plain["n_foreign"] == 0
    assert m["normals"].shape == m["vertices"].shape and m["face_normals"].shape == m["faces"].shape, ctx
    hvn, hfn = vc.mesh_normals_host(m["vertices"], m["faces"])
    rvn, rfn = NR.mesh_normals(m["vertices"], m["faces"])
    for name, got, host, ref in (("face", m["face_normals"], hfn, rfn), ("vertex", m["normals"], hvn, rvn)):
        bad_h = int((NR.bits(got) != NR.bits(host)).any(axis=1).sum()) if len(got) else 0
        bad_r = int((NR.bits(got) != NR.bits(ref)).any(axis=1).sum()) if len(got) else 0
        print("%s %s normals: %d rows, %d differ from the host walk, %d from numpy" % (ctx, name, len(got), bad_h, bad_r))
        assert bad_h == 0, "%s: %d of %d %s normals differ from vcy_mesh_normals_host" % (ctx, bad_h, len(got), name)
        assert bad_r == 0, "%s: %d of %d %s normals differ from the numpy restatement" % (ctx, bad_r, len(got), name)
    assert m["normals_device_ms"] >= 0.0
    return m


def carved_sphere(n, nv=4, uo=None, w=160, h=120):
    opt = synth.sphere_option(n, uo)
    views, masks = synth.sphere_views(n, nv, w, h)
    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    for i in range(nv):
        assert dev.CarveSilhouette(views[i], masks[i]), vc.last_error()
    return dev


@pytest.mark.parametrize("res", [10.0, 2.5])
@pytest.mark.parametrize("mode", ["default", "tsdf"])
def test_bunny_after_every_view(res, mode):
    """Item 5: the bunny after each of the six views, linear_interp on and off, kMax and weighted average with truncation."""
    uo = UpdateOption(**B.MODES[mode])
    opt = B.bunny_option(res, uo)
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    masks = B.load_masks()
    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    for i in range(6):
        assert dev.CarveSilhouette(views[i], masks[i]), vc.last_error()
        for interp in (True, False):
            m = check_normals(dev, 0.0, interp, "bunny res %g %s view %d interp=%s" % (res, mode, i, interp))
            assert len(m["vertices"]) > 0


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("mcskip", [0, 2])
@pytest.mark.parametrize("meshkeys", [1, 0])
def test_sphere_paths(n, mcskip, meshkeys):
    """Item 6: brick skipping on and off, "mcdirect" forced off and on (threshold below and above the mesh), with and
    without edge keys: the normals do not depend on how the mesh reaches the host."""
    dev = carved_sphere(n)
    dev.set_param("mcskip", mcskip)
    dev.set_param("meshkeys", meshkeys)
    got = []
    for direct in (0, 1 << 30, 1 << 12):
        dev.set_param("mcdirect", direct)
        for interp in (True, False):
            # (without keys the plain extraction returns none either)
            plain = dev.ExtractIsoSurface(0.0, interp)
            m = dev.ExtractIsoSurface(0.0, interp, normals=True)
            assert np.array_equal(NR.bits(m["vertices"]), NR.bits(plain["vertices"]))
            assert np.array_equal(m["faces"], plain["faces"]) and np.array_equal(m["keys"], plain["keys"])
            hvn, hfn = vc.mesh_normals_host(m["vertices"], m["faces"])
            rvn, rfn = NR.mesh_normals(m["vertices"], m["faces"])
            assert np.array_equal(NR.bits(m["normals"]), NR.bits(hvn)) and np.array_equal(NR.bits(m["normals"]), NR.bits(rvn))
            assert np.array_equal(NR.bits(m["face_normals"]), NR.bits(hfn))
            assert np.array_equal(NR.bits(m["face_normals"]), NR.bits(rfn))
            got.append((interp, m["normals"]))
    for interp, vn in got:
        first = next(v for i, v in got if i == interp)
        assert np.array_equal(NR.bits(vn), NR.bits(first))


def snap_band_state(dims, seed, iso):
    """A state in the snap band of VertexInterp: values within 1e-5 of the iso level, equal neighbours, never-updated
    voxels (invalid cells), and a surface that touches every face of the grid."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    n = nx * ny * nz
    base = rng.choice(np.array([-0.3, -0.05, 0.05, 0.3, 0.3], np.float32), size=n)
    near = (np.float32(iso) + rng.choice(np.array([-9e-6, -2e-6, 0.0, 2e-6, 9e-6, 2e-5, -2e-5], np.float32), size=n))
    sdf = np.where(rng.random(n) < 0.35, near, base).astype(np.float32)
    cnt = np.ones(n, np.int32)
    dead = rng.random(n) < 0.02
    sdf[dead] = np.finfo(np.float32).min
    cnt[dead] = 0
    return sdf, cnt


@pytest.mark.parametrize("seed,iso", [(1, 0.0), (2, 0.0125), (3, -0.05)])
def test_uploaded_states_in_the_snap_band(seed, iso):
    """Item 7 (and 8: the noise follows a small mesh on the same context, so the sizes guessed from the last extraction
    are too small and the chain -- normals included -- runs again).  Condition, checked on the CPU with the oracle's
    marching cubes and asserted here: the mesh has at least one zero-area face and at least one vertex on an edge of
    the grid's border (fewer than four cells around it)."""
    n = 24
    opt = synth.sphere_option(n)
    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    orc = O.OracleGrid(opt)
    dims = dev.dims
    # a small smooth mesh first: its sizes are the next extraction's guess
    zz, yy, xx = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    ball = (np.sqrt((xx - 12.0) ** 2 + (yy - 12.0) ** 2 + (zz - 12.0) ** 2) - 3.0).astype(np.float32).reshape(-1)
    dev.upload(ball, np.ones(ball.size, np.int32))
    small = check_normals(dev, 0.0, True, "small ball")
    sdf, cnt = snap_band_state(dims, seed, iso)
    dev.upload(sdf, cnt)
    orc.upload(sdf, cnt)
    for interp in (True, False):
        om = orc.marching_cubes(iso, interp)
        ovn, ofn = NR.mesh_normals(om["vertices"], om["faces"])
        zero_area = int((ofn == 0).all(axis=1).sum())
        k = om["keys"]
        cx, cy, cz = k % dims[0], (k // dims[0]) % dims[1], k // (dims[0] * dims[1])
        # an edge along an axis lies on the border when both its other coordinates... one of them sits on a grid face
        along = np.stack([cx[:, 0] != cx[:, 1], cy[:, 0] != cy[:, 1], cz[:, 0] != cz[:, 1]], axis=1)
        on_face = np.stack([(cx[:, 0] == 0) | (cx[:, 0] == dims[0] - 1), (cy[:, 0] == 0) | (cy[:, 0] == dims[1] - 1),
                            (cz[:, 0] == 0) | (cz[:, 0] == dims[2] - 1)], axis=1)
        border = int((on_face & ~along).any(axis=1).sum())
        print("seed %d iso %g interp %s: %d faces, %d zero-area, %d border vertices" % (seed, iso, interp, len(ofn), zero_area, border))
        assert zero_area >= 1 and border >= 1
        assert len(om["vertices"]) > 2 * len(small["vertices"])  # (the guess was too small: the rerun path)
        dev.upload(ball, np.ones(ball.size, np.int32))
        dev.ExtractIsoSurface(0.0, True)
        dev.upload(sdf, cnt)
        m = dev.ExtractIsoSurface(iso, interp, normals=True)
        assert np.array_equal(NR.bits(m["vertices"]), NR.bits(om["vertices"])) and np.array_equal(m["faces"], om["faces"])
        assert np.array_equal(NR.bits(m["normals"]), NR.bits(ovn)), "vertex normals differ from numpy on the oracle's mesh"
        assert np.array_equal(NR.bits(m["face_normals"]), NR.bits(ofn))
        check_normals(dev, iso, interp, "snap band seed %d interp=%s" % (seed, interp))


def test_eight_contexts_on_eight_streams():
    """Item 9: eight contexts extract with normals at the same time from eight host threads."""
    n, nv = 128, 5
    ctxs = [carved_sphere(n, nv) for _ in range(8)]
    for c in ctxs:
        c.sync()
    isos = [0.0, 0.013, -0.02]
    ref = ctxs[0]
    want = []
    for iso in isos:
        m = ref.ExtractIsoSurface(iso, True)
        want.append((m, NR.mesh_normals(m["vertices"], m["faces"])))
    errors = []
    outs = [[] for _ in ctxs]

    def run(c, out):
        try:
            for rnd in range(3):
                for k, iso in enumerate(isos):
                    out.append((k, c.ExtractIsoSurface(iso, True, normals=True)))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    ths = [threading.Thread(target=run, args=(c, o)) for c, o in zip(ctxs, outs)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=300)
    assert not errors, errors
    assert all(not t.is_alive() for t in ths)
    for o in outs:
        assert len(o) == 3 * len(isos)
        for k, m in o:
            pm, (rvn, rfn) = want[k]
            assert np.array_equal(NR.bits(m["vertices"]), NR.bits(pm["vertices"])) and np.array_equal(m["faces"], pm["faces"])
            assert np.array_equal(NR.bits(m["normals"]), NR.bits(rvn))
            assert np.array_equal(NR.bits(m["face_normals"]), NR.bits(rfn))


@pytest.mark.parametrize("world", [2, 4])
def test_slab_contexts_and_the_sharded_carver(world):
    """Item 10: a slab context refuses (VCY_ERR_UNSUPPORTED, with a message); the sharded carver's normals -- the host
    walk over the merged mesh -- equal the single-context device result bit for bit."""
    import ctypes as C
    from vacancy_amd import sharded
    n, nv = 64, 5
    opt = synth.sphere_option(n)
    views, masks = synth.sphere_views(n, nv, 160, 120)
    sdfs = [vc.make_sdf(m) for m in masks]
    whole = vc.VoxelCarver(opt)
    assert whole.Init(), vc.last_error()
    for i in range(nv):
        assert whole.Carve(views[i], sdfs[i])
    slab = vc.VoxelCarver(opt, z_range=(n // 2, n))
    assert slab.Init(), vc.last_error()
    lib = capi.load()
    m, mn = capi.Mesh(), capi.MeshNormals()
    rc = lib.vcy_extract_iso_normals(slab.ctx, 0.0, 1, capi.VCY_NORMALS_VERTEX, C.byref(m), C.byref(mn))
    assert rc == capi.VCY_ERR_UNSUPPORTED and "whole grid" in vc.last_error()
    assert not m.vertices and not mn.vertex_normals
    with pytest.raises(RuntimeError):
        slab.ExtractIsoSurface(0.0, True, normals=True)
    sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=world)
    assert sh.Init(), vc.last_error()
    for c in sh.slabs:
        for i in range(nv):
            assert c.Carve(views[i], sdfs[i])
    for iso, interp in ((0.0, True), (0.1, False)):
        want = check_normals(whole, iso, interp, "whole grid")
        got = sh.ExtractIsoSurface(iso, interp, normals=True)
        assert np.array_equal(NR.bits(got["vertices"]), NR.bits(want["vertices"])) and np.array_equal(got["faces"], want["faces"])
        assert np.array_equal(NR.bits(got["normals"]), NR.bits(want["normals"]))
        assert np.array_equal(NR.bits(got["face_normals"]), NR.bits(want["face_normals"]))


def test_full_size_property_512():
    """Item 11: 512^3, 16 views: device normals == the host walk; unit length within a few ulp wherever the host normal
    is not zero."""
    dev = carved_sphere(512, 16, w=640, h=480)
    m = dev.ExtractIsoSurface(0.0, True, normals=True)
    plain = dev.ExtractIsoSurface(0.0, True)
    assert np.array_equal(NR.bits(m["vertices"]), NR.bits(plain["vertices"])) and np.array_equal(m["faces"], plain["faces"])
    assert len(m["vertices"]) > 500000
    hvn, hfn = vc.mesh_normals_host(m["vertices"], m["faces"])
    assert np.array_equal(NR.bits(m["normals"]), NR.bits(hvn))
    assert np.array_equal(NR.bits(m["face_normals"]), NR.bits(hfn))
    nz = (hvn != 0).any(axis=1)
    length = np.sqrt((hvn[nz].astype(np.float64) ** 2).sum(axis=1))
    # v / sqrt(n2) per component: each component within 1 ulp (division) + 0.5 ulp (sqrt) + 1.5 ulp (n2) of exact
    assert np.abs(length - 1.0).max() <= 4 * np.finfo(np.float32).eps
    print("512^3: %d vertices, %d faces, extract %.3f ms + normals %.3f ms on the device"
          % (len(m["vertices"]), len(m["faces"]), m["device_ms"], m["normals_device_ms"]))


def test_cpp_facade_overload_equals_the_python_path(tmp_path):
    """Item 12: VoxelCarver::ExtractIsoSurface(mesh, iso, interp, with_normals = true) through examples/bunny.cc, which
    writes the last view's mesh with normals as a binary PLY: positions, normals and faces equal the Python path's."""
    import os
    import subprocess
    from test_mesh_normals import read_ply
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([os.path.join(root, "vacancy_amd", "host", "bunny"), B.BUNNY, str(tmp_path), "10"],
                         check=True, capture_output=True, text=True).stdout
    opt = B.bunny_option(10.0, UpdateOption())
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    for view, mask in zip(views, B.load_masks()):
        assert dev.CarveSilhouette(view, mask), vc.last_error()
    m = check_normals(dev, 0.0, True, "bunny res 10")
    row = [l for l in out.splitlines() if l.startswith("NORMALS")][0].split()
    assert row == ["NORMALS", "view", "5", "verts", str(len(m["vertices"])), "normals", str(len(m["vertices"])),
                   "face_normals", str(len(m["faces"]))], row
    header, props, vrec, faces = read_ply(str(tmp_path / "surface_normals_00005.ply"))
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(NR.bits(vrec[:, :3]), NR.bits(m["vertices"]))
    assert np.array_equal(NR.bits(vrec[:, 3:]), NR.bits(m["normals"]))
    assert np.array_equal(faces, m["faces"])
