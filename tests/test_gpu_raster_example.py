"""examples/bunny --mesh-agreement: VoxelCarver::MeshAgreement of the example's final mesh (smoothed and decimated, and the
chain's) against Python's MeshAgreement of the same mesh on the same masks, with the hull's own counts beside it."""
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import chain_cases as CH
from vacancy_amd import synth
from vacancy_amd import carver as vc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")


def rows(stdout, tag):
    out = [l.split() for l in stdout.splitlines() if l.startswith(tag + " view ")]
    assert [r[2] for r in out] == [str(i) for i in range(len(out))], stdout
    return np.array([[int(x) for x in r[3:6]] for r in out], np.int64)


def test_bunny_example_mesh_agreement_equals_python(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    masks = B.load_masks()
    dev = CH.make_dev(B.bunny_option(10.0))
    for v, m in zip(views, masks):
        assert dev.CarveSilhouette(v, m), vc.last_error()
    hull = dev.HullAgreement(views, masks)

    # the separate calls, with two slabs beside them; then the chain
    for extra, slabs in ((["2"], True), (["--chain"], False)):
        run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10"] + extra +
                             ["--smooth", "2", "--decimate", "2", "--mesh-agreement"], check=True, capture_output=True, text=True)
        got, got_hull = rows(run.stdout, "MESH_AGREEMENT"), rows(run.stdout, "HULL_AGREEMENT")
        m = dev.ExtractIsoSurface(0.0, True)
        s = dev.SmoothMesh(m["vertices"], m["faces"], 2, **CH.TAUBIN)
        d = dev.DecimateMesh(s["vertices"], m["faces"], 20.0)
        want = dev.MeshAgreement(d["vertices"], d["faces"], views, masks)
        assert got.shape == (len(views), 3) and np.array_equal(got, want), (run.stdout, want)
        assert np.array_equal(got_hull, hull)
        # the counts say something: the mesh of a visual hull covers most of every silhouette, and it is not the voxel staircase
        assert (want[:, 0] > want[:, 1]).all() and not np.array_equal(want, hull)
        assert ("MESH_AGREEMENTSHARDED slabs 2 identical 1" in run.stdout) == slabs, run.stdout
        last = [l.split() for l in run.stdout.splitlines() if l.startswith("MESH_AGREEMENT verts ")]
        assert len(last) == 1 and int(last[0][2]) == len(d["vertices"]) and int(last[0][4]) == len(d["faces"]), last
        assert float(last[0][8]) > 0.0 and float(last[0][10]) > 0.0
