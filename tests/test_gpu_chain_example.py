"""examples/bunny --chain: VoxelCarver::ExtractIsoSurfaceChain against the separate members in the example itself, and the
mesh it writes against Python's chain on the same masks."""
import os
import subprocess

import numpy as np
import pytest

import bunny_data as B
import chain_cases as CH
import test_gpu_smooth as TGS
from vacancy_amd import synth
from vacancy_amd import carver as vc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")


def test_bunny_example_chain_is_identical_to_its_separate_calls_and_to_python(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "--smooth", "2", "--decimate", "2", "--decimate-mode",
                          "quadric", "--chain"], check=True, capture_output=True, text=True)
    row = [l.split() for l in run.stdout.splitlines() if l.startswith("CHAIN ")]
    assert len(row) == 1 and row[0][-2:] == ["identical", "1"], run.stdout
    assert row[0][1:5] == ["smooth", "2", "decimate", "2"] and row[0][5] == "extracted" and row[0][8] == "verts" and row[0][10] == "faces", row[0]
    verts, normals, faces = TGS.read_binary_ply(str(tmp_path / "surface_chain.ply"))

    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    dev = CH.make_dev(B.bunny_option(10.0))
    for v, m in zip(views, B.load_masks()):
        assert dev.CarveSilhouette(v, m), vc.last_error()
    got = dev.ExtractIsoChain(0.0, True, dict(iterations=2, pin_boundary=0, **CH.TAUBIN), dict(cell=20.0, regularize=1e-3))
    assert [int(row[0][k]) for k in (6, 7, 9, 11, 13)] == [got["extracted"][0], got["extracted"][1], len(verts), len(faces), got["n_fallback"]]
    assert 100 < len(verts) == len(got["vertices"]) < got["extracted"][0] and np.array_equal(faces, got["faces"])
    assert np.array_equal(CH.bits(verts), CH.bits(got["vertices"])) and np.array_equal(CH.bits(normals), CH.bits(got["normals"]))
    for key in ("extract_ms", "table_ms", "passes_ms", "cluster_ms", "quadric_ms", "faces_emit_ms", "normals_ms", "wall_ms"):
        assert float(row[0][row[0].index(key) + 1]) > 0.0, key

    bad = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(tmp_path), "10", "--chain"], capture_output=True, text=True)
    assert bad.returncode == 10, (bad.returncode, bad.stderr)
