"""The C++ layer of the ray-cast over z-slabs on the GPU: ShardedVoxelCarver::RenderHullSlabs / HullAgreementSlabs must
give what VoxelCarver::RenderHull / HullAgreement give on the same carve (host_selftest slabrender), and the example must
say so when it renders with slabs (`examples/bunny <data> <out> 10 3 --render DIR`)."""
import os
import subprocess

import pytest

import bunny_data as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")


def test_selftest_slabrender():
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    r = subprocess.run([os.path.join(HOST, "host_selftest"), B.BUNNY, "slabrender", "10", "3"], check=True,
                       capture_output=True, text=True)
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("SLABRENDER")]
    # slabs | depth bytes equal, silhouette equal, counts equal
    assert rows == [["SLABRENDER", "3", "1", "1", "1"]], r.stdout + r.stderr


def test_bunny_example_compares_the_sharded_render(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    out_dir, png_dir = tmp_path / "out", tmp_path / "hull"
    out_dir.mkdir()
    png_dir.mkdir()
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(out_dir), "10", "3", "--render", str(png_dir)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [l for l in run.stdout.splitlines() if l.startswith("RENDERSHARDED")]
    assert lines == ["RENDERSHARDED slabs 3 views 6 depth and counts identical 1"], run.stdout
    assert len([l for l in run.stdout.splitlines() if l.startswith("RENDER view")]) == 6
    assert sorted(os.listdir(str(png_dir))) == ["hull_%05d.png" % i for i in range(6)]
