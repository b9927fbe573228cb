"""The C++ layer of the ray-cast of the hull on the GPU: `examples/bunny <data> <out> 10 --render DIR` (VoxelCarver::
RenderHull and HullAgreement) must write the silhouettes and print the counts that Python's RenderHull / HullAgreement
give on the same carve, and ShardedVoxelCarver must refuse both calls (host_selftest shardrender)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bunny_data as B
from vacancy_amd import carver as vc
from vacancy_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")


def read_gray_png(path):
    """What WritePng8 emits for one channel: 8 bit, not interlaced, every row filter 0."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(raw):
        (ln,), typ = struct.unpack(">I", raw[pos:pos + 4]), raw[pos + 4:pos + 8]
        body = raw[pos + 8:pos + 8 + ln]
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + ln
    w, h, depth, ctype, comp, flt, inter = ihdr
    assert (depth, ctype, comp, flt, inter) == (8, 0, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w + 1)
    assert not rows[:, 0].any()
    return rows[:, 1:]


def test_bunny_example_renders_what_python_renders(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    out_dir, png_dir = tmp_path / "out", tmp_path / "hull"
    out_dir.mkdir()
    png_dir.mkdir()
    run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(out_dir), "10", "--render", str(png_dir)],
                         check=True, capture_output=True, text=True)
    rows = [l.split() for l in run.stdout.splitlines() if l.startswith("RENDER view")]
    assert len(rows) == 6, run.stdout

    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    masks = B.load_masks()
    dev = vc.VoxelCarver(B.bunny_option(10.0))
    assert dev.Init(), vc.last_error()
    for v, m in zip(views, masks):                       # the example's own sequence: one view per call
        assert dev.CarveSilhouette(v, m), vc.last_error()
    images = dev.RenderHull(views, 0.0)
    counts = dev.HullAgreement(views, masks)
    for i, r in enumerate(rows):
        # RENDER view <i> mask&hull <a> mask-only <b> hull-only <c> IoU <x>
        assert r[2] == str(i) and [r[3], r[5], r[7], r[9]] == ["mask&hull", "mask-only", "hull-only", "IoU"], r
        got = [int(r[4]), int(r[6]), int(r[8])]
        assert got == counts[i].tolist(), (i, got, counts[i])
        union = sum(got)
        assert union > 0 and abs(float(r[10]) - got[0] / union) <= 0.5e-4 + 1e-12, r
        png = read_gray_png(str(png_dir / ("hull_%05d.png" % i)))
        want = np.where(np.isfinite(images[i]["depth"]), 255, 0).astype(np.uint8)
        assert png.shape == (B.HEIGHT, B.WIDTH) and np.array_equal(png, want), i
        assert int((want != 0).sum()) == got[0] + got[2] > 1000

    # --render without its value ends with a message and a code of its own, before anything is carved
    bad = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(out_dir), "10", "--render"], capture_output=True, text=True)
    assert bad.returncode == 10 and "--render needs a directory" in bad.stderr


def test_sharded_carver_refuses_and_bad_arguments_are_logged():
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    r = subprocess.run([os.path.join(HOST, "host_selftest"), B.BUNNY, "shardrender", "10", "3"], check=True,
                       capture_output=True, text=True)
    row = [l.split() for l in r.stdout.splitlines() if l.startswith("SHARDRENDER")][0]
    # slabs | sharded RenderHull, sharded HullAgreement, null depth, count mismatch, no list, before Init | a good call
    assert row[1:] == ["3", "0", "0", "0", "0", "0", "0", "1"], row
    log = r.stdout + r.stderr
    for text in ("ShardedVoxelCarver::RenderHull", "ShardedVoxelCarver::HullAgreement", "needs a depth image",
                 "one silhouette per camera", "has not been initialized"):
        assert text in log, text
