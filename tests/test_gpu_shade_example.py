"""examples/bunny --shade: VoxelCarver::ShadeMesh of the example's final mesh (smoothed and decimated, and the chain's) with
its normal map against Python's ShadeMesh of the same mesh: the pixel counts it prints and the PNGs it writes, byte for
byte."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bunny_data as B
import chain_cases as CH
from vacancy_amd import synth
from vacancy_amd import carver as vc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vacancy_amd", "host")


def read_rgb_png(path):
    """What WritePng8 emits for three channels: 8 bit, not interlaced, every row filter 0."""
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
    assert (depth, ctype, comp, flt, inter) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 3 * w + 1)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3)


def test_bunny_example_shades_what_python_shades(tmp_path):
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
    masks = B.load_masks()
    dev = CH.make_dev(B.bunny_option(10.0))
    for v, m in zip(views, masks):
        assert dev.CarveSilhouette(v, m), vc.last_error()
    m = dev.ExtractIsoSurface(0.0, True)
    s = dev.SmoothMesh(m["vertices"], m["faces"], 2, **CH.TAUBIN)
    d = dev.DecimateMesh(s["vertices"], m["faces"], 20.0, normals=True)
    attributes = np.float32(127.5) * d["normals"] + np.float32(127.5)   # (float, a product and a sum: the example's)
    assert attributes.dtype == np.float32
    want = dev.ShadeMesh(d["vertices"], d["faces"], attributes, views, value=False, value8=True)
    pixels = [int((w["value8"] != 0).any(axis=-1).sum()) for w in want]
    assert all(p > 1000 for p in pixels)

    # the separate calls, with two slabs beside them; then the chain
    for k, (extra, slabs) in enumerate(((["2"], True), (["--chain"], False))):
        out_dir, png_dir = tmp_path / ("out%d" % k), tmp_path / ("shade%d" % k)
        out_dir.mkdir()
        png_dir.mkdir()
        run = subprocess.run([os.path.join(HOST, "bunny"), B.BUNNY, str(out_dir), "10"] + extra +
                             ["--smooth", "2", "--decimate", "2", "--shade", str(png_dir)], check=True, capture_output=True, text=True)
        rows = [l.split() for l in run.stdout.splitlines() if l.startswith("SHADE view ")]
        assert [r[2] for r in rows] == [str(i) for i in range(len(views))], run.stdout
        assert [int(r[4]) for r in rows] == pixels, (run.stdout, pixels)
        for i, w in enumerate(want):
            png = read_rgb_png(str(png_dir / ("normal_%05d.png" % i)))
            assert png.shape == (B.HEIGHT, B.WIDTH, 3) and np.array_equal(png, w["value8"]), i
        assert ("SHADESHARDED slabs 2 identical 1" in run.stdout) == slabs, run.stdout
        last = [l.split() for l in run.stdout.splitlines() if l.startswith("SHADE verts ")]
        assert len(last) == 1 and int(last[0][2]) == len(d["vertices"]) and int(last[0][4]) == len(d["faces"]), last
        assert int(last[0][6]) == len(views) and float(last[0][8]) > 0.0 and float(last[0][10]) > 0.0
