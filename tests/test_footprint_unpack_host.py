"""The two readings of a footprint record agree (host only, no GPU).

carve_fused.h unpacks the 8-byte record of a (brick, view) pair in two ways: unpack_footprint, the TileInfo the kernels
with an LDS TileInfo per view use, and the integer form for a wave that keeps the records packed in registers
(footprint_ub_word, footprint_ub, unpack_footprint_scalar, footprint_base, footprint_bounds).  tests/footprint_unpack_check.cpp
calls both for tw, th in {0, 1, 15}, tx0, ty0 in {0, 1, 8190, 8191}, every `sure` and every pair of ROI-edge bits, and
bounds +-0, negative, positive, +inf and the round-up that carried into +inf: every field the same, bit for bit."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scalar_unpack_equals_unpack_footprint(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is part of the image"
    exe = str(tmp_path / "footprint_unpack_check")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "vacancy_amd", "csrc"),
                        os.path.join(ROOT, "tests", "footprint_unpack_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "13824 records, 0 mismatches" in r.stdout
