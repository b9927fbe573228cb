"""The scalar helpers of the fused kernel's view step agree with unpack_footprint (host only, no GPU).

Between two views' runs the fused carve kernels that keep their footprint records in registers read a record's two words
with the integer helpers of carve_fused.h (footprint_tile_word, footprint_has_tile, footprint_sure, footprint_tx0 / _ty0,
footprint_step_base, footprint_row_groups, footprint_window_unclamped) and address the view records, the c0 records and
a view's image with 32-bit byte offsets (view_byte_offset, c0_byte_offset, tile_origin_bytes), which the host guards with
carve_offsets_fit_32.  tests/view_step_check.cpp compares each with unpack_footprint, the two-sided clamp test and 64-bit
arithmetic: every edge value of every field (tw in {0, 1, 2, 14, 15}, th around every row-group boundary, origins up to
8191, every `sure` and edge bit, six bounds), 400 000 random pairs of words, the clamp test at and around its threshold,
and the guard at 2^31 - 1 record, 2^31 and beyond.  The second test builds the same program with the host sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path, name, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is part of the image"
    exe = str(tmp_path / name)
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off"] + extra +
                       ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "vacancy_amd", "csrc"),
                        os.path.join(ROOT, "tests", "view_step_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_view_step_helpers_equal_unpack_footprint(tmp_path):
    out = build_and_run(tmp_path, "view_step_check", [])
    # 5 * 9 * 6 * 6 * 4 * 4 * 6 edge records + 400 000 random ones + the "no tile" record
    assert "555521 records," in out and ", 0 mismatches" in out


def test_view_step_helpers_under_the_host_sanitizers(tmp_path):
    """The same stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer (host code; shifts, signed
    differences and the 64-bit products of the guard are what could be undefined)."""
    out = build_and_run(tmp_path, "view_step_check_san",
                        ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert ", 0 mismatches" in out
