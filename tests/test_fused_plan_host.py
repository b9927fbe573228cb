"""The decisions of a fused carve launch, stated and checked without a GPU.

Which instance of the fused carve kernel runs, over which grid, with which state flags and in chunks of how many brick
layers is decided by pure host code (vacancy_amd/csrc/carve_fused_plan.h: plan_fused_launch, plan_fused_chunk,
finish_fused_chunk, slab_image_rect).  Every flavour gives the same voxel state, so the GPU tests cannot see a driver
that picks another one.  tests/fused_plan_host_check.cpp asks every rule of DESIGN.md's table on both sides of its edge
and compares with literals.  The second test builds the same program with the host sanitizers.

The program also runs the two stages of the max_sdf reduction (max_reduce_kernel, carve_kernels.hip) as host loops over
the kernel's own pair order (vacancy_amd/csrc/max_element_pair.h) and compares with std::max_element: a NaN first pixel,
NaNs elsewhere, tied maxima, zeros of either sign, infinities."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path, name, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is part of the image"
    exe = str(tmp_path / name)
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off"] + extra +
                       ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "vacancy_amd", "csrc"),
                        os.path.join(ROOT, "tests", "fused_plan_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_fused_launch_plan_gives_the_stated_decisions(tmp_path):
    out = build_and_run(tmp_path, "fused_plan_host_check", [])
    m = re.search(r"(\d+) checks, 0 failures", out)
    assert m and int(m.group(1)) > 400, out[-500:]


def test_fused_launch_plan_under_the_host_sanitizers(tmp_path):
    """The same stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer (host code: the float-to-int
    conversions of the rectangle, the shifts and the 64-bit products of the chunk sizes are what could be undefined)."""
    out = build_and_run(tmp_path, "fused_plan_host_check_san",
                        ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert ", 0 failures" in out
