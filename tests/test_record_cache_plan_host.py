"""Which launches reuse the footprint records of the last one, stated and checked without a GPU.

The rule is pure host code (vacancy_amd/csrc/carve_fused_plan.h: fused_records_cacheable, fused_reuses_records).  A launch
that never reuses gives the same voxel state and is only slower, so the GPU tests see half of it at best.
tests/record_cache_plan_host_check.cpp asks every condition of the rule on both sides, one named case each, and compares
with literals.  The second test builds the same program with the host sanitizers."""
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
                        os.path.join(ROOT, "tests", "record_cache_plan_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_record_reuse_rule_gives_the_stated_decisions(tmp_path):
    out = build_and_run(tmp_path, "record_cache_plan_host_check", [])
    m = re.search(r"(\d+) checks, 0 failures", out)
    assert m and int(m.group(1)) > 100, out[-500:]


def test_record_reuse_rule_under_the_host_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "record_cache_plan_host_check_san",
                        ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert ", 0 failures" in out
