#!/usr/bin/env python3
"""Is the gfx950 code of the carve / pre-pass kernels of two source trees the same?

  compare_carve_isa.py OLD_TREE NEW_TREE [--jobs N] [--work DIR [--reuse]]

For both trees: compiles every unit of vacancy_amd/csrc that holds carve or pre-pass kernels (carve_fused*.hip,
carve_prepass.hip) to assembly with the FLAGS of that tree's csrc/Makefile plus `-S --cuda-device-only` -- and
carve_fused_u8.hip once more with -DVCY_DEV_BENCH_KERNELS_ONLY -- splits the output per function (label to its
.Lfunc_end: instructions and the .amdhsa_kernel block; plus the function's `.set` resource lines and, for a kernel, its
entry of the metadata), and compares function by function, keyed by demangled name without the parameter list.

Normalised, because it cannot matter: comment-only lines and trailing comments; the __hip_cuid_* symbol; every mangled
symbol is replaced by its key (the parameter part of a mangled name changes when a parameter TYPE changes namespace);
and the function's index in local labels (.LBB<i>_<n>, .Lfunc_end<i>, .LJTI<i>_<n>), which is the position of the
function in the unit, i.e. symbol ORDER only.  Required: the same keys in both trees, every kernel exactly once across
NEW_TREE's units, identical text for every key.  Prints one summary line per unit of NEW_TREE; exit status 0 = same.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
MANGLED = re.compile(r"_Z[A-Za-z0-9_]+")


def units_of(tree):
    src = os.path.join(tree, "vacancy_amd", "csrc")
    names = sorted(glob.glob(os.path.join(src, "carve_fused*.hip")) + glob.glob(os.path.join(src, "carve_prepass.hip")))
    return src, [os.path.basename(n) for n in names]


def compile_cmd(src):
    out = subprocess.run(["make", "-s", "-C", src, "--no-print-directory", "--eval", "vcy-print-flags: ; @echo $(HIPCC) $(FLAGS)",
                          "vcy-print-flags"], check=True, capture_output=True, text=True).stdout
    return out.split()


def compile_unit(src, unit, extra, out, reuse):
    if not (reuse and os.path.exists(out)):
        subprocess.run(compile_cmd(src) + extra + ["-S", "--cuda-device-only", "-o", out, unit], cwd=src, check=True,
                       stderr=subprocess.DEVNULL)
    return out


def key_of(demangled):
    s = demangled.replace("(anonymous namespace)", "{anon}")
    depth = 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return s[:i]
    return s


def functions_of(path):
    """{key: (is_kernel, normalised text)} of one assembly file; a list of keys that occur more than once"""
    lines = open(path).read().split("\n")
    symbols = sorted(set(MANGLED.findall("\n".join(lines))))
    dem = subprocess.run([CXXFILT], input="\n".join(symbols), check=True, capture_output=True, text=True).stdout.split("\n")
    key = {s: key_of(d) for s, d in zip(symbols, dem)}

    def norm(line):
        line = line.split(";")[0].rstrip()
        line = MANGLED.sub(lambda m: "<" + key[m.group(0)] + ">", line)
        line = re.sub(r"__hip_cuid_\w+", "__hip_cuid", line)
        return re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI)\d+", r".\1", line)

    body, extra = {}, {}
    is_function = set(re.findall(r"^\s*\.type\s+(_Z[A-Za-z0-9_]+),@function", "\n".join(lines), re.M))
    cur = None
    for raw in lines:
        m = re.match(r"(_Z[A-Za-z0-9_]+):", raw)
        if m and cur is None and m.group(1) in is_function:
            cur = m.group(1)
            body.setdefault(cur, []).append([])
        if cur is not None:
            n = norm(raw)
            if n:
                body[cur][-1].append(n)
            if raw.startswith(".Lfunc_end"):
                cur = None
            continue
        m = re.match(r"\s*\.set (?:\.L)?(_Z[A-Za-z0-9_]+)\.", raw)
        if m:
            extra.setdefault(m.group(1), []).append(norm(raw))
    # metadata entries of the kernels
    text = "\n".join(lines)
    md = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.target", text, re.M | re.S)
    kernels = set()
    if md:
        for entry in re.split(r"^(?=  - \.)", md.group(1), flags=re.M):
            m = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
            if m:
                kernels.add(m.group(1))
                extra.setdefault(m.group(1), []).extend(norm(l) for l in entry.split("\n") if l.strip())
    out, dup = {}, []
    for sym, bodies in body.items():
        k = key[sym]
        if k in out or len(bodies) > 1:
            dup.append(k)
        out[k] = (sym in kernels, "\n".join(bodies[0] + extra.get(sym, [])))
    return out, dup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--work", help="keep the assembly files here")
    ap.add_argument("--reuse", action="store_true", help="take assembly files already in --work as they are")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="vcy_isa_")
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        for side, tree in (("old", a.old_tree), ("new", a.new_tree)):
            src, units = units_of(tree)
            os.makedirs(os.path.join(work, side), exist_ok=True)
            for build, extra in (("default", []), ("devbench", ["-DVCY_DEV_BENCH_KERNELS_ONLY"])):
                for u in units if build == "default" else ["carve_fused_u8.hip"]:
                    out = os.path.join(work, side, "%s.%s.s" % (u[:-4], build))
                    jobs[(build, side, u)] = pool.submit(compile_unit, src, u, extra, out, a.reuse)
    print("normalised: comments, __hip_cuid_*, mangled parameter suffixes, the function's index in local labels (symbol order)")
    ok, default_keys = True, set()
    for build in ("default", "devbench"):
        funcs = {"old": {}, "new": {}}    # side -> unit -> {key: (is_kernel, text)}
        for (b, side, u), job in jobs.items():
            if b == build:
                funcs[side][u], dup = functions_of(job.result())
                if dup:
                    ok = False
                    print("%s %s %s: defined more than once: %s" % (build, side, u, ", ".join(dup)))
        old_text = {}  # key -> set of texts over the old units
        for fs in funcs["old"].values():
            for k, (_, t) in fs.items():
                old_text.setdefault(k, set()).add(t)
        new_keys = {}
        for u, fs in sorted(funcs["new"].items()):
            differ = [k for k, (_, t) in fs.items() if k in old_text and t not in old_text[k]]
            added = [k for k in fs if k not in old_text]
            for k, (is_kernel, _) in fs.items():
                new_keys.setdefault(k, []).append((u, is_kernel))
            n_carve = sum(1 for k in fs if "carve_fused_kernel<" in k)
            print("%-8s %-20s %4d functions (%d carve_fused_kernel instances, %d other kernels, %d device functions): "
                  "%d identical, %d differ, %d not in the old tree" %
                  (build, u, len(fs), n_carve, sum(1 for k, v in fs.items() if v[0]) - n_carve,
                   sum(1 for v in fs.values() if not v[0]), len(fs) - len(differ) - len(added), len(differ), len(added)))
            for k in (differ + added)[:20]:
                print("    %s: %s" % ("differs" if k in differ else "new", k))
            ok = ok and not differ and not added
        # (the one unit of the devbench build: a kernel that left it for another unit is in the default build's list)
        missing = sorted(set(old_text) - set(new_keys) - (default_keys if build == "devbench" else set()))
        if build == "default":
            default_keys = set(new_keys)
        twice = sorted(k for k, where in new_keys.items() if where[0][1] and len(where) > 1)
        if missing:
            print("%s: in the old tree only: %s" % (build, ", ".join(missing[:20])))
        if twice:
            print("%s: kernels in more than one unit of the new tree: %s" % (build, ", ".join(twice)))
        ok = ok and not missing and not twice
    print("RESULT: %s" % ("identical device code" if ok else "DIFFERENT"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
