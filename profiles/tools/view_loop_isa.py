#!/usr/bin/env python3
"""Development aid (build machine, no GPU): what the view loop of one carve kernel instance is made of.

Compiles one carve unit device-only to assembly -- with the Makefile's flags, in a temporary directory outside the tree --
and prints, for the instance named on the command line, every basic block of its view loop with the counts of VALU,
SALU, v_mov_b32, ds_read and v_rcp instructions, which blocks are loop headers and latches (from the loop comments the
compiler writes into the assembly), and the kernel's register and scratch figures.  The view loop is the outermost loop
around the first block that holds eight v_rcp (a run over a lane's eight voxels).

  profiles/tools/view_loop_isa.py 'carve_fused_kernel<unsigned char, 0, false, true, false, 16, false, 2, 1>'
  profiles/tools/view_loop_isa.py --unit carve_fused_u16.hip 'carve_fused_kernel<unsigned short, 0, false, true, ...'

The instance is matched as a prefix of the demangled name (blanks ignored).  --asm FILE reads an assembly file that is
already there instead of compiling (a parent build's, for a before / after pair).  Writes nothing into the repository.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "vacancy_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
# (the flags of vacancy_amd/csrc/Makefile)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero", "-fno-slp-vectorize",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
NOT_SALU = ("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_setprio", "s_load", "s_buffer_load",
            "s_sleep", "s_memtime")


def compile_unit(unit, extra, out):
    cmd = [os.path.join(ROCM, "bin", "hipcc")] + FLAGS + extra + ["-S", "--cuda-device-only", "-o", out,
                                                                  os.path.join(CSRC, unit)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit(r.stdout)


def demangle(names):
    tools = [os.path.join(ROCM, "llvm", "bin", "llvm-cxxfilt"), "c++filt", "llvm-cxxfilt", "x86_64-linux-gnu-c++filt"]
    tool = next((t for t in tools if shutil.which(t)), None)
    if tool is None:
        sys.exit("no c++filt / llvm-cxxfilt on this machine")
    r = subprocess.run([tool], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True, check=True)
    return r.stdout.splitlines()


def squeeze(s):
    return re.sub(r"\s+", "", s).replace("(anonymousnamespace)::", "").replace("vcy::", "").replace("void", "", 1)


def function_blocks(lines):
    """[{name, ins, header_depth, loops}] of one function body, in layout order.  `loops`: the headers of the loops the
    block lies in, by depth, from the loop comments the compiler writes behind every block label."""
    blocks = [dict(name="entry", ins=[], header_depth=0, loops={})]
    for l in lines:
        m = re.match(r"^(?:(\.LBB\d+_\d+):|; (%bb\.\d+):)(.*)", l)
        if m:
            blocks.append(dict(name=m.group(1) or m.group(2), ins=[], header_depth=0, loops={}))
            l = ";" + m.group(3)
        b = blocks[-1]
        if l.strip().startswith(";"):
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", l) or re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", l)
            if m:
                b["loops"][int(m.group(2))] = "." + "L" + m.group(1)
            m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", l)
            if m:
                b["header_depth"] = int(m.group(1))
                b["loops"][int(m.group(1))] = b["name"]
        elif l.startswith("\t") and not l.strip().startswith((";", ".")):
            b["ins"].append(l.strip().split(";")[0].strip())
    # (a block of an inner loop only names that loop's header: the loops around it are the header's)
    by_name = {b["name"]: b for b in blocks}
    for b in blocks:
        for d in sorted(b["loops"], reverse=True):
            for dd, h in by_name.get(b["loops"][d], b)["loops"].items():
                b["loops"].setdefault(dd, h)
    return blocks


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("instance", help="demangled name of the kernel instance, or a prefix of it")
    ap.add_argument("--unit", default="carve_fused_u8.hip")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling")
    ap.add_argument("--all-blocks", action="store_true", help="every block of the kernel, not only the view loop")
    ap.add_argument("flags", nargs="*", help="extra compiler flags (after --)")
    a = ap.parse_args()

    with tempfile.TemporaryDirectory(prefix="view_loop_isa_") as tmp:
        path = a.asm
        if path is None:
            path = os.path.join(tmp, "unit.s")
            compile_unit(a.unit, a.flags, path)
        txt = open(path).read()

    syms = re.findall(r"^(_Z\w*carve_fused_kernel\w*):", txt, re.M)
    want = squeeze(a.instance)
    hits = [s for s, d in zip(syms, demangle(syms)) if squeeze(d).startswith(want)]
    if len(hits) != 1:
        print("%d instances match; the unit has:" % len(hits))
        for d in demangle(syms):
            print("  " + re.sub(r">\(.*", ">", d))
        sys.exit(1)
    sym = hits[0]
    start = txt.index("\n" + sym + ":") + 1
    end = txt.index(".Lfunc_end", start)
    blocks = function_blocks(txt[start:end].split("\n")[1:])
    tail = txt[end:]  # (the kernel's resource comments follow its body)
    print(re.sub(r">\(.*", ">", demangle([sym])[0]))
    for key in ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "Occupancy"):
        m = re.search(r"^; %s: (\d+)" % key, tail, re.M)
        if m:
            print("  %s %s" % (key, m.group(1)))

    hot = [b for b in blocks if sum(s.startswith("v_rcp") for s in b["ins"]) >= 8 and 1 in b["loops"]]
    if not hot:
        sys.exit("no loop with a block of eight v_rcp in this instance")
    top = hot[0]["loops"][1]
    loop = blocks if a.all_blocks else [b for b in blocks if b["loops"].get(1) == top]
    inner = [b["name"] for b in loop if b["header_depth"] > 1]
    print("  view loop: header %s, %d blocks; loops inside it: %s" % (top, len(loop), ", ".join(inner) or "none"))
    print("  %-12s %5s %5s %5s %9s %7s %5s  %s" % ("block", "insts", "VALU", "SALU", "v_mov_b32", "ds_read", "v_rcp", ""))
    headers = {b["name"] for b in loop if b["header_depth"]}
    tot = [0] * 6
    for b in loop:
        ins = b["ins"]
        c = [len(ins), sum(s.startswith("v_") for s in ins),
             sum(s.startswith("s_") and not s.startswith(NOT_SALU) for s in ins),
             sum(s.startswith("v_mov_b32") for s in ins), sum(s.startswith("ds_read") for s in ins),
             sum(s.startswith("v_rcp") for s in ins)]
        tot = [x + y for x, y in zip(tot, c)]
        notes = []
        if b["header_depth"]:
            notes.append("header (depth %d)" % b["header_depth"])
        back = [m.group(1) for s in ins for m in [re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", s)] if m and m.group(1) in headers
                and b["loops"].get(next(x["header_depth"] for x in loop if x["name"] == m.group(1))) == m.group(1)]
        if back:
            notes.append("latch -> " + ", ".join(back))
        if c[5] >= 7:
            notes.append("run")
        print("  %-12s %5d %5d %5d %9d %7d %5d  %s" % (b["name"], c[0], c[1], c[2], c[3], c[4], c[5], "; ".join(notes)))
    print("  %-12s %5d %5d %5d %9d %7d %5d" % ("total", *tot))


if __name__ == "__main__":
    main()
