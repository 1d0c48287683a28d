#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    tools/isa_compare.py BEFORE_DIR AFTER_DIR [--list]

Both directories hold the assembly of the same translation units, written by

    hipcc <flags of uno_amd/build.py, per-source extra flags included> --cuda-device-only -S file.hip -o DIR/file.s

A kernel is "identical" when its instruction stream (and its kernel descriptor) is the same line by line after dropping comments and
the function index in basic-block labels (.LBB<n>_k, .Lfunc_end<n>: they number the functions of a unit, so a changed include or
instantiation order renumbers them).  A kernel that differs is printed with instruction count, VGPRs, AGPRs, scratch bytes per lane
and waves per SIMD on both sides (the figures the assembler comments carry, the same that -Rpass-analysis=kernel-resource-usage prints).
Exit status 1 if any kernel differs or exists on one side only.  profiles/k1_shared_stages_isa.txt and k3_shared_stages_isa.txt were
made this way."""
import argparse
import os
import re
import shutil
import subprocess
import sys

_LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+")
_FIGURES = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("scratch", "ScratchSize"), ("waves", "Occupancy"))


def kernels(path):
    """-> {mangled name: (normalised lines, figures)} of the __global__ functions in an assembly file"""
    out = {}
    lines = open(path).read().split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        body, fig = [], {}
        i += 1
        while i < len(lines) and not re.match(r"\.Lfunc_end\d+:", lines[i]):
            txt = lines[i].split(";")[0].strip()
            if txt:
                body.append(_LABEL.sub(r".\1", " ".join(txt.split())))
            i += 1
        while i < len(lines) and not re.match(r"\s*\.(globl|type)\s", lines[i]):
            for key, word in _FIGURES:
                mm = re.match(r";\s*%s:\s*(\d+)" % word, lines[i])
                if mm and key not in fig:
                    fig[key] = int(mm.group(1))
            i += 1
        if any(l.startswith(".amdhsa_kernel") for l in body):
            fig["instr"] = sum(1 for l in body[:body.index(next(l for l in body if l.startswith(".amdhsa_kernel")))]
                               if not l.startswith(".") and not l.endswith(":"))
            out[name] = (body, fig)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
        nice = [re.sub(r"^void uno::|\(uno::Dft2dParams\)$|\(.*\)$", "", n) for n in r.stdout.split("\n")]
        return dict(zip(names, nice))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def _fig(f):
    return "{instr} instructions, {vgpr} VGPRs, {agpr} AGPRs, scratch {scratch} B/lane, {waves} waves/SIMD".format(**f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--list", action="store_true", help="print the verdict of every kernel, not only of those that differ")
    a = ap.parse_args()
    units = sorted(f for f in os.listdir(a.before) if f.endswith(".s"))
    bad = 0
    for unit in units:
        if not os.path.exists(os.path.join(a.after, unit)):
            print(f"== {unit}: missing in {a.after}")
            bad += 1
            continue
        old, new = kernels(os.path.join(a.before, unit)), kernels(os.path.join(a.after, unit))
        nice = demangle(sorted(set(old) | set(new)))
        same = [n for n in old if n in new and old[n][0] == new[n][0]]
        print(f"== {os.path.splitext(unit)[0]}.hip: {len(old)} kernels, {len(same)} identical")
        for n in sorted(set(old) | set(new), key=lambda n: nice[n]):
            if n not in old or n not in new:
                print(f"{nice[n]:<50} only in {'after' if n in new else 'before'}")
                bad += 1
            elif n in same:
                if a.list:
                    print(f"{nice[n]:<50} identical")
            else:
                bad += 1
                gained = new[n][1]["scratch"] > old[n][1]["scratch"] or new[n][1]["waves"] < old[n][1]["waves"]
                print(f"{nice[n]:<50} DIFFERS{' (more scratch or fewer waves)' if gained else ''}\n    before: {_fig(old[n][1])}\n    after:  {_fig(new[n][1])}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
