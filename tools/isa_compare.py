#!/usr/bin/env python
"""Compare the gfx950 device code of two checkouts, kernel by kernel (CPU only: hipcc cross-compiles).

    python tools/isa_compare.py <tree A> <tree B> [unit.hip ...]

Every unit of gnf_hip/build.py's SOURCES is compiled to device assembly with that tree's own FLAGS / EXTRA_FLAGS; comments
and the per-compile __hip_cuid_ symbol are dropped, the function ordinal in local labels is removed.  Per kernel: `same`, or the resources and instruction count of both sides.
Kernels that only changed their order in the unit (templates instantiated in another order) count as the same and are
reported as `reordered`.  Exit status 1 if anything differs."""
import os
import re
import runpy
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

KEYS = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size"]
# local symbols carry the function's ordinal in its unit (.LBB41_3, .Lfunc_end41): a function that only moved is the same
LOCAL = re.compile(r"\.L(BB|JTI|CPI|func_begin|func_end)\d+")


def device_asm(tree, unit, tmp):
    b = runpy.run_path(os.path.join(tree, "graphical-normalizing-flows_amd", "gnf_hip", "build.py"))
    if unit not in b["SOURCES"]:
        return None
    out = os.path.join(tmp, "%d_%s.s" % (abs(hash(tree)), unit))
    subprocess.run([b["_hipcc"]()] + b["FLAGS"] + b["EXTRA_FLAGS"].get(unit, []) +
                   ["--offload-device-only", "-S", os.path.join(b["CSRC"], unit), "-o", out], check=True)
    lines = []
    for ln in open(out):
        ln = LOCAL.sub(r".L\1", ln.split(";")[0].rstrip())
        if ln.strip() and "__hip_cuid_" not in ln:
            lines.append(ln)
    return lines


def split(lines):
    """-> ({function: body lines}, {kernel: metadata}, everything outside function bodies)"""
    funcs, meta, rest, cur = {}, {}, [], None
    names = {m.group(1) for m in (re.match(r"\s*\.type\s+([^,\s]+),@function", ln) for ln in lines) if m}
    for ln in lines:
        if cur is None and ln.endswith(":") and ln[:-1] in names:
            cur = ln[:-1]
            funcs[cur] = []
        elif cur is not None and ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            funcs[cur].append(ln)
        else:
            rest.append(ln)
    for entry in re.split(r"\n  - (?=\.)", "\n".join(rest)):
        name = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if name and ".vgpr_count" in entry:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", entry, re.M) if k in KEYS}
    return funcs, meta, rest


def describe(body, meta):
    n = sum(1 for ln in body if ln[:1] in " \t" and not ln.strip().startswith("."))
    return " ".join("%s=%s" % (k.replace("_count", "").replace("_fixed_size", ""), meta.get(k, "-")) for k in KEYS) + " instr=%d" % n


def main():
    a, b = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    units = sys.argv[3:] or runpy.run_path(os.path.join(b, "graphical-normalizing-flows_amd", "gnf_hip", "build.py"))["SOURCES"]
    differs = False
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(os.cpu_count() or 4) as pool:
        jobs = [(u, pool.submit(device_asm, a, u, tmp), pool.submit(device_asm, b, u, tmp)) for u in units]
        for u, ja, jb in jobs:
            la, lb = ja.result(), jb.result()
            if la is None or lb is None:
                print("%s: only in tree %s" % (u, "B" if la is None else "A"))
                differs = True
                continue
            (fa, ma, ra), (fb, mb, rb) = split(la), split(lb)
            print("%s: %d functions, %s" % (u, len(fb), "identical" if la == lb else "not identical, kernel by kernel:"))
            for k in sorted(set(fa) | set(fb)):
                if fa.get(k) == fb.get(k) and ma.get(k) == mb.get(k):
                    print("  same     %s" % k)
                    continue
                differs = True
                print("  DIFFERS  %s" % k)
                for side, f, m in (("A", fa, ma), ("B", fb, mb)):
                    print("    %s: %s" % (side, describe(f[k], m.get(k, {})) if k in f else "absent"))
            if sorted(ra) != sorted(rb):   # descriptors, metadata, data: reported once per unit
                differs = True
                print("  DIFFERS  (outside the function bodies)")
            elif ra != rb:               # the same lines: templates instantiated in another order move whole kernels (each in its
                print("  reordered  (outside the function bodies: the same lines in another order)")    # own section, 256-B aligned)
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
