#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds kernel by kernel (no GPU needed).

    tools/isacmp.py PARENT_DIR NEW_DIR file.s [file.s ...] [--parent-sub REGEX REPL] [--table FRAGMENT ...]

Both directories hold `hipcc <the Makefile's flags> -S --cuda-device-only csrc/X.hip -o X.s`.  Comment lines, .file / .ident / .loc
lines and the numbers of temporary labels are stripped before the comparison.  Per file: "identical" or the number of differing
lines; for files that differ, every kernel is listed -- "identical" or its differing lines -- and kernels whose name contains
one of the --table fragments also get VGPR / SGPR / LDS / scratch / instruction counts of both builds.
--parent-sub renames the parent's kernels first (a template parameter that left)."""
import argparse
import difflib
import os
import re

META_KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def clean(line):
    line = line.split(";", 1)[0].rstrip()
    if not line.strip() or re.match(r"\s*\.(file|ident|loc)\b", line):
        return None
    return re.sub(r"\.L(BB|tmp|func_end|func_begin)\d+", r".L\1", line)         # .LBB12_3 -> .LBB_3: the function's number goes


def kernels(path, rename):
    """name -> (cleaned code lines, metadata dict)"""
    text = open(path).read()
    code = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        code[rename(m.group(1))] = [c for c in map(clean, m.group(2).split("\n")) if c is not None]
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n((?:    .*\n)+)", text):
        name = re.search(r"\.name:\s+(\S+)", m.group(1))
        if name:
            meta[rename(name.group(1))] = {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(META_KEYS), m.group(1))}
    return {k: (code[k], meta[k]) for k in meta if k in code}


def ndiff(a, b):
    return sum(1 for line in difflib.unified_diff(a, b, lineterm="", n=0) if line[:1] in "+-" and line[:3] not in ("+++", "---"))


def ninst(lines):
    return sum(1 for line in lines if re.match(r"\s+[a-z]", line) and not line.lstrip().startswith("."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--parent-sub", nargs=2, metavar=("REGEX", "REPL"))
    ap.add_argument("--table", nargs="*", default=[])
    a = ap.parse_args()
    sub = (lambda n: re.sub(a.parent_sub[0], a.parent_sub[1], n)) if a.parent_sub else (lambda n: n)
    for f in a.files:
        old, new = kernels(os.path.join(a.parent, f), sub), kernels(os.path.join(a.new, f), lambda n: n)
        same_names = sorted(old) == sorted(new)
        diffs = {k: ndiff(old[k][0], new[k][0]) for k in old if k in new}
        total = sum(diffs.values())
        verdict = "identical" if same_names and total == 0 else f"{total} lines differ"
        print(f"{f}: {len(new)} kernels (parent {len(old)}), names {'equal' if same_names else 'DIFFER'}: {verdict}")
        if verdict == "identical":
            continue
        for k in sorted(set(old) ^ set(new)):
            print(f"  only in {'parent' if k in old else 'new'}: {k}")
        rows = [k for k in sorted(diffs) if any(t in k for t in a.table)]
        for k in sorted(diffs):
            if k not in rows:
                print(f"  {k}: {'identical' if not diffs[k] else str(diffs[k]) + ' lines differ'}")
        if rows:
            print(f"  {'kernel':<78} {'VGPR':>9} {'SGPR':>9} {'LDS':>15} {'scratch':>9} {'instructions':>20}")
        for k in rows:
            (co, mo), (cn, mn) = old[k], new[k]
            io, inn = ninst(co), ninst(cn)
            cells = [f"{mo[key]}>{mn[key]}" if mo[key] != mn[key] else str(mn[key]) for key in META_KEYS]
            print(f"  {k:<78} {cells[0]:>9} {cells[1]:>9} {cells[2]:>15} {cells[3]:>9} {f'{io}>{inn} ({100.0 * (inn - io) / io:+.2f}%)':>20}")


if __name__ == "__main__":
    main()
