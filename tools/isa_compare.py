#!/usr/bin/env python3
"""Per-kernel comparison of two builds' gfx950 assembly listings: are the code objects the same?

    for f in vr_brush vr_stamp ...; do hipcc <build.py's FLAGS> -S --cuda-device-only vrenderer_amd/csrc/$f.hip -o DIR/$f.s; done
    (once in a checkout of the parent commit, once at the head)
    python tools/isa_compare.py PARENT_DIR HEAD_DIR > profiles/<name>.txt

A kernel is `identical` when its body - every line between its label and its .Lfunc_end label, comments and blank lines dropped -
and its .amdhsa_ resource lines are the same text in both listings.  Exit status 1 if any kernel differs or is missing."""
import os
import re
import sys


def kernels(path):
    """{name: (body lines, {amdhsa key: value})} of one listing"""
    lines = open(path).read().splitlines()
    out = {}
    for name in [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        at = next(i for i, l in enumerate(lines) if l.strip() == ".amdhsa_kernel " + name)      # the descriptor stands between the last instruction and .Lfunc_end
        body = [t for t in (l.split(";")[0].strip() for l in lines[start + 1:at]) if t]
        stop = next(i for i in range(at, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        out[name] = (body, dict(l.split()[:2] for l in lines[at + 1:stop] if l.strip().startswith(".amdhsa_")))
    return out


def main():
    parent_dir, head_dir = sys.argv[1], sys.argv[2]
    print(f"{'file':12s} {'kernel':72s} {'instr':>6s} {'VGPR':>5s} {'SGPR':>5s} {'LDS':>6s} {'scratch':>7s}  identical")
    bad = 0
    for f in sorted(os.listdir(parent_dir)):
        if not f.endswith(".s"):
            continue
        a, b = kernels(os.path.join(parent_dir, f)), kernels(os.path.join(head_dir, f))
        for name in sorted(set(a) | set(b)):
            same = name in a and name in b and a[name] == b[name]
            bad += not same
            body, res = b.get(name) or a[name]
            instr = sum(1 for t in body if not re.match(r"^[.\w$]+:$", t) and not t.startswith("."))
            print(f"{f[:-2]:12s} {name:72s} {instr:6d} {res['.amdhsa_next_free_vgpr']:>5s} {res['.amdhsa_next_free_sgpr']:>5s} "
                  f"{res['.amdhsa_group_segment_fixed_size']:>6s} {res['.amdhsa_private_segment_fixed_size']:>7s}  {'yes' if same else 'NO'}")
    print(f"\n{'every kernel is identical' if not bad else str(bad) + ' kernel(s) differ'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
