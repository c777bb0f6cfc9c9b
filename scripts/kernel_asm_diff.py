#!/usr/bin/env python
"""CPU only: do the kernels of a translation unit compile to the same instructions at two commits?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S csrc/X.hip -o new.s
    (the same on a checkout of the other commit -> old.s)
    python scripts/kernel_asm_diff.py old.s new.s [--dropped-flag N]

Compares, kernel by kernel, the instruction text of every kernel of old.s with the kernel of the same name in new.s
(comments dropped; the kernel's own name in its labels and the numbering of local labels normalised). A kernel that
gained trailing template flags keeps its old instantiations under a longer mangled name: --dropped-flag N strips N
trailing `false` template arguments from the names of new.s before matching, and kernels of new.s that match no old
name are listed as new. Exit status 1 if a kernel of old.s is missing or differs.
"""
import argparse
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w*kernel\w*):", line)
        if m:
            cur = out[m.group(1)] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        text = line.split(";")[0].rstrip()
        if text.strip():
            cur.append(text)
    return out


def normalised(name, body):
    out = []
    for line in body:
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.replace(name, "K"))
        out.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", line))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--dropped-flag", type=int, default=0)
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    by_old_name = {}
    for name in new:
        key = re.sub(r"(Lb0E){%d}(EEv)" % a.dropped_flag, r"\2", name, count=1) if a.dropped_flag else name
        by_old_name.setdefault(key, name)
    same, bad = 0, 0
    for name, body in sorted(old.items()):
        if name not in by_old_name:
            print("missing in new:", name)
            bad += 1
            continue
        other = by_old_name[name]
        x, y = normalised(name, body), normalised(other, new[other])
        if x == y:
            same += 1
            continue
        bad += 1
        first = next(((p, q) for p, q in zip(x, y) if p != q), None)
        print(f"differs: {name} ({len(x)} / {len(y)} instruction lines), first difference: {first}")
    matched = set(by_old_name[n] for n in old if n in by_old_name)
    print(f"{same} kernels identical, {bad} missing or different, {len(new) - len(matched)} new in {a.new}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
