#!/usr/bin/env python3
"""Compare two sets of `make isa` listings kernel by kernel.

  python tools/isa_compare.py --a OLD/isa/*.s --b NEW/isa/*.s [--allow REGEX]

Kernels are paired by mangled name, whichever listing of a set holds them.  A
kernel's text is its instructions with comments stripped and the function's
local labels (.LBB<n>_<m>, .Lfunc_end<n>) renumbered in order of appearance;
its descriptor is the .amdhsa_kernel block.  Prints one line per kernel and
exits 1 unless both sets hold the same kernels and every kernel is identical.
--allow: kernels whose name matches may differ in text and in the descriptor's
SGPR fields if VGPRs, LDS and scratch are equal, SGPRs are not higher in B and
the instruction count is within 1 % of A's.
"""
import argparse
import re
import sys

LABEL = re.compile(r"\.LBB\d+_\d+|\.Lfunc_(?:begin|end)\d+")
SGPR_FIELDS = (".amdhsa_next_free_sgpr", ".amdhsa_reserve_vcc", ".amdhsa_reserve_xnack_mask")
HELD_EQUAL = (".amdhsa_next_free_vgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size")


def strip(line):
    return line.split(";", 1)[0].strip()


def parse(paths):
    """{kernel: (text lines, {descriptor field: value})} over the listings"""
    bodies, desc = {}, {}
    for path in paths:
        name = fields = None   # the function, the descriptor block the lines are in
        for line in open(path):
            t = strip(line)
            m = re.match(r"\.type\s+(\S+),@function", t)
            if m:
                name, names = m.group(1), {}
                bodies[name] = []
            elif name is None or not t or t == name + ":":
                pass
            elif re.match(r"\.Lfunc_end\d+:", t):
                name = None
            elif t.startswith(".amdhsa_kernel"):
                fields = desc[name] = {}
            elif t.startswith(".end_amdhsa_kernel"):
                fields = None
            elif fields is not None:
                f = t.split(None, 1)
                fields[f[0]] = f[1] if len(f) > 1 else ""
            else:
                bodies[name].append(LABEL.sub(lambda l: names.setdefault(l.group(0), ".L%d" % len(names)), t))
    return {k: (bodies[k], desc[k]) for k in desc}


def instructions(body):
    return sum(1 for t in body if not t.endswith(":") and not t.startswith("."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--allow", default=None)
    arg = ap.parse_args()
    a, b = parse(arg.a), parse(arg.b)
    bad = 0
    for k in sorted(set(a) ^ set(b)):
        print("%-12s %s" % ("only in A" if k in a else "only in B", k))
        bad += 1
    same = 0
    for k in sorted(set(a) & set(b)):
        (ta, da), (tb, db) = a[k], b[k]
        if ta == tb and da == db:
            same += 1
            print("identical    %s" % k)
            continue
        na, nb = instructions(ta), instructions(tb)
        fields = sorted(f for f in set(da) | set(db) if da.get(f) != db.get(f))
        note = "text %s (%d -> %d instructions); descriptor %s" % (
            "same" if ta == tb else "differs", na, nb, ", ".join("%s %s -> %s" % (f, da.get(f), db.get(f)) for f in fields) or "same")
        ok = (arg.allow and re.search(arg.allow, k) and all(da.get(f) == db.get(f) for f in HELD_EQUAL) and
              all(f in SGPR_FIELDS for f in fields) and
              int(db[".amdhsa_next_free_sgpr"]) <= int(da[".amdhsa_next_free_sgpr"]) and abs(nb - na) * 100 <= na)
        print("%-12s %s: %s" % ("allowed" if ok else "DIFFERS", k, note))
        bad += 0 if ok else 1
    print("%d kernels in A, %d in B, %d identical, %d not accepted" % (len(a), len(b), same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
