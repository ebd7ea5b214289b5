#!/usr/bin/env python3
"""Compares two device assemblies of the library kernel by kernel (hipcc -O3 -std=c++17 --offload-arch=gfx950
--cuda-device-only -S of sedef_amd/csrc/sdf_unity.hip, once per source tree): the set of function symbols, per function
the instruction text after dropping comments and renumbering local labels in order of appearance, and per kernel the
descriptor fields that decide occupancy (VGPRs, SGPRs, accum offset, LDS and scratch bytes).
usage: isa_same.py parent.s branch.s [parent_symbol=branch_symbol ...]      (exit status 1 when anything differs)
A kernel that became one instantiation of a template has a new mangled name: `old=new` compares the branch's `new` under the
parent's name `old` (stats_columns_kernel -> stats_columns_kernel<false>, for instance)."""
import re
import sys

FIELDS = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_accum_offset", ".amdhsa_group_segment_fixed_size",
          ".amdhsa_private_segment_fixed_size")
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def parse(path):
    funcs, desc = {}, {}
    name, body, kern = None, None, None
    for raw in open(path):
        line = raw.rstrip("\n")
        t = line.strip()
        m = re.match(r"\.type\s+(\S+),@function", t)
        if m:
            name, body = m.group(1), None
            continue
        if name and body is None and t.split(";")[0].strip() == name + ":":
            body = []
            continue
        if name and body is not None and kern is None and not t.startswith(".amdhsa_kernel"):
            if t.startswith(".Lfunc_end"):
                funcs[name] = body
                name, body = None, None
                continue
            t = t.split(";")[0].split("//")[0].strip()
            # (.section / .text: where the function's bytes go -- a template instantiation gets a COMDAT section of its own name)
            if t and not t.startswith((".p2align", ".loc", ".file", ".cfi", ".section", ".text")):
                body.append(t)
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", t)
        if m:
            kern = m.group(1)
            desc[kern] = {}
            continue
        if kern:
            if t.startswith(".end_amdhsa_kernel"):
                kern = None
            else:
                p = t.split()
                if p and p[0] in FIELDS:
                    desc[kern][p[0]] = p[1]
    return funcs, desc


def normal(body):
    seen = {}
    return [LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), t) for t in body]


def main():
    (fa, da), (fb, db) = parse(sys.argv[1]), parse(sys.argv[2])
    for old, new in (a.split("=", 1) for a in sys.argv[3:]):
        if new not in fb or old in fb:
            print("alias %s=%s: the branch has no %s, or has both" % (old, new, new))
            return 1
        fb[old] = [t.replace(new, old) for t in fb.pop(new)]
        if new in db:
            db[old] = db.pop(new)
    bad = 0
    for s in sorted(set(fa) ^ set(fb)):
        print("only in %s: %s" % ("parent" if s in fa else "branch", s))
        bad += 1
    same = 0
    for s in sorted(set(fa) & set(fb)):
        a, b = normal(fa[s]), normal(fb[s])
        if a != b:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("DIFFERENT %s: %d / %d instructions and labels, first difference at %d" % (s, len(a), len(b), first))
            bad += 1
        elif s in da and da[s] != db.get(s):
            print("DIFFERENT descriptor %s: %s / %s" % (s, da[s], db.get(s)))
            bad += 1
        else:
            same += 1
    kernels = len(set(da) & set(db))
    print("%d functions (%d kernels with descriptors) in both, %d identical, %d different or missing" %
          (len(set(fa) & set(fb)), kernels, same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
