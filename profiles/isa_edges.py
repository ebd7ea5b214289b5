#!/usr/bin/env python3
"""Vector instructions of extz2_pair_kernel<3,false,false> OUTSIDE its innermost loops (the row loops), by what they do, from
the device assembly (hipcc -O3 --offload-arch=gfx950 -S --cuda-device-only of sedef_amd/csrc/sdf_unity.hip): the static side
of "what a row costs beyond its steady row".  Static counts of the whole function, every row flavour's entry and exit
included -- not the executed path of one period.
usage: isa_edges.py unity.s [more.s ...]"""
import re
import sys

KERNEL = "_ZN3sdf17extz2_pair_kernelILi3ELb0ELb0EE"
GROUPS = (
    ("v_mov_b32 register <- register (copies)", lambda op, a: op.startswith("v_mov_b32") and re.match(r"^v\d+, v\d+$", a)),
    ("v_mov_b32 register <- constant / scalar (clears, set-up)", lambda op, a: op.startswith("v_mov_b32")),
    ("v_accvgpr / scratch moves", lambda op, a: op.startswith("v_accvgpr")),
    ("v_perm_b32 (flag packing, score tables)", lambda op, a: op.startswith("v_perm_b32")),
    ("v_cndmask_b32 (re-base selects, zeroing selects, tables)", lambda op, a: op.startswith("v_cndmask")),
    ("v_cmp* (lane predicates)", lambda op, a: op.startswith("v_cmp")),
    ("64-bit address arithmetic (v_mad_u64, v_lshlrev_b64, v_add_co / v_addc_co, v_ashrrev_i32)", lambda op, a: op.startswith(
        ("v_mad_u64", "v_mad_i64", "v_lshlrev_b64", "v_lshl_add_u64", "v_add_co", "v_addc_co", "v_ashrrev_i32", "v_mad_u32_u24"))),
    ("v_readlane / v_readfirstlane / v_writelane", lambda op, a: op.startswith(("v_readlane", "v_readfirstlane", "v_writelane"))),
    ("v_pk_* (packed 16-bit)", lambda op, a: op.startswith("v_pk_")),
    ("DPP moves / shifts", lambda op, a: "dpp" in op or "row_" in a or "quad_perm" in a or "wave_" in a),
    ("shifts, and / or / xor, bfe (table rebuild, masks)", lambda op, a: op.startswith(
        ("v_lshl", "v_lshr", "v_and", "v_or", "v_xor", "v_bfe", "v_not", "v_and_or", "v_lshl_or", "v_bfi"))),
    ("32-bit add / sub / min / max / mul", lambda op, a: op.startswith(("v_add", "v_sub", "v_min", "v_max", "v_mul", "v_mad", "v_mbcnt"))),
)


def kernel_ins(path):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL) and l.rstrip().endswith("sdf_result"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    labels, ins = {}, []
    for l in lines[start:end]:
        t = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        t = t.split(";")[0].strip()
        if not t or t.startswith((".", "//")) or t.endswith(":"):
            continue
        parts = t.split(None, 1)
        ins.append((parts[0], parts[1] if len(parts) > 1 else ""))
    return labels, ins


def main():
    for path in sys.argv[1:]:
        labels, ins = kernel_ins(path)
        loops = [(labels[a.strip()], k) for k, (op, a) in enumerate(ins)
                 if (op.startswith("s_cbranch") or op == "s_branch") and a.strip() in labels and labels[a.strip()] <= k]
        inner = [(a, b) for (a, b) in loops if not any(a <= c and d <= b and (c, d) != (a, b) for (c, d) in loops)]
        in_loop = [False] * len(ins)
        for a, b in inner:
            for k in range(a, b + 1):
                in_loop[k] = True
        cnt, other = {g: 0 for g, _ in GROUPS}, {}
        valu_in = valu_out = lds_out = vmem_out = salu_out = 0
        for k, (op, a) in enumerate(ins):
            if in_loop[k]:
                valu_in += op.startswith("v_")
                continue
            lds_out += op.startswith("ds_")
            vmem_out += op.startswith(("global_", "scratch_", "buffer_", "flat_"))
            salu_out += op.startswith("s_")
            if not op.startswith("v_"):
                continue
            valu_out += 1
            for g, f in GROUPS:
                if f(op, a):
                    cnt[g] += 1
                    break
            else:
                other[op] = other.get(op, 0) + 1
        print("%s: %d instructions, %d innermost loops holding %d VALU; outside them %d VALU, %d LDS, %d memory, %d scalar" %
              (path, len(ins), len(inner), valu_in, valu_out, lds_out, vmem_out, salu_out))
        for g, _ in GROUPS:
            print("  %6d  %s" % (cnt[g], g))
        print("  %6d  other: %s" % (sum(other.values()), " ".join("%s %d" % kv for kv in sorted(other.items(), key=lambda kv: -kv[1])[:12])))


if __name__ == "__main__":
    main()
