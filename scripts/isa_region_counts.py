"""Static instruction counts of one kernel's ISA (hipcc -S output), per basic block and class.

usage: isa_region_counts.py FILE.s KERNEL_SUBSTRING [--blocks]

Classes: VALU (v_*), SALU (s_* without waits / branches / nops), LDS (ds_*), VMEM (buffer_* /
global_* / flat_* / scratch_*), SMEM (s_load_* / s_buffer_load_*), and the rest (waits, branches).
With --blocks every basic block is listed with the landmarks that tell the kernel's regions
apart (8-byte buffer loads and v_perm: the counting; ds_max / ds_min: the slot placement; ds_or:
the MD events; s_memtime: a phase clock read); without it only the kernel's totals.
"""
import re
import sys


def classify(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_load_", "s_buffer_load_")):
        return "SMEM"
    if op.startswith(("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_setpc", "s_sleep")):
        return "other"
    if op.startswith("s_"):
        return "SALU"
    return "other"


MARKS = (("buffer_load_dwordx2", "ld8"), ("v_perm_b32", "perm"), ("ds_max", "dsmax"), ("ds_min", "dsmin"),
         ("ds_or", "dsor"), ("ds_add", "dsadd"), ("s_memtime", "clk"), ("s_memrealtime", "clk"),
         ("ds_write_b128", "zero16"), ("ds_bpermute", "bperm"), ("_dpp", "dpp"), ("global_atomic", "gatom"),
         ("global_store", "gstore"), ("buffer_load_dword ", "ld4"), ("global_load", "gload"), ("v_readlane", "rdlane"))


def kernel_blocks(path, name):
    blocks, cur, inside = [], None, False
    for line in open(path):
        s = line.split(";")[0].strip()  # (a trailing comment is no instruction)
        if not inside:
            if s.endswith(":") and name in s and not s.startswith("."):
                inside = True
                cur = [s[:-1][-40:], {}, {}]
                blocks.append(cur)
            continue
        if s.startswith(".Lfunc_end") or s.startswith(".size"):
            break
        if not s or s.startswith((";", "//")):
            continue
        if s.endswith(":"):
            cur = [s[:-1], {}, {}]
            blocks.append(cur)
            continue
        if s.startswith("."):
            continue
        op = s.split()[0]
        k = classify(op)
        cur[1][k] = cur[1].get(k, 0) + 1
        for pat, tag in MARKS:
            if pat in s + " ":
                cur[2][tag] = cur[2].get(tag, 0) + 1
    return blocks


def main():
    path, name = sys.argv[1], sys.argv[2]
    blocks = kernel_blocks(path, name)
    tot = {}
    for _, c, _ in blocks:
        for k, v in c.items():
            tot[k] = tot.get(k, 0) + v
    if "--blocks" in sys.argv:
        for i, (lab, c, m) in enumerate(blocks):
            if not c:
                continue
            print("%4d %-14s V %4d S %4d L %3d M %3d  %s" % (i, lab[-14:], c.get("VALU", 0), c.get("SALU", 0),
                                                           c.get("LDS", 0), c.get("VMEM", 0),
                                                           " ".join("%s:%d" % kv for kv in sorted(m.items()))))
    print("total", " ".join("%s %d" % kv for kv in sorted(tot.items())), "blocks", len(blocks))


if __name__ == "__main__":
    main()
