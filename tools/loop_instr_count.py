#!/usr/bin/env python3
"""Instruction counts of the loops of one kernel in a device-only assembly file (hipcc ... --cuda-device-only -S): a
counting aid and nothing more.

  python tools/loop_instr_count.py ps.s xaac_ps_kernel [--min 100] [--hist N]

The kernel is the first function whose (mangled) name contains the given string.  A loop is a label and a later branch
back to it; per loop the script prints the number of VALU (v_*), SALU (s_*), LDS (ds_*) and global (global_* / flat_* /
buffer_* / scratch_*) instructions between the two -- inner loops included, each instruction counted once, whatever the
control flow in between -- and the N most frequent opcodes.  Loops with fewer than --min instructions are left out.
"""
import argparse
import collections
import re

CLASSES = (("VALU", ("v_",)), ("SALU", ("s_",)), ("LDS", ("ds_",)), ("global", ("global_", "flat_", "buffer_", "scratch_")))


def kernel_body(lines, name):
    start = None
    for i, ln in enumerate(lines):
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", ln)
        if start is None:
            if m and name in m.group(1) and not m.group(1).startswith(".L"):
                start = i
        elif ln.strip().startswith((".Lfunc_end", ".end_amdhsa_kernel")):   # (not the first s_endpgm: early exits)
            return lines[start:i + 1]
    if start is None:
        raise SystemExit("no function with %r in its name" % name)
    return lines[start:]


def classify(op):
    for cls, prefixes in CLASSES:
        if op.startswith(prefixes):
            return cls
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--min", type=int, default=100, help="smallest loop to print (instructions)")
    ap.add_argument("--hist", type=int, default=24, help="opcodes in the histogram")
    a = ap.parse_args()
    body = kernel_body(open(a.asm).read().split("\n"), a.kernel)
    instrs, labels = [], {}  # (opcode, branch target or None); label -> index of the next instruction
    for ln in body:
        s = ln.split(";")[0].strip()
        m = re.match(r"^(\.L[\w.$]+):", s)
        if m:
            labels[m.group(1)] = len(instrs)
            continue
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        parts = s.split()
        tgt = parts[1] if parts[0].startswith(("s_cbranch", "s_branch")) and len(parts) > 1 else None
        instrs.append((parts[0], tgt))
    total = collections.Counter(classify(op) for op, _ in instrs)
    print("%s: %d instructions  " % (a.kernel, len(instrs)) + "  ".join("%s %d" % (c, total[c]) for c, _ in CLASSES))
    loops = sorted({(labels[t], i) for i, (_, t) in enumerate(instrs) if t in labels and labels[t] <= i})
    for b, e in loops:
        if e - b + 1 < a.min:
            continue
        ops = [op for op, _ in instrs[b:e + 1]]
        cnt = collections.Counter(classify(op) for op in ops)
        print("\nloop at instruction %d..%d (%d)  " % (b, e, len(ops)) + "  ".join("%s %d" % (c, cnt[c]) for c, _ in CLASSES))
        for op, n in collections.Counter(ops).most_common(a.hist):
            print("  %5d  %s" % (n, op))


if __name__ == "__main__":
    main()
