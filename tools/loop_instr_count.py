#!/usr/bin/env python3
"""Instruction counts of the loops of one kernel in a device-only assembly file (hipcc ... --cuda-device-only -S): a
counting aid and nothing more.

  python tools/loop_instr_count.py ps.s xaac_ps_kernel [--min 100] [--hist N]

The kernel is the first function whose (mangled) name contains the given string.  A loop is a label and a later branch
back to it; per loop the script prints the number of VALU (v_*), SALU (s_*), LDS (ds_*) and global (global_* / flat_* /
buffer_* / scratch_*) instructions between the two -- inner loops included, each instruction counted once, whatever the
control flow in between -- and the N most frequent opcodes.  Loops with fewer than --min instructions are left out.

  python tools/loop_instr_count.py ps_marks.s xaac_ps_kernelILi32 --phases [--min 20]

With --phases the kernel is cut at the "; XP_PHASE n" comment lines a -DXP_PHASE_MARKS build of sbr_ps_kernel.hip leaves at its
phase borders: per region the same four counts and the loops that lie inside it (profiles/ps_prep_instr.txt).
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
    ap.add_argument("--phases", action="store_true", help="counts per region between the '; XP_PHASE n' markers of a "
                    "-DXP_PHASE_MARKS build (sbr_ps_kernel.hip), with the loops that lie inside each region")
    a = ap.parse_args()
    body = kernel_body(open(a.asm).read().split("\n"), a.kernel)
    instrs, labels = [], {}  # (opcode, branch target or None); label -> index of the next instruction
    marks = []               # (index of the next instruction, phase number) of every "; XP_PHASE n" marker
    for ln in body:
        m = re.search(r"XP_PHASE (\d+)", ln)
        if m:
            marks.append((len(instrs), int(m.group(1))))
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
    if a.phases:
        # regions in the order of the code: from one marker to the next (the compiler may lay a phase's cold blocks out
        # behind the kernel's last marker: they count where they stand)
        edges = [(0, "start")] + [(i, "after mark %d" % n) for i, n in marks] + [(len(instrs), None)]
        for (b, name), (e, _) in zip(edges, edges[1:]):
            cnt = collections.Counter(classify(op) for op, _ in instrs[b:e])
            print("\nregion %-14s %5d..%-5d (%4d)  " % (name, b, e - 1, e - b) + "  ".join("%s %d" % (c, cnt[c]) for c, _ in CLASSES))
            for lb, le in loops:
                if b <= lb and le < e and le - lb + 1 >= a.min:
                    lc = collections.Counter(classify(op) for op, _ in instrs[lb:le + 1])
                    print("    loop %5d..%-5d (%4d)  " % (lb, le, le - lb + 1) + "  ".join("%s %d" % (c, lc[c]) for c, _ in CLASSES))
        return
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
