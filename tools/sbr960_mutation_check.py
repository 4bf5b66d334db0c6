#!/usr/bin/env python3
"""Mutation check of the 30-slot fuzz cases (profiles/sbr960_fuzz_coverage.txt): builds the HOST ORACLE ALONE -- never the
product library -- four times, each with one comparison constant of the 30-slot decoder changed (a value, never an index or a
loop bound), so that the tests pinned to the oracle can be run against each mutant and be seen to notice:

  a  the hybrid delay shift of the PS slot loop starts at NS - 4 instead of NS - 6          (oracle_sbr.cpp, -DXO_MUT_HYB_DELAY)
  b  the envelope adjuster changes its exponents at QMF slot NS + 2 instead of NS          (a patched copy of sbr_core.h)
  c  the time slot at which an envelope counts for the next frame's exponent (env_calc.c:811-837) is NS / 2 + 1 instead of NS / 2
                                                                                         (a patched copy of sbr_core.h)
  d  PS borders are held to 0..NS + 2 instead of 0..NS                                     (oracle_sbr.cpp, -DXO_MUT_PS_CLAMP)

The sources are copied to a temporary directory and patched / compiled there; the mutants land in oracle/_mut/liboracle_<x>.so
(git-ignored) next to a copy of the real oracle, each exporting xo_mutation_id().

  sbr960_mutation_check.py build            build the four mutants
  sbr960_mutation_check.py run TEST...      for the real oracle and each mutant: put it in the place of oracle/liboracle.so, run
                                            pytest on the given files (extra arguments after -- go to pytest), print which tests
                                            failed and the first assertion message; the real oracle is put back at the end"""
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUT = os.path.join(ROOT, "oracle", "_mut")
SO = os.path.join(ROOT, "oracle", "liboracle.so")


def _patch_b(text):
    """the slot at which the adjuster's exponents change: every comparison of a slot number with Q::NS inside the adjuster"""
    n = 0
    out = []
    for line in text.split("\n"):
        if "seg_end" not in line:
            line, k = re.subn(r"\b(l|sl_i) (==|<|>=) Q::NS\b", r"\1 \2 (Q::NS + 2)", line)
            n += k
        out.append(line)
    assert n >= 8, n
    return "\n".join(out)


def _patch_c(text):
    old = ": Q::NS / 2;"
    assert text.count(old) == 1 and "frame_end_slot" in text.split(old)[0].split("\n")[-1]
    return text.replace(old, ": Q::NS / 2 + 1;")


MUTANTS = {"a": (["-DXO_MUT_HYB_DELAY"], None), "b": ([], _patch_b), "c": ([], _patch_c), "d": (["-DXO_MUT_PS_CLAMP"], None)}


def build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    os.makedirs(MUT, exist_ok=True)
    shutil.copy2(SO, os.path.join(MUT, "liboracle_real.so"))
    for name, (flags, patch) in MUTANTS.items():
        with tempfile.TemporaryDirectory() as d:
            for sub in ("oracle", "include", os.path.join("libxaac_amd", "csrc")):
                os.makedirs(os.path.join(d, sub))
                for f in glob.glob(os.path.join(ROOT, sub, "*")):
                    if os.path.isfile(f) and f.endswith((".c", ".cpp", ".h", ".inc")):
                        shutil.copy2(f, os.path.join(d, sub))
            if patch:
                core = os.path.join(d, "libxaac_amd", "csrc", "sbr_core.h")
                text = open(core).read()
                open(core, "w").write(patch(text))
            o = os.path.join(d, "oracle")
            subprocess.check_call(["gcc", "-O3", "-std=c99", "-fPIC", "-c"] + sorted(glob.glob(os.path.join(o, "oracle_*.c"))) +
                                  ["-o", os.path.join(o, "oracle_c.o")])
            dst = os.path.join(MUT, "liboracle_%s.so" % name)
            subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                                   '-DXO_MUTATION_ID="%s"' % name] + flags + ["-o", dst] +
                                  sorted(glob.glob(os.path.join(o, "oracle_*.cpp"))) + [os.path.join(o, "oracle_c.o")])
            lib = ctypes.CDLL(dst)
            lib.xo_mutation_id.restype = ctypes.c_char_p
            assert lib.xo_mutation_id().decode() == name
            print("built", dst)


def run(args):
    tests, extra = (args[:args.index("--")], args[args.index("--") + 1:]) if "--" in args else (args, [])
    real = os.path.join(MUT, "liboracle_real.so")
    assert os.path.exists(real), "build first"
    try:
        for name in ["real"] + sorted(MUTANTS):
            shutil.copyfile(os.path.join(MUT, "liboracle_%s.so" % name), SO)      # (fresh mtime: make leaves it alone)
            p = subprocess.run([sys.executable, "-m", "pytest", "-q", "--tb=line", "-p", "no:cacheprovider"] + extra + tests,
                               cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            lines = p.stdout.strip().split("\n")
            failed = [ln for ln in lines if ln.startswith("FAILED") or ln.startswith("ERROR")]
            first = [ln for ln in lines if "AssertionError" in ln or "Error:" in ln][:1]
            print("== oracle %s: exit %d, %s" % (name, p.returncode, lines[-1]))
            for ln in failed + first:
                print("   " + ln[:600])
            sys.stdout.flush()
    finally:
        shutil.copyfile(real, SO)


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "build":
        build()
    elif len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2:])
    else:
        sys.exit(__doc__)
