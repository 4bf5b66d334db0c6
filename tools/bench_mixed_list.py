#!/usr/bin/env python3
"""What decoding a list of several kinds of stream in one process gains over one process per kind.

The ten committed mono / stereo streams of tests/golden/streams (six kinds), each copied M times (--copies, default 256) into a
temporary directory, as one list, decoded three ways on one device, wall clock of the whole process (start to exit: context, code
objects, warm-up, reading the inputs and writing the WAV files included -- what a user waits for), median of five, the ways taking
turns within a repetition:

  (a) side_by_side       xaacdec_amd -ilist on the mixed list: the groups side by side
  (b) serial_groups      the same with -serialgroups:1: one process, the groups one after the other
  (c) process_per_kind   one xaacdec_amd -ilist process per kind, one after the other: the only way before mixed lists

Beside each run's wall clock the seconds the processes count themselves from their first shard thread's start to their last
one's end are kept (wall_s of their closing lines, summed over a way's processes: device set-up, context, warm-up, allocations and
the decode); what is left of a run is loading the program, reading the inputs and writing the files.
The three ways' files are compared for equality (SHA-256 of every file, taken in the first repetition); nothing else is checked
here.  -> one JSON document (--out, default profiles/mixed_list_bench.json) with the frames per second of each way, the spread
of its five runs and the three ratios."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
NAMES = ["mix_aot2_64k", "mix_aot5_48k", "mono_aot5_32k", "harm_aot5_48k", "mix_aot29_32k", "synth_lc_a", "synth_lc_b",
         "synth_lc_mono", "lc_aot2_16k_mono", "he_aot5_44k"]


def run(lists, odir, extra):
    """decodes the lists, one process each, one after the other -> (seconds from the first start to the last exit, frames, the
    seconds the processes themselves count from their first shard's start to their last one's end: wall_s of their closing lines)"""
    frames, inside = 0, 0.0
    t0 = time.perf_counter()
    for lst in lists:
        p = subprocess.run([CLI, "-ilist:" + lst, "-odir:" + odir] + extra, capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit("xaacdec_amd %s failed (%d): %s" % (lst, p.returncode, p.stderr[-500:]))
        info = json.loads(p.stdout.strip().splitlines()[-1])
        frames, inside = frames + info["frames"], inside + info["wall_s"]
    return time.perf_counter() - t0, frames, inside


def digests(odir):
    out = {}
    for f in sorted(os.listdir(odir)):
        with open(os.path.join(odir, f), "rb") as fh:
            out[f] = hashlib.sha256(fh.read()).hexdigest()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--copies", type=int, default=256, help="copies of each of the ten streams in the list")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_list_bench.json"))
    ap.add_argument("--flags", default="", help="further flags for every xaacdec_amd call, space separated (e.g. -esbr:0)")
    args = ap.parse_args()
    extra = args.flags.split()
    tmp = tempfile.mkdtemp(prefix="xaac_mixed_bench_")
    try:
        paths = []
        for k in range(args.copies):      # copy k of every stream, then copy k + 1: the kinds are spread over the whole list
            for n in NAMES:
                dst = os.path.join(tmp, "%s_%04d.aac" % (n, k))
                shutil.copyfile(os.path.join(STREAMS, n + ".aac"), dst)
                paths.append(dst)
        mixed = os.path.join(tmp, "mixed.txt")
        with open(mixed, "w") as f:
            f.write("".join(p + "\n" for p in paths))
        # the kinds, as the decoder itself sorts the list (-plan: no device is touched)
        p = subprocess.run([CLI, "-plan", "-ilist:" + mixed, "-odir:" + tmp] + extra, capture_output=True, text=True)
        if p.returncode != 0:
            sys.exit("xaacdec_amd -plan failed: " + p.stderr[-500:])
        plan = json.loads(p.stdout)
        per_kind = []
        for g, group in enumerate(plan["groups"]):
            lst = os.path.join(tmp, "kind_%d.txt" % g)
            with open(lst, "w") as f:
                f.write("".join(paths[i] + "\n" for i in group["list_index"]))
            per_kind.append(lst)
        ways = [("side_by_side", [mixed], []), ("serial_groups", [mixed], ["-serialgroups:1"]), ("process_per_kind", per_kind, [])]
        seconds, inside = {name: [] for name, _, _ in ways}, {name: [] for name, _, _ in ways}
        frames, files = {}, {}
        for rep in range(args.reps):
            for name, lists, flags in ways:
                odir = os.path.join(tmp, "out")
                os.mkdir(odir)
                s, frames[name], d = run(lists, odir, flags + extra)
                seconds[name].append(s), inside[name].append(d)
                if rep == 0:
                    files[name] = digests(odir)
                shutil.rmtree(odir)
        same = files["side_by_side"] == files["serial_groups"] == files["process_per_kind"] and len(files["side_by_side"]) == len(paths)
        result = {"copies": args.copies, "streams": len(paths), "reps": args.reps, "flags": extra, "files_equal": same,
                  "groups": [{k: g[k] for k in ("rate", "channels", "sbr", "streams", "threads")} for g in plan["groups"]]}
        for name, _, _ in ways:
            med = statistics.median(seconds[name])
            result[name] = {"frames": frames[name], "seconds": [round(s, 4) for s in seconds[name]], "median_s": round(med, 4),
                            "frames_per_s": round(frames[name] / med, 1),
                            "frames_per_s_slowest_run": round(frames[name] / max(seconds[name]), 1),
                            "frames_per_s_fastest_run": round(frames[name] / min(seconds[name]), 1),
                            # from the start of the first shard's thread to the end of the last one's (device set-up, context, warm-up
                            # and allocations are inside; reading the inputs and writing the files are not): not one of the three
                            # figures, but where running side by side has to show
                            "decode_seconds": [round(d, 4) for d in inside[name]],
                            "decode_median_s": round(statistics.median(inside[name]), 4)}
        fps = lambda name: result[name]["frames_per_s"]
        result["ratio_side_by_side_over_process_per_kind"] = round(fps("side_by_side") / fps("process_per_kind"), 3)
        result["ratio_side_by_side_over_serial_groups"] = round(fps("side_by_side") / fps("serial_groups"), 3)
        result["ratio_serial_groups_over_process_per_kind"] = round(fps("serial_groups") / fps("process_per_kind"), 3)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        print(json.dumps(result))
        if not same:
            sys.exit("the three ways did not write the same files")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
