#!/usr/bin/env python3
"""Multichannel HE-AAC end to end and its two hand-off kernels alone.

  python tools/bench_mc_sbr.py [--copies 8192] [--rounds 7] [--out profiles/mc_sbr_bench.json]

End to end: `xaacdec_amd -mcsbr:1 -copies:N` on tests/golden/streams_wide/mc6_aot5.aac (5.1 HE-AAC, six channel rows a frame) and,
for scale, the stereo HE-AAC decode of tests/golden/streams/mix_aot5_48k.aac with the same binary (that path is the parent
commit's code), `--rounds` processes each, taking turns (A B A B ...); every process reports the rate behind its first step.
Kernels: xaac_mc_core_from_out32_batch and xaac_mc_pcm16_from_float_batch on N streams x 6 channels with events around each call,
the median of `--iters` calls behind a warm-up, in a process of their own (`--child`)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")


def child(args):
    import numpy as np
    import torch
    import libxaac_amd
    n, n_ch = args.copies, 6
    rng = np.random.default_rng(5)
    ctx = libxaac_amd.XaacContext(0, torch.cuda.current_stream().cuda_stream)
    out32 = torch.from_numpy(rng.integers(-(1 << 28), 1 << 28, (64 * n_ch, 1024)).astype(np.int32)).cuda().repeat(n // 64, 1)
    qadj = torch.full((n * n_ch,), 2, dtype=torch.int8, device="cuda")
    core = torch.zeros(n * n_ch, 1024, dtype=torch.float32, device="cuda")
    planes = (torch.randn(64 * n_ch, 2048, device="cuda") * 9000.0).repeat(n // 64, 1)
    pcm = torch.zeros(n * 2048 * n_ch, dtype=torch.int16, device="cuda")
    calls = {"xaac_mc_core_from_out32_batch": lambda: ctx.mc_core_from_out32(out32, qadj, core, n_ch),
             "xaac_mc_pcm16_from_float_batch": lambda: ctx.mc_pcm16_from_planes(planes, pcm, (2, 0, 1, 4, 5, 3))}
    res = {}
    for name, fn in calls.items():
        times = []
        for it in range(args.warmup + args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= args.warmup:
                times.append(a.elapsed_time(b) * 1e3)
        res[name] = {"median_us": statistics.median(times), "min_us": min(times), "max_us": max(times)}
    ctx.close()
    print(json.dumps(res))


def decode(path, copies, flags):
    p = subprocess.run([CLI, "-ifile:" + path, "-ofile:/dev/null", "-copies:%d" % copies, *flags], capture_output=True, text=True, timeout=900)
    if p.returncode:
        raise SystemExit("xaacdec_amd failed (%d): %s" % (p.returncode, p.stderr[-400:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_sbr_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    mc6 = os.path.join(ROOT, "tests", "golden", "streams_wide", "mc6_aot5.aac")
    stereo = os.path.join(ROOT, "tests", "golden", "streams", "mix_aot5_48k.aac")
    runs = {"mc6_aot5": [], "mix_aot5_48k": []}
    for _ in range(args.rounds):
        runs["mc6_aot5"].append(decode(mc6, args.copies, ["-mcsbr:1"]))
        runs["mix_aot5_48k"].append(decode(stereo, args.copies, []))
    out = {"copies": args.copies, "rounds": args.rounds, "end_to_end": {}}
    for name, rs in runs.items():
        steady = [r["frames_per_s_after_first_step"] for r in rs]
        ch = rs[0]["channels"]
        out["end_to_end"][name] = {"channels": ch, "frames": rs[0]["frames"], "frames_per_s": [r["frames_per_s"] for r in rs],
                                   "frames_per_s_after_first_step": steady, "median_after_first_step": statistics.median(steady),
                                   "channel_frames_per_s_median": ch * statistics.median(steady)}
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--copies", str(args.copies), "--iters", str(args.iters),
                        "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=900)
    if p.returncode:
        raise SystemExit("kernel timing failed: " + p.stderr[-400:])
    out["kernels"] = json.loads(p.stdout.strip().splitlines()[-1])
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
