#!/usr/bin/env python3
"""A/B of the peak limiter on multichannel blocks: 8192 streams x 6 channels x 1024 samples, planar WORD32 in, PCM16 out
(xaac_peak_limiter_process_batch with planar = 1, what the multichannel decode chain calls), one library against another.

  python tools/bench_mc_limiter.py --a <other libxaac_amd.so> [--b <this tree's>] [--rounds 7] [--out profiles/mc_limiter_ab.json]

Every measurement is a process of its own (XAAC_AMD_LIBRARY picks the library), A and B take turns (A B A B ...), a process
times `--iters` calls with events around each after a warm-up and reports their median; the result holds every process's
figure, the two medians and the two spreads.  `--child` is the measuring process."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(args):
    import numpy as np
    import torch
    import libxaac_amd
    import limiter_cases as lc
    n, nch, L = args.streams, args.channels, 1024
    rng = np.random.default_rng(11)
    # 64 different streams, tiled: bursts (quiet with loud stretches: attack and release both run) and quiet ones, half and half
    base = np.stack([lc.signal(rng, "bursts" if i & 1 else "quiet", L, nch).reshape(L, nch).T.reshape(-1) for i in range(64)])
    x0 = torch.from_numpy(np.tile(base, (n // 64, 1)).reshape(-1)).cuda()
    q = torch.from_numpy(np.full(n * nch, 2, np.int8)).cuda()
    st0, _ = libxaac_amd.peak_limiter_init(nch, 48000)
    state0 = torch.from_numpy(np.tile(np.frombuffer(bytes(st0), np.uint8), (n, 1)).copy()).cuda()
    ctx = libxaac_amd.XaacContext(0, torch.cuda.current_stream().cuda_stream)
    ws = torch.zeros(ctx.peak_limiter_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    pcm = torch.zeros(n * L * nch, dtype=torch.int16, device="cuda")
    x, state = x0.clone(), state0.clone()
    times = []
    for it in range(args.warmup + args.iters):
        x.copy_(x0)
        if it % 4 == 0:
            state.copy_(state0)       # chains of four frames: a new stream's state, then three frames on
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.peak_limiter_process_batch(x, q, state, nch, ws, pcm16=pcm, planar=True)
        b.record()
        b.synchronize()
        if it >= args.warmup:
            times.append(a.elapsed_time(b) * 1e3)
    ctx.close()
    print(json.dumps({"median_us": statistics.median(times), "min_us": min(times), "max_us": max(times),
                      "checksum": int(pcm.to(torch.int64).sum().item())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", help="the library to compare against (the parent commit's build)")
    ap.add_argument("--b", default=os.path.join(ROOT, "libxaac_amd", "libxaac_amd.so"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--channels", type=int, default=6)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = {"a": [], "b": []}
    for r in range(args.rounds):
        for side in ("a", "b"):
            env = dict(os.environ, XAAC_AMD_LIBRARY=os.path.abspath(getattr(args, side)))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--warmup", str(args.warmup),
                                "--streams", str(args.streams), "--channels", str(args.channels)], env=env, capture_output=True, text=True,
                               timeout=300)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                return 1
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(side, r, runs[side][-1], flush=True)
    assert len({x["checksum"] for v in runs.values() for x in v}) == 1, "the two libraries do not compute the same PCM"
    res = {"shape": {"streams": args.streams, "channels": args.channels, "samples": 1024, "planar": 1, "pcm16": 1},
           "unit": "microseconds per xaac_peak_limiter_process_batch call (three kernels), median of %d calls per process" % args.iters,
           "rounds": args.rounds, "order": "a b a b ..."}
    for side in ("a", "b"):
        m = [x["median_us"] for x in runs[side]]
        res[side] = {"library": getattr(args, side), "per_process_median_us": m, "median_us": statistics.median(m), "min_us": min(m),
                     "max_us": max(m)}
    res["b_over_a"] = res["b"]["median_us"] / res["a"]["median_us"]
    res["b_outside_a_band_on_the_fast_side"] = res["b"]["median_us"] < res["a"]["min_us"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
