#!/usr/bin/env python3
"""The output maps on the GPU: what the downmix to stereo costs or saves, as a call and end to end.

  python tools/bench_out_map.py [--copies 8192] [--rounds 7] [--out profiles/out_map_bench.json]

(i)  The limiter call: 8192 streams x 6 channels x 1024 samples, planar WORD32 in -- xaac_peak_limiter_process_batch (PCM16 of six
     channels out) against xaac_peak_limiter_process_map_batch with the 5.1 downmix (PCM16 of two channels out), the same library, the
     same inputs and chains of four frames (tools/bench_mc_limiter.py's shape).  Every measurement is a process of its own
     (`--child`), the two take turns (A B A B ...), a process reports the median of `--iters` calls behind a warm-up.
(ii) End to end: `xaacdec_amd -copies:N` on tests/golden/streams_wide/mc6_aot2.aac and, with -mcsbr:1, on mc6_aot5.aac, without and
     with -downmix:1, `--rounds` processes each, taking turns; every process reports the rate behind its first step."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
WIDE = os.path.join(ROOT, "tests", "golden", "streams_wide")


def child(args):
    import numpy as np
    import torch
    import libxaac_amd
    import limiter_cases as lc
    n, nch, L = args.copies, 6, 1024
    rng = np.random.default_rng(11)
    base = np.stack([lc.signal(rng, "bursts" if i & 1 else "quiet", L, nch).reshape(L, nch).T.reshape(-1) for i in range(64)])
    x0 = torch.from_numpy(np.tile(base, (n // 64, 1)).reshape(-1)).cuda()
    q = torch.from_numpy(np.full(n * nch, 2, np.int8)).cuda()
    st0, _ = libxaac_amd.peak_limiter_init(nch, 48000)
    state0 = torch.from_numpy(np.tile(np.frombuffer(bytes(st0), np.uint8), (n, 1)).copy()).cuda()
    ctx = libxaac_amd.XaacContext(0, torch.cuda.current_stream().cuda_stream)
    ws = torch.zeros(ctx.peak_limiter_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    mapped = args.child == "mapped"
    m = libxaac_amd.out_map("downmix", nch)
    pcm = torch.zeros(n * L * (2 if mapped else nch), dtype=torch.int16, device="cuda")
    x, state = x0.clone(), state0.clone()
    times = []
    for it in range(args.warmup + args.iters):
        x.copy_(x0)
        if it % 4 == 0:
            state.copy_(state0)       # chains of four frames: a new stream's state, then three frames on
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if mapped:
            ctx.peak_limiter_process_map_batch(x, q, state, nch, ws, pcm, m, planar=True)
        else:
            ctx.peak_limiter_process_batch(x, q, state, nch, ws, pcm16=pcm, planar=True)
        b.record()
        b.synchronize()
        if it >= args.warmup:
            times.append(a.elapsed_time(b) * 1e3)
    ctx.close()
    print(json.dumps({"median_us": statistics.median(times), "min_us": min(times), "max_us": max(times),
                      "samples_checksum": int(x.to(torch.int64).sum().item())}))


def decode(path, copies, flags):
    p = subprocess.run([CLI, "-ifile:" + path, "-ofile:/dev/null", "-copies:%d" % copies, *flags], capture_output=True, text=True, timeout=900)
    if p.returncode:
        raise SystemExit("xaacdec_amd failed (%d): %s" % (p.returncode, p.stderr[-400:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def spread(v):
    return {"per_process": v, "median": statistics.median(v), "fastest": max(v), "slowest": min(v)}     # (rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out")
    ap.add_argument("--skip-decodes", action="store_true")
    ap.add_argument("--child", choices=["plain", "mapped"])
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = {"plain": [], "mapped": []}
    for r in range(args.rounds):
        for side in ("plain", "mapped"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--iters", str(args.iters), "--warmup",
                                str(args.warmup), "--copies", str(args.copies)], capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                return 1
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(side, r, runs[side][-1], flush=True)
    assert len({x["samples_checksum"] for v in runs.values() for x in v}) == 1, "the two calls do not leave the same samples"
    res = {"limiter_call": {"shape": {"streams": args.copies, "channels": 6, "samples": 1024, "planar": 1},
                            "unit": "microseconds per call (three kernels), median of %d calls per process" % args.iters,
                            "rounds": args.rounds, "order": "plain mapped plain mapped ..."}}
    for side, what in (("plain", "xaac_peak_limiter_process_batch, six channels of PCM16 out"),
                       ("mapped", "xaac_peak_limiter_process_map_batch, 5.1 downmix: two channels of PCM16 out")):
        m = [x["median_us"] for x in runs[side]]
        res["limiter_call"][side] = {"call": what, "per_process_median_us": m, "median_us": statistics.median(m), "min_us": min(m),
                                     "max_us": max(m)}
    lc_ = res["limiter_call"]
    lc_["mapped_over_plain"] = lc_["mapped"]["median_us"] / lc_["plain"]["median_us"]
    lc_["mapped_no_slower_than_plain_band"] = lc_["mapped"]["median_us"] <= lc_["plain"]["max_us"]
    if not args.skip_decodes:
        cases = [("mc6_aot2", ()), ("mc6_aot2", ("-downmix:1",)), ("mc6_aot5", ("-mcsbr:1",)), ("mc6_aot5", ("-mcsbr:1", "-downmix:1"))]
        rates = {i: [] for i in range(len(cases))}
        for r in range(args.rounds):
            for i, (name, flags) in enumerate(cases):
                d = decode(os.path.join(WIDE, name + ".aac"), args.copies, flags)
                rates[i].append(d["frames_per_s_after_first_step"])
                print(name, flags, r, d["frames_per_s_after_first_step"], flush=True)
        res["decodes"] = {"unit": "frames/s behind the first step, xaacdec_amd -copies:%d (a frame is six coded channels)" % args.copies,
                          "rounds": args.rounds, "order": "the four cases take turns",
                          "cases": [dict(stream=name + ".aac", flags=list(flags), **spread(rates[i])) for i, (name, flags) in enumerate(cases)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
