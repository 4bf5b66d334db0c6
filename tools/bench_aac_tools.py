#!/usr/bin/env python3
"""What the AAC spectral tools cost on either side of the bus.  Prints one JSON object and writes it to --out.

  host    the batch parser's frames/s on --threads threads at stage 2 (tools in the parser) against stage 1 + the tools' side
          rows (tools left to the GPU): the share of the front end the tools were.  CPU only.
  kernel  xaac_aac_tools_process_batch on 8192 channel pairs of random, syntax-legal side info (tests/aac_tools_cases.py) --
          long windows and EIGHT_SHORT, with and without TNS -- beside xaac_imdct_process_batch on the same 16384 channel-frames.
          Device time from events around single launches, median.
  e2e     xaacdec_amd -copies:N on a committed stream with and without -gputools:1, frames/s behind the first step, median
          of --runs runs.

  python tools/bench_aac_tools.py [host] [kernel] [e2e] [--threads 16] [--streams 2048] [--copies 4096] [--runs 5] [--out f.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")


def host_rates(name, n_streams, threads, runs):
    from libxaac_amd import CORE_TOOLS_SIDE_BYTES, PS_FRAME_BYTES, SBR_FRAME_BYTES, SBR_HEADER_BYTES, decoder
    data = open(os.path.join(STREAMS, name + ".aac"), "rb").read()
    out = {}
    for label, stage in (("stage2", 2), ("stage1_plus_side", 1)):
        rates = []
        for _ in range(runs):
            bp = decoder.BatchParser([data] * n_streams, threads=threads, stage=stage)
            n, nc = bp.n, bp.n * bp.n_ch
            spec, ics = np.zeros((nc, 1024), np.int32), np.zeros((nc, 2), np.uint8)
            hdr = frm = psf = flags = None
            if bp.sbr:
                hdr, frm = np.zeros((nc, SBR_HEADER_BYTES), np.uint8), np.zeros((nc, SBR_FRAME_BYTES), np.uint8)
                flags = np.zeros((n, 8), np.int32)
                psf = np.zeros((n, PS_FRAME_BYTES), np.uint8) if bp.n_ch == 1 else None
            side = np.zeros((n, CORE_TOOLS_SIDE_BYTES), np.uint8) if stage == 1 else None
            frames, t0 = 0, time.perf_counter()
            while True:
                got = bp.step(spec, ics, hdr, frm, psf, flags, tools_side=side)
                if not got.any():
                    break
                frames += int(got.sum())
            rates.append(frames / (time.perf_counter() - t0))
            bp.close()
        out[label] = {"frames_per_s_median": statistics.median(rates), "runs": [round(r) for r in rates]}
    out["stage1_over_stage2"] = out["stage1_plus_side"]["frames_per_s_median"] / out["stage2"]["frames_per_s_median"]
    return out


def kernel_times(n_pairs, reps):
    import torch
    import aac_tools_cases as tc
    import libxaac_amd
    from libxaac_amd import decoder
    ctx = libxaac_amd.XaacContext(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1)
    pools = {"long": [], "short": []}
    while min(len(v) for v in pools.values()) < 128:
        side, spec, state = tc.random_element(rng)
        s = decoder.CoreToolsSide.from_buffer(side)
        if s.n_ch != 2:
            continue
        kinds = {("short" if s.ch[c].window_sequence == 2 else "long") for c in range(2)}
        if len(kinds) == 1 and len(pools[kinds.pop()]) < 128:
            pools["short" if s.ch[0].window_sequence == 2 else "long"].append((side, spec, state))

    def timed(fn, restore):
        ts = []
        for k in range(reps + 3):
            restore()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if k >= 3:
                ts.append(a.elapsed_time(b) * 1000.0)
        return statistics.median(ts)

    out = {}
    for kind, pool in pools.items():
        for tns in (True, False):
            sides = np.stack([c[0] for c in pool]).copy()
            if not tns:
                for row in sides:
                    s = decoder.CoreToolsSide.from_buffer(row)
                    s.ch[0].tns_present = s.ch[1].tns_present = 0
            tile = lambda a: np.tile(a, (n_pairs // len(pool),) + (1,) * (a.ndim - 1))
            side_d = torch.from_numpy(tile(sides)).cuda()
            spec0 = torch.from_numpy(tile(np.stack([c[1] for c in pool]))).cuda()
            state0 = torch.from_numpy(tile(np.stack([c[2] for c in pool]))).cuda()
            spec_d, state_d = spec0.clone(), state0.clone()
            status = torch.zeros(n_pairs, dtype=torch.int32, device="cuda")

            def restore():
                spec_d.copy_(spec0), state_d.copy_(state0)
            t_tools = timed(lambda: ctx.aac_tools_process_batch(spec_d, side_d, state_d, status), restore)
            assert not status.cpu().numpy().any()
            seq = np.array([[decoder.CoreToolsSide.from_buffer(r.copy()).ch[c].window_sequence for c in range(2)] for r in tile(sides)], np.uint8)
            ics = torch.from_numpy(np.stack([seq.reshape(-1), np.zeros(2 * n_pairs, np.uint8)], 1).copy()).cuda()
            ovl = torch.zeros((2 * n_pairs, 512), dtype=torch.int32, device="cuda")
            ovl_state = ics.clone()
            pcm = torch.zeros(2 * n_pairs * 1024, dtype=torch.int16, device="cuda")
            t_imdct = timed(lambda: ctx.imdct_process_batch(spec_d.view(-1, 1024), ics, ovl, ovl_state, pcm16=pcm, ch_fac=2), restore)
            out["%s_%s" % (kind, "tns" if tns else "no_tns")] = {"tools_us": round(t_tools, 1), "imdct_us": round(t_imdct, 1)}
    out["note"] = "per %d channel pairs; fuzz-tier elements: ~70 %% of the channels of a TNS batch carry filters (orders up to 12), " \
                  "about one band in six is a noise band -- denser tool use than encoded streams have" % n_pairs
    return out


def e2e(name, copies, runs, flags):
    cli = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
    out = {}
    for label, extra in (("without_flag", []), ("gputools", ["-gputools:1"])):
        rates = []
        for _ in range(runs):
            p = subprocess.run([cli, "-ifile:" + os.path.join(STREAMS, name + ".aac"), "-ofile:/tmp/bench_aac_tools.wav",
                                "-copies:%d" % copies, *flags, *extra], capture_output=True, text=True, timeout=600, check=True)
            rates.append(json.loads(p.stdout.strip().splitlines()[-1])["frames_per_s_after_first_step"])
        out[label] = {"frames_per_s_median": statistics.median(rates), "runs": [round(r) for r in rates]}
    out["gputools_over_without"] = out["gputools"]["frames_per_s_median"] / out["without_flag"]["frames_per_s_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["host"])
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--copies", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if "host" in a.what:
        res["host_parser"] = {"threads": a.threads, "streams": a.streams,
                              **{n: host_rates(n, a.streams, a.threads, a.runs) for n in ("mix_aot29_32k", "mix_aot5_48k", "mix_aot2_64k")}}
    if "kernel" in a.what:
        res["kernel"] = kernel_times(8192, 20)
    if "e2e" in a.what:
        res["end_to_end"] = {"copies": a.copies, "mix_aot29_32k_esbr0": e2e("mix_aot29_32k", a.copies, a.runs, ["-esbr:0"]),
                             "mix_aot2_64k": e2e("mix_aot2_64k", a.copies, a.runs, [])}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
