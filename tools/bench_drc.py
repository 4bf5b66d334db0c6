#!/usr/bin/env python3
"""What dynamic range control costs on the GPU.  Prints one JSON object and writes it to --out.

  kernel  xaac_drc_apply_batch on 8192 channel-frames: every row active (three bands over the whole row, factors other than 1.0:
          4 KB read and 4 KB written per row), and every row the identity (the wave reads its side row and returns).  Device
          time from events around single launches, median of --reps launches behind three warm-up launches, the spectra restored
          in between; the active rows' share of the HBM roof (8 KB moved per row over the measured copy rate of 6.29 TB/s),
          beside xaac_imdct_process_batch on the same rows.
  e2e     xaacdec_amd -copies:N on a committed DRC stream with and without the -drc_* flags, frames/s behind the first step,
          median of --runs runs, the two alternating; the same with -peak_limiter_off:1 on both sides (the limiter's work depends
          on how loud the frames are, and DRC changes that), and at 16 times the copies.

  python tools/bench_drc.py [kernel] [e2e] [--copies 256] [--runs 5] [--reps 50] [--out profiles/drc_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_COPY_RATE = 6.29e12   # bytes/s, the measured float4 copy


def kernel_times(n, reps):
    import torch
    import drc_cases as dc
    import libxaac_amd
    ctx = libxaac_amd.XaacContext(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    spec0 = torch.from_numpy(rng.integers(-(1 << 24), 1 << 24, (n, 1024), dtype=np.int64).astype(np.int32)).cuda()
    spec_d = spec0.clone()

    def timed(fn):
        ts = []
        for k in range(reps + 3):
            spec_d.copy_(spec0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if k >= 3:
                ts.append(a.elapsed_time(b) * 1000.0)
        return statistics.median(ts), min(ts), max(ts)

    out = {"rows": n}
    for label, row in (("active", dc.side_row([256, 640, 1024], [20000000, 50000000, 41234567])), ("identity", dc.side_row([1024], [dc.ONE]))):
        side_d = torch.from_numpy(np.tile(row, (n, 1))).cuda()
        med, lo, hi = timed(lambda: ctx.drc_apply_batch(spec_d, side_d))
        out[label] = {"us_median": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2)}
        out["launch"] = ctx.last_launch()
    moved = 8192.0 * n
    out["active"]["bytes_moved"] = int(moved)
    out["active"]["share_of_hbm_copy_rate"] = round(moved / HBM_COPY_RATE / (out["active"]["us_median"] * 1e-6), 3)
    ics = torch.zeros((n, 2), dtype=torch.uint8, device="cuda")
    ovl, ovl_state = torch.zeros((n, 512), dtype=torch.int32, device="cuda"), torch.zeros((n, 2), dtype=torch.uint8, device="cuda")
    pcm = torch.zeros(n * 1024, dtype=torch.int16, device="cuda")
    med, lo, hi = timed(lambda: ctx.imdct_process_batch(spec_d, ics, ovl, ovl_state, pcm16=pcm, ch_fac=2))
    out["imdct_same_rows"] = {"us_median": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2)}
    return out


def e2e(name, copies, runs, flags, common=()):
    cli = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
    src = os.path.join(ROOT, "tests", "golden", "streams_drc", name + ".aac")
    rates = {"without_flags": [], "with_flags": []}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(runs):   # alternating, so that what else the host does meets both alike
            for label, extra in (("without_flags", []), ("with_flags", list(flags))):
                p = subprocess.run([cli, "-ifile:" + src, "-ofile:" + os.path.join(tmp, "o.wav"), "-copies:%d" % copies, *common, *extra],
                                   capture_output=True, text=True, timeout=600, check=True)
                rates[label].append(json.loads(p.stdout.strip().splitlines()[-1])["frames_per_s_after_first_step"])
    out = {k: {"frames_per_s_median": statistics.median(v), "runs": [round(r) for r in v]} for k, v in rates.items()}
    out["with_over_without"] = round(out["with_flags"]["frames_per_s_median"] / out["without_flags"]["frames_per_s_median"], 4)
    out["stream"], out["copies"], out["flags"], out["common_flags"] = name, copies, list(flags), list(common)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "e2e"])
    ap.add_argument("--copies", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if "kernel" in a.what:
        res["kernel"] = kernel_times(8192, a.reps)
    if "e2e" in a.what:
        flags = ("-drc_cut_fac:1", "-drc_boost_fac:1", "-drc_target_level:96")
        res["end_to_end"] = e2e("drc_stereo_2band", a.copies, a.runs, flags)
        res["end_to_end_limiter_off"] = e2e("drc_stereo_2band", a.copies, a.runs, flags, ("-peak_limiter_off:1",))
        res["end_to_end_16x_copies"] = e2e("drc_stereo_2band", 16 * a.copies, a.runs, flags)
        res["end_to_end_16x_copies_limiter_off"] = e2e("drc_stereo_2band", 16 * a.copies, a.runs, flags, ("-peak_limiter_off:1",))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
