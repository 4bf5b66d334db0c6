"""Throughput of the SBR chains for 960-sample cores (30 QMF slots a frame) next to the 1024-sample ones (32 slots), 8192
channel-frames (stream-frames) per step: the low-power chain (xaac_sbr_lp960_process_batch / xaac_sbr_lp_process_batch, rows
lp960 / lp1024) and the HQ chain with parametric stereo (xaac_sbr_hq960_process_batch / xaac_sbr_hq_process_batch, rows hq960 /
hq1024).  All record sets come from the same source: one stereo signal that oracle/_ref/xaacenc encodes as HE-AAC and as
HE-AACv2, each with 960- and with 1024-line frames (same rate, same bit rate: the same SBR band layout), decoded by
oracle/_ref/xaacdec_capture with -esbr:0; the records are replicated to fill the batch, every step starts from the records' own
states.  Prints one JSON line: ms per step and channel-frames/s of each chain.
--per-kernel runs the same measurement again in a child process under rocprofv3 --kernel-trace --stats and adds each kernel's
mean time and channel-frames/s."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_records(tmp, framesize, fs=48000, br=64000, seconds=3.0, aot=5):
    """HE-AAC (aot 5: low-power SBR records) or HE-AACv2 (aot 29: HQ + PS records) of one fixed stereo signal with
    `framesize`-line frames -> the reference's SBR records"""
    import wave
    import sbr_capture as cap
    ref = os.path.join(ROOT, "oracle", "_ref")
    wav = os.path.join(tmp, "in.wav")
    if not os.path.exists(wav):
        t = np.arange(int(fs * seconds)) / fs
        x = 0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t * (1 + 0.3 * t))
        x = x + 0.15 * np.random.default_rng(1).standard_normal(t.size) * (np.sin(2 * np.pi * 1.5 * t) > 0)
        pcm = np.stack([x, np.roll(x, 97)], 1)
        with wave.open(wav, "wb") as w:
            w.setnchannels(2)
            w.setsampwidth(2)
            w.setframerate(fs)
            w.writeframes(np.clip(np.round(pcm * 32767), -32768, 32767).astype(np.int16).tobytes())
    aac, out = os.path.join(tmp, "he%d_%d.aac" % (aot, framesize)), os.path.join(tmp, "he%d_%d.cap" % (aot, framesize))
    subprocess.run([os.path.join(ref, "xaacenc"), "-ifile:" + wav, "-ofile:" + aac, "-br:%d" % br, "-aot:%d" % aot,
                    "-framesize:%d" % framesize], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600, check=True)
    subprocess.run([os.path.join(ref, "xaacdec_capture"), "-ifile:" + aac, "-ofile:" + out + ".wav", "-esbr:0", "-mp4:1",
                    "-imeta:" + aac[:-4] + ".txt"], env=dict(os.environ, XAAC_CAPTURE_FILE=out), stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=600, check=True)
    hq = aot == 29
    recs = [r for r in cap.read_records(out)
            if r["low_pow"] == (0 if hq else 1) and r["ps"] == hq and r["header"].num_columns == framesize // 32]
    assert len(recs) > 50, (framesize, len(recs))
    return recs


def per_kernel(args, n):
    """the same run in a child process under rocprofv3 --kernel-trace --stats: mean time of each kernel"""
    import csv
    import glob
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "r", "--", sys.executable, os.path.abspath(__file__),
               "--n", str(n), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900, check=True)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert files, ("rocprofv3 wrote no kernel statistics", [os.path.relpath(f, d) for f in glob.glob(os.path.join(d, "**"), recursive=True)][:20])
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name, calls, avg = row.get("Name", ""), int(row.get("Calls", 0)), float(row.get("AverageNs", 0))
                if "sbr" not in name and "qmf" not in name and "ps_kernel" not in name:
                    continue
                out[name] = {"calls": calls, "us_mean": round(avg / 1e3, 2), "channel_frames_per_s": round(n / avg * 1e9)}
        return out


def time_entry(ctx, recs, n, n_in, entry, steps, warmup):
    """HQ records (with PS side info) go through an HQ entry with their PS frames and states"""
    import torch
    idx = np.arange(n) % len(recs)
    row = lambda key: torch.from_numpy(np.stack([np.frombuffer(bytes(recs[i][key]), np.uint8) for i in idx])).cuda()
    hdr, frm, st0 = row("header"), row("frame"), row("st0")
    st = st0.clone()
    hq = bool(recs[0]["ps"])
    pf, ps0 = (row("ps_frame"), row("ps0")) if hq else (None, None)
    ps = ps0.clone() if hq else None
    pcm_in = torch.from_numpy(np.concatenate([recs[i]["pcm_in"][:n_in] for i in idx])).cuda()
    out = torch.empty(n * 2 * n_in * (2 if hq else 1), dtype=torch.int16, device="cuda")
    ws = torch.empty(ctx.sbr_hq_workspace_bytes(n, True) if hq else ctx.sbr_lp_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    fn = getattr(ctx, entry)
    times = []
    for k in range(warmup + steps):
        st.copy_(st0)
        if hq:
            ps.copy_(ps0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if hq:
            fn(pcm_in, hdr, frm, st, out, ws, pf, ps, status)
        else:
            fn(pcm_in, hdr, frm, st, out, ws, status)
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b))
    bad = int((status != 0).sum().item())
    ms = float(np.median(times))
    return {"ms_median": round(ms, 4), "ms_min": round(float(np.min(times)), 4), "channel_frames_per_s": round(n / ms * 1e3),
            "refused": bad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192, help="channel-frames per step")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per-kernel", action="store_true", help="add per-kernel times from a rocprofv3 run of the same measurement")
    a = ap.parse_args()
    import torch
    import libxaac_amd
    ctx = libxaac_amd.XaacContext(0, torch.cuda.current_stream().cuda_stream)
    with tempfile.TemporaryDirectory() as tmp:
        r1024, r960 = make_records(tmp, 1024), make_records(tmp, 960)
        h1024, h960 = make_records(tmp, 1024, br=32000, aot=29), make_records(tmp, 960, br=32000, aot=29)
    res = {"lp1024": time_entry(ctx, r1024, a.n, 1024, "sbr_lp_process_batch", a.steps, a.warmup),
           "lp960": time_entry(ctx, r960, a.n, 960, "sbr_lp960_process_batch", a.steps, a.warmup),
           "hq1024": time_entry(ctx, h1024, a.n, 1024, "sbr_hq_process_batch", a.steps, a.warmup),
           "hq960": time_entry(ctx, h960, a.n, 960, "sbr_hq960_process_batch", a.steps, a.warmup)}
    res["ratio_960_to_1024_time"] = round(res["lp960"]["ms_median"] / res["lp1024"]["ms_median"], 4)
    res["ratio_hq960_to_hq1024_time"] = round(res["hq960"]["ms_median"] / res["hq1024"]["ms_median"], 4)
    res.update(n=a.n, steps=a.steps, records_960=len(r960), records_1024=len(r1024), records_hq960=len(h960),
               records_hq1024=len(h1024))
    ctx.close()
    if a.per_kernel:
        res["kernels"] = per_kernel(a, a.n)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
