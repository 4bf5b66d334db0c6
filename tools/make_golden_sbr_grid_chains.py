#!/usr/bin/env python3
"""Build tests/golden/sbr_grid_chains.npz: chains of the REAL ixheaacd_sbr_dec in low-power mode and in HQ mode with
parametric stereo on FUZZED LEGAL ENVELOPE GRIDS, the state carried from call to call by the reference itself
(oracle/ref_sbr_adapter.c drives the compiled reference, oracle/_ref/libref_harness.so).

tests/golden/sbr_chains.npz (tools/make_golden_sbr_chains.py) keeps the grids of its captured streams; here every step's
grid is drawn by tests/sbr_grid_cases.py: legal_grid_frame -- the legal halves of the grid fuzz of
tests/test_env_pairs_cpu.py -- alternating kind 0 (0 = b0 < .. < b_n = 16) and kind 1 (first border 0..3, last border
13..19), with random freq_res per envelope, noise borders, transient_env, envelope and noise-floor words; on top of it
the fuzz of make_golden_sbr_chains.py (fuzz_sbr: inverse-filter modes, limiter gains, interpolation, smoothing,
harmonics; fuzz_ps for HE-AACv2).  The band limit stays the stream's own.

A chain starts from the state (and keeps the header tables) of one record of tests/golden/sbr_lp_records.bin.gz /
sbr_hq_ps_records.bin.gz.  The core PCM of a step is chain_pcm(kind 4 = LP / 5 = HQ, chain, step) of
make_golden_sbr_chains.py and is not stored.  Stored per step, as in sbr_chains.npz: header, frame, PS frame, the
reference's return code, CRC32s of its PCM and of its state(s) after the call; the full states at each chain's start.

Every chain's reference calls run in a child process under a time limit: a reference that hangs or dies on a grid ends
the generator with a message, and no file is written.  The coverage conditions of sbr_grid_cases.grid_coverage_gaps are
asserted before the file is written (tests/test_sbr_grid_chains.py asserts them again on the committed file), and the
table profiles/sbr_grid_chains_coverage.txt (which grids sbr_chains.npz has, which this file has) is rewritten.
Data only; runs only where the reference has been built."""
import ctypes
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sbr_capture as c  # noqa: E402
from make_golden_sbr_chains import chain_pcm, crc, fuzz_ps, fuzz_sbr  # noqa: E402
from sbr_grid_cases import grid_coverage_gaps, grid_key, legal_grid_frame  # noqa: E402

P16 = ctypes.POINTER(ctypes.c_int16)
CHAINS, STEPS = 16, 24
PCM_KIND = {False: 4, True: 5}      # chain_pcm kinds of this file (0 / 1: sbr_chains.npz, 2: the eSBR chains, 3: the ELD chains)
SEED = 2031
CHAIN_TIME_LIMIT = 120              # seconds for the STEPS reference calls of one chain (they take well under one)
DST = os.path.join(ROOT, "tests", "golden", "sbr_grid_chains.npz")
TABLE = os.path.join(ROOT, "profiles", "sbr_grid_chains_coverage.txt")


def base_records(hq):
    """the captured records, without the ones that were fuzzed at capture ("enh", as make_golden_sbr_chains.py leaves them out):
    some of those carry fine-quantiser IID indices, which fuzz_ps would leave standing in the rows behind its own envelopes when
    it switches to the coarse quantiser -- a PS frame no parser makes, which the boundary refuses (sbr_ps.h: xp_frame_sanitize)
    and the reference, which never reads those rows, does not"""
    recs = c.read_records(os.path.join(ROOT, "tests", "golden", "sbr_hq_ps_records.bin.gz" if hq else "sbr_lp_records.bin.gz"))
    return [r for r in recs if r["enh"] == 0]


def walk_chain(hq, ci, conn):
    """child process: one chain through the reference -> its rows over the pipe"""
    ref = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_harness.so"))
    recs = base_records(hq)
    r = recs[ci * len(recs) // CHAINS]
    rng = np.random.default_rng([SEED, int(hq), ci])
    st = c.State.from_buffer_copy(bytes(r["st0"]))
    ps = c.PsState.from_buffer_copy(bytes(r["ps0"])) if hq else None
    row = dict(st0=bytes(st), ps0=bytes(ps) if hq else b"", header=[], frame=[], ps_frame=[], ret=[], crc_pcm=[], crc_state=[], crc_ps=[])
    for s in range(STEPS):
        h = c.Header.from_buffer_copy(bytes(r["header"]))
        f = c.Frame.from_buffer_copy(bytes(r["frame"]))
        legal_grid_frame(rng, h, f, (ci + s) % 2)
        fuzz_sbr(rng, h, f, hq)
        if not hq:
            h.smoothing_mode = int(rng.integers(0, 2))      # (fuzz_sbr draws it for HQ only)
        pin = np.ascontiguousarray(chain_pcm(PCM_KIND[hq], ci, s))
        if hq:
            pf = c.PsFrame.from_buffer_copy(bytes(r["ps_frame"]))
            fuzz_ps(rng, pf)
            po = np.zeros(4096, np.int16)
            ret = ref.ref_sbr_dec_hq(ctypes.byref(h), ctypes.byref(f), ctypes.byref(st), ctypes.byref(pf), ctypes.byref(ps),
                                     pin.ctypes.data_as(P16), 1, po.ctypes.data_as(P16), 2)
            row["ps_frame"].append(bytes(pf)); row["crc_ps"].append(crc(ps))
        else:
            po = np.zeros(2048, np.int16)
            ret = ref.ref_sbr_dec_lp(ctypes.byref(h), ctypes.byref(f), ctypes.byref(st), pin.ctypes.data_as(P16), 1,
                                     po.ctypes.data_as(P16), 1)
        row["header"].append(bytes(h)); row["frame"].append(bytes(f)); row["ret"].append(int(ret))
        row["crc_pcm"].append(crc(po.tobytes())); row["crc_state"].append(crc(st))
    conn.send(row)
    conn.close()


def build(hq):
    mp = multiprocessing.get_context("fork")
    rows = []
    for ci in range(CHAINS):
        rx, tx = mp.Pipe(duplex=False)
        p = mp.Process(target=walk_chain, args=(hq, ci, tx))
        p.start()
        tx.close()
        tag = "%s chain %d" % ("HQ" if hq else "LP", ci)
        if not rx.poll(CHAIN_TIME_LIMIT):
            p.kill()
            p.join()
            sys.exit("%s: the reference did not finish within %d s -- nothing written" % (tag, CHAIN_TIME_LIMIT))
        try:
            row = rx.recv()
        except EOFError:        # the child died and its end of the pipe closed
            p.join()
            sys.exit("%s: the reference's process ended with exit code %s -- nothing written" % (tag, p.exitcode))
        p.join()
        rows.append(row)
    pre = "hq_" if hq else "lp_"
    u8 = lambda key: np.array([[np.frombuffer(b, np.uint8) for b in row[key]] for row in rows])
    d = {pre + "header": u8("header"), pre + "frame": u8("frame"), pre + "ret": np.array([row["ret"] for row in rows], np.int32),
         pre + "crc_pcm": np.array([row["crc_pcm"] for row in rows], np.uint32),
         pre + "crc_state": np.array([row["crc_state"] for row in rows], np.uint32),
         pre + "st0": np.array([np.frombuffer(row["st0"], np.uint8) for row in rows])}
    if hq:
        d.update({"hq_ps_frame": u8("ps_frame"), "hq_crc_ps": np.array([row["crc_ps"] for row in rows], np.uint32),
                  "hq_ps0": np.array([np.frombuffer(row["ps0"], np.uint8) for row in rows])})
    return d


def structs(d, pre):
    """the frames and headers of one kind ("lp_" / "hq_") of a chain file as ctypes structs"""
    fr = [c.Frame.from_buffer_copy(np.ascontiguousarray(x).tobytes()) for x in d[pre + "frame"].reshape(-1, d[pre + "frame"].shape[-1])]
    hd = [c.Header.from_buffer_copy(np.ascontiguousarray(x).tobytes()) for x in d[pre + "header"].reshape(-1, d[pre + "header"].shape[-1])]
    return fr, hd


def coverage_table(old, new):
    """(num_env, first border, last border) x transient position, per kind: what sbr_chains.npz has beside what this file has"""
    order = ("none", "first", "inner", "end")
    lines = ["Envelope grids of the reference-made fixed-point SBR chains: tests/golden/sbr_chains.npz (the captured streams' own",
             "grids) beside tests/golden/sbr_grid_chains.npz (legal fuzzed grids).  One row per (num_env, first border, last border);",
             "the columns list the positions of transient_env seen with it: none (-1), first (0), inner, end (= num_env); '-' = the",
             "grid does not occur.  Written by tools/make_golden_sbr_grid_chains.py.", ""]
    for pre, name in (("lp_", "low power"), ("hq_", "HQ + PS")):
        keys, lengths = {}, {"old": set(), "new": set()}
        for which, d in (("old", old), ("new", new)):
            for f in structs(d, pre)[0]:
                n, b0, bn, t = grid_key(f)
                keys.setdefault((n, b0, bn), {"old": set(), "new": set()})[which].add(t)
                lengths[which].update(f.border_vec[e + 1] - f.border_vec[e] for e in range(n))
        n_old = sum(1 for v in keys.values() if v["old"])
        n_new = sum(1 for v in keys.values() if v["new"])
        only_new = sum(1 for v in keys.values() if not v["old"])
        lines += ["%s: %d grids in sbr_chains.npz, %d in sbr_grid_chains.npz, %d of them in the new file only" % (name, n_old, n_new, only_new),
                  "envelope lengths in time slots: %s in sbr_chains.npz; in the new file also %s" %
                  (sorted(lengths["old"]), sorted(lengths["new"] - lengths["old"])),
                  "%-8s %-6s %-5s  %-26s %s" % ("num_env", "first", "last", "sbr_chains.npz", "sbr_grid_chains.npz")]
        for (n, b0, bn), v in sorted(keys.items()):
            cell = lambda s: ",".join(t for t in order if t in s) or "-"
            lines.append("%-8d %-6d %-5d  %-26s %s" % (n, b0, bn, cell(v["old"]), cell(v["new"])))
        lines.append("")
    return "\n".join(lines)


def main():
    d = build(False)
    d.update(build(True))
    for pre in ("lp_", "hq_"):
        fr, hd = structs(d, pre)
        gaps = grid_coverage_gaps(fr, hd, d[pre + "ret"])
        if gaps:
            sys.exit("%s chains miss their coverage: %s -- nothing written" % (pre[:2].upper(), "; ".join(gaps)))
    tmp = DST + ".tmp.npz"
    np.savez_compressed(tmp, **d)
    os.replace(tmp, DST)
    with open(TABLE, "w") as out:
        out.write(coverage_table(np.load(os.path.join(ROOT, "tests", "golden", "sbr_chains.npz")), d))
    print(DST, os.path.getsize(DST), "bytes;", d["lp_ret"].size, "LP steps,", d["hq_ret"].size, "HQ+PS steps")


if __name__ == "__main__":
    main()
