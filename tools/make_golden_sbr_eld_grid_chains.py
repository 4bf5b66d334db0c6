#!/usr/bin/env python3
"""Build tests/golden/sbr_eld_grid_chains.npz: chains of the REAL ixheaacd_sbr_dec run as an AAC-ELD channel's (low-delay SBR,
16 or 15 QMF slots a frame, the LD complex banks; oracle/ref_sbr_adapter.c: ref_sbr_dec_eld drives the compiled reference,
oracle/_ref/libref_harness.so) on EVERY GRID A LOW-DELAY BITSTREAM CAN SAY and on several band layouts, the state carried
from call to call by the reference itself.

tests/golden/sbr_eld_chains.npz (tools/make_golden_sbr_eld_chains.py) keeps the grids and the one band layout of its two
streams.  Here there is one chain per (stream, channel) of the layout streams of tools/make_golden_streams.py
(ELD_LAYOUT_STREAMS): the side info is what the reference decoder held while it decoded the stream
(oracle/_ref/xaacdec_capture), walked in order and round again for STEPS steps, so the band layout stays the stream's own
inside a chain.  Every fourth step keeps the captured frame; the others take tests/sbr_grid_cases.py: legal_ld_grid_frame
-- FIXFIX with 1, 2, 4 or 8 envelopes (4 and 8: empty envelopes and an empty noise envelope) or LD_TRAN at one of the 16 (15)
transient positions, with random freq_res, harmonics, envelope and noise-floor words -- and on top of it the fuzz of
make_golden_sbr_chains.py (fuzz_sbr: inverse-filter modes, limiter gains, interpolation, smoothing, harmonics, envelope
exponents).

The core PCM of a step is chain_pcm(kind 3, PCM_CHAIN0 + chain, step) of make_golden_sbr_chains.py, 32 samples per slot (chains
0..15 of kind 3 are sbr_eld_chains.npz's), and is not stored.  Stored, as in sbr_eld_chains.npz: per step header, frame, the
return code, CRC32s of the PCM, of the state after the call and of the rows the synthesis bank hands on, and the step's chain;
per chain the state at its start and its slots per frame.

Every chain's reference calls run in a child process under a time limit: a reference that hangs or dies ends the generator
with a message, and no file is written.  The coverage conditions of sbr_grid_cases.ld_grid_coverage_gaps are asserted before
the file is written (tests/test_sbr_eld_grid_chains.py asserts them again on the committed file), and the table
profiles/sbr_eld_grid_chains_coverage.txt (grids and band layouts of sbr_eld_chains.npz beside this file's) is rewritten.
Data only; runs only where the reference has been built."""
import ctypes
import multiprocessing
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sbr_capture as c  # noqa: E402
from make_golden_sbr_chains import chain_pcm, crc, fuzz_sbr  # noqa: E402
from make_golden_streams import ELD_LAYOUT_STREAMS  # noqa: E402
from sbr_grid_cases import band_layout, ld_grid, ld_grid_coverage_gaps, ld_grid_kind, ld_grid_kinds, legal_ld_grid_frame  # noqa: E402

P16, P32 = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_int32)
STEPS = 96
PCM_CHAIN0 = 16                     # chain_pcm(3, 0..15, .) feed sbr_eld_chains.npz
SEED = 2039
CHAIN_TIME_LIMIT = 120              # seconds for the STEPS reference calls of one chain (they take well under one)
DST = os.path.join(ROOT, "tests", "golden", "sbr_eld_grid_chains.npz")
OLD = os.path.join(ROOT, "tests", "golden", "sbr_eld_chains.npz")
TABLE = os.path.join(ROOT, "profiles", "sbr_eld_grid_chains_coverage.txt")


def captured(name):
    """the records of the reference decoder's ixheaacd_sbr_dec calls on one committed stream"""
    src = os.path.join(ROOT, "tests", "golden", "streams_ld", name + ".aac")
    with tempfile.TemporaryDirectory() as tmp:
        cap = os.path.join(tmp, "cap.bin")
        subprocess.run([os.path.join(ROOT, "oracle", "_ref", "xaacdec_capture"), "-ifile:" + src, "-ofile:" + os.path.join(tmp, "out.wav"),
                        "-mp4:1", "-imeta:" + src[:-4] + ".txt"], env=dict(os.environ, XAAC_CAPTURE_FILE=cap), check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return c.read_records(cap)


def chain_list():
    """(stream, channels, channel) of every chain, in the file's order"""
    return [(name, n_ch, ch) for name, (_, n_ch, _, _) in ELD_LAYOUT_STREAMS.items() for ch in range(n_ch)]


def walk_chain(ci, conn):
    """child process: one chain through the reference -> its rows over the pipe"""
    ref = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_harness.so"))
    ref.ref_sbr_dec_eld.restype = ctypes.c_int
    ref.ref_sbr_dec_eld.argtypes = [ctypes.c_void_p] * 3 + [P16, ctypes.c_int, P16, ctypes.c_int, P32]
    name, n_ch, ch = chain_list()[ci]
    recs = captured(name)
    assert recs and all(r["aot"] == 39 and not r["low_pow"] for r in recs), name
    mine = [r for i, r in enumerate(recs) if i % n_ch == ch]        # a stereo stream's calls alternate between its channels
    n = int(mine[0]["header"].num_time_slots)
    assert n == int(name[3:6]) // 32 and all(r["header"].num_time_slots == n for r in mine), name
    rng = np.random.default_rng([SEED, ci])
    st = c.eld_state_from(mine[0]["st0"])
    row = dict(st0=bytes(st), n_slots=n, header=[], frame=[], ret=[], crc=[])
    for s in range(STEPS):
        r = mine[s % len(mine)]
        h = c.Header.from_buffer_copy(bytes(r["header"]))
        f = c.Frame.from_buffer_copy(bytes(r["frame"]))
        if s % 4 != 3:
            legal_ld_grid_frame(rng, h, f, n)
            fuzz_sbr(rng, h, f, True)       # (True: it draws smoothing_mode too)
        pin = np.ascontiguousarray(chain_pcm(3, PCM_CHAIN0 + ci, s)[:32 * n])
        po = np.zeros(64 * n, np.int16)
        hand = np.zeros(16 * 128, np.int32)
        ret = ref.ref_sbr_dec_eld(ctypes.byref(h), ctypes.byref(f), ctypes.byref(st), pin.ctypes.data_as(P16), 1,
                                  po.ctypes.data_as(P16), 1, hand.ctypes.data_as(P32))
        row["header"].append(bytes(h)); row["frame"].append(bytes(f)); row["ret"].append(int(ret))
        row["crc"].append((crc(po.tobytes()), crc(st), crc(hand[:128 * n].tobytes())))
    conn.send(row)
    conn.close()


def build():
    mp = multiprocessing.get_context("fork")
    rows = []
    for ci, (name, _, ch) in enumerate(chain_list()):
        rx, tx = mp.Pipe(duplex=False)
        p = mp.Process(target=walk_chain, args=(ci, tx))
        p.start()
        tx.close()
        tag = "chain %d (%s, channel %d)" % (ci, name, ch)
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
    u8 = lambda key: np.array([np.frombuffer(b, np.uint8) for row in rows for b in row[key]])
    return dict(header=u8("header"), frame=u8("frame"), ret=np.array([r for row in rows for r in row["ret"]], np.int32),
                crc=np.array([v for row in rows for v in row["crc"]], np.uint32),
                step_chain=np.repeat(np.arange(len(rows), dtype=np.int32), STEPS),
                st0=np.array([np.frombuffer(row["st0"], np.uint8) for row in rows]),
                n_slots=np.array([row["n_slots"] for row in rows], np.int32))


def structs(d):
    """the frames and headers of an ELD chain file as ctypes structs"""
    return ([c.Frame.from_buffer_copy(np.ascontiguousarray(x).tobytes()) for x in d["frame"]],
            [c.Header.from_buffer_copy(np.ascontiguousarray(x).tobytes()) for x in d["header"]])


def coverage_table(old, new):
    """grid x frame length and band layout x (channel_mode, coupling_mode): step counts of sbr_eld_chains.npz beside this file's"""
    lines = ["Low-delay SBR (AAC-ELD) grids and band layouts of the reference-made chains: tests/golden/sbr_eld_chains.npz (two",
             "streams' own side info) beside tests/golden/sbr_eld_grid_chains.npz (every legal low-delay grid on eight streams' band",
             "layouts).  Cells: number of steps.  Written by tools/make_golden_sbr_eld_grid_chains.py.", ""]
    both = {"sbr_eld_chains.npz": structs(old), "sbr_eld_grid_chains.npz": structs(new)}
    for n in (16, 15):
        lines += ["%d time slots a frame (%d-sample core frames)" % (n, 32 * n),
                  "%-10s %-9s %-18s %-14s %-20s %s" % ("class", "position", "borders", "transient_env", "sbr_eld_chains.npz", "sbr_eld_grid_chains.npz")]
        count = {}
        for which, (fr, hd) in both.items():
            for f, h in zip(fr, hd):
                if h.num_time_slots == n:
                    k = (ld_grid_kind(f, n), which)
                    count[k] = count.get(k, 0) + 1
        for kind in ld_grid_kinds(n) + [None]:
            if kind is None:
                if not any(k[0] is None for k in count):
                    continue
                cells = ("other", "-", "-", "-")
            else:
                b, _, t = ld_grid(kind, n)
                cells = ("FIXFIX" if kind[0] == "fixfix" else "LD_TRAN", "%d env" % kind[1] if kind[0] == "fixfix" else str(kind[1]),
                         ",".join(map(str, b)), str(t))
            lines.append("%-10s %-9s %-18s %-14s %-20d %d" % (cells + (count.get((kind, "sbr_eld_chains.npz"), 0), count.get((kind, "sbr_eld_grid_chains.npz"), 0))))
        for which, (fr, hd) in both.items():
            mine = [f for f, h in zip(fr, hd) if h.num_time_slots == n]
            lines.append("%s: most envelopes in a frame %d; frames whose freq_res changes inside: %d" %
                         (which, max(f.num_env for f in mine), sum(any(f.freq_res[e] != f.freq_res[e + 1] for e in range(f.num_env - 1)) for f in mine)))
        lines.append("")
    lines += ["band layouts", "%-6s %-15s %-14s %-12s %-13s %-12s %-12s %-13s %-20s %s" %
              ("slots", "sub_band_start", "sub_band_end", "num_sf_bands", "num_nf_bands", "num_patches", "channel_mode", "coupling_mode",
               "sbr_eld_chains.npz", "sbr_eld_grid_chains.npz")]
    count = {}
    for which, (fr, hd) in both.items():
        for f, h in zip(fr, hd):
            k = (int(h.num_time_slots),) + band_layout(h) + (int(h.channel_mode), int(f.coupling_mode))
            count.setdefault(k, {})[which] = count.setdefault(k, {}).get(which, 0) + 1
    for k in sorted(count, key=lambda k: (-k[0],) + k[1:]):
        lines.append("%-6d %-15d %-14d %-12s %-13d %-12d %-12d %-13d %-20d %d" %
                     (k[0], k[1], k[2], "%d, %d" % k[3], k[4], k[5], k[6], k[7], count[k].get("sbr_eld_chains.npz", 0), count[k].get("sbr_eld_grid_chains.npz", 0)))
    lines.append("")
    return "\n".join(lines)


def main():
    d = build()
    fr, hd = structs(d)
    gaps = ld_grid_coverage_gaps(fr, hd, d["ret"], step_chain=d["step_chain"])
    if gaps:
        sys.exit("the chains miss their coverage: %s -- nothing written" % "; ".join(gaps))
    tmp = DST + ".tmp.npz"
    np.savez_compressed(tmp, **d)
    os.replace(tmp, DST)
    with open(TABLE, "w") as out:
        out.write(coverage_table(np.load(OLD), d))
    print(DST, os.path.getsize(DST), "bytes;", d["ret"].size, "steps in", len(d["n_slots"]), "chains; slots per frame:", d["n_slots"].tolist())


if __name__ == "__main__":
    main()
