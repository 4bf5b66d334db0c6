#!/usr/bin/env python3
"""Build tests/golden/sbr960_lp_records.bin.gz and tests/golden/sbr960_hq_ps_records.bin.gz: the first calls (at most 24
each) of the REAL ixheaacd_sbr_dec on 960-sample cores (15 time slots, 30 QMF slots a frame), as oracle/_ref/xaacdec_capture
records them while the reference decodes the committed streams tests/golden/streams_wide/he960_aot5 (HE-AAC, low-power SBR)
and he960_aot29 (HE-AACv2: HQ SBR + parametric stereo) with -esbr:0.  Format: oracle/ref_capture.c's, the one
tests/sbr_capture.read_records reads.  They give the 30-slot fuzz cases (tests/sbr960_fuzz_cases.py) their start states and
header tables on a box that has no reference.  Needs oracle/_ref."""
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sbr_capture as c  # noqa: E402

LIMIT = 24


def pack(r):
    meta = [0x58414331, r["call"], r["low_pow"], r["ch_fac"], r["aot"], r["ps"], r["ret"], r["enh"]]
    b = (np.asarray(meta, np.int32).tobytes() + bytes(r["header"]) + bytes(r["frame"]) + bytes(r["st0"]) +
         r["pcm_in"].astype(np.int16).tobytes() + bytes(r["st1"]) + r["pcm_out"].astype(np.int16).tobytes())
    if r["ps"]:
        b += bytes(r["ps_frame"]) + bytes(r["ps0"]) + bytes(r["ps1"])
    return b


def capture(aac, out):
    subprocess.run([os.path.join(ROOT, "oracle", "_ref", "xaacdec_capture"), "-ifile:" + aac, "-ofile:" + out + ".wav", "-esbr:0",
                    "-mp4:1", "-imeta:" + aac[:-4] + ".txt"], env=dict(os.environ, XAAC_CAPTURE_FILE=out),
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600, check=True)
    return c.read_records(out, limit=LIMIT)


def main():
    with tempfile.TemporaryDirectory() as d:
        for stream, name, low_pow, ps in (("he960_aot5", "sbr960_lp_records.bin.gz", 1, 0),
                                          ("he960_aot29", "sbr960_hq_ps_records.bin.gz", 0, 1)):
            recs = capture(os.path.join(ROOT, "tests", "golden", "streams_wide", stream + ".aac"), os.path.join(d, stream + ".cap"))
            assert len(recs) == LIMIT and all(r["low_pow"] == low_pow and r["ps"] == ps and r["ret"] == 0 for r in recs)
            assert all((r["header"].num_time_slots, r["header"].time_step, r["header"].num_columns) == (15, 2, 30) for r in recs)
            dst = os.path.join(ROOT, "tests", "golden", name)
            with open(dst, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0, filename="") as g:
                g.write(b"".join(pack(r) for r in recs))
            back = c.read_records(dst)
            assert len(back) == len(recs) and all(pack(a) == pack(b) for a, b in zip(back, recs))
            assert os.path.getsize(dst) < 1000000, os.path.getsize(dst)
            print(dst, os.path.getsize(dst), "bytes,", len(recs), "records")


if __name__ == "__main__":
    main()
