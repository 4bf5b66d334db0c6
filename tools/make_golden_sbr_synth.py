#!/usr/bin/env python3
"""Build tests/golden/sbr_synth_ref.npz from the REAL reference decoder run on tests/golden/streams_synth_sbr/*.aac
(tools/make_synth_sbr_streams.py): per stream, frame and channel the CRC32 of the SBR header tables, the frame data and the PS
frame the reference holds at every ixheaacd_sbr_dec call with -esbr:0 (<name>_sbr), the same plus the xaac_esbr_side members
and the QMF transposer's parameters with its default flags (<name>_esbr, <name>_hbe), both through tools/make_golden_parser.py's
capture / capture_esbr; what the records say about the stream, for the coverage test (<name>_cov, columns
tests/sbr_synth_cases.py: COV); and CRC32 and size of the files `xaacdec -esbr:0` and plain `xaacdec` write, with the CRC32 of their samples alone (<name>_wav:
three words per flag set).
Data only; runs only where oracle/_ref is built."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sbr_synth_cases as cs  # noqa: E402


def main():
    d = {}
    with tempfile.TemporaryDirectory() as tmp:
        for row in cs.ROWS:
            name, kind = row[0], row[3]
            plain, esbr, _ = cs.reference_rows(cs.path(name), tmp, cs.channels(kind))
            d[name + "_sbr"], _ = cs.crc_rows(plain, False)
            d[name + "_esbr"], d[name + "_hbe"] = cs.crc_rows(esbr, True)
            d[name + "_cov"] = cs.coverage_rows(plain, esbr)
            wav = []
            for flags in cs.FLAG_SETS:
                blob = cs.checked_reference_wav(row, flags, tmp) if row[6] else cs.reference_wav(cs.path(name), flags, tmp)
                wav += [cs.crc(blob), len(blob), cs.crc(cs.wav_facts(blob)[3])]
            d[name + "_wav"] = np.array(wav, np.uint32)
            print(name, "frames", len(plain), "applied", int(d[name + "_cov"][:, 0, 4].sum()), "wav bytes", wav[1], wav[4])
    np.savez_compressed(cs.GOLD, **d)


if __name__ == "__main__":
    main()
