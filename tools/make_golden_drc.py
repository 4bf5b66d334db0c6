#!/usr/bin/env python3
"""Build tests/golden/drc_spec.npz from the REAL reference decoder run on the committed DRC streams (tests/golden/streams_drc,
tools/make_drc_streams.py): the spectra ixheaacd_imdct_process receives (oracle/ref_capture.c: XAAC_SPEC_DUMP type-2 records,
i.e. behind ixheaacd_drc_apply) for the first FRAMES frames of every stream, once without a DRC flag -- the input of
xaac_drc_apply_host / xaac_drc_apply_batch -- and once with each flag set of FLAG_SETS -- what they have to make of it.
Data only; runs only where the reference was built (oracle/_ref/xaacdec_capture)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_drc_streams import FLAG_SETS, NAMES, OUT as STREAMS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
FRAMES = 8


def reference_spectra(path, flags, n_ch):
    """[frames][n_ch][1024], the first frame's initialisation pass dropped"""
    with tempfile.TemporaryDirectory() as tmp:
        spec = os.path.join(tmp, "spec.bin")
        subprocess.run([os.path.join(REF, "xaacdec_capture"), "-ifile:" + path, "-ofile:" + os.path.join(tmp, "o.wav"), *flags],
                       env=dict(os.environ, XAAC_SPEC_DUMP=spec), check=True, capture_output=True, timeout=600)
        raw = np.fromfile(spec, dtype=np.int32).reshape(-1, 1030)
    return raw[raw[:, 0] == 2][n_ch:, 6:].reshape(-1, n_ch, 1024)


def main():
    out = {"names": np.array(NAMES), "flag_sets": np.array([" ".join(f) for f in FLAG_SETS])}
    for name in NAMES:
        n_ch = 1 if "mono_" in name else 2
        path = os.path.join(STREAMS, name + ".aac")
        plain = reference_spectra(path, (), n_ch)
        out[name + "_in"] = plain[:FRAMES]
        for k, flags in enumerate(FLAG_SETS):
            got = reference_spectra(path, flags, n_ch)
            assert got.shape == plain.shape and not np.array_equal(got, plain), (name, flags)
            out["%s_out%d" % (name, k)] = got[:FRAMES]
    dst = os.path.join(ROOT, "tests", "golden", "drc_spec.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
