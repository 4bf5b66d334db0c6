"""Pins the 30-slot host oracle (xo_sbr_dec_lp960 / xo_sbr_dec_hq960: the 960-sample cores of DAB+ / DRM, 15 time slots,
30 QMF slots a frame) to the compiled reference, on the CPU: every ixheaacd_sbr_dec call oracle/_ref/xaacdec_capture records
while the reference decodes 960-line streams with -esbr:0 -- the two committed streams of tests/golden/streams_wide and
streams the reference encoder makes on the spot with -framesize:960, at the rates and bit rates tests/test_sbr960_gpu.py
and tests/test_sbr_hq960_gpu.py use -- goes through the oracle from its own recorded states: return code, PCM, SBR state and
PS state word for word against the record.  Then each stream's calls as chains, the oracle's own states carried.

The fuzzed 30-slot cases of tests/sbr960_fuzz_cases.py are pinned to this oracle, so this file is what decides whether it
is right.  Needs oracle/_ref."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sbr_capture as cap
from test_sbr960_gpu import WIDE, REF, _wav, capture

P16 = ctypes.POINTER(ctypes.c_int16)
N_IN, N_OUT = 960, 1920
LP_POINTS = [(fs, br) for fs in (32000, 44100, 48000) for br in (32000, 96000)]          # tests/test_sbr960_gpu.py
HQ_POINTS = [(fs, br) for fs in (32000, 44100, 48000) for br in (24000, 40000)]          # tests/test_sbr_hq960_gpu.py


def run_oracle(lib, r, st, ps):
    """one record's call through the 30-slot oracle, on the given states (updated in place) -> (rc, pcm [channels, 1920])"""
    pin = np.ascontiguousarray(r["pcm_in"][:N_IN])
    if r["low_pow"]:
        out = np.zeros(N_OUT, np.int16)
        rc = lib.xo_sbr_dec_lp960(ctypes.byref(r["header"]), ctypes.byref(r["frame"]), ctypes.byref(st), pin.ctypes.data_as(P16),
                                  1, out.ctypes.data_as(P16), 1)
        return rc, out[None]
    if r["ps"]:
        out = np.zeros(2 * N_OUT, np.int16)
        rc = lib.xo_sbr_dec_hq960(ctypes.byref(r["header"]), ctypes.byref(r["frame"]), ctypes.byref(st),
                                  ctypes.byref(r["ps_frame"]), ctypes.byref(ps), pin.ctypes.data_as(P16), 1,
                                  out.ctypes.data_as(P16), 2)
        return rc, np.stack([out[0::2], out[1::2]])
    out = np.zeros(N_OUT, np.int16)
    rc = lib.xo_sbr_dec_hq960(ctypes.byref(r["header"]), ctypes.byref(r["frame"]), ctypes.byref(st), None, None,
                              pin.ctypes.data_as(P16), 1, out.ctypes.data_as(P16), 1)
    return rc, out[None]


def check_records(lib, recs, tag):
    """every call from its own st0 / ps0, no record left out; then the calls as chains with the oracle's states carried (a
    call's st0 is the st1 of that channel's previous call), whose final states are the last records' st1 / ps1"""
    for r in recs:
        assert (r["header"].num_time_slots, r["header"].time_step, r["header"].num_columns) == (15, 2, 30), (tag, r["call"])
        st = cap.State.from_buffer_copy(bytes(r["st0"]))
        ps = cap.PsState.from_buffer_copy(bytes(r["ps0"])) if r["ps"] else None
        rc, out = run_oracle(lib, r, st, ps)
        assert rc == r["ret"], (tag, r["call"], rc, r["ret"])
        for c in range(out.shape[0]):
            bad = np.nonzero(out[c] != r["pcm_out"][c][:N_OUT])[0]
            assert bad.size == 0, (tag, "pcm", r["call"], c, int(bad[0]), int(out[c][bad[0]]), int(r["pcm_out"][c][bad[0]]))
        assert not cap.diff_state(st, r["st1"]), (tag, r["call"], cap.diff_state(st, r["st1"])[:3])
        if ps is not None:
            assert not cap.diff_state(ps, r["ps1"]), (tag, "ps", r["call"], cap.diff_state(ps, r["ps1"])[:3])
    chains = []
    for r in recs:
        for c in chains:
            if bytes(c[-1]["st1"]) == bytes(r["st0"]) and (not r["ps"] or bytes(c[-1]["ps1"]) == bytes(r["ps0"])):
                c.append(r)
                break
        else:
            chains.append([r])
    assert max(len(c) for c in chains) >= 35, (tag, [len(c) for c in chains])
    for c in chains:
        st = cap.State.from_buffer_copy(bytes(c[0]["st0"]))
        ps = cap.PsState.from_buffer_copy(bytes(c[0]["ps0"])) if c[0]["ps"] else None
        for r in c:
            rc, out = run_oracle(lib, r, st, ps)
            assert rc == r["ret"] and all(np.array_equal(out[k], r["pcm_out"][k][:N_OUT]) for k in range(out.shape[0])), \
                (tag, "chain", r["call"])
        assert bytes(st) == bytes(c[-1]["st1"]), (tag, "final state", c[-1]["call"], cap.diff_state(st, c[-1]["st1"])[:3])
        if ps is not None:
            assert bytes(ps) == bytes(c[-1]["ps1"]), (tag, "final PS state", c[-1]["call"])


def late(recs):
    """records whose last envelope border lies behind time slot 15 (QMF slot 30)"""
    return sum(bool(r["frame"].apply_processing) and r["frame"].border_vec[r["frame"].num_env] > 15 for r in recs)


def encode(tmp_path, fs, ch, br, aot):
    wav, aac = str(tmp_path / "in.wav"), str(tmp_path / ("enc960_%d_%d_%d_%d.aac" % (aot, ch, fs, br)))
    _wav(wav, fs, ch, seconds=3.0)
    subprocess.run([os.path.join(REF, "xaacenc"), "-ifile:" + wav, "-ofile:" + aac, "-br:%d" % br, "-aot:%d" % aot,
                    "-framesize:960"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert os.path.exists(aac) and os.path.exists(aac[:-4] + ".txt"), "the encoder refused the configuration"
    return aac


def test_committed_lp_stream(oracle, reference, tmp_path):
    recs = capture(os.path.join(WIDE, "he960_aot5.aac"), tmp_path)
    assert len(recs) >= 80 and all(r["low_pow"] == 1 and not r["ps"] for r in recs), len(recs)
    assert late(recs) >= 10
    check_records(oracle.lib, recs, "he960_aot5")


def test_committed_hq_ps_stream(oracle, reference, tmp_path):
    recs = capture(os.path.join(WIDE, "he960_aot29.aac"), tmp_path)
    assert len(recs) >= 40 and all(r["low_pow"] == 0 and r["ps"] == 1 for r in recs), len(recs)
    assert late(recs) >= 10
    check_records(oracle.lib, recs, "he960_aot29")


@pytest.mark.parametrize("fs,br", LP_POINTS)
def test_encoder_made_lp_streams(oracle, reference, tmp_path, fs, br):
    """HE-AAC channel pairs: the reference decodes them in low-power mode"""
    recs = capture(encode(tmp_path, fs, 2, br, 5), tmp_path)
    assert len(recs) >= 45 and all(r["low_pow"] == 1 and not r["ps"] for r in recs), len(recs)
    assert late(recs) >= 1
    check_records(oracle.lib, recs, "lp/%d/%d" % (fs, br))


@pytest.mark.parametrize("fs,br", HQ_POINTS)
@pytest.mark.parametrize("aot,ch", [(29, 2), (5, 1)], ids=["aot29", "aot5mono"])
def test_encoder_made_hq_streams(oracle, reference, tmp_path, fs, br, aot, ch):
    """HE-AACv2 (HQ SBR + PS) and mono HE-AAC (HQ SBR without PS)"""
    recs = capture(encode(tmp_path, fs, ch, br, aot), tmp_path)
    assert len(recs) >= 45 and all(r["low_pow"] == 0 and r["ps"] == (aot == 29) for r in recs), len(recs)
    assert late(recs) >= 1
    check_records(oracle.lib, recs, "hq/%d/%d/%d" % (aot, fs, br))
