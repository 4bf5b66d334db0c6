"""Fuzzed cases for the 30-slot SBR and PS entry points (the 960-sample cores of DAB+ / DRM: xaac_sbr_lp960_process_batch,
xaac_sbr_hq960_process_batch), shared by tests/test_sbr960_fuzz_cpu.py -- what the cases cover, on the oracle's side -- and
tests/test_sbr960_fuzz_gpu.py -- the kernels against them, word for word.  Every case is built once from the 30-slot host
oracle (xo_sbr_dec_lp960 / xo_sbr_dec_hq960, which tests/test_sbr960_oracle_vs_reference.py pins to the reference on captured
960-line calls) and kept.

Start states and header tables are the reference's own: the first calls it made on the two committed 960-line streams
(tests/golden/sbr960_lp_records.bin.gz, sbr960_hq_ps_records.bin.gz; tools/make_golden_sbr960.py).  The side info comes
from the generators of the 32-slot tests at 15 time slots / 30 QMF slots (sbr_grid_cases.legal_grid_frame,
ps_walk_cases._fuzz_ps / _borders_off_zero).

  ps_cases      the case table of tests/test_ps_prep_gpu.py forced at 30 slots: 30 chains of 3 frames
  hq_chain      10 streams x 6 frames of fuzzed grids, header switches, harmonics and a moving band limit: HQ + PS, or mono HQ
  lp_chain      the same for the low-power entry: 10 channels (5 interleaved pairs) or 5 mono channels x 6 frames
  list_case     a batch of five in which two streams reach above band 48 (the 64-band list launch of the HQ core)
  malformed     a batch of five with one SBR frame and one PS frame of random bytes"""
import ctypes
import functools
import os

import numpy as np

import ps_walk_cases as pw
import sbr_capture as cap
from sbr_grid_cases import legal_grid_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = ctypes.POINTER(ctypes.c_int16)
LP_GOLDEN = os.path.join(ROOT, "tests", "golden", "sbr960_lp_records.bin.gz")
HQ_GOLDEN = os.path.join(ROOT, "tests", "golden", "sbr960_hq_ps_records.bin.gz")
NQ, NTS, N_IN, N_OUT = 30, 15, 960, 1920
BATCH = 4 + 1            # the PS kernel and the narrow HQ core hold four stream-frames a workgroup: one stream more
MAX = 0x7fffffff

PS_CASES, PS_FRAMES, PS_SEED = 30, 3, 77
MID = [3, 9, 15]         # first borders inside the frame with border + 14 < 30
LATE_BORDER = NQ - 1     # a PS border at the frame's last slot
ZERO_BUMP = [0, 2, 0, 1]  # on top of ps_walk_cases.RAISE in front of frame 1: these streams' common_shift comes out at -2 there
                          # from a start of -11 and at -1 from -10, so that some cases meet 0
STREAMS, FRAMES = 10, 6  # two and a half workgroups of the narrow HQ core
AMPS = [32767, 3000, 9]  # core PCM: full scale, +-3000, +-9


@functools.lru_cache(maxsize=None)
def lp_records():
    return cap.read_records(LP_GOLDEN)


@functools.lru_cache(maxsize=None)
def hq_records():
    return cap.read_records(HQ_GOLDEN)


def run_hq(oracle, h, f, st, pf, ps, pcm):
    """one frame through xo_sbr_dec_hq960 on copies of the states -> (rc, pcm [1920] or L,R pairs [3840], state, ps state)"""
    s = cap.State.from_buffer_copy(bytes(st))
    if pf is None:
        out = np.zeros(N_OUT, np.int16)
        rc = oracle.lib.xo_sbr_dec_hq960(ctypes.byref(h), ctypes.byref(f), ctypes.byref(s), None, None, pcm.ctypes.data_as(P16), 1,
                                         out.ctypes.data_as(P16), 1)
        return rc, out, s, None
    p = cap.PsState.from_buffer_copy(bytes(ps))
    out = np.zeros(2 * N_OUT, np.int16)
    rc = oracle.lib.xo_sbr_dec_hq960(ctypes.byref(h), ctypes.byref(f), ctypes.byref(s), ctypes.byref(pf), ctypes.byref(p),
                                     pcm.ctypes.data_as(P16), 1, out.ctypes.data_as(P16), 2)
    return rc, out, s, p


def run_lp(oracle, h, f, st, pcm):
    s = cap.State.from_buffer_copy(bytes(st))
    out = np.zeros(N_OUT, np.int16)
    rc = oracle.lib.xo_sbr_dec_lp960(ctypes.byref(h), ctypes.byref(f), ctypes.byref(s), pcm.ctypes.data_as(P16), 1,
                                     out.ctypes.data_as(P16), 1)
    return rc, out, s


_built = {}


def _once(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


# ---- the PS kernel's case table -----------------------------------------------------------------------------------------
def ps_borders(pf):
    """the borders a PS frame's slot walk can meet: the entries up to the first that is not above its predecessor"""
    b = [int(pf.border_position[e]) for e in range(7)]
    n = 1
    while n < 7 and b[n] > b[n - 1]:
        n += 1
    return b[:n]


def _add_border(pf, slot):
    """puts a border at `slot` in front of the frame's last one (in place of the last inner one where all five envelopes
    are taken); the first border stays"""
    b = [int(pf.border_position[e]) for e in range(7)]
    end = b.index(NQ)
    if slot in b[:end]:
        return
    if end < 5:
        b[end:end + 2] = [slot, NQ]
    else:
        b[end - 1] = slot
    for e in range(7):
        pf.border_position[e] = b[e]


def ps_cases(oracle):
    """-> list over cases of dict(rec, mode, det, steps): steps = list over frames of dict(frame, ps_frame, pcm, st_in,
    ps_in, want, common_shift, usb_prev)"""
    return _once("ps", lambda: _ps_cases(oracle))


def _ps_cases(oracle):
    recs = [r for r in hq_records() if r["ps0"].usb > 0]       # (the stream's first calls still carry a new PS state)
    rng = np.random.default_rng(PS_SEED)
    out = []
    for k in range(PS_CASES):
        r = recs[(5 * k) % len(recs)]
        mode = ["zero", "mid", "never"][k % 3]
        det = {0: "zeroed", 3: "full"}.get(k % 7, "recorded")
        st = cap.State.from_buffer_copy(bytes(r["st0"]))
        ps = cap.PsState.from_buffer_copy(bytes(r["ps0"]))
        ps.idx_long = k % 14
        for name in ("peak_decay_diff", "energy_prev", "peak_decay_diff_prev"):
            if det != "recorded":
                for b in range(20):
                    getattr(ps, name)[b] = 0 if det == "zeroed" else MAX
        limit = 20 if det == "zeroed" else int(r["st0"].syn_usb)   # zeroed: nothing above band 20, bins 18 and 19 stay silent
        st.syn_usb = limit
        steps = []
        for step in range(PS_FRAMES):
            f = cap.Frame.from_buffer_copy(bytes(r["frame"]))
            pf = cap.PsFrame.from_buffer_copy(bytes(r["ps_frame"]))
            pw._fuzz_ps(rng, pf, NQ)
            st = cap.State.from_buffer_copy(bytes(st))
            st.st_syn_scale += pw.RAISE[step] + (ZERO_BUMP[k % 4] if step == 1 else 0)
            if mode == "mid":
                pw._borders_off_zero(rng, pf, NQ)
                rest = sorted(int(pf.border_position[e]) for e in range(1, 7) if int(pf.border_position[e]) > MID[k % 3])
                first = [MID[k % 3]] + rest
                for e in range(7):
                    pf.border_position[e] = first[e] if e < len(first) else int(rng.integers(0, NQ + 1))
            if k % 5 == 4 and step != 1:
                _add_border(pf, LATE_BORDER)
            if mode != "never":
                if step == 1:
                    st.syn_usb = int(rng.integers(8, min(23, limit)))
                if step == 2:
                    st.syn_usb = limit
            pcm = rng.integers(-pw.AMP, pw.AMP + 1, N_IN).astype(np.int16)
            want = run_hq(oracle, r["header"], f, st, pf, ps, pcm)
            steps.append(dict(frame=f, ps_frame=pf, pcm=pcm, st_in=st, ps_in=ps, want=want, usb_prev=int(ps.usb),
                              common_shift=int(st.st_syn_scale) - int(want[2].ps_scale) - 8))
            st, ps = want[2], want[3]
        out.append(dict(rec=r, mode=mode, det=det, steps=steps))
    return out


# ---- HQ core, banks and pair synthesis; the low-power entry --------------------------------------------------------------
def _fuzz_sbr(rng, h, f, kind, step):
    """a legal envelope grid at 15 time slots with everything that hangs on it (sbr_grid_cases.set_grid: freq_res,
    transient_env, inverse-filter modes, harmonics, envelope and noise words), the header's switches, frames without
    harmonics, and on some frames a band limit moved by up to 6 bands"""
    legal_grid_frame(rng, h, f, kind, NTS)
    h.limiter_gains = int(rng.integers(0, 4))
    h.interpol_freq = int(rng.integers(0, 2))
    h.smoothing_mode = int(rng.integers(0, 2))
    if rng.integers(0, 3) == 0:
        for k in range(len(f.add_harmonics)):
            f.add_harmonics[k] = 0
    if step % 3 == 2:
        f.max_qmf_subband_aac = int(np.clip(f.max_qmf_subband_aac + rng.integers(-6, 7), h.sub_band_start, 32))


def hq_chain(oracle, with_ps):
    """-> list over frames of dict(headers, frames, ps_frames, pcm, st_in, ps_in, want): lists over the 10 streams; want[i] =
    (rc, pcm, state, ps state).  with_ps False: the same streams as mono HQ (channel_mode mono, no PS buffers)"""
    return _once(("hq", with_ps), lambda: _hq_chain(oracle, with_ps))


def _hq_chain(oracle, with_ps):
    recs = hq_records()[2:2 + 2 * STREAMS:2]
    rng = np.random.default_rng(961 if with_ps else 2960)
    states = [cap.State.from_buffer_copy(bytes(r["st0"])) for r in recs]
    pstates = [cap.PsState.from_buffer_copy(bytes(r["ps0"])) if with_ps else None for r in recs]
    hdrs = [cap.Header.from_buffer_copy(bytes(r["header"])) for r in recs]
    steps = []
    for step in range(FRAMES):
        d = dict(headers=[], frames=[], ps_frames=[], pcm=[], st_in=[], ps_in=[], want=[])
        for i, r in enumerate(recs):
            h = cap.Header.from_buffer_copy(bytes(hdrs[i]))
            f = cap.Frame.from_buffer_copy(bytes(r["frame"]))
            _fuzz_sbr(rng, h, f, int((i + step) % 3 != 0), step)   # two variable grids to one fixed
            pf = None
            if with_ps:
                pf = cap.PsFrame.from_buffer_copy(bytes(r["ps_frame"]))
                pw._fuzz_ps(rng, pf, NQ)
            else:
                h.channel_mode = 1
            amp = AMPS[(i + step) % 3]
            pcm = rng.integers(-amp, amp + 1, N_IN).astype(np.int16)
            want = run_hq(oracle, h, f, states[i], pf, pstates[i], pcm)
            d["headers"].append(h); d["frames"].append(f); d["ps_frames"].append(pf); d["pcm"].append(pcm)
            d["st_in"].append(states[i]); d["ps_in"].append(pstates[i]); d["want"].append(want)
            states[i], pstates[i], hdrs[i] = want[2], want[3], h
        steps.append(d)
    return steps


def lp_chain(oracle, stereo):
    """-> list over frames of dict(headers, frames, pcm, st_in, want): lists over the channels -- 10 (five interleaved pairs)
    or, stereo False, 5 mono channels; want[i] = (rc, pcm, state)"""
    return _once(("lp", stereo), lambda: _lp_chain(oracle, stereo))


def _lp_chain(oracle, stereo):
    n = 2 * BATCH if stereo else BATCH
    recs = lp_records()[4:4 + n] if stereo else lp_records()[6:6 + 3 * n:3]
    rng = np.random.default_rng(1960 + stereo)
    states = [cap.State.from_buffer_copy(bytes(r["st0"])) for r in recs]
    hdrs = [cap.Header.from_buffer_copy(bytes(r["header"])) for r in recs]
    steps = []
    for step in range(FRAMES):
        d = dict(headers=[], frames=[], pcm=[], st_in=[], want=[])
        for i, r in enumerate(recs):
            h = cap.Header.from_buffer_copy(bytes(hdrs[i]))
            f = cap.Frame.from_buffer_copy(bytes(r["frame"]))
            _fuzz_sbr(rng, h, f, int((i + step) % 3 != 0), step)   # two variable grids to one fixed
            amp = AMPS[(i // 2 + step) % 3]
            pcm = rng.integers(-amp, amp + 1, N_IN).astype(np.int16)
            want = run_lp(oracle, h, f, states[i], pcm)
            d["headers"].append(h); d["frames"].append(f); d["pcm"].append(pcm); d["st_in"].append(states[i]); d["want"].append(want)
            states[i], hdrs[i] = want[2], h
        steps.append(d)
    return steps


# ---- the list launch; malformed side info -------------------------------------------------------------------------------
WIDE_STREAMS = (1, 3)    # of the list case: the two streams that reach above band 48


def list_case(oracle):
    """five HQ + PS streams over two frames as the reference recorded them, but stream 1 with its synthesis bank's limit at band
    52 and stream 3 with overlap words above band 48 (left there by a frame with a wider SBR range): both need the 64-band
    rows.  -> list over frames of dict(recs, st_in, ps_in, want)"""
    return _once("list", lambda: _list_case(oracle))


def _list_case(oracle):
    recs = hq_records()
    rng = np.random.default_rng(23)
    pick = [4, 7, 10, 13, 16]
    states = [cap.State.from_buffer_copy(bytes(recs[j]["st0"])) for j in pick]
    pstates = [cap.PsState.from_buffer_copy(bytes(recs[j]["ps0"])) for j in pick]
    states[WIDE_STREAMS[0]].syn_usb = 52
    ov = np.frombuffer(states[WIDE_STREAMS[1]], dtype=np.int32, count=6 * 128, offset=cap.State.overlap.offset).reshape(6, 2, 64)
    ov[:, :, 50:] = rng.integers(-2000, 2000, ov[:, :, 50:].shape)
    steps = []
    for step in range(2):
        batch = [recs[j + step] for j in pick]
        pcm = [rng.integers(-9000, 9001, N_IN).astype(np.int16) for _ in pick]
        want = [run_hq(oracle, r["header"], r["frame"], states[i], r["ps_frame"], pstates[i], pcm[i]) for i, r in enumerate(batch)]
        steps.append(dict(recs=batch, pcm=pcm, st_in=states, ps_in=pstates, want=want))
        states, pstates = [w[2] for w in want], [w[3] for w in want]
    return steps


MALFORMED_BORDERS = (0, 12, NQ + 1)
BAD_SBR, BAD_PS = 1, 3   # of the malformed batch: the stream with a random SBR frame / a random PS frame


def malformed(oracle):
    """-> dict(recs, frames, ps_frames, want): five recorded calls, stream 1's SBR frame and stream 3's PS frame random bytes"""
    return _once("malformed", lambda: _malformed(oracle))


def _malformed(oracle):
    recs = hq_records()[5:5 + BATCH]
    rng = np.random.default_rng(8)
    frames = [cap.Frame.from_buffer_copy(bytes(r["frame"])) for r in recs]
    psf = [cap.PsFrame.from_buffer_copy(bytes(r["ps_frame"])) for r in recs]
    frames[BAD_SBR] = cap.Frame.from_buffer_copy(rng.integers(0, 256, ctypes.sizeof(cap.Frame), dtype=np.uint8).tobytes())
    frames[BAD_SBR].apply_processing = 1
    psf[BAD_PS] = cap.PsFrame.from_buffer_copy(rng.integers(0, 256, ctypes.sizeof(cap.PsFrame), dtype=np.uint8).tobytes())
    # ... of which the first borders are 0, 12 and 31: legal at 32 slots, behind the frame at 30, where the boundary holds it
    # to 30 -- and the second envelope's length, 18 slots then and not 19, is heard in every slot from 12 on
    for e, v in enumerate(MALFORMED_BORDERS):
        psf[BAD_PS].border_position[e] = v
    want = [run_hq(oracle, r["header"], frames[i], r["st0"], psf[i], r["ps0"], np.ascontiguousarray(r["pcm_in"][:N_IN]))
            for i, r in enumerate(recs)]
    return dict(recs=recs, frames=frames, ps_frames=psf, want=want)
