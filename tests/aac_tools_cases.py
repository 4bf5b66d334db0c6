"""Shared by tests/test_aac_tools_cpu.py and tests/test_aac_tools_gpu.py: the streams the AAC spectral tools are walked over
(the committed ADTS streams plus streams oracle/_ref/xaacenc makes on the spot from a transient-rich signal), the
reference's own spectra behind the tools (oracle/_ref/xaacdec_capture, XAAC_SPEC_DUMP type-2 records), a frame walker on
the host parser (stage 1 + side info, stage 2), the host twin, and the generator of random but syntax-legal elements."""
import ctypes
import os
import subprocess
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libxaac_amd import decoder  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
COMMITTED = ["mix_aot2_64k", "mix_aot5_48k", "mono_aot5_32k", "harm_aot5_48k", "mix_aot29_32k", "synth_lc_a", "synth_lc_b",
             "synth_lc_mono", "lc_aot2_16k_mono", "he_aot5_44k"]
# (name, sampling rate of the input, channels, encoder arguments): AAC-LC and HE-AAC, mono and stereo, core rates 16 .. 48 kHz,
# low and high bit rates
ENCODED = [("lc_48k_st_hi", 48000, 2, ["-aot:2", "-br:192000"]), ("lc_48k_st_lo", 48000, 2, ["-aot:2", "-br:48000"]),
           ("lc_32k_st", 32000, 2, ["-aot:2", "-br:96000"]), ("lc_24k_mono", 24000, 1, ["-aot:2", "-br:32000"]),
           ("lc_16k_st", 16000, 2, ["-aot:2", "-br:40000"]), ("he_48k_st", 48000, 2, ["-aot:5", "-br:64000"]),
           ("he_32k_mono", 32000, 1, ["-aot:5", "-br:24000"])]


def need(binary):
    import pytest
    if not os.path.exists(os.path.join(REF, binary)):
        pytest.fail("oracle/_ref/%s missing: the reference binaries (built by oracle/Makefile.ref where the reference tree "
                    "exists, git-ignored) did not travel with the snapshot -- the tools' evidence must not vanish silently" % binary)


def transient_signal(rate, channels, seconds=1.3, seed=7):
    """castanet-like clicks and tone bursts over a quiet noise floor: block switching, TNS and M/S in the encoder"""
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    t = np.arange(n) / rate
    x = 0.02 * rng.standard_normal((n, channels))
    for k in range(int(seconds * 9)):
        at = int(rng.integers(0, n - 2000))
        length = int(rng.integers(40, 900))
        env = np.exp(-np.arange(length) / (length / 5.0))
        burst = env * (rng.standard_normal(length) * 0.6 + np.sin(2 * np.pi * rng.uniform(500, 0.4 * rate) * np.arange(length) / rate))
        for c in range(channels):
            x[at:at + length, c] += burst * (0.8 if c == 0 or k % 3 else -0.5)
    x += 0.15 * np.sin(2 * np.pi * 440.0 * t)[:, None]
    if channels == 2:
        x[:, 1] += 0.1 * np.sin(2 * np.pi * 1320.0 * t)
    return np.clip(x, -0.98, 0.98)


def stream_files(tmp):
    """-> [(name, path)]: the committed streams, then the encoder-made ones (written under tmp)"""
    need("xaacenc")
    out = [(n, os.path.join(STREAMS, n + ".aac")) for n in COMMITTED]
    for name, rate, ch, args in ENCODED:
        wav, aac = os.path.join(tmp, name + ".wav"), os.path.join(tmp, name + ".aac")
        if not os.path.exists(aac):
            pcm = np.round(transient_signal(rate, ch) * 32767.0).astype(np.int16)
            with wave.open(wav, "wb") as w:
                w.setnchannels(ch), w.setsampwidth(2), w.setframerate(rate)
                w.writeframes(pcm.tobytes())
            subprocess.run([os.path.join(REF, "xaacenc"), "-ifile:" + wav, "-ofile:" + aac, "-adts:1"] + args,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=600)
        out.append((name, aac))
    return out


def reference_spectra(path, tmp, n_ch, record=2):
    """the reference's spectra as ixheaacd_imdct_process receives them: [frames][n_ch][1024] (XAAC_SPEC_DUMP type-2 records of
    oracle/ref_capture.c, the first frame's initialisation pass dropped); record=1: its type-1 records, the spectra in front of
    the tools"""
    need("xaacdec_capture")
    spec = os.path.join(tmp, "spec_%s.bin" % os.path.basename(path))
    if os.path.exists(spec):
        os.remove(spec)
    subprocess.run([os.path.join(REF, "xaacdec_capture"), "-ifile:" + path, "-ofile:" + spec + ".wav", "-esbr:0"],
                   env=dict(os.environ, XAAC_SPEC_DUMP=spec), check=True, capture_output=True, timeout=600)
    raw = np.fromfile(spec, dtype=np.int32).reshape(-1, 1030)
    t2 = raw[raw[:, 0] == record][n_ch:, 6:]
    return t2.reshape(-1, n_ch, 1024)


def walk(data):
    """every frame of an ADTS stream -> (stage-1 spectra int32[2,1024], side info uint8[CORE_TOOLS_SIDE_BYTES], XAAC_TOOL_* bits,
    n_ch); and the stage-2 spectra of a second parser [frames][n_ch][1024]"""
    lib = decoder.load_host_library()
    frames = []
    p = ctypes.c_void_p()
    assert lib.xaac_parser_create(ctypes.byref(p)) == 0
    core, used, pos = decoder.CoreFrame(), ctypes.c_size_t(), 0
    try:
        while pos + 7 <= len(data):
            rc = lib.xaac_parse_adts_frame(p, data[pos:], len(data) - pos, 1, ctypes.byref(core), ctypes.byref(used))
            if rc != 0:
                break
            pos += used.value
            side = np.zeros(decoder.CORE_TOOLS_SIDE_BYTES, np.uint8)
            assert lib.xaac_parse_core_tools_side(p, side.ctypes.data) == 0
            spec = np.zeros((2, 1024), np.int32)
            spec[:core.n_ch] = np.ctypeslib.as_array(core.spec)[:core.n_ch]
            frames.append((spec, side, int(core.tools), int(core.n_ch)))
    finally:
        lib.xaac_parser_destroy(p)
    after = [f[0] for f in decoder.parse_stream(data, stage=2)]
    return frames, after


def apply_host(spec, side, state):
    """xaac_core_tools_apply_host on copies -> (status, spectra, state)"""
    lib = decoder.load_host_library()
    spec, state = np.ascontiguousarray(spec).copy(), np.ascontiguousarray(state).copy()
    rc = lib.xaac_core_tools_apply_host(np.ascontiguousarray(side).ctypes.data, state.ctypes.data, spec.ctypes.data)
    return rc, spec, state


# ---- random elements ----------------------------------------------------------------------------------------------------
NUM_SWB_LONG = [41, 41, 47, 49, 49, 51, 47, 47, 43, 43, 43, 40]
NUM_SWB_SHORT = [12, 12, 12, 14, 14, 14, 15, 15, 15, 15, 15, 15]


def _random_channel(rng, ch, sr, ics=None):
    if ics is None:
        seq = int(rng.integers(0, 4))
        if seq == 2:
            cuts = sorted(rng.choice(np.arange(1, 8), size=int(rng.integers(0, 8)), replace=False).tolist())
            lens = np.diff([0] + cuts + [8]).tolist()
            max_sfb = int(rng.integers(0, NUM_SWB_SHORT[sr] + 1))
        else:
            lens = [1]
            max_sfb = int(rng.integers(0, NUM_SWB_LONG[sr] + 1))
        ics = (seq, max_sfb, lens)
    seq, max_sfb, lens = ics
    ch.window_sequence, ch.max_sfb, ch.num_groups = seq, max_sfb, len(lens)
    for g, v in enumerate(lens):
        ch.group_len[g] = v
    for g in range(len(lens)):
        for sfb in range(max_sfb):
            b = 16 * g + sfb
            ch.cb[b] = int(rng.choice([0, 1, 3, 5, 7, 9, 11, 11, 13, 13, 14, 15]))
            ch.sf[b] = int(rng.integers(-60, 200)) if ch.cb[b] >= 13 else int(rng.integers(60, 200))
            if ch.cb[b] == 13:
                ch.pns_used[b] = 1
                ch.pns_active = 1
    if rng.random() < 0.7:
        ch.tns_present = 1
        for w in range(8 if seq == 2 else 1):
            n_filt = int(rng.integers(0, 2 if seq == 2 else 4))
            ch.n_filt[w] = n_filt
            top = NUM_SWB_SHORT[sr] if seq == 2 else NUM_SWB_LONG[sr]
            for f in range(n_filt):
                flt = ch.tns[w if seq == 2 else f]
                length = int(rng.integers(0, 16 if seq == 2 else 64))
                top = max(top, length)
                flt.start_band, flt.stop_band = top - length, top
                top = flt.start_band
                flt.order = int(rng.integers(0, 8 if (seq == 2 and rng.random() < 0.5) else 13))
                if flt.order:
                    flt.direction = -1 if rng.random() < 0.5 else 1
                    flt.resolution = int(rng.integers(0, 2))
                    bits = flt.resolution + 3 - int(rng.integers(0, 2))
                    for i in range(flt.order):
                        flt.coef[i] = int(rng.integers(-(1 << (bits - 1)), 1 << (bits - 1)))
                else:
                    flt.direction = 1
    return ics


def random_element(rng):
    """-> (side uint8[...], spec int32[2,1024], state uint8[...]): random but syntax-legal side info over random stage-1 spectra
    (full-scale, small and zero bands mixed)"""
    side = decoder.CoreToolsSide()
    side.sr_index = int(rng.integers(0, 12))
    side.n_ch = 2 if rng.random() < 0.8 else 1
    side.element_id = 1 if side.n_ch == 2 else 0
    side.common_window = int(side.n_ch == 2 and rng.random() < 0.7)
    ics = _random_channel(rng, side.ch[0], side.sr_index)
    if side.n_ch == 2:
        _random_channel(rng, side.ch[1], side.sr_index, ics if side.common_window else None)
    if side.common_window:
        mask = int(rng.integers(0, 3))
        l, r = side.ch[0], side.ch[1]
        pns = l.pns_active or r.pns_active
        for g in range(l.num_groups):
            for sfb in range(l.max_sfb):
                b = 16 * g + sfb
                ms = int(rng.integers(0, 2)) if mask == 1 else int(mask == 2)
                if ms and pns:                       # channel.c:702-725
                    side.pns_correlated[b] = 1
                    if l.pns_used[b] and r.pns_used[b]:
                        ms = 0
                side.ms_used[b] = ms
    spec = np.zeros((2, 1024), np.int32)
    for c in range(side.n_ch):
        for lo in range(0, 1024, 32):
            kind = rng.random()
            if kind < 0.25:
                continue
            mag = 31 if kind < 0.4 else (int(rng.integers(4, 12)) if kind < 0.6 else int(rng.integers(12, 30)))
            spec[c, lo:lo + 32] = rng.integers(-(1 << mag), 1 << mag, 32, dtype=np.int64).astype(np.int32)
    state = rng.integers(-2 ** 31, 2 ** 31, 129, dtype=np.int64).astype(np.int32).view(np.uint8).copy()
    return np.frombuffer(bytes(side), np.uint8).copy(), spec, state


# ---- the generator-made streams of tests/golden/streams_synth ----------------------------------------------------------------
SYNTH = os.path.join(ROOT, "tests", "golden", "streams_synth")
sys.path.insert(0, os.path.join(ROOT, "tools"))
UNSUPPORTED = -3
_synth_cache = {}


def synth_rows():
    """tools/make_synth_streams.py: synth_set() -- (name, seed, sampling frequency index, frames, level, kind, avoid); kind: 1 mono,
    2 stereo, ADTS channel_configuration 3 / 6"""
    import make_synth_streams
    return make_synth_streams.synth_set()


def synth_path(name):
    return os.path.join(SYNTH, name + ".aac")


def synth_channels(kind):
    return {1: 1, 2: 2, 3: 3, 6: 6}[kind]


def new_states(data):
    """what the noise generators of a new stream start from, one per channel element: xaac_parse_core_tools_state_mc of a
    stage-1 parser behind the first frame"""
    lib = decoder.load_host_library()
    p = ctypes.c_void_p()
    assert lib.xaac_parser_create(ctypes.byref(p)) == 0
    try:
        state = np.zeros(decoder.CORE_TOOLS_STATE_BYTES, np.uint8)
        assert lib.xaac_parse_core_tools_state_mc(p, 0, state.ctypes.data) == -2       # no frame yet
        elems, n, used = (decoder.CoreFrame * decoder.MC_MAX_ELEMENTS)(), ctypes.c_int32(), ctypes.c_size_t()
        rc = lib.xaac_parse_adts_frame_mc(p, data, len(data), 1, elems, decoder.MC_MAX_ELEMENTS, ctypes.byref(n), ctypes.byref(used))
        assert rc == 0, rc
        out = []
        for k in range(n.value):
            assert lib.xaac_parse_core_tools_state_mc(p, k, state.ctypes.data) == 0
            out.append(state.copy())
        return out
    finally:
        lib.xaac_parser_destroy(p)


def element_rows(ids):
    """[(first channel row, channels)] of a frame's channel elements, bitstream order"""
    rows, at = [], 0
    for e in ids:
        rows.append((at, 2 if e == 1 else 1))
        at += rows[-1][1]
    return rows


def twin_walk(before, states):
    """stage-1 frames of decoder.parse_stream_mc through xaac_core_tools_apply_host, every element from its own state ->
    ([frames] int32[channels, 1024], the final states)"""
    states = [s.copy() for s in states]
    out = []
    for s1, _, _, ids, sides in before:
        got = s1.copy()
        for k, (row, n) in enumerate(element_rows(ids)):
            spec = np.zeros((2, 1024), np.int32)
            spec[:n] = s1[row:row + n]
            rc, spec, states[k] = apply_host(spec, np.frombuffer(sides[k], np.uint8), states[k])
            assert rc == 0
            got[row:row + n] = spec[:n]
        out.append(got)
    return out, states


def synth_walk(name, data=None):
    """(stage-1 frames, stage-2 frames) of decoder.parse_stream_mc -- which takes streams of one element too --, once per run"""
    if data is not None:
        return decoder.parse_stream_mc(data, stage=1), decoder.parse_stream_mc(data, stage=2)
    if name not in _synth_cache:
        data = open(synth_path(name), "rb").read()
        _synth_cache[name] = (decoder.parse_stream_mc(data, stage=1), decoder.parse_stream_mc(data, stage=2))
    return _synth_cache[name]


def right_only_bands(side_bytes):
    """the bands of an element where the right channel substitutes noise under a set ms_used bit and the left one does not: their
    noise starts from the seed the band's last correlated left-channel noise left"""
    s = decoder.CoreToolsSide.from_buffer_copy(side_bytes)
    if s.n_ch != 2 or not s.common_window:
        return []
    return [b for b in range(128) if s.pns_correlated[b] and s.ch[1].pns_used[b] and not s.ch[0].pns_used[b]]


def coverage(tools, side_bytes):
    """which of the tools an element of a frame shows, from its XAAC_TOOL_* bits and side info -> set of names"""
    s = decoder.CoreToolsSide.from_buffer_copy(side_bytes)
    got = set()
    for c in range(s.n_ch):
        ch = s.ch[c]
        if not ch.tns_present:
            continue
        short = ch.window_sequence == 2
        orders = [ch.tns[w if short else f].order for w in range(8 if short else 1) for f in range(min(ch.n_filt[w], 1 if short else 3))]
        if any(o > 0 for o in orders):
            got.add("tns_short" if short else "tns_long")
        if any(o >= 8 for o in orders):
            got.add("tns_order8")
    if tools & decoder.TOOL_MS:
        got.add("ms")
    if tools & decoder.TOOL_INTENSITY:
        got.add("intensity")
    if tools & decoder.TOOL_PNS:
        got.add("pns")
        if s.n_ch == 2 and s.common_window and any(s.pns_correlated[b] and (s.ch[0].pns_used[b] or s.ch[1].pns_used[b]) for b in range(128)):
            got.add("pns_corr")
    return got
