"""Shared by tests/test_sbr_synth_cpu.py, tests/test_sbr_synth_gpu.py and tools/make_golden_sbr_synth.py: the generator-made
HE-AAC / HE-AACv2 streams of tests/golden/streams_synth_sbr (tools/make_synth_sbr_streams.py), what the reference decoder holds
while it decodes one of them, what this project's host front end makes of the same bytes, and the comparison of the two that
names the first differing field.  Test infrastructure."""
import ctypes
import os
import subprocess
import sys
import wave
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_parser as mg  # noqa: E402
import make_synth_sbr_streams as gen  # noqa: E402
import sbr_capture as sc  # noqa: E402
from esbr_structs import EsbrSide  # noqa: E402
from hbe_structs import HbeState  # noqa: E402
from libxaac_amd import decoder  # noqa: E402

DIR = gen.OUT
REF = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(ROOT, "tests", "golden", "sbr_synth_ref.npz")
ROWS = gen.synth_set()
DECODED = [r for r in ROWS if r[6]]
REFUSED = [r for r in ROWS if not r[6]]
FLAG_SETS = (("-esbr:0",), ())          # the fixed-point tools, and the reference's default reading
KINDS = (("header", sc.Header), ("frame", sc.Frame), ("ps_frame", sc.PsFrame), ("esbr_side", EsbrSide))
# one row of a stream's *_cov array (per frame and channel, from the reference's records with -esbr:0; limiter_bands and
# reset_flag from the records of the default reading, which run one frame late)
COV = ("frame_class", "num_env", "amp_res", "coupling_mode", "apply_processing", "invf_modes", "harmonics", "sub_band_start",
       "sub_band_end", "num_lo", "num_hi", "num_nf", "num_patches", "limiter_gains", "interpol_freq", "smoothing_mode", "num_lim",
       "limiter_bands", "reset_flag", "ps", "ps_iid_quant", "ps_iid_res", "ps_num_env", "ps_borders_explicit")


def crc(b):
    return zlib.crc32(bytes(b)) & 0xffffffff


def path(name):
    return os.path.join(DIR, name + ".aac")


def channels(kind):
    return 2 if kind == "st" else 1


def have_reference(binary="xaacdec_capture"):
    return os.path.exists(os.path.join(REF, binary))


def hbe_params(st):
    return [st.synth_size, st.k_start, st.start_band, st.end_band] + list(st.x_over_qmf) + [st.max_stretch]


# ---- what the reference holds ---------------------------------------------------------------------------------------------------
def reference_rows(src, tmp, n_ch):
    """-> (rows of -esbr:0, rows of the default reading, the -esbr:0 capture records): rows[f][c] = dict(header, frame, ps_frame or
    None, and in the default reading esbr_side and hbe).  The initialisation pass over frame 0 is dropped."""
    _, recs = mg.capture(src, tmp)
    recs = recs[n_ch:]
    assert len(recs) % n_ch == 0
    plain = [[dict(header=bytes(r["header"]), frame=bytes(r["frame"]), ps_frame=bytes(r["ps_frame"]) if r["ps"] else None)
              for r in recs[f * n_ch:(f + 1) * n_ch]] for f in range(len(recs) // n_ch)]
    er = mg.capture_esbr(src, tmp)[n_ch:]
    assert len(er) % n_ch == 0
    esbr = [[dict(header=h, frame=fr, esbr_side=e, ps_frame=p if meta[2] else None, hbe=[int(v) for v in par])
             for meta, h, fr, e, p, par in er[f * n_ch:(f + 1) * n_ch]] for f in range(len(er) // n_ch)]
    return plain, esbr, recs


# ---- what this project's front end makes of the bytes -----------------------------------------------------------------------------
def parser_rows(data, n_ch):
    """the same two lists from decoder.parse_stream, plus per frame the parser's flags (apply, reset, frame_ok) of -esbr:0"""
    lib = decoder.load_host_library()
    plain, flags = [], []
    for _, _, _, side in decoder.parse_stream(data, stage=2):
        plain.append([dict(header=bytes(side.header), frame=bytes(side.frame[c]), ps_frame=bytes(side.ps_frame) if side.ps else None)
                      for c in range(n_ch)])
        flags.append((int(side.apply), int(side.reset), int(side.frame_ok)))
    esbr = []
    hbe = [HbeState(), HbeState()]
    for st in hbe:
        lib.xaac_hbe_state_init(ctypes.byref(st))
    for _, _, _, side, eside in decoder.parse_stream(data, esbr=True):
        if side.reset:   # ixheaacd_sbr_dec_reset: the transposer's parameters follow the new band tables
            for c in range(side.reset_channels):
                assert lib.xaac_hbe_state_reinit(ctypes.byref(hbe[c]), ctypes.byref(side, decoder.SbrSide.header.offset)) == 0
        esbr.append([dict(header=bytes(side.header), frame=bytes(side.frame[c]), esbr_side=bytes(eside[c]),
                          ps_frame=bytes(side.ps_frame) if side.ps else None, hbe=hbe_params(hbe[c])) for c in range(n_ch)])
    return plain, esbr, flags


def crc_rows(rows, esbr):
    """rows -> uint32 [frames, channels, 3 or 4] (0 for a PS frame that is not there), and the transposer parameters"""
    keys = ("header", "frame", "esbr_side", "ps_frame") if esbr else ("header", "frame", "ps_frame")
    out = np.zeros((len(rows), len(rows[0]), len(keys)), np.uint32)
    for f, row in enumerate(rows):
        for c, r in enumerate(row):
            out[f, c] = [crc(r[k]) if r[k] is not None else 0 for k in keys]
    hbe = np.array([[r["hbe"] for r in row] for row in rows], np.int32) if esbr else None
    return out, hbe


def diff_struct(cls, a, b):
    """the members of a struct of type cls in which the images a and b differ: [(member, first indices, got, want)]"""
    out = []
    for name, _ in cls._fields_:
        d = getattr(cls, name)
        xa, xb = a[d.offset:d.offset + d.size], b[d.offset:d.offset + d.size]
        if xa != xb:
            width = 4 if d.size % 4 == 0 and name.startswith(("flt_", "sbr_invf", "coupling", "max_qmf", "out_samp", "pitch", "inter_")) else 2 \
                if d.size % 2 == 0 else 1
            va, vb = (np.frombuffer(x, {4: np.int32, 2: np.int16, 1: np.uint8}[width]) for x in (xa, xb))
            at = np.nonzero(va != vb)[0][:6]
            out.append((name, at.tolist(), va[at].tolist(), vb[at].tolist()))
    return out


def first_difference(got, want):
    """None, or a sentence that names the first frame, channel, struct and members in which two row lists differ"""
    if len(got) != len(want):
        return "%d frames against the reference's %d" % (len(got), len(want))
    for f, (gr, wr) in enumerate(zip(got, want)):
        for c, (g, w) in enumerate(zip(gr, wr)):
            for key, cls in KINDS:
                if key not in w:
                    continue
                if (g[key] is None) != (w[key] is None):
                    return "frame %d channel %d: %s %s here, %s in the reference" % (
                        f, c, key, "missing" if g[key] is None else "present", "missing" if w[key] is None else "present")
                if g[key] is not None and g[key] != w[key]:
                    return "frame %d channel %d: %s differs in %s" % (f, c, key, diff_struct(cls, g[key], w[key])[:4])
            if "hbe" in w and g["hbe"] != w["hbe"]:
                return "frame %d channel %d: transposer parameters %s against %s" % (f, c, g["hbe"], w["hbe"])
    return None


# ---- the default flags' ixheaacd_sbr_dec calls (the float chain), for the oracle's walk ---------------------------------------------
def esbr_chain_records(src, tmp):
    """every call of the reference's eSBR branch while it decodes `src` with its default flags, through oracle/ref_capture.c's
    chain records ($XAAC_ESBR_CHAIN_FILE with _FULL: the states in front of and behind every call and the left output; _CORE_FILE:
    the stream's own core samples stay and are written out): dicts of chain, step, eps, apply, est0 / hbs0 / eps0, header, frame,
    side, ps_frame, ret, crc (out, out_r, ...), est1 / hbs1 / eps1, out, core"""
    import struct
    import make_golden_esbr_chains as gc
    z = gc.sizes()
    chain, core = os.path.join(tmp, "esbr_chain.bin"), os.path.join(tmp, "esbr_core.bin")
    for f in (chain, core):
        if os.path.exists(f):
            os.remove(f)
    subprocess.run([os.path.join(REF, "xaacdec_capture"), "-ifile:" + src, "-ofile:" + os.path.join(tmp, "o.wav")], check=True, capture_output=True,
                   env=dict(os.environ, XAAC_ESBR_CHAIN_FILE=chain, XAAC_ESBR_CHAIN_CORE_FILE=core, XAAC_ESBR_CHAIN_FULL="1"), timeout=120)
    b, cores = open(chain, "rb").read(), np.fromfile(core, np.float32).reshape(-1, 1024)
    o, recs = 0, []

    def take(n):
        nonlocal o
        o += n
        return np.frombuffer(b[o - n:o], np.uint8).copy()
    while o < len(b):
        magic, c, step, eps, first, apply = struct.unpack_from("<6i", b, o)
        assert magic == 0x58414332 and first == 1 and eps >> 8 == 0, (hex(magic), first, eps)      # (the 2:1 ratio)
        o += 24
        r = dict(chain=c, step=step, eps=eps & 1, apply=apply, est0=take(z["est"]), hbs0=take(z["hbs"]))
        r["eps0"] = take(z["eps"]) if r["eps"] else None
        r.update(header=take(z["hd"]), frame=take(z["fr"]), side=take(z["sd"]), ps_frame=take(z["psf"]))
        r["ret"], *r["crc"] = struct.unpack_from("<i5I", b, o)
        o += 24
        r.update(est1=take(z["est"]), hbs1=take(z["hbs"]))
        r["eps1"] = take(z["eps"]) if r["eps"] else None
        r["out"] = take(4 * 2048).view(np.float32)
        r["core"] = cores[len(recs)]
        recs.append(r)
    assert len(recs) == len(cores)
    return recs


def esbr_state_as_read(st, header, frame, apply, hbs):
    """an xaac_esbr_state image without the words no later call reads before they are written again: of the sbr_qmf_out history the
    rows from the frame's last border on and the bands below the cross-over (oracle/ref_capture.c masks the same for its CRC,
    tests/test_esbr_chains.py: state_crc), and of the transposer's ph rows the bands outside its range start_band .. end_band - 1
    -- the reference's buffer keeps there what a wider range left before a reset narrowed it, a frame-by-frame restatement has
    zeros; every frame and every reset writes all the bands of the range in force (hbe_trans.c), and nothing else is read"""
    from esbr_structs import EsbrState
    h, f, hb = sc.Header.from_buffer_copy(header.tobytes()), sc.Frame.from_buffer_copy(frame.tobytes()), HbeState.from_buffer_copy(hbs.tobytes())
    keep = 2 + 2 * f.border_vec[f.num_env] - 32 if apply else 8
    b = np.array(st, copy=True)
    for name in ("out_re", "out_im", "ph_re", "ph_im"):
        fld = getattr(EsbrState, name)
        m = b[fld.offset:fld.offset + fld.size].view(np.float32).reshape(8, 64)
        if name.startswith("out"):
            m[max(keep, 0):, :] = 0
            m[:, :h.sub_band_start] = 0
        else:
            m[:, :max(hb.start_band, 0)] = 0
            m[:, max(hb.end_band, 0):] = 0
    return b.tobytes()


# ---- coverage rows: what the reference's records say about a stream ---------------------------------------------------------------
def coverage_rows(plain, esbr):
    """-> int32 [frames, channels, len(COV)]"""
    out = np.zeros((len(plain), len(plain[0]), len(COV)), np.int32)
    for f, row in enumerate(plain):
        for c, r in enumerate(row):
            h, fr = sc.Header.from_buffer_copy(r["header"]), sc.Frame.from_buffer_copy(r["frame"])
            # the default reading decodes a payload one frame late: frame f's payload is its frame f + 1
            e = EsbrSide.from_buffer_copy(esbr[f + 1][c]["esbr_side"]) if f + 1 < len(esbr) else None
            modes = 0
            for k in range(h.num_nf_bands):
                modes |= 1 << fr.sbr_invf_mode[k]
            ps = [0, 0, 0, 0, 0]
            if r["ps_frame"] is not None:
                p = sc.PsFrame.from_buffer_copy(r["ps_frame"])
                even = [(32 * k) // max(p.num_env, 1) for k in range(p.num_env + 1)]
                ps = [1, p.iid_quant, p.freq_res_ipd, p.num_env, int(list(p.border_position[:p.num_env + 1]) != even)]
            out[f, c] = [fr.frame_class, fr.num_env, fr.amp_res, fr.coupling_mode, fr.apply_processing, modes, int(any(fr.add_harmonics)),
                         h.sub_band_start, h.sub_band_end, h.num_sf_bands[0], h.num_sf_bands[1], h.num_nf_bands, h.num_patches,
                         h.limiter_gains, h.interpol_freq, h.smoothing_mode, h.num_lf_bands, e.limiter_bands if e else -1,
                         e.reset_flag if e else -1] + ps
    return out


# ---- the reference's PCM ----------------------------------------------------------------------------------------------------------
_wav_cache = {}


def reference_wav(src, flags, tmp):
    """the bytes of the file `oracle/_ref/xaacdec` writes for a stream and a flag set, made once"""
    key = (src, tuple(flags))
    if key not in _wav_cache:
        out = os.path.join(tmp, "ref_%d.wav" % len(_wav_cache))
        subprocess.run([os.path.join(REF, "xaacdec"), "-ifile:" + src, "-ofile:" + out, *flags], check=True, capture_output=True, timeout=120)
        _wav_cache[key] = open(out, "rb").read()
    return _wav_cache[key]


def core_only(row):
    """the stream's AAC-LC frames without their SBR fill elements (the core generator draws on its own)"""
    import make_synth_streams as m
    name, seed, sr, kind, frames, level = row[:6]
    return m.make(seed, sr, frames, level, channels(kind), busy=True)


def wav_facts(blob):
    """-> (channels, rate, samples per channel, PCM bytes) of a WAV image"""
    import io
    with wave.open(io.BytesIO(blob)) as w:
        return w.getnchannels(), w.getframerate(), w.getnframes(), w.readframes(w.getnframes())


def checked_reference_wav(row, flags, tmp):
    """the reference's file for a committed stream, after the check every comparison makes first: stereo at twice the core's rate,
    2048 samples for every frame (but for the one the default flags cut: they decode a payload one frame late), where its decode of the core frames alone
    (which has every frame) has 1024, and not those samples"""
    name, _, sr, kind, frames = row[:5]
    blob = reference_wav(path(name), flags, tmp)
    core_path = os.path.join(tmp, name + "_core.aac")
    if not os.path.exists(core_path):
        open(core_path, "wb").write(core_only(row))
    core = wav_facts(reference_wav(core_path, flags, tmp))
    ch, rate, samples, pcm = wav_facts(blob)
    assert (ch, rate) == (2, 2 * gen.RATES[sr]) and core[1] == gen.RATES[sr], (name, ch, rate)
    cut = 0 if "-esbr:0" in flags else 1      # the default path decodes a payload one frame late and cuts that frame
    assert core[2] == 1024 * frames and samples == 2048 * (frames - cut), (name, flags, samples, core[2])
    assert pcm != core[3] and any(pcm), name
    return blob
