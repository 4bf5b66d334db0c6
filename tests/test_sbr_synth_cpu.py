"""The SBR / PS front end on the host (libxaac_amd/host/sbr_side.cpp through decoder.parse_stream) against the reference decoder
on generator-made HE-AAC and HE-AACv2 streams, without a GPU.

tests/golden/streams_synth_sbr is written by tools/make_synth_sbr_streams.py: for every core sampling frequency index at which
xaacdec_amd decodes SBR (6 .. 11: output rates up to 48 kHz) a stereo stream of 24 frames, a mono stream of 12 and a mono stream
with parametric stereo of 24, half of each kind loud, half of each kind with EXT_SBR_DATA_CRC payloads (one CRC wrong); and one
PS stream at a 32 kHz core, which xaacdec_amd refuses (the down-sampled bank).  The reference's encoder writes one or two band
layouts per rate, two patches, no bs_header_extra_2, inverse filtering mode 0 and one PS layout; these streams draw all of it.

For every stream, in both readings (-esbr:0, and xaac_parser_set_esbr for the reference's default flags), what parse_stream hands
out equals what the reference holds at every ixheaacd_sbr_dec call, frame by frame and channel by channel: header tables, frame
data, PS frame, the xaac_esbr_side members and the QMF transposer's parameters after every reset -- against committed CRCs
(tests/golden/sbr_synth_ref.npz, tools/make_golden_sbr_synth.py) and, where oracle/_ref is built, word for word against a fresh
run, with the first differing member named.  The oracle's fixed-point chains (xo_sbr_dec_lp, xo_sbr_dec_hq with PS) walk every call
the reference makes with -esbr:0 on these streams, and its float chain (xo_esbr_sbr_frame_hbe: HF generator, envelope adjuster, QMF
transposer, float PS) every call it makes with its default flags: return code, output and the states behind the call.  A sweep of
further seeds made on the spot is compared the same way.

What the set covers is asserted from the reference's own records (the *_cov rows of the golden file) as far as the records
hold it.  They do not hold the raw fields bs_freq_scale, bs_alter_scale, bs_noise_bands, bs_xover_band, the ICC band count, the PS
enable flags, a PS num_env of 0 or whether a frame had a PS element: those are asserted from the generator's own notes of what it
wrote, not from the reference.  What ties the two is the tests above: on the same frames the parser, which reads those fields,
equals the reference in everything derived from them.

The first pass found one difference: in the default reading a frame with a wrong CRC left the start values of the envelopes coded
along frequency dequantised twice in the reference (it steps over them, env_dec.c:144-148) and once here."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sbr_capture as sc  # noqa: E402
import sbr_synth_cases as cs  # noqa: E402

IDS = [r[0] for r in cs.ROWS]
P16 = ctypes.POINTER(ctypes.c_int16)
_ref, _own = {}, {}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("sbr_synth"))


@pytest.fixture(scope="module")
def gold():
    return np.load(cs.GOLD)


def own(row):
    """the parser's rows of a committed stream, made once"""
    if row[0] not in _own:
        _own[row[0]] = cs.parser_rows(open(cs.path(row[0]), "rb").read(), cs.channels(row[3]))
    return _own[row[0]]


def reference(row, tmp):
    if row[0] not in _ref:
        _ref[row[0]] = cs.reference_rows(cs.path(row[0]), tmp, cs.channels(row[3]))
    return _ref[row[0]]


def test_the_generator_writes_the_committed_streams_byte_for_byte():
    """every file of tests/golden/streams_synth_sbr; nothing else lies there; no file above 64 KB, the directory under 700 KB"""
    sizes = []
    for name, seed, sr, kind, frames, level, _, crc in cs.ROWS:
        data = open(cs.path(name), "rb").read()
        assert cs.gen.make(seed, sr, kind, frames, level, crc) == data, name
        sizes.append(len(data))
    assert sorted(os.listdir(cs.DIR)) == sorted(r[0] + ".aac" for r in cs.ROWS)
    assert max(sizes) <= 64 * 1024 and sum(sizes) < 700 * 1024


def test_the_set_is_what_it_is_meant_to_be():
    m = cs.gen.core
    for kind, frames in (("st", 24), ("mono", 12), ("ps", 24)):
        rows = [r for r in cs.DECODED if r[3] == kind]
        assert sorted(r[2] for r in rows) == cs.gen.DECODED == [6, 7, 8, 9, 10, 11] and all(r[4] == frames for r in rows)
        assert sum(r[5] == m.LOUD for r in rows) == 3 and sum(r[5] == m.QUIET for r in rows) == 3
        assert sum(r[7] for r in rows) == 3
    assert all(2 * cs.gen.RATES[sr] <= 48000 for sr in cs.gen.DECODED) and 2 * cs.gen.RATES[5] > 48000
    assert [(r[2], r[3]) for r in cs.REFUSED] == [(5, "ps")]


@pytest.mark.parametrize("row", cs.ROWS, ids=IDS)
def test_side_info_equals_the_references_committed_crcs_in_both_readings(row, gold):
    name, frames = row[0], row[4]
    plain, esbr, flags = own(row)
    assert len(plain) == len(esbr) == frames
    got, _ = cs.crc_rows(plain, False)
    want = gold[name + "_sbr"]
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert not len(bad), ("-esbr:0: frame, channel, (header | frame | PS frame)", bad[:6].tolist())
    got, hbe = cs.crc_rows(esbr, True)
    bad = np.argwhere(got != gold[name + "_esbr"])
    assert not len(bad), ("default flags: frame, channel, (header | frame | eSBR side | PS frame)", bad[:6].tolist())
    bad = np.argwhere(hbe != gold[name + "_hbe"])
    assert not len(bad), ("transposer parameters: frame, channel, word", bad[:6].tolist())


@pytest.mark.parametrize("row", cs.ROWS, ids=IDS)
def test_side_info_equals_a_fresh_run_of_the_reference_word_for_word(row, tmp):
    if not cs.have_reference():
        pytest.skip("oracle/_ref/xaacdec_capture missing (built where the reference's sources are)")
    plain, esbr, _ = own(row)
    ref_plain, ref_esbr, _ = reference(row, tmp)
    assert cs.first_difference(plain, ref_plain) is None, "-esbr:0: " + cs.first_difference(plain, ref_plain)
    assert cs.first_difference(esbr, ref_esbr) is None, "default flags: " + cs.first_difference(esbr, ref_esbr)


def test_the_comparison_names_the_member_that_differs():
    row = cs.ROWS[0]
    plain = own(row)[0]
    other = [[dict(r) for r in f] for f in plain]
    image = bytearray(other[3][1]["frame"])
    image[sc.Frame.border_vec.offset + 2] ^= 1
    other[3][1]["frame"] = bytes(image)
    said = cs.first_difference(plain, other)
    assert said.startswith("frame 3 channel 1: frame differs in [('border_vec', [1]"), said
    assert cs.first_difference(plain, plain) is None and "frames" in cs.first_difference(plain, plain[:-1])


@pytest.mark.parametrize("row", cs.ROWS, ids=IDS)
def test_the_oracle_walks_every_fixed_point_call_of_the_reference(row, oracle, tmp):
    """xo_sbr_dec_lp / xo_sbr_dec_hq (with PS) on the -esbr:0 capture records: return code, PCM, the state behind the call"""
    if not cs.have_reference():
        pytest.skip("oracle/_ref/xaacdec_capture missing (built where the reference's sources are)")
    recs = reference(row, tmp)[2]
    assert len(recs) == row[4] * cs.channels(row[3])
    seen = set()
    for r in recs:
        st = sc.State.from_buffer_copy(bytes(r["st0"]))
        pin = np.ascontiguousarray(r["pcm_in"])
        if r["low_pow"]:
            out = np.zeros(2048, np.int16)
            rc = oracle.lib.xo_sbr_dec_lp(ctypes.byref(r["header"]), ctypes.byref(r["frame"]), ctypes.byref(st), pin.ctypes.data_as(P16), 1,
                                          out.ctypes.data_as(P16), 1)
            assert rc == r["ret"] and np.array_equal(out, r["pcm_out"][0]), (row[0], r["call"], "low power")
        else:
            out = np.zeros(4096, np.int16)
            ps = sc.PsState.from_buffer_copy(bytes(r["ps0"])) if r["ps"] else None
            rc = oracle.lib.xo_sbr_dec_hq(ctypes.byref(r["header"]), ctypes.byref(r["frame"]), ctypes.byref(st),
                                          ctypes.byref(r["ps_frame"]) if r["ps"] else None, ctypes.byref(ps) if r["ps"] else None,
                                          pin.ctypes.data_as(P16), 1, out.ctypes.data_as(P16), 2 if r["ps"] else 1)
            assert rc == r["ret"], (row[0], r["call"])
            if r["ps"]:
                assert np.array_equal(out[0::2], r["pcm_out"][0]) and np.array_equal(out[1::2], r["pcm_out"][1]), (row[0], r["call"], "PS")
                assert not sc.diff_state(ps, r["ps1"]), (row[0], r["call"], sc.diff_state(ps, r["ps1"])[:3])
            else:
                assert np.array_equal(out[:2048], r["pcm_out"][0]), (row[0], r["call"], "HQ")
        assert not sc.diff_state(st, r["st1"]), (row[0], r["call"], sc.diff_state(st, r["st1"])[:3])
        seen.add((r["low_pow"], r["ps"]))
    assert seen == ({(1, 0)} if row[3] == "st" else {(0, 1)} if row[3] == "ps" else {(0, 0)}), seen


@pytest.mark.parametrize("row", cs.ROWS, ids=IDS)
def test_the_oracle_walks_every_float_call_of_the_reference(row, oracle, tmp):
    """the reference's default flags: xo_esbr_sbr_frame_hbe (HF generator, envelope adjuster, QMF transposer, float PS, the banks)
    over every call of ixheaacd_sbr_dec's eSBR branch on the stream's own core samples, its own states carried along a chain (a
    chain ends where the decoder's outer layers touch the state: a reset) -- return code, every output word of the left channel, the
    right channel's CRC, and the eSBR, transposer and PS states behind the call, the first differing member named"""
    if not cs.have_reference():
        pytest.skip("oracle/_ref/xaacdec_capture missing (built where the reference's sources are)")
    from esbr_structs import EsbrPsState, EsbrState
    PF = ctypes.POINTER(ctypes.c_float)
    fn = oracle.lib.xo_esbr_sbr_frame_hbe
    fn.restype = ctypes.c_int
    fn.argtypes = [PF] + [ctypes.c_void_p] * 6 + [PF, PF, ctypes.c_void_p]
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    recs = cs.esbr_chain_records(cs.path(row[0]), tmp)
    n_ch = cs.channels(row[3])
    assert len(recs) == (row[4] + 1) * n_ch                   # every call takes the branch (frame 0 is decoded twice)
    with_ps = sum(r["eps"] for r in recs)      # (the calls in front of a PS stream's first decoded payload have none)
    assert with_ps >= row[4] - 2 if row[3] == "ps" else with_ps == 0, with_ps
    live, applied = {}, 0
    for k, r in enumerate(recs):
        if r["step"] == 0:
            live[r["chain"]] = [r["est0"].copy(), r["hbs0"].copy(), r["eps0"].copy() if r["eps"] else None]
        st, hb, ps = live[r["chain"]]
        eps = bool(r["eps"])
        out, out_r = np.zeros(2048, np.float32), np.zeros(2048, np.float32)
        core = np.ascontiguousarray(r["core"])
        rc = fn(core.ctypes.data_as(PF), vp(r["header"]), vp(r["frame"]), vp(r["side"]), vp(st), vp(r["ps_frame"]) if eps else None,
                vp(ps) if eps else None, out.ctypes.data_as(PF), out_r.ctypes.data_as(PF) if eps else None, vp(hb))
        where = (row[0], "call", k, "chain", r["chain"], "step", r["step"])
        assert rc == r["ret"] == 0, where
        bad = np.nonzero(out.view(np.uint32) != r["out"].view(np.uint32))[0]
        assert not len(bad), (where, "left output", bad[:6].tolist())
        if eps and r["apply"]:
            assert cs.crc(out_r) == r["crc"][1], (where, "right output")
        got = cs.esbr_state_as_read(st, r["header"], r["frame"], r["apply"], r["hbs1"])
        want = cs.esbr_state_as_read(r["est1"], r["header"], r["frame"], r["apply"], r["hbs1"])
        assert got == want, (where, "eSBR state", cs.diff_struct(EsbrState, got, want)[:3])
        assert hb.tobytes() == r["hbs1"].tobytes(), (where, "transposer state", cs.diff_struct(cs.HbeState, hb.tobytes(), r["hbs1"].tobytes())[:3])
        if eps:
            assert ps.tobytes() == r["eps1"].tobytes(), (where, "PS state", cs.diff_struct(EsbrPsState, ps.tobytes(), r["eps1"].tobytes())[:3])
        applied += r["apply"]
    assert applied >= (row[4] - 1) * n_ch and len(live) >= 2 * n_ch      # the payload runs one frame late; a chain per reset at least


def test_coverage(gold):
    """what the committed set says: from the reference's records (COV rows) where they hold it; the raw header fields and PS
    modes and flags they do not hold from the generator's notes of what it wrote (see the module's docstring)"""
    col = {k: i for i, k in enumerate(cs.COV)}
    rows = np.concatenate([gold[r[0] + "_cov"].reshape(-1, len(cs.COV)) for r in cs.DECODED])

    def seen(key, only=None):
        return set((rows if only is None else rows[only])[:, col[key]].tolist())
    for key, want in (("limiter_bands", {0, 1, 2, 3}), ("limiter_gains", {0, 1, 2, 3}), ("interpol_freq", {0, 1}), ("smoothing_mode", {0, 1}),
                      ("amp_res", {0, 1}), ("frame_class", {0, 1, 2, 3}), ("harmonics", {0, 1}), ("coupling_mode", {0, 1, 2})):
        assert seen(key) - {-1} == want, (key, seen(key))
    layouts = set(map(tuple, rows[:, [col[k] for k in ("sub_band_start", "sub_band_end", "num_lo", "num_hi", "num_nf")]].tolist()))
    assert len(layouts) >= 20, len(layouts)
    assert seen("num_patches") >= {1, 2, 3, 4}, seen("num_patches")
    assert seen("num_nf") >= {1, 2, 3, 4}
    modes = 0
    for v in seen("invf_modes"):
        modes |= v
    assert modes == 15                                           # each inverse filtering mode 0 .. 3
    # every envelope count the grids of 4.6.18.3.3 allow: FIXFIX 1 2 4, FIXVAR / VARFIX 1 .. 4, VARVAR 1 .. 5
    grids = set(map(tuple, rows[:, [col["frame_class"], col["num_env"]]].tolist()))
    assert grids >= {(0, 1), (0, 2), (0, 4)} | {(c, n) for c in (1, 2) for n in (1, 2, 3, 4)} | {(3, n) for n in (1, 2, 3, 4, 5)}, grids
    ps = rows[:, col["ps"]] == 1
    assert seen("ps_iid_quant", ps) == {0, 1} and seen("ps_iid_res", ps) == {0, 1, 2} and seen("ps_num_env", ps) >= {1, 2, 3, 4, 5}
    assert seen("ps_borders_explicit", ps) == {0, 1}
    notes_seen = dict(freq_scale=set(), alter_scale=set(), noise_bands=set(), xover=set(), icc_bands=set(), iid_mode=set(), icc_mode=set(),
                      iid_off=0, icc_off=0, ext=0, ps_env0=0, no_ps=0, ps_class=set())
    for row in cs.DECODED:
        name, seed, sr, kind, frames, level, _, crc = row
        cov = gold[name + "_cov"]
        applied = cov[:, 0, col["apply_processing"]]
        assert applied.sum() * 4 >= 3 * frames, (name, int(applied.sum()))   # the condition: three quarters of the frames, at least
        _, notes = cs.gen.make_with_notes(seed, sr, kind, frames, level, crc)
        _, _, flags = own(row)
        headers = [n["frame"] for n in notes if n["header"]]
        resets = [n["frame"] for n in notes if n.get("reset")]
        # a header in frame 0 and three more: one unchanged, one changed in bs_header_extra_2 alone, one that resets
        assert len(headers) == 4 and headers[0] == 0 and len(resets) == 2 and resets[0] == 0, (name, headers, resets)
        assert [f for f in range(frames) if flags[f][1]] == resets, name                       # the parser resets there and only there
        late = cov[:, 0, col["reset_flag"]]                                                 # the default reading's record of frame f + 1
        assert all(late[f] == 1 for f in resets if f + 1 < frames) and all(late[f] == 0 for f in headers if f not in resets and f + 1 < frames), name
        bad = [n["frame"] for n in notes if n.get("bad_crc")]
        assert len(bad) == (1 if crc else 0) and [f for f in range(frames) if not flags[f][2]] == bad, (name, bad)
        if kind == "st":
            c = cov[:, 0, col["coupling_mode"]]
            on = [int(v != 0) for v in c]
            assert (0, 1) in zip(on, on[1:]) and (1, 0) in zip(on, on[1:]), (name, on)          # a switch in both directions
        for n in notes:
            if n.get("header_fields"):
                h = n["header_fields"]
                notes_seen["freq_scale"].add(h["freq_scale"]), notes_seen["alter_scale"].add(h["alter_scale"])
                notes_seen["noise_bands"].add(h["noise_bands"]), notes_seen["xover"].add(h["xover_band"])
            if kind == "ps":
                if "ps" not in n:
                    notes_seen["no_ps"] += 1
                    continue
                p = n["ps"]
                notes_seen["ps_class"].add(p["cls"])
                notes_seen["ps_env0"] += p["n_env"] == 0
                notes_seen["iid_off"] += not p["enable_iid"]
                notes_seen["icc_off"] += not p["enable_icc"]
                notes_seen["ext"] += p["enable_ext"]
                if p["enable_iid"]:
                    notes_seen["iid_mode"].add(p["iid_mode"])
                if p["enable_icc"]:
                    notes_seen["icc_mode"].add(p["icc_mode"])
    assert notes_seen["freq_scale"] == {0, 1, 2, 3} and notes_seen["alter_scale"] == {0, 1} and notes_seen["noise_bands"] == {0, 1, 2, 3}
    assert notes_seen["xover"] - {0}
    assert notes_seen["iid_mode"] == set(range(6)) and notes_seen["icc_mode"] == set(range(6)) and notes_seen["ps_class"] == {0, 1}
    assert min(notes_seen[k] for k in ("iid_off", "icc_off", "ext", "ps_env0", "no_ps")) >= 1, notes_seen
    for kind in ("st", "mono", "ps"):   # a concealed frame and a wrong CRC per kind
        assert any(r[7] for r in cs.DECODED if r[3] == kind)


def test_a_seed_sweep_made_on_the_spot_equals_the_reference(tmp):
    """further seeds, never committed: eight of each kind at every index, both readings, 12 frames (144 streams, some ten seconds)"""
    if not cs.have_reference():
        pytest.skip("oracle/_ref/xaacdec_capture missing (built where the reference's sources are)")
    bad = []
    for j, (sr, n) in enumerate((sr, n) for n in range(8) for sr in (6, 8, 11, 7, 9, 10)):
        for k, kind in enumerate(("st", "mono", "ps")):
            seed = 7000 + 100 * n + 10 * sr + k
            data = cs.gen.make(seed, sr, kind, 12, cs.gen.core.LOUD if (j + k) & 1 else cs.gen.core.QUIET, bool(j & 1))
            src = os.path.join(tmp, "sweep.aac")
            open(src, "wb").write(data)
            n_ch = cs.channels(kind)
            ref_plain, ref_esbr, _ = cs.reference_rows(src, tmp, n_ch)
            plain, esbr, _ = cs.parser_rows(data, n_ch)
            for what, got, want in (("-esbr:0", plain, ref_plain), ("default flags", esbr, ref_esbr)):
                said = cs.first_difference(got, want)
                if said or len(want) != 12:
                    bad.append((sr, kind, seed, what, said))
    assert not bad, bad
