"""MPEG-4 dynamic range control on the CPU: the side rows the host parser makes of a frame's dynamic_range_info
(xaac_parse_drc_config / xaac_parse_drc_side: the bit syntax, ixheaacd_drc_map_channels and the gain factors of
libxaac_amd/csrc/drc.h) and the host twin of the GPU kernel (xaac_drc_apply_host) turn the reference's unflagged spectra into the
reference's own flagged spectra, word for word, on every record of tests/golden/drc_spec.npz (oracle/_ref/xaacdec_capture, type-2
XAAC_SPEC_DUMP records: the lines ixheaacd_imdct_process receives, i.e. behind ixheaacd_drc_apply); the twin against a numpy int64
model on made-up rows; the refusals; the doubly covered channel; the committed tables against the reference's image.  CPU only."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import drc_cases as dc
from libxaac_amd import decoder

PLAIN = os.path.join(dc.ROOT, "tests", "golden", "streams")


@pytest.mark.parametrize("k", range(len(dc.FLAG_SETS)), ids=["cut1_boost1", "cut.5_boost.25_t96", "t96", "t124"])
@pytest.mark.parametrize("name", dc.NAMES)
def test_parser_rows_and_host_twin_equal_the_reference_records(name, k):
    g = dc.gold()
    want_in, want_out = g[name + "_in"], g["%s_out%d" % (name, k)]
    assert want_in.shape == want_out.shape and len(want_in) >= 6 and not np.array_equal(want_in, want_out)
    p = decoder.StreamParser(dc.stream(name), drc=dc.DRC_ARGS[k])
    active = 0
    for f in range(len(want_in)):
        assert p.next()
        n_ch = p.core.n_ch
        spec = np.ctypeslib.as_array(p.core.spec)[:n_ch].copy()
        assert np.array_equal(spec, want_in[f]), (f, "the parser's spectra with DRC configured are the unflagged reference's")
        side = p.drc_side()
        for c in range(n_ch):
            assert decoder.drc_apply_host(side[c], spec[c]) == 0
            assert np.array_equal(spec[c], dc.model(side[c], want_in[f][c])), (f, c, "twin against the model")
            active += int(np.any(side[c][17:17 + side[c][0]] != dc.ONE))
        assert np.array_equal(spec, want_out[f]), (f, "frame differs from the reference's record")
    assert active >= len(want_in)
    p.close()


def test_streams_hold_what_they_are_for():
    """the generator's cases as the parser sees them: band counts, ends that do not rise, a channel that keeps its rows over frames
    without an element, rows that differ between the channels of a pair, short windows beside sixteen bands"""
    cfg = dict(cut=1, boost=1)
    rows = {}
    for name in dc.NAMES:
        p = decoder.StreamParser(dc.stream(name), drc=cfg)
        rows[name] = []
        while p.next():
            rows[name].append((p.drc_side(), [p.core.ics[c][0] for c in range(p.core.n_ch)]))
        assert len(rows[name]) == 24
    assert all(s[0][0] == 1 and s[0][1] == 1024 for s, _ in rows["drc_mono_1band"])
    assert all(list(s[c][:3]) == [2, 256, 1024] for s, _ in rows["drc_stereo_2band"] for c in range(2))
    assert all(s[0][0] == 16 for s, _ in rows["drc_stereo_16band"]) and any(w[0] == 2 for _, w in rows["drc_stereo_16band"])
    assert any(s[0][16] < 1024 for s, _ in rows["drc_stereo_16band"])   # a last end below 1024: the tail untouched
    ex = rows["drc_stereo_excl"]
    assert any(not np.array_equal(s[0], s[1]) for s, _ in ex)
    assert np.array_equal(ex[2][0], ex[1][0]) and np.array_equal(ex[3][0], ex[1][0])   # frames 2, 3: no element
    nm = rows["drc_stereo_nonmono"]
    assert sum(any(s[0][1 + b] < s[0][b] for b in range(1, s[0][0])) for s, _ in nm) >= 8


def test_without_the_config_call_nothing_is_read():
    p = decoder.StreamParser(dc.stream("drc_stereo_2band"))
    assert p.next()
    with pytest.raises(decoder.ParseError):
        p.drc_side()
    want = dc.gold()["drc_stereo_2band_in"]
    assert np.array_equal(np.ctypeslib.as_array(p.core.spec)[:2], want[0])


def test_a_stream_without_elements_gets_identity_rows():
    """-drc_target_level alone on a stream without dynamic_range_info changes nothing: prog_ref_level starts as the target"""
    p = decoder.StreamParser(open(os.path.join(PLAIN, "synth_lc_a.aac"), "rb").read(), drc=dict(target_level=96))
    for _ in range(6):
        assert p.next()
        side = p.drc_side()
        assert all(list(side[c][:2]) == [1, 1024] and side[c][17] == dc.ONE for c in range(2))


@pytest.mark.parametrize("n", [13, 200])
def test_host_twin_equals_the_model(n):
    refused = 0
    for what, row, spec in dc.rows(n):
        got = spec.copy()
        rc = decoder.drc_apply_host(row, got)
        assert rc == (0 if dc.row_ok(row) else -1), what
        assert np.array_equal(got, dc.model(row, spec)), what
        refused += rc != 0
        if what == "identity" or rc:
            assert np.array_equal(got, spec), what
    assert refused == 3


def test_the_model_does_what_its_cases_say():
    """the fixed rows reach what they name: saturation at both ends, the floor of negative lines, lines multiplied twice"""
    cases = {what: (row, spec) for what, row, spec in dc.fixed_rows()}
    row, spec = cases["saturating factors"]
    out = dc.model(row, spec)
    assert out[0] == 0x7fffffff and out[1] == -0x80000000 and out[4] == 0x7fffffff and out[5] == -0x80000000
    row, spec = cases["negative lines"]
    out = dc.model(row, spec)
    assert np.all(out == spec) and np.all(spec < 0)   # (x * (2^25 - 1)) >> 25 of a small negative x is x: floor; toward zero it were x + 1
    row, spec = cases["non-monotonic ends"]
    once = dc.model(dc.side_row([512], [row[17]]), spec)
    assert not np.array_equal(dc.model(row, spec)[128:512], once[128:512])
    row, spec = cases["a last end below 1024"]
    assert np.array_equal(dc.model(row, spec)[700:], spec[700:])


def test_two_elements_on_one_channel_end_the_stream():
    """IA_XHEAAC_DEC_EXE_FATAL_INVALID_DRC_DATA: the frame does not parse; in a batch only that stream ends"""
    good = dc.stream("drc_stereo_2band")
    bad = dc.with_two_elements_on_one_channel(good, 5)
    p = decoder.StreamParser(bad, drc=dict(cut=1))
    for _ in range(5):
        assert p.next()
    with pytest.raises(decoder.ParseError) as e:
        p.next()
    assert e.value.code == -2 and e.value.frame == 5
    q = decoder.StreamParser(bad)   # without DRC the elements are not looked at
    for _ in range(24):
        assert q.next()
    bp = decoder.BatchParser([good, bad, good], drc=decoder.drc_config(dict(cut=1)))
    spec, ics = np.zeros((6, 1024), np.int32), np.zeros((6, 2), np.uint8)
    side = np.zeros((6, dc.WORDS), np.int32)
    try:
        for f in range(5):
            assert bp.step(spec, ics, drc_side=side).all()
            assert np.array_equal(side[0:2], side[2:4]) and np.array_equal(side[0:2], side[4:6]) and side[0][0] == 2
        with pytest.raises(decoder.ParseError):
            bp.step(spec, ics, drc_side=side)
        assert list(bp.status) == [0, -2, 0]
    finally:
        bp.close()


def test_batch_rows_are_identity_without_the_config_call():
    bp = decoder.BatchParser([dc.stream("drc_stereo_2band")])
    spec, ics, side = np.zeros((2, 1024), np.int32), np.zeros((2, 2), np.uint8), np.full((2, dc.WORDS), -1, np.int32)
    try:
        assert bp.step(spec, ics, drc_side=side).all()
        assert all(list(side[c][:2]) == [1, 1024] and side[c][17] == dc.ONE for c in range(2))
    finally:
        bp.close()


def _cli(*args):
    assert os.path.exists(dc.CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
    return subprocess.run([dc.CLI, *args], capture_output=True, text=True, timeout=120)


def test_plan_shows_the_config_the_reference_keeps():
    src = "-ifile:" + os.path.join(dc.STREAMS, "drc_stereo_2band.aac")
    assert "drc" not in json.loads(_cli(src, "-plan").stdout)
    assert json.loads(_cli(src, "-plan", "-drc_target_level:96").stdout)["drc"] == {"cut": 100, "boost": 100, "target_level": 96}
    got = json.loads(_cli(src, "-plan", "-drc_cut_fac:0.5", "-drc_boost_fac:0.25").stdout)["drc"]
    assert got == {"cut": 50, "boost": 25, "target_level": 108}
    for cut, boost in ((0.29, 0.57), (0.07, 0.999), (0.013, 0.58)):   # (WORD32)(float * 100), the same on both sides
        got = json.loads(_cli(src, "-plan", "-drc_cut_fac:%s" % cut, "-drc_boost_fac:%s" % boost).stdout)["drc"]
        cfg = decoder.drc_config(dict(cut=cut, boost=boost))
        assert (cfg.cut, cfg.boost, cfg.target_level) == (got["cut"], got["boost"], 108)
        assert cfg.cut == int(np.float32(cut) * np.float32(100)) and cfg.boost in (int(boost * 100), int(boost * 100) + 1)


@pytest.mark.parametrize("src, flags, message", [
    ("streams/mix_aot5_48k", ("-drc_cut_fac:1",), "a -drc_* flag on a stream with SBR"),
    ("streams/mix_aot29_32k", ("-drc_target_level:96",), "a -drc_* flag on a stream with SBR"),
    ("streams_drc/drc_stereo_2band", ("-drc_heavy_comp:1",), "-drc_heavy_comp:1"),
    ("streams_drc/drc_stereo_2band", ("-drc_cut_fac:1.5",), "-drc_cut_fac takes 0 .. 1"),
    ("streams_drc/drc_stereo_2band", ("-drc_boost_fac:-0.1",), "-drc_boost_fac takes 0 .. 1"),
    ("streams_drc/drc_stereo_2band", ("-drc_target_level:128",), "-drc_target_level takes 0 .. 127"),
])
@pytest.mark.parametrize("plan", [True, False], ids=["plan", "decode"])
def test_refusals_have_their_own_message_and_leave_no_file(tmp_path, src, flags, message, plan):
    """refused before a device is looked at (this test runs where there is none) or a file written"""
    out = str(tmp_path / "o.wav")
    p = _cli("-ifile:" + os.path.join(dc.ROOT, "tests", "golden", src + ".aac"), "-ofile:" + out, *flags, *(["-plan"] if plan else []))
    assert p.returncode == 2 and message in p.stderr and not os.path.exists(out)


def test_a_list_with_an_sbr_stream_is_refused_with_that_file(tmp_path):
    lst = tmp_path / "list.txt"
    sbr = os.path.join(PLAIN, "mix_aot5_48k.aac")
    lst.write_text(os.path.join(dc.STREAMS, "drc_stereo_2band.aac") + "\n" + sbr + "\n")
    out = tmp_path / "out"
    out.mkdir()
    p = _cli("-ilist:" + str(lst), "-odir:" + str(out), "-drc_cut_fac:1")
    assert p.returncode == 2 and sbr + ": a -drc_* flag on a stream with SBR" in p.stderr and not os.listdir(out)


def _multichannel_stream():
    path = os.path.join(dc.ROOT, "tests", "golden", "streams_wide", "mc6_aot2.aac")   # 5.1 AAC-LC
    return path if os.path.exists(path) else None


def test_python_refusals():
    lc, sbr = dc.stream("drc_stereo_2band"), open(os.path.join(PLAIN, "mix_aot5_48k.aac"), "rb").read()
    for bad in (dict(cut=1.5), dict(boost=-1), dict(target_level=128), dict(target_level=-1), dict(heavy_comp=1), dict(level=3), 7):
        with pytest.raises(ValueError):
            decoder.plan_mixed([lc], drc=bad)
    with pytest.raises(ValueError, match="stream 1: drc on a stream with SBR"):
        decoder.plan_mixed([lc, sbr], drc=dict(cut=1))
    assert len(decoder.plan_mixed([lc, sbr])) == 2 and len(decoder.plan_mixed([lc, dc.stream("drc_mono_1band")], drc=dict(cut=1))) == 2
    with pytest.raises(ValueError, match="SBR"):   # decode_streams' own check comes before any GPU work too
        decoder.decode_streams([sbr], drc=dict(cut=1), device="cpu")


def test_more_than_two_channels_are_refused(tmp_path):
    path = _multichannel_stream()
    assert path is not None, "no committed multichannel stream"
    p = _cli("-ifile:" + path, "-ofile:" + str(tmp_path / "o.wav"), "-drc_cut_fac:1", "-plan")
    assert p.returncode == 2 and "a -drc_* flag on a stream of more than two channels" in p.stderr
    with pytest.raises(ValueError, match="more than two channels"):
        decoder.plan_mixed([open(path, "rb").read()], drc=dict(cut=1))


def test_struct_layouts_match_the_header(tmp_path):
    import libxaac_amd
    src, exe = tmp_path / "d.c", tmp_path / "d"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xaac_parse.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(xaac_drc_side), offsetof(xaac_drc_side, fac), sizeof(xaac_drc_config), sizeof(xaac_drc_batch), '
                   'offsetof(xaac_drc_batch, status), sizeof(xaac_parse_batch), offsetof(xaac_parse_batch, drc_side)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(dc.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S, B, P = libxaac_amd.DrcSide, libxaac_amd.abi.DrcBatch, decoder._ParseBatch
    assert got == [ctypes.sizeof(S), S.fac.offset, ctypes.sizeof(libxaac_amd.DrcConfig), ctypes.sizeof(B), B.status.offset,
                   ctypes.sizeof(P), P.drc_side.offset]
    assert ctypes.sizeof(S) == 4 * libxaac_amd.DRC_SIDE_WORDS == 4 * dc.WORDS


def test_tables_match_the_reference_image():
    """libxaac_amd/csrc/tables_drc.inc regenerated from the compiled reference's image equals the committed file"""
    dc.need("libref_harness.so")
    import gen_tables_drc as g
    inc = os.path.join(dc.ROOT, "libxaac_amd", "csrc", "tables_drc.inc")
    assert g.render(*g.reference_tables()) == open(inc).read()


def test_committed_streams_and_records_are_small():
    sizes = [os.path.getsize(os.path.join(dc.STREAMS, n + ".aac")) for n in dc.NAMES]
    largest = max(os.path.getsize(os.path.join(PLAIN, f)) for f in os.listdir(PLAIN))
    assert max(sizes) < largest / 2 and os.path.getsize(os.path.join(dc.ROOT, "tests", "golden", "drc_spec.npz")) < 512 * 1024
