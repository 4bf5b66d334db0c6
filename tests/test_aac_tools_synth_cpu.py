"""The AAC spectral tools (M/S, intensity, PNS, TNS: libxaac_amd/csrc/aac_tools.h through the parser's stage 2 and its twin
xaac_core_tools_apply_host) against the reference decoder's own spectra on generator-made streams, without a GPU.

tests/golden/streams_synth is written by tools/make_synth_streams.py (synth_set): for every sampling frequency index 0 .. 11 a
stereo stream of 24 frames and a mono stream of 12, half of them with global gains up to 250 (stage-1 spectra of 31 to 32
magnitude bits); ADTS channel_configuration 3 and 6 streams (SCE CPE [CPE LFE]) that bring intensity, PNS and pulse data to the
arithmetic of streams with more than two channels; one configuration-6 stream the multichannel entry points refuse.  The
reference's encoder uses none of these tools, and the three older generator-made streams all have index 3.

For every stream: stage 1 + twin from the stream's initial generator state (xaac_parse_core_tools_state) == stage 2 == the
type-2 XAAC_SPEC_DUMP records of oracle/_ref/xaacdec_capture, word for word.  Five stereo streams (indices 3, 5, 7, 8, 9) have
in frame 0 a noise band of the right channel under a set ms_used bit where the left channel has no noise: the band's seed is
what the reference's initialisation pass over that frame left in scratch memory, which an all-zero initial state gets wrong
(the last test pins that the streams show it).

Coverage per sampling frequency index, in frames of the stereo + mono stream (asserted: at least 5 each):

    index  TNS long  TNS short  M/S  intensity  correlated PNS
      0        8         7        7     11            5
      1       12         6       16     12            9
      2        6         5       14     10           11
      3       12         6       11     10            9
      4        6         5       13     11            7
      5       10         6       10      8            5
      6       11         5       10      6            7
      7        9         5       12      9           11
      8       10         6       13      7            9
      9       12         7       13     10            8
     10       10         5       10     12            8
     11        9         5        6      8            5

A sweep of four more seeds per index, made on the spot and never committed, is compared the same way."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aac_tools_cases as tc  # noqa: E402
from libxaac_amd import decoder  # noqa: E402

ROWS = tc.synth_rows()
DECODED = [r for r in ROWS if r[5] <= 2 or r[6]]          # every stream but the refused one
REFUSED = [r for r in ROWS if r[5] > 2 and not r[6]]
FRAME0 = ["st_sr03", "st_sr05", "st_sr07", "st_sr08", "st_sr09"]
_refs = {}


def reference(name, kind, tmp):
    if name not in _refs:
        _refs[name] = tc.reference_spectra(tc.synth_path(name), tmp, tc.synth_channels(kind))
    return _refs[name]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("synth"))


def test_the_generator_writes_the_committed_streams_byte_for_byte():
    """the three older streams of tests/golden/streams (the generator's first form) and every file of tests/golden/streams_synth;
    nothing else lies in that directory; no file above 64 KB, the directory under 700 KB"""
    import make_synth_streams as m
    for name, seed, sr, frames, level, kind, avoid in m.FIRST:
        assert m.make(seed, sr, frames, level, kind, avoid, busy=False) == open(os.path.join(tc.STREAMS, name + ".aac"), "rb").read(), name
    sizes = []
    for name, seed, sr, frames, level, kind, avoid in ROWS:
        data = open(tc.synth_path(name), "rb").read()
        assert m.make(seed, sr, frames, level, kind, avoid) == data, name
        sizes.append(len(data))
    assert sorted(os.listdir(tc.SYNTH)) == sorted(r[0] + ".aac" for r in ROWS)
    assert max(sizes) <= 64 * 1024 and sum(sizes) < 700 * 1024


def test_the_set_is_what_it_is_meant_to_be():
    import make_synth_streams as m
    stereo = [r for r in ROWS if r[5] == 2]
    mono = [r for r in ROWS if r[5] == 1]
    assert sorted(r[2] for r in stereo) == list(range(12)) and sorted(r[2] for r in mono) == list(range(12))
    assert all(r[3] == 24 for r in stereo) and all(r[3] == 12 for r in mono)
    assert sum(r[4] == m.LOUD for r in stereo) == 6 and sum(r[4] == m.LOUD for r in mono) == 6
    wide = sorted((r[5], r[2], r[4] == m.LOUD) for r in ROWS if r[5] > 2 and r[6])
    assert wide == [(3, 3, False), (3, 8, False), (6, 3, False), (6, 3, True), (6, 5, False), (6, 11, False)]
    assert all(r[3] == 24 for r in ROWS if r[5] > 2 and r[6]) and len(REFUSED) == 1 and REFUSED[0][5] == 6


@pytest.mark.parametrize("row", DECODED, ids=[r[0] for r in DECODED])
def test_stage_1_and_the_twin_equal_stage_2_and_the_reference(row, tmp):
    name, _, sr, frames, _, kind, _ = row
    before, after = tc.synth_walk(name)
    ref = reference(name, kind, tmp)
    assert len(before) == len(after) == len(ref) == frames
    data = open(tc.synth_path(name), "rb").read()
    twin, _ = tc.twin_walk(before, tc.new_states(data))
    for f in range(frames):
        for side in before[f][4]:
            s = decoder.CoreToolsSide.from_buffer_copy(side)
            assert s.sr_index == sr and s.ch[0].wide == int(kind > 2)
        assert before[f][0].shape == (tc.synth_channels(kind), 1024)
        bad = np.nonzero((after[f][0] != ref[f]).any(axis=1))[0]
        assert not len(bad), ("stage 2 against the reference", name, f, bad)
        assert np.array_equal(twin[f], after[f][0]), ("stage 1 + twin against stage 2", name, f)


def test_the_parsers_own_state_is_the_streams_initial_state_at_stage_1_and_runs_on_at_stage_2():
    lib = decoder.load_host_library()
    data = open(tc.synth_path("st_sr05"), "rb").read()
    first = tc.new_states(data)[0]
    assert first[:4].view(np.int32)[0] == 0 and first[4:].any()          # pns_seed 0, seeds of frame 0's correlated bands
    before, _ = tc.synth_walk("st_sr05")
    _, final = tc.twin_walk(before, [first])
    for stage, want in ((1, first), (2, final[0])):
        p, core, used, pos = ctypes.c_void_p(), decoder.CoreFrame(), ctypes.c_size_t(), 0
        assert lib.xaac_parser_create(ctypes.byref(p)) == 0
        try:
            while pos + 7 <= len(data):
                assert lib.xaac_parse_adts_frame(p, data[pos:], len(data) - pos, stage, ctypes.byref(core), ctypes.byref(used)) == 0
                pos += used.value
            got = np.zeros(decoder.CORE_TOOLS_STATE_BYTES, np.uint8)
            assert lib.xaac_parse_core_tools_state(p, got.ctypes.data) == 0
            assert lib.xaac_parse_core_tools_state_mc(p, 1, got.ctypes.data) == -2      # no slot behind the first
            assert np.array_equal(got, want), stage
        finally:
            lib.xaac_parser_destroy(p)


def test_coverage(capsys):
    """every sampling frequency index: at least 5 frames each of TNS on long windows, TNS on EIGHT_SHORT, M/S, intensity and
    correlated PNS; at least four stereo streams at three or more indices with a right-only correlated noise band in frame 0;
    behind the first element of every multichannel stream at least 5 frames each of PNS, intensity, TNS of order 8 or more and
    TNS on short windows"""
    need = ("tns_long", "tns_short", "ms", "intensity", "pns_corr")
    later_need = ("pns", "intensity", "tns_order8", "tns_short")
    per_sr = {sr: dict.fromkeys(need, 0) for sr in range(12)}
    later = {}
    frame0 = []
    for name, _, sr, _, _, kind, _ in DECODED:
        before, _ = tc.synth_walk(name)
        for f, (_, _, tools, ids, sides) in enumerate(before):
            for k in range(len(ids)):
                got = tc.coverage(tools[k], sides[k])
                if kind <= 2:
                    for c in need:
                        per_sr[sr][c] += c in got
                elif k > 0:
                    row = later.setdefault(name, dict.fromkeys(later_need, 0))
                    for c in later_need:
                        row[c] += c in got
        if kind == 2 and tc.right_only_bands(before[0][4][0]):
            frame0.append((name, sr))
    with capsys.disabled():
        print("\nindex  " + "  ".join(need))
        for sr in range(12):
            print("%5d  " % sr + "  ".join("%*d" % (len(c), per_sr[sr][c]) for c in need))
        for name in later:
            print(name, "behind the first element:", later[name])
        print("a right-only correlated noise band in frame 0:", frame0)
    for sr in range(12):
        assert min(per_sr[sr].values()) >= 5, (sr, per_sr[sr])
    assert sorted(n for n, _ in frame0) == FRAME0 and len({sr for _, sr in frame0}) >= 3
    assert len(later) == 6
    for name in later:
        assert min(later[name].values()) >= 5, (name, later[name])


def test_the_generators_notes_agree_with_the_parsers_side_info():
    """which frames hold a right-only correlated noise band: as the generator wrote them against the side info the parser hands
    out -- the streams with the avoidance switch on have none"""
    import make_synth_streams as m
    for name, seed, sr, frames, level, kind, avoid in DECODED:
        _, noted = m.make_with_notes(seed, sr, frames, level, kind, avoid)
        before, _ = tc.synth_walk(name)
        seen = [f for f in range(frames) if any(tc.right_only_bands(s) for s in before[f][4])]
        assert noted == seen, name
        assert not (avoid and seen), name


def test_a_seed_sweep_made_on_the_spot_equals_the_reference(tmp):
    """four further seeds per sampling frequency index, stereo, 16 frames, levels alternating"""
    import make_synth_streams as m
    bad = []
    for sr in range(12):
        for j in range(4):
            seed = 5000 + 12 * j + sr
            data = m.make(seed, sr, 16, m.LOUD if j & 1 else m.QUIET, 2)
            path = os.path.join(tmp, "sweep_%d_%d.aac" % (sr, j))
            open(path, "wb").write(data)
            before, after = tc.synth_walk(None, data)
            ref = tc.reference_spectra(path, tmp, 2)
            twin, _ = tc.twin_walk(before, tc.new_states(data))
            assert len(before) == len(after) == len(ref) == 16, (sr, seed)
            for f in range(16):
                if not (np.array_equal(after[f][0], ref[f]) and np.array_equal(twin[f], ref[f])):
                    bad.append((sr, seed, f))
    assert not bad, bad


def test_a_right_only_correlated_noise_band_behind_the_first_frame_is_refused_in_a_multichannel_stream():
    """include/xaac_parse.h: such a band's seed is shared by the elements in the reference and per element here, so the frame is
    XAAC_PARSE_ERR_UNSUPPORTED -- at the first frame the generator wrote the pattern into, not before, at either stage, and
    nothing of the frame is handed out"""
    import make_synth_streams as m
    name, seed, sr, frames, level, kind, avoid = REFUSED[0]
    data, noted = m.make_with_notes(seed, sr, frames, level, kind, avoid)
    assert data == open(tc.synth_path(name), "rb").read() and noted and 0 < noted[0] < frames
    lib = decoder.load_host_library()
    for stage in (1, 2):
        p = ctypes.c_void_p()
        assert lib.xaac_parser_create(ctypes.byref(p)) == 0
        try:
            elems, n, used, pos = (decoder.CoreFrame * decoder.MC_MAX_ELEMENTS)(), ctypes.c_int32(), ctypes.c_size_t(), 0
            side = (ctypes.c_uint8 * decoder.CORE_TOOLS_SIDE_BYTES)()
            for f in range(noted[0]):
                assert lib.xaac_parse_adts_frame_mc(p, data[pos:], len(data) - pos, stage, elems, decoder.MC_MAX_ELEMENTS, ctypes.byref(n),
                                                    ctypes.byref(used)) == 0, (stage, f)
                assert n.value == 4 and lib.xaac_parse_core_tools_side_mc(p, 1, side) == 0
                pos += used.value
            assert lib.xaac_parse_adts_frame_mc(p, data[pos:], len(data) - pos, stage, elems, decoder.MC_MAX_ELEMENTS, ctypes.byref(n),
                                                ctypes.byref(used)) == tc.UNSUPPORTED
            assert n.value == 0 and lib.xaac_parse_core_tools_side_mc(p, 1, side) == -2
        finally:
            lib.xaac_parser_destroy(p)
        with pytest.raises(decoder.ParseError) as e:
            decoder.parse_stream_mc(data, stage=stage)
        assert (e.value.code, e.value.frame) == (tc.UNSUPPORTED, noted[0])


@pytest.mark.parametrize("name", FRAME0)
def test_from_an_all_zero_state_the_frame_0_streams_differ_from_the_reference(name, tmp):
    """the rule `zero for a new stream` is wrong exactly here: the streams exercise the path"""
    before, _ = tc.synth_walk(name)
    ref = reference(name, 2, tmp)
    zero, _ = tc.twin_walk(before, [np.zeros(decoder.CORE_TOOLS_STATE_BYTES, np.uint8)])
    differing = [f for f in range(len(ref)) if not np.array_equal(zero[f], ref[f])]
    assert differing, name
    bands = tc.right_only_bands(before[0][4][0])
    assert bands and not (tc.new_states(open(tc.synth_path(name), "rb").read())[0][4:].view(np.int32)[bands] == 0).all()
