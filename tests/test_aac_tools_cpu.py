"""The AAC spectral tools on the CPU: the side info the parser hands out for a stage-1 frame (xaac_parse_core_tools_side) and
the host twin of the GPU kernel (xaac_core_tools_apply_host, the arithmetic of libxaac_amd/csrc/aac_tools.h) turn stage-1
spectra into exactly the stage-2 parse's spectra and into the reference's own type-2 XAAC_SPEC_DUMP records
(oracle/_ref/xaacdec_capture), word for word, frame after frame with the noise generator's state carried by the caller --
on the committed ADTS streams and on streams oracle/_ref/xaacenc makes on the spot (AAC-LC and HE-AAC, mono and stereo,
16 - 48 kHz cores, low and high bit rates, transient-rich input).  CPU only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import aac_tools_cases as tc  # noqa: E402
from libxaac_amd import decoder  # noqa: E402


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return tc.stream_files(str(tmp_path_factory.mktemp("aac_tools")))


@pytest.mark.parametrize("index", range(len(tc.COMMITTED) + len(tc.ENCODED)))
def test_stage1_plus_tools_equals_stage2_and_the_reference(files, index, tmp_path):
    name, path = files[index]
    data = open(path, "rb").read()
    frames, after = tc.walk(data)
    assert len(frames) == len(after) and len(frames) > 10, name
    n_ch = frames[0][3]
    ref = tc.reference_spectra(path, str(tmp_path), n_ch)
    assert len(ref) == len(frames), (name, len(ref), len(frames))
    state = np.zeros(decoder.CORE_TOOLS_STATE_BYTES, np.uint8)
    for f, (spec, side, _, n) in enumerate(frames):
        rc, got, state = tc.apply_host(spec, side, state)
        assert rc == 0 and n == n_ch, (name, f)
        for c in range(n_ch):
            assert np.array_equal(got[c], after[f][c]), (name, f, c, "stage 2", np.nonzero(got[c] != after[f][c])[0][:8])
            assert np.array_equal(got[c], ref[f, c]), (name, f, c, "reference", np.nonzero(got[c] != ref[f, c])[0][:8])


def test_a_stage1_parse_leaves_the_parsers_noise_generator_alone():
    """stage-1 parsing of a stream with PNS with the side info taken from every frame, then the same parser at stage 2 over the
    stream again: the spectra equal a fresh parser's, so neither the stage-1 pass nor xaac_parse_core_tools_side moved the
    parser's own seeds; and the side call refuses a parser whose last frame failed"""
    data = open(os.path.join(tc.STREAMS, "synth_lc_a.aac"), "rb").read()
    lib = decoder.load_host_library()
    p = ctypes.c_void_p()
    lib.xaac_parser_create(ctypes.byref(p))
    core, used = decoder.CoreFrame(), ctypes.c_size_t()
    want = decoder.parse_stream(data, stage=2)
    for stage in (1, 2):
        pos = 0
        for f in range(len(want)):
            assert lib.xaac_parse_adts_frame(p, data[pos:], len(data) - pos, stage, ctypes.byref(core), ctypes.byref(used)) == 0
            pos += used.value
            if stage == 1:   # the new call works on the parser's element (it derives the PNS correlation flags there)
                side = np.zeros(decoder.CORE_TOOLS_SIDE_BYTES, np.uint8)
                assert lib.xaac_parse_core_tools_side(p, side.ctypes.data) == 0
                assert lib.xaac_parse_core_tools_side(p, side.ctypes.data) == 0   # ... once per frame, however often it is asked
            if stage == 2:
                assert np.array_equal(np.ctypeslib.as_array(core.spec)[:core.n_ch], want[f][0]), f
    side = np.zeros(decoder.CORE_TOOLS_SIDE_BYTES, np.uint8)
    assert lib.xaac_parse_adts_frame(p, b"\xff\xf1\x50\x80\x02\x1f\xfc" + b"\xff" * 9, 16, 1, ctypes.byref(core), ctypes.byref(used)) != 0
    assert lib.xaac_parse_core_tools_side(p, side.ctypes.data) == -2
    lib.xaac_parser_destroy(p)


def test_refused_side_info_leaves_spectra_and_state():
    rng = np.random.default_rng(5)
    for breakage in ("max_sfb", "order", "n_ch", "groups"):
        side, spec, state = tc.random_element(rng)
        s = decoder.CoreToolsSide.from_buffer(side)
        if breakage == "max_sfb":
            s.ch[0].max_sfb = 60
        elif breakage == "order":
            s.ch[0].window_sequence, s.ch[0].num_groups, s.ch[0].group_len[0], s.common_window = 0, 1, 1, 0
            s.ch[0].max_sfb = min(s.ch[0].max_sfb, 40)
            s.ch[0].tns_present, s.ch[0].n_filt[0] = 1, 1
            s.ch[0].tns[0].order, s.ch[0].tns[0].direction = 13, 1
        elif breakage == "n_ch":
            s.n_ch = 3
        else:
            s.ch[0].window_sequence, s.ch[0].num_groups, s.common_window = 2, 2, 0
            s.ch[0].group_len[0], s.ch[0].group_len[1] = 3, 4
            s.ch[0].max_sfb = min(s.ch[0].max_sfb, 12)
        rc, got, st = tc.apply_host(spec, side, state)
        assert rc == -1 and np.array_equal(got, spec) and np.array_equal(st, state), breakage


def test_struct_layouts_match_the_header(tmp_path):
    """the ctypes mirrors (libxaac_amd/decoder.py, libxaac_amd/__init__.py) against what a C compiler makes of the headers"""
    import libxaac_amd
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xaac_amd.h"\n#include "xaac_parse.h"\nint main(void) { '
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(xaac_core_tools_side), offsetof(xaac_core_tools_side, ch), '
                   'sizeof(xaac_core_tools_channel), offsetof(xaac_core_tools_channel, sf), offsetof(xaac_core_tools_channel, tns), '
                   'sizeof(xaac_core_tools_state), sizeof(xaac_aac_tools_batch), offsetof(xaac_aac_tools_batch, status)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    B = libxaac_amd.abi.AacToolsBatch
    assert got == [ctypes.sizeof(decoder.CoreToolsSide), decoder.CoreToolsSide.ch.offset, ctypes.sizeof(decoder.CoreToolsChannel),
                   decoder.CoreToolsChannel.sf.offset, decoder.CoreToolsChannel.tns.offset, ctypes.sizeof(decoder.CoreToolsState),
                   ctypes.sizeof(B), B.status.offset]
    assert (libxaac_amd.CORE_TOOLS_SIDE_BYTES, libxaac_amd.CORE_TOOLS_STATE_BYTES) == (got[0], got[5])


def test_shared_tables_are_the_parsers(tmp_path):
    """libxaac_amd/csrc/tables_aac_tools.inc regenerated from libxaac_amd/host/tables_aac.inc equals the committed file"""
    import gen_tables_aac_tools as g
    assert g.render() == open(os.path.join(ROOT, "libxaac_amd", "csrc", "tables_aac_tools.inc")).read()


def test_fuzz_elements_are_accepted_by_the_host_twin():
    """the random elements of the GPU fuzz tier are legal side info (status 0) and exercise every tool"""
    rng = np.random.default_rng(11)
    seen = {"ms": 0, "intensity": 0, "pns_corr": 0, "tns_long": 0, "tns_short": 0}
    for _ in range(300):
        side, spec, state = tc.random_element(rng)
        rc, got, st = tc.apply_host(spec, side, state)
        assert rc == 0
        s = decoder.CoreToolsSide.from_buffer(side)
        seen["ms"] += any(s.ms_used)
        seen["pns_corr"] += any(s.pns_correlated)
        seen["intensity"] += s.n_ch == 2 and any(c >= 14 for c in s.ch[1].cb)
        for c in range(s.n_ch):
            if s.ch[c].tns_present and any(s.ch[c].n_filt):
                seen["tns_short" if s.ch[c].window_sequence == 2 else "tns_long"] += 1
    assert all(v >= 20 for v in seen.values()), seen
