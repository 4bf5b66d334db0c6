"""The host front end's channel-element slots: what xaac_parse_batch_run_sized writes is pinned array by array to a recording of
the library before mono / stereo and multichannel streams went through one path (tests/golden/parser_batch_pin.json, made by
tools/make_golden_parser_batch.py: intact, truncated, bit-flipped, spliced and two-block copies of the committed streams), and the
single-element entry points are the element-0 case of the multichannel ones.  No GPU."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_parser_batch as pin  # noqa: E402
from libxaac_amd import CORE_TOOLS_SIDE_BYTES, ESBR_SIDE_BYTES, decoder  # noqa: E402

STREAMS = sorted(n for n in pin.streams() if not n.startswith("mc6_"))


def test_batch_output_is_what_it_was():
    want = json.load(open(pin.PIN))
    assert want["seed"] == pin.SEED
    got, frames = pin.replay()
    assert frames > 10000 and sorted(got) == sorted(want["runs"])
    names = pin.ARRAYS + ("rc",)
    bad = [(run, [n for n, a, b in zip(names, got[run].split(), want["runs"][run].split()) if a != b] or "other arrays")
           for run in sorted(got) if got[run] != want["runs"][run]]
    assert not bad, (len(bad), bad[:8])


def _walk(lib, data, stage, esbr, multi, ps_enable=0, switch_at=None):
    """every frame of a one-element stream through the single-element entry points, or (multi; from frame switch_at on) through the
    _mc ones with element 0 -> [(consumed, n_elems, xaac_core_frame, tools side, sbr side or None, esbr sides, pitch)] as bytes"""
    p = ctypes.c_void_p()
    assert lib.xaac_parser_create(ctypes.byref(p)) == 0 and lib.xaac_parser_set_esbr(p, esbr) == 0
    elems, n, used = (decoder.CoreFrame * 4)(), ctypes.c_int32(1), ctypes.c_size_t()
    tside, side, pitch = (ctypes.c_uint8 * CORE_TOOLS_SIDE_BYTES)(), decoder.SbrSide(), ctypes.c_int32()
    eside = [(ctypes.c_uint8 * ESBR_SIDE_BYTES)(), (ctypes.c_uint8 * ESBR_SIDE_BYTES)()]
    out, at = [], 0
    while len(data) - at >= 7:
        rest = data[at:]
        mc = multi or (switch_at is not None and len(out) >= switch_at)
        if mc:
            rc = lib.xaac_parse_adts_frame_mc(p, rest, len(rest), stage, elems, 4, ctypes.byref(n), ctypes.byref(used))
        else:
            rc = lib.xaac_parse_adts_frame(p, rest, len(rest), stage, ctypes.byref(elems[0]), ctypes.byref(used))
        if rc == 1:
            break
        assert rc == 0
        at += used.value
        assert (lib.xaac_parse_core_tools_side_mc(p, 0, tside) if mc else lib.xaac_parse_core_tools_side(p, tside)) == 0
        sbr = elems[0].sbr_bytes > 0 or any(f[4] is not None for f in out)
        if sbr:
            assert (lib.xaac_parse_sbr_side_mc(p, 0, ctypes.byref(side)) if mc else lib.xaac_parse_sbr_side(p, ps_enable, ctypes.byref(side))) == 0
            if esbr:
                for c in range(elems[0].n_ch):
                    assert (lib.xaac_parse_esbr_side_mc(p, 0, c, eside[c]) if mc else lib.xaac_parse_esbr_side(p, c, eside[c])) == 0
            assert (lib.xaac_parse_reset_pitch_mc(p, 0, ctypes.byref(pitch)) if mc else lib.xaac_parse_reset_pitch(p, ctypes.byref(pitch))) == 0
        out.append((used.value, n.value, bytes(elems[0]), bytes(tside), bytes(side) if sbr else None,
                    [bytes(e) for e in eside] if sbr and esbr else None, pitch.value if sbr else None))
    lib.xaac_parser_destroy(p)
    return out


@pytest.mark.parametrize("name", STREAMS)
def test_both_families_agree_on_one_element_streams(name):
    lib, data = decoder.load_host_library(), pin.streams()[name]
    for stage in (1, 2):
        for esbr in (0, 1):
            a, b = _walk(lib, data, stage, esbr, False), _walk(lib, data, stage, esbr, True)
            assert len(a) == len(b) == len(pin.frame_offsets(data)) - 1
            for k, (fa, fb) in enumerate(zip(a, b)):
                assert fb[1] == 1 and fa == fb, (stage, esbr, k)


def test_both_families_continue_one_decoder():
    """xaac_parse_sbr_side(ps_enable = 1) on frame k and xaac_parse_sbr_side_mc(p, 0) from frame k + 1 on address the same SBR front
    end of element 0: the side info, parametric stereo included, is the single-element family's"""
    lib, data = decoder.load_host_library(), pin.streams()["mix_aot29_32k"]
    for esbr in (0, 1):
        want = _walk(lib, data, 2, esbr, False, ps_enable=1)
        ps = [decoder.SbrSide.from_buffer_copy(f[4]).ps for f in want]
        k = next(i for i in range(2, len(ps) - 1) if ps[i] and ps[i + 1])
        got = _walk(lib, data, 2, esbr, False, ps_enable=1, switch_at=k + 1)
        assert len(got) == len(want) and sum(ps[k + 1:]) > 0
        assert got == want
