"""The host front end on multichannel HE-AAC streams (channel_config 3 .. 6, an SBR payload per channel element): every frame of
the committed 5.1 stream and of the three streams the reference encoder makes parses with xaac_parse_batch::mc_sbr in both readings
of the payload, the LFE's rows never say `apply`, a pair's rows carry equal header copies, the switch is off by default, and the
new entry points are memory-safe on damaged frames.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aac_tools_cases as tc
import mc_sbr_cases as cases
import multichannel_cases as mc
from libxaac_amd import ESBR_SIDE_BYTES, SBR_FRAME_BYTES, SBR_HEADER_BYTES, decoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -3


def _parse_all(data, esbr):
    """every frame of one stream through BatchParser(mc_sbr=True): -> (channel_config, [(flags [n_elems, 8], header rows, frame rows)])"""
    bp = decoder.BatchParser([data], esbr=esbr, mc_sbr=True)
    try:
        assert bp.mc_sbr and bp.sbr and bp.channel_config == mc.channel_config(data)
        n_ch, n_el = bp.n_ch, bp.n_elems
        spec, ics = np.zeros((n_ch, 1024), np.int32), np.zeros((n_ch, 2), np.uint8)
        hdr, frm = np.zeros((n_ch, SBR_HEADER_BYTES), np.uint8), np.zeros((n_ch, SBR_FRAME_BYTES), np.uint8)
        eside = np.zeros((n_ch, ESBR_SIDE_BYTES), np.uint8) if esbr else None
        flags = np.full((1, n_el, 8), 77, np.int32)
        out = []
        while bp.step(spec, ics, hdr, frm, None, flags, eside)[0]:
            out.append((flags[0].copy(), hdr.copy(), frm.copy()))
        return bp.channel_config, out
    finally:
        bp.close()


@pytest.mark.parametrize("esbr", [False, True])
@pytest.mark.parametrize("name", cases.NAMES)
def test_every_frame_parses_per_element(name, esbr):
    if name != "mc6_aot5":
        tc.need("xaacenc")
    data = cases.stream(name)
    config, frames = _parse_all(data, esbr)
    elements, _, _ = mc.LAYOUT[config]
    assert len(frames) == len(cases.adts_frames(data)) and len(frames) >= 16
    first_ch = np.concatenate([[0], np.cumsum([2 if e == 1 else 1 for e in elements])[:-1]])
    applied = np.zeros(len(elements), int)
    for flags, hdr, frm in frames:
        assert not (flags == 77).any()                           # every element's row was written
        for k, e in enumerate(elements):
            applied[k] += flags[k, decoder.F_APPLY]
            if e == 3:                                           # the LFE: SBR data missing, never `apply`, never a reset
                assert flags[k, decoder.F_APPLY] == 0 and flags[k, decoder.F_RESET] == 0 and flags[k, decoder.F_FRAME_OK] == 0
            if e == 1:                                           # a pair: both channel rows carry the pair's header
                assert flags[k, decoder.F_STEREO] == 1
                assert bytes(hdr[first_ch[k]]) == bytes(hdr[first_ch[k] + 1])
            assert flags[k, decoder.F_PS] == 0                   # no parametric stereo in a frame of several elements
    for k, e in enumerate(elements):                             # every element but the LFE runs its SBR tool (the default reading one
        assert applied[k] == 0 if e == 3 else applied[k] >= len(frames) - 2    # frame late)


def _first_frame_batch(data, mc_sbr, size=None):
    lib = decoder.load_host_library()
    lib.xaac_parse_batch_run_sized.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    n_ch = mc.channel_config(data)
    h = ctypes.c_void_p()
    assert lib.xaac_parser_create(ctypes.byref(h)) == 0
    parsers = (ctypes.c_void_p * 1)(h)
    blob = np.frombuffer(data, np.uint8).copy()
    ptrs, size_b = np.array([blob.ctypes.data], np.uint64), np.array([len(data)], np.uint64)
    spec, ics = np.zeros((n_ch, 1024), np.int32), np.zeros((n_ch, 2), np.uint8)
    hdr, frm = np.zeros((n_ch, SBR_HEADER_BYTES), np.uint8), np.zeros((n_ch, SBR_FRAME_BYTES), np.uint8)
    flags, consumed, status = np.zeros((4, 8), np.int32), np.zeros(1, np.uint64), np.full(1, 77, np.int32)
    b = decoder._ParseBatch()
    b.n_streams, b.n_ch, b.with_sbr, b.ps_enable, b.stage, b.threads = 1, n_ch, 1, 1, 2, 1
    b.parser, b.data, b.bytes = ctypes.addressof(parsers), ptrs.ctypes.data, size_b.ctypes.data
    b.spec, b.ics, b.header, b.frame, b.flags = spec.ctypes.data, ics.ctypes.data, hdr.ctypes.data, frm.ctypes.data, flags.ctypes.data
    b.consumed, b.status, b.channel_config, b.mc_sbr = consumed.ctypes.data, status.ctypes.data, n_ch, mc_sbr
    rc = lib.xaac_parse_batch_run_sized(ctypes.byref(b), ctypes.sizeof(b) if size is None else size)
    lib.xaac_parser_destroy(h)
    return rc, int(status[0])


def test_the_switch_is_off_by_default():
    he = cases.stream("mc6_aot5")
    assert _first_frame_batch(he, 1) == (1, 0)
    assert _first_frame_batch(he, 0) == (UNSUPPORTED, 77)
    # a descriptor that ends in front of the new member (a binary built before it): as mc_sbr = 0, whatever lies behind it
    assert _first_frame_batch(he, 1, size=decoder._ParseBatch.mc_sbr.offset) == (UNSUPPORTED, 77)
    assert _first_frame_batch(he, 2)[0] == -2                    # a bad descriptor
    with pytest.raises(ValueError, match="multichannel SBR"):
        decoder.BatchParser([he])
    with pytest.raises(ValueError, match="multichannel SBR"):
        decoder.BatchParser([he], mc_sbr=False)


def test_parse_batch_mirror_matches_header(tmp_path):
    """decoder._ParseBatch (grown by mc_sbr) against what a C compiler makes of include/xaac_parse.h"""
    src, exe = tmp_path / "h.c", tmp_path / "h"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xaac_parse.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(xaac_parse_batch), offsetof(xaac_parse_batch, channel_config), offsetof(xaac_parse_batch, mc_sbr)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(decoder._ParseBatch), decoder._ParseBatch.channel_config.offset, decoder._ParseBatch.mc_sbr.offset]


def test_single_frame_entry_points():
    """xaac_parse_sbr_side_mc / _esbr_side_mc / _reset_pitch_mc frame by frame against the batch's rows of the same stream"""
    lib = decoder.load_host_library()
    data = cases.stream("mc6_aot5")
    _, want = _parse_all(data, True)
    elems, n, used, p = (decoder.CoreFrame * 4)(), ctypes.c_int32(), ctypes.c_size_t(), ctypes.c_void_p()
    side, eside, pitch = decoder.SbrSide(), (ctypes.c_uint8 * ESBR_SIDE_BYTES)(), ctypes.c_int32()
    lib.xaac_parser_create(ctypes.byref(p))
    assert lib.xaac_parser_set_esbr(p, 1) == 0
    assert lib.xaac_parse_sbr_side_mc(p, 0, ctypes.byref(side)) == -2          # no frame yet
    at = 0
    for flags, hdr, frm in want:
        rest = data[at:]
        assert lib.xaac_parse_adts_frame_mc(p, rest, len(rest), 2, elems, 4, ctypes.byref(n), ctypes.byref(used)) == 0 and n.value == 4
        at += used.value
        assert [int(elems[k].sbr_bytes) > 0 for k in range(4)] == [True, True, True, False]   # every element's payload is kept; the LFE has none
        row = 0
        for k in range(4):
            assert lib.xaac_parse_sbr_side_mc(p, k, ctypes.byref(side)) == 0
            got = [side.apply, side.reset, side.reset_channels, side.upsampling, side.stereo, side.ps, side.ps_start, side.frame_ok]
            assert got == list(flags[k])
            for c in range(elems[k].n_ch):
                assert bytes(side.header) == bytes(hdr[row]) and bytes(side.frame[c]) == bytes(frm[row])
                assert lib.xaac_parse_esbr_side_mc(p, k, c, eside) == 0
                row += 1
            assert lib.xaac_parse_reset_pitch_mc(p, k, ctypes.byref(pitch)) == 0
        assert lib.xaac_parse_sbr_side_mc(p, 4, ctypes.byref(side)) == -2 and lib.xaac_parse_esbr_side_mc(p, 0, 2, eside) == -2
    assert lib.xaac_parser_set_esbr(p, 0) == -2                                 # the reading is fixed by the first side info call
    lib.xaac_parser_destroy(p)


def test_damaged_frames_are_memory_safe(tmp_path):
    """tests/fuzz/fuzz_parser_mc_sbr.cpp with the host sources under ASan + UBSan: truncated, bit-flipped, randomised and spliced
    frames of the committed 5.1 HE-AAC stream through the per-element entry points and the batch with mc_sbr; a stand-alone
    program, nothing is loaded into Python"""
    host = os.path.join(ROOT, "libxaac_amd", "host")
    exe = str(tmp_path / "fuzz_parser_mc_sbr")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "fuzz_parser_mc_sbr.cpp")] + [os.path.join(host, f) for f in ("xaac_parse.cpp", "aac_core.cpp", "sbr_side.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fwrapv", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", *srcs, "-o", exe, "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, cases.stream_path("mc6_aot5"), "4242", "240"], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-300:], p.stderr[-3000:])
    assert "frames parsed" in p.stdout and "frames parsed 0," not in p.stdout and "element side infos 0," not in p.stdout
