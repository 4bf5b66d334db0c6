"""Multichannel AAC-LC (ADTS channel_config 3 .. 6) through the host front end, without a GPU: xaac_parse_adts_frame_mc and the
batch call with xaac_parse_batch::channel_config on the committed 5.1 stream and on streams of channel_config 3, 4 and 5 that
oracle/_ref/xaacenc makes on the spot (48 kHz, one of them at 32 kHz; distinct content per channel, a click train in the first
channel pair):
  * the element sequence of every frame; the batch call against the single-stream call word for word;
  * stage 1 + xaac_core_tools_apply_host per element against stage 2;
  * end to end: stage-2 spectra -> the oracle's IMDCT and peak limiter (oracle/liboracle.so) -> the payload of the reference
    decoder's WAV file, byte for byte -- which pins the arithmetic such streams take in every element (q_factor 34, three bits
    down behind the stereo tools, the 32-bit TNS variant), the per-element noise generators and the output channel order;
  * what is refused: an SBR batch, a changing element sequence, a channel count that is not the configuration's;
  * the entry points under AddressSanitizer + UBSan on damaged copies of the 5.1 stream (a stand-alone program).
Which tools the streams show in an element behind the first is asserted with the XAAC_TOOL_* bits: short windows, M/S and TNS.
(Intensity stereo, PNS and pulse data are not asserted: the reference's encoder does not use them, see test_parser.py.)"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import limiter_cases as lc  # noqa: E402
import multichannel_cases as mc  # noqa: E402
import oracle_lib  # noqa: E402
from libxaac_amd import LimiterState, decoder  # noqa: E402

UNSUPPORTED = -3
_parsed = {}


def parsed(name, stage):
    """decoder.parse_stream_mc of a stream, once per test run (read-only)"""
    if (name, stage) not in _parsed:
        _parsed[(name, stage)] = decoder.parse_stream_mc(mc.stream(name), stage=stage)
    return _parsed[(name, stage)]


@pytest.mark.parametrize("name", mc.NAMES)
def test_every_frame_delivers_the_configurations_element_sequence(name):
    data = mc.stream(name)
    config = mc.channel_config(data)
    elements, route, _ = mc.LAYOUT[config]
    frames = parsed(name, 2)
    rate = decoder.AdtsHeader()
    assert decoder.load_host_library().xaac_adts_parse_header(data, len(data), ctypes.byref(rate)) == 0
    assert len(frames) == (47 if rate.sampling_rate == 48000 else 32)       # one second
    for f, (spec, ics, tools, ids, sides) in enumerate(frames):
        assert tuple(ids) == elements, f
        assert spec.shape == (len(route), 1024) and ics.shape == (len(route), 4)
    # the single-element entry keeps refusing such a frame
    lib, core, used, p = decoder.load_host_library(), decoder.CoreFrame(), ctypes.c_size_t(), ctypes.c_void_p()
    lib.xaac_parser_create(ctypes.byref(p))
    assert lib.xaac_parse_adts_frame(p, data, len(data), 2, ctypes.byref(core), ctypes.byref(used)) == UNSUPPORTED
    lib.xaac_parser_destroy(p)


def test_the_streams_show_short_windows_ms_and_tns_behind_the_first_element():
    """so that a pass of the comparisons below means something for the elements the multichannel path adds"""
    later = 0
    for name in mc.NAMES:
        for _, _, tools, _, _ in parsed(name, 2):
            for t in tools[1:]:
                later |= t
    for bit in (decoder.TOOL_SHORT, decoder.TOOL_MS, decoder.TOOL_TNS):
        assert later & bit, bit


@pytest.mark.parametrize("name", mc.NAMES)
def test_stage_1_and_the_host_tools_per_element_equal_stage_2(name):
    """every element with a noise generator of its own (zero for a new stream), as the reference keeps one core decoder
    instance per element"""
    lib = decoder.load_host_library()
    before, after = parsed(name, 1), parsed(name, 2)
    assert len(before) == len(after)
    states = [np.zeros(decoder.CORE_TOOLS_STATE_BYTES, np.uint8) for _ in before[0][3]]
    for f, ((s1, _, _, ids, sides), (s2, _, _, _, _)) in enumerate(zip(before, after)):
        row = 0
        for k, element_id in enumerate(ids):
            n = 2 if element_id == 1 else 1
            spec = np.zeros((2, 1024), np.int32)
            spec[:n] = s1[row:row + n]
            side = np.frombuffer(sides[k], np.uint8).copy()
            assert decoder.CoreToolsSide.from_buffer_copy(sides[k]).ch[0].wide == 1
            assert lib.xaac_core_tools_apply_host(side.ctypes.data, states[k].ctypes.data, spec.ctypes.data) == 0
            assert np.array_equal(spec[:n], s2[row:row + n]), (f, k)
            row += n


@pytest.mark.parametrize("frames", [1, 4])
@pytest.mark.parametrize("name", mc.NAMES)
def test_batch_call_equals_the_single_stream_call(name, frames):
    """spectra, window info, tool bits (the OR over the elements), lines (the maximum over the channels) and the element-major
    tools_side rows of a stage-1 batch of three streams -- whole, cut behind frame 9, whole -- against parse_stream_mc"""
    whole = mc.stream(name)
    want = parsed(name, 1)
    lens, pos = [], 0
    while pos + 7 <= len(whole):
        n = ((whole[pos + 3] & 3) << 11) | (whole[pos + 4] << 3) | (whole[pos + 5] >> 5)
        lens.append(n)
        pos += n
    datas = [whole, whole[:sum(lens[:9])], whole]
    ends = [len(want), 9, len(want)]
    bp = decoder.BatchParser(datas, threads=2, stage=1)
    try:
        n, n_ch, n_els, T = bp.n, bp.n_ch, bp.n_elems, frames
        assert (bp.channel_config, n_ch, n_els) == (mc.channel_config(whole), want[0][0].shape[0], len(want[0][3]))
        spec, ics = np.zeros((T, n * n_ch, 1024), np.int32), np.zeros((T, n * n_ch, 2), np.uint8)
        tools, lines, status = np.zeros((T, n), np.int32), np.zeros((T, n), np.int32), np.zeros((T, n), np.int32)
        tside = np.zeros((T, n_els, n, decoder.CORE_TOOLS_SIDE_BYTES), np.uint8)
        step = 0
        while step < len(want) + T:
            b = bp._descriptor(spec, ics, None, None, None, None, False, status=status, frames=T, lines=lines, tools_side=tside)
            b.tools = tools.ctypes.data
            assert bp.lib.xaac_parse_batch_run_sized(ctypes.byref(b), ctypes.sizeof(b)) >= 0
            for t in range(T):
                for i in range(n):
                    if step + t >= ends[i]:
                        assert status[t, i] == 1, (step + t, i)        # XAAC_PARSE_NEED_DATA
                        continue
                    assert status[t, i] == 0, (step + t, i)
                    w_spec, w_ics, w_tools, _, w_sides = want[step + t]
                    rows = spec[t, i * n_ch:(i + 1) * n_ch]
                    assert np.array_equal(rows, w_spec), (step + t, i)
                    assert np.array_equal(ics[t, i * n_ch:(i + 1) * n_ch], w_ics[:, :2].astype(np.uint8)), (step + t, i)
                    assert int(tools[t, i]) == int(np.bitwise_or.reduce(w_tools))
                    for k in range(n_els):
                        assert bytes(tside[t, k, i]) == w_sides[k], (step + t, i, k)
                    L = int(lines[t, i])
                    assert L % 16 == 0 and 0 < L <= 1024 and not rows[:, L:].any()
            step += T
    finally:
        bp.close()


@pytest.mark.parametrize("name", mc.NAMES)
def test_end_to_end_on_the_cpu_equals_the_reference_decoders_wav(name):
    """stage-2 spectra, the channels put in the reference's output order -> the oracle's IMDCT (a row per channel) -> the oracle's
    peak limiter over the interleaved block -> round16, the limiter's delay cut from the front and its delay line flushed at the
    end: the payload of the WAV file oracle/_ref/xaacdec writes"""
    orc = oracle_lib.load_oracle()
    init, _, batch = lc.bind(orc.lib, "xo")
    data = mc.stream(name)
    elements, route, mask = mc.LAYOUT[mc.channel_config(data)]
    hdr = decoder.AdtsHeader()
    decoder.load_host_library().xaac_adts_parse_header(data, len(data), ctypes.byref(hdr))
    nch = len(route)
    ovl, state = np.zeros((nch, 512), np.int32), np.zeros((nch, 2), np.uint8)
    st = LimiterState()
    delay = init(ctypes.byref(st), nch, hdr.sampling_rate)
    out = []
    for f, (spec, ics, _, _, _) in enumerate(parsed(name, 2)):
        sp, ic = np.zeros_like(spec), np.zeros((nch, 2), np.uint8)
        for c, to in enumerate(route):
            sp[to], ic[to] = spec[c], ics[c, :2]
        r = orc.imdct_batch(sp, ic, ovl, state, ch_fac=1)
        ovl, state = r["overlap"], r["state"]
        blk = np.ascontiguousarray(r["out32"].T).reshape(-1)
        qadj = np.ascontiguousarray(r["qshift_adj"])
        pcm = np.zeros(1024 * nch, np.int16)
        batch(1, 1024, nch, blk.ctypes.data_as(lc.P32), 1024 * nch, qadj.ctypes.data_as(lc.P8), ctypes.byref(st), pcm.ctypes.data_as(lc.P16))
        out.append(pcm.reshape(1024, nch)[delay if f == 0 else 0:])
    att, idx = st.attack_time_samples, st.delayed_input_index
    d = np.ctypeslib.as_array(st.delayed_input)[:att * nch].reshape(att, nch)
    tail = np.trunc(np.concatenate([d[idx:], d[:idx]]).astype(np.float64)).astype(np.int64)
    out.append((np.clip(tail + 0x8000, -(1 << 31), (1 << 31) - 1) >> 16).astype(np.int16))
    ref = mc.reference_wav(mc.stream_path(name))
    # the reference's header: WAVE_FORMAT_EXTENSIBLE, the channel count and the mask of the configuration
    assert ref[20:22] == b"\xfe\xff" and int.from_bytes(ref[22:24], "little") == nch and int.from_bytes(ref[40:44], "little") == mask
    assert ref[mc.WAV_HEADER_BYTES - 8:mc.WAV_HEADER_BYTES - 4] == b"data"
    assert np.concatenate(out).tobytes() == ref[mc.WAV_HEADER_BYTES:]


def _batch_rc(datas, n_ch, channel_config, with_sbr):
    """the return value and status words of one xaac_parse_batch_run_sized call over first frames"""
    from libxaac_amd import SBR_FRAME_BYTES, SBR_HEADER_BYTES
    lib = decoder.load_host_library()      # (by hand: BatchParser's constructor refuses what this test hands the library)
    lib.xaac_parse_batch_run_sized.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    n = len(datas)
    parsers = (ctypes.c_void_p * n)()
    for i in range(n):
        h = ctypes.c_void_p()
        assert lib.xaac_parser_create(ctypes.byref(h)) == 0
        parsers[i] = h
    blobs = [np.frombuffer(d, np.uint8).copy() for d in datas]
    ptrs = np.array([b.ctypes.data for b in blobs], np.uint64)
    size = np.array([len(d) for d in datas], np.uint64)
    spec, ics = np.zeros((n * n_ch, 1024), np.int32), np.zeros((n * n_ch, 2), np.uint8)
    hdr, frm = np.zeros((n * n_ch, SBR_HEADER_BYTES), np.uint8), np.zeros((n * n_ch, SBR_FRAME_BYTES), np.uint8)
    flags, consumed, status = np.zeros((n, 8), np.int32), np.zeros(n, np.uint64), np.full(n, 77, np.int32)
    b = decoder._ParseBatch()
    b.n_streams, b.n_ch, b.with_sbr, b.ps_enable, b.stage, b.threads = n, n_ch, with_sbr, 1, 2, 1
    b.parser, b.data, b.bytes = ctypes.addressof(parsers), ptrs.ctypes.data, size.ctypes.data
    b.spec, b.ics, b.header, b.frame, b.flags = spec.ctypes.data, ics.ctypes.data, hdr.ctypes.data, frm.ctypes.data, flags.ctypes.data
    b.consumed, b.status, b.channel_config = consumed.ctypes.data, status.ctypes.data, channel_config
    rc = lib.xaac_parse_batch_run_sized(ctypes.byref(b), ctypes.sizeof(b))
    for i in range(n):
        lib.xaac_parser_destroy(parsers[i])
    return rc, status


def test_what_the_multichannel_entry_points_refuse():
    he = open(os.path.join(mc.WIDE, "mc6_aot5.aac"), "rb").read()
    five_one, three = mc.stream("mc6_aot2"), mc.stream("mc3_48k")
    # an HE-AAC 5.1 first frame with with_sbr = 1: per-element SBR is not built
    rc, status = _batch_rc([he], 6, 6, 1)
    assert rc == UNSUPPORTED and status[0] == 77
    # ... and in Python, from the probe
    with pytest.raises(ValueError, match="multichannel SBR"):
        decoder.BatchParser([he])
    # n_ch that is not the configuration's channel count
    assert _batch_rc([five_one], 5, 6, 0)[0] == UNSUPPORTED
    assert _batch_rc([five_one], 2, 6, 0)[0] == UNSUPPORTED
    # a stream of another configuration in the batch: that stream's status word, the other one parses
    rc, status = _batch_rc([five_one, three], 6, 6, 0)
    assert rc == 1 and list(status) == [0, UNSUPPORTED]
    # a configuration outside 0, 3 .. 6 is a bad descriptor
    assert _batch_rc([five_one], 6, 7, 0)[0] == -2
    # a frame whose sequence changes: frames of the 3.0 stream behind frames of the 5.1 stream; and a frame whose sequence is not
    # the one of its channel_config (the 3.0 stream's frame with the header field rewritten to 5)
    lib = decoder.load_host_library()
    elems, n, used, p = (decoder.CoreFrame * 4)(), ctypes.c_int32(), ctypes.c_size_t(), ctypes.c_void_p()
    lib.xaac_parser_create(ctypes.byref(p))
    assert lib.xaac_parse_adts_frame_mc(p, five_one, len(five_one), 2, elems, 4, ctypes.byref(n), ctypes.byref(used)) == 0 and n.value == 4
    first = used.value
    assert lib.xaac_parse_adts_frame_mc(p, three, len(three), 2, elems, 4, ctypes.byref(n), ctypes.byref(used)) == UNSUPPORTED
    assert lib.xaac_parse_core_tools_side_mc(p, 0, (ctypes.c_uint8 * decoder.CORE_TOOLS_SIDE_BYTES)()) == -2   # no frame delivered
    rest = five_one[first:]
    assert lib.xaac_parse_adts_frame_mc(p, rest, len(rest), 2, elems, 4, ctypes.byref(n), ctypes.byref(used)) == 0   # the stream goes on
    assert lib.xaac_parse_adts_frame_mc(p, five_one, len(five_one), 2, elems, 3, ctypes.byref(n), ctypes.byref(used)) == -2   # cap too small
    lib.xaac_parser_destroy(p)
    p = ctypes.c_void_p()
    lib.xaac_parser_create(ctypes.byref(p))
    bad = bytearray(three)
    bad[2], bad[3] = (bad[2] & 0xfe) | 1, (bad[3] & 0x3f) | 0x40          # channel_config 5
    assert lib.xaac_parse_adts_frame_mc(p, bytes(bad), len(bad), 2, elems, 4, ctypes.byref(n), ctypes.byref(used)) == UNSUPPORTED
    lib.xaac_parser_destroy(p)
    # lists that mix configurations are refused before anything is parsed
    with pytest.raises(ValueError, match="channel configurations"):
        decoder.BatchParser([five_one, three])


def test_damaged_multichannel_streams_are_memory_safe(tmp_path):
    """tests/fuzz/fuzz_parser_mc.cpp with the host sources under ASan + UBSan: the committed 5.1 stream and truncated, bit-flipped,
    randomised and spliced copies of it through xaac_parse_adts_frame_mc and the batch; a stand-alone program, nothing is
    loaded into Python"""
    host = os.path.join(ROOT, "libxaac_amd", "host")
    exe = str(tmp_path / "fuzz_parser_mc")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "fuzz_parser_mc.cpp")] + [os.path.join(host, f) for f in ("xaac_parse.cpp", "aac_core.cpp", "sbr_side.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fwrapv", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", *srcs, "-o", exe, "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, os.path.join(mc.WIDE, "mc6_aot2.aac"), "4242", "240"], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-300:], p.stderr[-3000:])
    assert "frames parsed" in p.stdout and "frames parsed 0," not in p.stdout
