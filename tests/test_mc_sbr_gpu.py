"""Multichannel HE-AAC (ADTS channel_config 3 .. 6 with an SBR payload per channel element) from the bitstream to the WAV file on
the GPU, behind the opt-in switch (xaacdec_amd -mcsbr:1, decode_streams(mc_sbr=True)): the committed 5.1 stream and one stream per
channel_config 3, 4, 5 that oracle/_ref/xaacenc -aot:5 makes on the spot, against the file oracle/_ref/xaacdec writes with the same
flags -- byte for byte, the 68-byte header included; what stays refused; and the element-strided hand-offs alone against numpy
models (bit-exact: their arithmetic is integer conversion, clamping, truncation and a permutation).

-esbr:0 (the fixed-point tools, low-power SBR on every element) is not built for such streams: it stays refused under -mcsbr:1 with
a message naming the flag, and the tests of that flag assert the refusal."""
import os
import subprocess

import numpy as np
import pytest

import mc_sbr_cases as cases
import multichannel_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")

pytestmark = pytest.mark.gpu


def cli(path, out, *flags):
    assert os.path.exists(CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
    return subprocess.run([CLI, "-ifile:" + path, "-ofile:" + out, "-quiet", "-mcsbr:1", *flags], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flags", [(), ("-copies:3", "-verify"), ("-gputools:1",)], ids=["default", "copies3", "gputools"])
@pytest.mark.parametrize("name", cases.NAMES)
def test_wav_file_equals_the_reference_decoders(name, flags, tmp_path):
    path = cases.stream_path(name)
    want = cases.reference_wav(path)
    out = str(tmp_path / "out.wav")
    p = cli(path, out, *flags)
    assert p.returncode == 0, p.stderr[-500:]
    got = open(out, "rb").read()
    config = mc.channel_config(cases.stream(name))
    assert int.from_bytes(want[22:24], "little") == config and int.from_bytes(want[40:44], "little") == mc.LAYOUT[config][2]
    assert got[:mc.WAV_HEADER_BYTES] == want[:mc.WAV_HEADER_BYTES]          # extensible header: channels, doubled rate, mask, sizes
    assert got == want


@pytest.mark.parametrize("name", cases.NAMES)
def test_esbr_0_stays_refused(name, tmp_path):
    """the reference decodes these streams with -esbr:0 too (low-power SBR on every element, mono ones included); this decoder
    does not yet: a message that names the flag and a non-zero exit code, no file"""
    path, out = cases.stream_path(name), str(tmp_path / "no.wav")
    assert len(cases.reference_wav(path, "-esbr:0")) > len(cases.reference_wav(path))      # (the reference writes the first frame there)
    p = cli(path, out, "-esbr:0")
    assert p.returncode != 0 and "-esbr:0" in p.stderr and "-mcsbr:1" in p.stderr and not os.path.exists(out)


def test_a_list_of_two_different_streams(tmp_path):
    """-ilist / -odir: the committed stream and its first 12 frames as a second file in one batch: one runs dry first"""
    whole = cases.stream("mc6_aot5")
    short = str(tmp_path / "short.aac")
    open(short, "wb").write(whole[:cases.adts_frames(whole)[11][1]])
    lst, odir = str(tmp_path / "list.txt"), str(tmp_path / "out")
    os.makedirs(odir)
    open(lst, "w").write(cases.stream_path("mc6_aot5") + "\n" + short + "\n")
    for flags in ((), ("-gpus:2", "-wrap_devices")):     # (two shards, on one device where there is only one)
        p = subprocess.run([CLI, "-ilist:" + lst, "-odir:" + odir, "-quiet", "-mcsbr:1", *flags], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (flags, p.stderr[-500:])
        assert open(os.path.join(odir, "mc6_aot5.wav"), "rb").read() == cases.reference_wav(cases.stream_path("mc6_aot5")), flags
        assert open(os.path.join(odir, "short.wav"), "rb").read() == cases.reference_wav(short), flags
        os.remove(os.path.join(odir, "mc6_aot5.wav")), os.remove(os.path.join(odir, "short.wav"))


@pytest.mark.parametrize("name", cases.NAMES)
def test_decode_streams_gives_the_same_pcm(name):
    from libxaac_amd import decoder
    data = cases.stream(name)
    want = cases.reference_wav(cases.stream_path(name))
    pcm, rate = decoder.decode_streams([data, data], esbr=True, mc_sbr=True)
    assert rate == int.from_bytes(want[24:28], "little")
    for x in pcm:
        assert x.shape[1] == mc.channel_config(data)
        assert np.ascontiguousarray(x).tobytes() == want[mc.WAV_HEADER_BYTES:]
    with pytest.raises(ValueError, match="esbr=False"):                      # the fixed-point tools: refused, see above
        decoder.decode_streams([data], esbr=False, mc_sbr=True)


def _with_header_field(data, sr_index=None, channel_config=None):
    """the stream with a field of every ADTS header rewritten"""
    b = bytearray(data)
    for at, _ in cases.adts_frames(data):
        if sr_index is not None:
            b[at + 2] = (b[at + 2] & 0xc3) | (sr_index << 2)
        if channel_config is not None:
            b[at + 2], b[at + 3] = (b[at + 2] & 0xfe) | (channel_config >> 2), (b[at + 3] & 0x3f) | ((channel_config & 3) << 6)
    return bytes(b)


def test_what_stays_refused(tmp_path):
    """each with a message of its own and a non-zero exit code / a ValueError, never audio"""
    from libxaac_amd import decoder
    he, out = cases.stream_path("mc6_aot5"), str(tmp_path / "no.wav")
    p = cli(he, out, "-esbr_hq:1")
    assert p.returncode != 0 and "-esbr_hq:1" in p.stderr and not os.path.exists(out)
    # a core rate above 24 kHz: the output rate would ask for the down-sampled bank (the 5.0 stream's headers rewritten to 48 kHz: its
    # first frame, which is all that is looked at before the refusal, parses with that rate's band tables too)
    fast = str(tmp_path / "fast.aac")
    open(fast, "wb").write(_with_header_field(cases.stream("mc5_he_48k"), sr_index=3))
    p = cli(fast, out)
    assert p.returncode != 0 and "down-sampled" in p.stderr and not os.path.exists(out)
    with pytest.raises(ValueError, match="down-sampled"):
        decoder.decode_streams([open(fast, "rb").read()], esbr=True, mc_sbr=True)
    # channel_config 7, as before
    seven = str(tmp_path / "seven.aac")
    open(seven, "wb").write(_with_header_field(cases.stream("mc6_aot5"), channel_config=7))
    p = cli(seven, out)
    assert p.returncode != 0 and not os.path.exists(out)
    # ... and without the switch everything is as it was
    p = subprocess.run([CLI, "-ifile:" + he, "-ofile:" + out, "-quiet"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "multichannel SBR" in p.stderr and not os.path.exists(out)


# ---- the hand-offs alone ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import libxaac_amd
    c = libxaac_amd.XaacContext(0)
    yield c
    c.close()


def _planes(rng, rows, stride, sentinel):
    x = np.full((rows, stride), sentinel, np.float32)
    v = (rng.standard_normal((rows, 2048)) * 20000.0).astype(np.float32)
    edge = np.array([32767.0, 32766.5, 32767.5, 32768.0, -32768.0, -32768.5, -32767.5, -32769.0, 0.9, -0.9, 0.0, -0.0, np.inf, -np.inf,
                     1e30, -1e30, 32766.99, -32767.99], np.float32)
    at = rng.integers(0, 2048, (rows, 4 * len(edge)))
    for r in range(rows):
        v[r, at[r]] = np.tile(edge, 4)
    v[:, :len(edge)] = edge
    x[:, :2048] = v
    return x


@pytest.mark.parametrize("stride", [2048, 2048 + 6])
@pytest.mark.parametrize("n_ch", [3, 4, 5, 6])
def test_planes_to_block_vs_numpy(ctx, n_ch, stride):
    """xaac_mc_pcm16_from_float_batch (ixheaacd_samples_sat_mc: clamp to [-32768, 32767], truncate towards zero) and its int16 twin:
    3 streams, plane c to output channel slot[c], values at and around the clamping points, +-0.9, +-inf and random floats; a
    stride larger than a plane; sentinel words behind the block and behind every plane"""
    import torch
    n, slot = 3, mc.LAYOUT[n_ch][1]
    rng = np.random.default_rng(31 * n_ch + stride)
    x = _planes(rng, n * n_ch, stride, 12345.0)
    want = np.zeros((n, 2048, n_ch), np.int16)
    sat = np.trunc(np.clip(x[:, :2048].astype(np.float64), -32768.0, 32767.0)).astype(np.int16).reshape(n, n_ch, 2048)
    for c, to in enumerate(slot):
        want[:, :, to] = sat[:, c]
    guard = 64
    for planes_h, want_h in ((x, want), (None, None)):
        if planes_h is None:      # the int16 twin: the planes as they are
            planes_h = np.full((n * n_ch, stride), 0x3abc, np.int16)
            planes_h[:, :2048] = rng.integers(-32768, 32768, (n * n_ch, 2048))
            want_h = np.zeros((n, 2048, n_ch), np.int16)
            for c, to in enumerate(slot):
                want_h[:, :, to] = planes_h.reshape(n, n_ch, stride)[:, c, :2048]
        planes = torch.from_numpy(planes_h.copy()).cuda()
        pcm_all = torch.full((n * 2048 * n_ch + guard,), 0x1234, dtype=torch.int16, device="cuda")
        ctx.mc_pcm16_from_planes(planes, pcm_all[:n * 2048 * n_ch], slot, stride=stride)
        ctx.sync()
        got = pcm_all.cpu().numpy()
        assert (got[n * 2048 * n_ch:] == 0x1234).all()
        assert np.array_equal(got[:n * 2048 * n_ch].reshape(n, 2048, n_ch), want_h)
        assert np.array_equal(planes.cpu().numpy().view(np.int32 if planes_h.dtype == np.float32 else np.int16),
                              planes_h.view(np.int32 if planes_h.dtype == np.float32 else np.int16))      # the planes are read only


def _reference_block_conversion(out32, qadj, config):
    """what the reference does to a frame's block of `config` channels between the core decoder and the SBR calls, restated
    literally on one piece of memory: every element's IMDCT writes WORD32 samples at stride total_channels from the element's
    slot (aacdecoder.c:988-994), ixheaacd_allocate_sbr_scr converts them to WORD16 IN PLACE, channel after channel, channel j with
    qshift_adj[j] of the frame (api.c:351-359), and api.c:3414-3434 reads the WORD16 samples as floats.  -> core [n_ch, 1024] in
    bitstream order"""
    elements, slot, _ = mc.LAYOUT[config]
    total = config
    mem = np.zeros(1024 * total, np.int32)
    w16 = mem.view(np.int16)
    core = np.zeros((total, 1024), np.float32)
    ch = 0
    for e in elements:
        n = 2 if e == 1 else 1
        s = slot[ch]
        for j in range(n):
            mem[s + j + total * np.arange(1024)] = out32[ch + j]
        for j in range(n):
            q = int(qadj[j])                                  # the j-th channel the frame decoded
            for i in range(1024):
                v = int(mem[s + total * i + j])
                v = max(min(v << q, 2147483647), -2147483648)             # shl32_sat
                w16[s + total * i + j] = np.int16(min(v + 0x8000, 2147483647) >> 16)   # round16
        for j in range(n):
            core[ch + j] = w16[s + j + total * np.arange(1024)]
        ch += n
    return core


@pytest.mark.parametrize("config", [3, 4, 5, 6])
def test_core_hand_in_vs_the_block_conversion(ctx, config):
    """xaac_mc_core_from_out32_batch against the in-place conversion restated on a block of memory: 3 streams, samples up to full
    scale (the shift saturates), every qshift_adj 0 .. 3 differing between the channels; sentinel words behind the planes"""
    import torch
    n = 3
    rng = np.random.default_rng(700 + config)
    out32 = rng.integers(-(1 << 29), 1 << 29, (n, config, 1024)).astype(np.int32)
    out32[:, :, ::7] = rng.integers(-(1 << 31), (1 << 31) - 1, (n, config, 147)).astype(np.int32)
    out32[:, :, 5::64] >>= 14                                              # quiet samples: the halves that leak in dominate
    qadj = rng.integers(0, 4, (n, config)).astype(np.int8)
    want = np.stack([_reference_block_conversion(out32[i], qadj[i], config) for i in range(n)])
    guard = 32
    core_all = torch.full((n * config * 1024 + guard,), 777.0, dtype=torch.float32, device="cuda")
    core = core_all[:n * config * 1024].view(n * config, 1024)
    ctx.mc_core_from_out32(torch.from_numpy(out32.reshape(n * config, 1024)).cuda(), torch.from_numpy(qadj.reshape(-1)).cuda(), core, config)
    ctx.sync()
    got = core_all.cpu().numpy()
    assert (got[n * config * 1024:] == 777.0).all()
    assert np.array_equal(got[:n * config * 1024].reshape(n, config, 1024), want)
