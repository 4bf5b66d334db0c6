"""Multichannel AAC-LC (ADTS channel_config 3 .. 6) from the bitstream to the WAV file on the GPU: libxaac_amd/xaacdec_amd and
decode_streams on the committed 5.1 stream and on one stream per channel_config 3, 4, 5 that oracle/_ref/xaacenc makes on the
spot, against the file oracle/_ref/xaacdec writes -- byte for byte, the 68-byte WAVE_FORMAT_EXTENSIBLE header with its channel
mask included; the peak limiter alone on planar blocks of 3 .. 6 channels (the instantiations that hold all channels of a sample
in one lane) and of 8 (the generic path beside them) against the oracle; the same with the spectral tools on the GPU
(-gputools:1 / gpu_tools=True: one launch per element index); what is refused (an SBR payload in such a stream); and a stereo and a mono stream through the same helper, which keep their paths."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import limiter_cases as lc
import multichannel_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")

pytestmark = pytest.mark.gpu


def cli(path, out, *flags):
    assert os.path.exists(CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
    return subprocess.run([CLI, "-ifile:" + path, "-ofile:" + out, "-quiet", *flags], capture_output=True, text=True, timeout=300)


def decoded(path, tmp_path, *flags):
    out = str(tmp_path / "out.wav")
    p = cli(path, out, *flags)
    assert p.returncode == 0, p.stderr[-500:]
    return open(out, "rb").read()


@pytest.mark.parametrize("flags", [(), ("-copies:3", "-verify"), ("-gputools:1",), ("-gputools:1", "-copies:3", "-verify")],
                         ids=["one", "copies3", "gputools", "gputools_copies3"])
@pytest.mark.parametrize("name", mc.NAMES)
def test_wav_file_equals_the_reference_decoders(name, flags, tmp_path):
    path = mc.stream_path(name)
    want = mc.reference_wav(path)
    got = decoded(path, tmp_path, *flags)
    assert got[:mc.WAV_HEADER_BYTES] == want[:mc.WAV_HEADER_BYTES]          # extensible header: channels, rate, mask, sizes
    assert got == want


def test_a_list_of_two_different_streams(tmp_path):
    """-ilist / -odir: the committed 5.1 stream and a second one (its first 30 frames: another length, the limiter's tail flushed
    behind each) in one batch"""
    whole = mc.stream("mc6_aot2")
    pos = 0
    for _ in range(30):
        pos += ((whole[pos + 3] & 3) << 11) | (whole[pos + 4] << 3) | (whole[pos + 5] >> 5)
    short = str(tmp_path / "short.aac")
    open(short, "wb").write(whole[:pos])
    lst, odir = str(tmp_path / "list.txt"), str(tmp_path / "out")
    os.makedirs(odir)
    open(lst, "w").write(mc.stream_path("mc6_aot2") + "\n" + short + "\n")
    for flags in ((), ("-gputools:1",), ("-gpus:2", "-wrap_devices")):     # (two shards, on one device where there is only one)
        p = subprocess.run([CLI, "-ilist:" + lst, "-odir:" + odir, "-quiet", *flags], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (flags, p.stderr[-500:])
        assert open(os.path.join(odir, "mc6_aot2.wav"), "rb").read() == mc.reference_wav(mc.stream_path("mc6_aot2")), flags
        assert open(os.path.join(odir, "short.wav"), "rb").read() == mc.reference_wav(short), flags
        os.remove(os.path.join(odir, "mc6_aot2.wav")), os.remove(os.path.join(odir, "short.wav"))
    # a list that mixes channel configurations is refused up front
    open(lst, "w").write(mc.stream_path("mc6_aot2") + "\n" + mc.stream_path("mc5_48k") + "\n")
    p = subprocess.run([CLI, "-ilist:" + lst, "-odir:" + odir, "-quiet"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "different kinds" in p.stderr


@pytest.mark.parametrize("gpu_tools", [False, True], ids=["tools_in_parser", "gpu_tools"])
@pytest.mark.parametrize("name", mc.NAMES)
def test_decode_streams_gives_the_same_pcm(name, gpu_tools):
    from libxaac_amd import decoder
    data = mc.stream(name)
    want = mc.reference_wav(mc.stream_path(name))
    pcm, rate = decoder.decode_streams([data, data], gpu_tools=gpu_tools)
    assert rate == int.from_bytes(want[24:28], "little")
    for x in pcm:
        assert x.shape[1] == len(mc.LAYOUT[mc.channel_config(data)][1])
        assert np.ascontiguousarray(x).tobytes() == want[mc.WAV_HEADER_BYTES:]


def test_what_is_refused(tmp_path):
    """an SBR payload in a stream of more than two channels: a non-zero exit code and a message / a ValueError, never wrong
    audio; and a Python batch that mixes a multichannel stream with another kind, whichever comes first"""
    from libxaac_amd import decoder
    he = os.path.join(mc.WIDE, "mc6_aot5.aac")
    out = str(tmp_path / "no.wav")
    for flags in ((), ("-esbr:0",), ("-gputools:1",)):
        p = cli(he, out, *flags)
        assert p.returncode != 0 and "multichannel SBR" in p.stderr and not os.path.exists(out)
    with pytest.raises(ValueError, match="multichannel SBR"):
        decoder.decode_streams([open(he, "rb").read()])
    stereo = open(os.path.join(STREAMS, "mix_aot2_64k.aac"), "rb").read()
    for pair in ([stereo, mc.stream("mc6_aot2")], [mc.stream("mc6_aot2"), stereo]):
        with pytest.raises(ValueError, match="channel configurations"):
            decoder.decode_streams(pair)


@pytest.mark.parametrize("name", ["mix_aot2_64k", "lc_aot2_16k_mono"])
def test_stereo_and_mono_streams_keep_their_paths(name, tmp_path):
    """regression check: the same helper on a stereo and a mono AAC-LC stream, with the tools in the parser and on the GPU"""
    path = os.path.join(STREAMS, name + ".aac")
    want = mc.reference_wav(path)
    assert decoded(path, tmp_path) == want
    assert decoded(path, tmp_path, "-gputools:1") == want


def test_tools_kernel_with_the_multichannel_variant_equals_the_host_twin(ctx):
    """random but syntax-legal elements (full-scale, small and empty bands; TNS of order up to 12 in ~70 % of the channels, noise
    bands) marked as belonging to a stream of more than two channels -- the three-bit shift, the 32-bit TNS variant -- through
    xaac_aac_tools_process_batch against xaac_core_tools_apply_host, which the CPU tests pin to the reference decoder: spectra
    and noise generator states word for word.  Far denser tool use than the encoder's streams show."""
    import torch
    import aac_tools_cases as tc
    from libxaac_amd import decoder
    rng = np.random.default_rng(515)
    n = 512
    cases = [tc.random_element(rng) for _ in range(n)]
    side, spec, state = (np.stack([c[k] for c in cases]) for k in range(3))
    for i in range(n):
        s = decoder.CoreToolsSide.from_buffer(side[i])
        s.ch[0].wide = 1
        s.ch[1].wide = 1 if s.n_ch == 2 else 0
    t_spec, t_state = torch.from_numpy(spec.copy()).cuda(), torch.from_numpy(state.copy()).cuda()
    status = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    ctx.aac_tools_process_batch(t_spec, torch.from_numpy(side.copy()).cuda(), t_state, status)
    ctx.sync()
    got, got_state = t_spec.cpu().numpy(), t_state.cpu().numpy()
    assert not status.cpu().numpy().any()
    differs = 0
    for i in range(n):
        rc, want, want_state = tc.apply_host(spec[i], side[i], state[i])
        assert rc == 0
        n_ch = decoder.CoreToolsSide.from_buffer(side[i]).n_ch
        assert np.array_equal(got[i, :n_ch], want[:n_ch]), (i, np.nonzero(got[i, :n_ch] != want[:n_ch]))
        assert np.array_equal(got_state[i], want_state), i
        narrow = side[i].copy()
        s = decoder.CoreToolsSide.from_buffer(narrow)
        s.ch[0].wide = s.ch[1].wide = 0
        differs += not np.array_equal(tc.apply_host(spec[i], narrow, state[i])[1], want)
    assert differs > n // 2       # (the variant is not the two-channel arithmetic: the comparison above means something)


# ---- the limiter alone ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import libxaac_amd
    c = libxaac_amd.XaacContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("frame_len", [1024, 777])
@pytest.mark.parametrize("nch", [3, 4, 5, 6, 8])
def test_planar_limiter_vs_oracle(ctx, oracle, nch, frame_len):
    """planar = 1 over 16 streams, 6 chained frames with the state carried on the GPU; half of the streams loud (limiting active),
    half quiet (the frames the front kernel finishes itself), kinds changing from frame to frame: PCM16, the WORD32 block (planar,
    in place) and the whole state bit-exact against the oracle on the interleaved block; sentinel words behind the PCM and behind
    every stream's block"""
    import torch
    init, _, batch = lc.bind(oracle.lib, "xo")
    n, rate = 16, 48000
    rng = np.random.default_rng(100 * nch + frame_len)
    so = (lc.LimiterState * n)()
    for i in range(n):
        init(ctypes.byref(so[i]), nch, rate)
    st = torch.from_numpy(np.frombuffer(bytes(so), np.uint8).reshape(n, -1).copy()).cuda()
    ws = torch.zeros(ctx.peak_limiter_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    stride, guard = frame_len * nch + 8, 64
    loud, quiet = ("loud", "bursts", "steps", "decay", "fullscale"), ("quiet", "zeros")
    for frame in range(6):
        x = np.zeros((n, frame_len, nch), np.int32)
        for i in range(n):
            kinds = quiet if (i & 1) and frame != 3 else loud      # (frame 3: every stream limits, the quiet ones release after it)
            x[i] = lc.signal(rng, kinds[(i // 2 + frame) % len(kinds)], frame_len, nch).reshape(frame_len, nch)
        q = rng.integers(0 if frame == 4 else 1, 3, n * nch).astype(np.int8)
        xo = np.ascontiguousarray(x).reshape(-1).copy()
        po = np.zeros(n * frame_len * nch, np.int16)
        batch(n, frame_len, nch, xo.ctypes.data_as(lc.P32), frame_len * nch, q.ctypes.data_as(lc.P8), so, po.ctypes.data_as(lc.P16))
        planar = np.full((n, stride), 0x5a5a5a5a, np.int32)
        planar[:, :frame_len * nch] = x.transpose(0, 2, 1).reshape(n, -1)
        xs = torch.from_numpy(planar.reshape(-1)).cuda()
        pcm_all = torch.full((n * frame_len * nch + guard,), 0x1234, dtype=torch.int16, device="cuda")
        pcm = pcm_all[:n * frame_len * nch]       # (the wrapper checks the length: the sentinel words lie behind the view)
        status = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        ctx.peak_limiter_process_batch(xs, torch.from_numpy(q).cuda(), st, nch, ws, frame_len=frame_len, pcm16=pcm, stride=stride,
                                       status=status, planar=True)
        ctx.sync()
        assert not status.cpu().numpy().any()
        got = xs.cpu().numpy().reshape(n, stride)
        assert (got[:, frame_len * nch:] == 0x5a5a5a5a).all(), frame
        want = xo.reshape(n, frame_len, nch).transpose(0, 2, 1).reshape(n, -1)
        assert np.array_equal(got[:, :frame_len * nch], want), frame
        pg = pcm_all.cpu().numpy()
        assert (pg[n * frame_len * nch:] == 0x1234).all() and np.array_equal(pg[:n * frame_len * nch], po), frame
        raw = np.ascontiguousarray(st.cpu().numpy())
        sg = (lc.LimiterState * n)()
        ctypes.memmove(sg, raw.ctypes.data, raw.nbytes)
        for i in range(n):
            assert lc.state_view(sg[i]) == lc.state_view(so[i]), (frame, i)
