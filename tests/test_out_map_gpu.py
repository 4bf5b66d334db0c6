"""The output stage on the GPU: the mapped limiter call, the mapped multichannel hand-offs and the limiter-off hand-off against the
CPU twin applied to the unmapped calls' PCM; the command line decoder and decode_streams with -downmix:1 / -dmix:1 / -tostereo:1 /
-peak_limiter_off:1 against the reference decoder's files and the restatement of the unflagged decode."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mc_sbr_cases as mcs  # noqa: E402
import multichannel_cases as mc  # noqa: E402
import out_map_cases as oc  # noqa: E402

CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import libxaac_amd
    c = libxaac_amd.XaacContext(0)
    yield c
    c.close()


def _twin(kind, n_ch, pcm):
    import libxaac_amd
    from libxaac_amd import decoder
    return decoder.out_map_apply_host(libxaac_amd.out_map(kind, n_ch), pcm)


# ---- kernel level -------------------------------------------------------------------------------------------------------------

LIMITER_CASES = [(3, "downmix", True), (4, "downmix", True), (5, "downmix", True), (6, "downmix", True), (4, "downmix", False),
                 (6, "downmix", False), (2, "mono", False), (2, "mono_dup", False), (2, "mono", True), (1, "dup", False)]


def _limiter_frames(rng, n, n_ch, planar):
    """two chained frames of WORD32 samples, the first half of each quiet and the second loud enough for the limiter (the scaled
    magnitude passes 2^31), and qshift_adj differing per channel"""
    q = rng.integers(1, 4, (n, n_ch)).astype(np.int8)
    frames = []
    for _ in range(2):
        x = rng.integers(-(1 << 20), 1 << 20, (n, 1024, n_ch)).astype(np.int64)
        x[:, 512:] = rng.integers(-(1 << 31), 1 << 31, (n, 512, n_ch)) * (rng.random((n, 512, 1)) < 0.3)
        x = x.astype(np.int32)
        frames.append(np.ascontiguousarray(x.transpose(0, 2, 1)) if planar else x)
    return q, frames


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("n_ch,kind,planar", LIMITER_CASES)
def test_mapped_limiter_equals_the_twin_of_the_unmapped_call(ctx, n_ch, kind, planar, n):
    """xaac_peak_limiter_process_map_batch over two chained frames: pcm16 is the CPU twin of the unmapped call's pcm16, the samples and
    the limiter states are bit-equal to the unmapped call's, nothing is written behind the mapped block"""
    import libxaac_amd
    import torch
    rng = np.random.default_rng(1000 * n_ch + 10 * n + len(kind) + planar)
    q, frames = _limiter_frames(rng, n, n_ch, planar)
    m = libxaac_amd.out_map(kind, n_ch)
    out_ch = libxaac_amd.out_map_channels(m, n_ch)
    st0, _ = libxaac_amd.peak_limiter_init(n_ch, 48000)
    states = [torch.from_numpy(np.tile(np.frombuffer(bytes(st0), np.uint8), (n, 1)).copy()).cuda() for _ in range(2)]
    ws = torch.zeros(ctx.peak_limiter_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    qd = torch.from_numpy(q.reshape(-1).copy()).cuda()
    engaged = False
    for x in frames:
        a, b = torch.from_numpy(x.reshape(-1).copy()).cuda(), torch.from_numpy(x.reshape(-1).copy()).cuda()
        plain = torch.zeros(n * 1024 * n_ch, dtype=torch.int16, device="cuda")
        mapped = torch.full((n * 1024 * out_ch + 64,), 0x1234, dtype=torch.int16, device="cuda")
        ctx.peak_limiter_process_batch(a, qd, states[0], n_ch, ws, pcm16=plain, planar=planar)
        ctx.sync()
        ctx.peak_limiter_process_map_batch(b, qd, states[1], n_ch, ws, mapped[:n * 1024 * out_ch], m, planar=planar)
        assert ctx.last_launch() == {"grid": n, "block": 64, "lds_bytes": 12288}
        ctx.sync()
        got = mapped.cpu().numpy()
        assert (got[n * 1024 * out_ch:] == 0x1234).all()
        want = _twin(kind, n_ch, plain.cpu().numpy().reshape(n * 1024, n_ch))
        assert np.array_equal(got[:n * 1024 * out_ch].reshape(n * 1024, out_ch), want)
        assert torch.equal(a, b) and torch.equal(states[0], states[1])
        engaged = engaged or libxaac_amd.LimiterState.from_buffer_copy(states[0][0].cpu().numpy().tobytes()).min_gain < 1.0
    assert engaged   # the loud halves did ask for limiting


def test_mapped_limiter_honours_status(ctx):
    """a stream whose state does not fit the batch is refused (status -1) and its mapped output is left untouched"""
    import libxaac_amd
    import torch
    n, n_ch = 3, 6
    rng = np.random.default_rng(5)
    q, frames = _limiter_frames(rng, n, n_ch, True)
    st0, _ = libxaac_amd.peak_limiter_init(n_ch, 48000)
    bad, _ = libxaac_amd.peak_limiter_init(2, 48000)       # a stereo stream's state in a 5.1 batch
    rows = np.tile(np.frombuffer(bytes(st0), np.uint8), (n, 1)).copy()
    rows[1] = np.frombuffer(bytes(bad), np.uint8)
    state = torch.from_numpy(rows).cuda()
    ws = torch.zeros(ctx.peak_limiter_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    x = torch.from_numpy(frames[0].reshape(-1).copy()).cuda()
    pcm = torch.full((n * 1024 * 2,), 0x1234, dtype=torch.int16, device="cuda")
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ctx.peak_limiter_process_map_batch(x, torch.from_numpy(q.reshape(-1).copy()).cuda(), state, n_ch, ws, pcm,
                                       libxaac_amd.out_map("downmix", n_ch), status=status, planar=True)
    ctx.sync()
    assert status.cpu().tolist() == [0, -1, 0]
    got = pcm.cpu().numpy().reshape(n, 2048)
    assert (got[1] == 0x1234).all() and not (got[0] == 0x1234).all() and not (got[2] == 0x1234).all()
    assert np.array_equal(x.cpu().numpy().reshape(n, -1)[1], frames[0].reshape(n, -1)[1])
    assert np.array_equal(state[1].cpu().numpy(), rows[1])


def test_mapped_calls_refuse_what_no_kernel_takes(ctx):
    import libxaac_amd
    import torch
    n = 1
    ws = torch.zeros(ctx.peak_limiter_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    for n_ch, kind in ((2, "downmix"), (6, "mono"), (2, "dup"), (1, "mono")):
        st0, _ = libxaac_amd.peak_limiter_init(n_ch, 48000)
        state = torch.from_numpy(np.frombuffer(bytes(st0), np.uint8).copy()[None]).cuda()
        x = torch.zeros(1024 * n_ch, dtype=torch.int32, device="cuda")
        q = torch.zeros(n_ch, dtype=torch.int8, device="cuda")
        pcm = torch.zeros(1024, dtype=torch.int16, device="cuda")
        with pytest.raises(libxaac_amd.XaacError):
            ctx.peak_limiter_process_map_batch(x, q, state, n_ch, ws, pcm, libxaac_amd.out_map(kind, 6))
        with pytest.raises(libxaac_amd.XaacError):
            ctx.pcm16_scale_adjust_map_batch(x, q, n_ch, pcm, libxaac_amd.out_map(kind, 6))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("n_ch", [3, 4, 5, 6])
def test_mapped_multichannel_hand_offs_equal_the_twin(ctx, n_ch, n):
    """xaac_mc_pcm16_from_float_map_batch and its int16 twin: 2048 samples a plane, a stride above 2048; the stereo block is the CPU
    twin of the unmapped call's block"""
    import libxaac_amd
    import torch
    stride, slot = 2048 + 256, mc.LAYOUT[n_ch][1]
    rng = np.random.default_rng(77 * n_ch + n)
    m = libxaac_amd.out_map("downmix", n_ch)
    flt = (rng.standard_normal((n * n_ch, stride)) * 20000.0).astype(np.float32)      # some of it beyond the clamp
    flt[:, :8] = [-32768.0, -32769.5, 32767.0, 40000.0, -0.9, 0.9, -32767.9, 1.0]
    i16 = rng.integers(-32768, 32768, (n * n_ch, stride)).astype(np.int16)
    i16[:, :4] = -32768
    for planes_h in (flt, i16):
        planes = torch.from_numpy(planes_h.copy()).cuda()
        plain = torch.zeros(n * 2048 * n_ch, dtype=torch.int16, device="cuda")
        mapped = torch.full((n * 2048 * 2 + 64,), 0x1234, dtype=torch.int16, device="cuda")
        ctx.mc_pcm16_from_planes(planes, plain, slot, stride=stride)
        ctx.mc_pcm16_from_planes(planes, mapped[:n * 2048 * 2], slot, stride=stride, out_map=m)
        ctx.sync()
        got = mapped.cpu().numpy()
        assert (got[n * 2048 * 2:] == 0x1234).all()
        want = _twin("downmix", n_ch, plain.cpu().numpy().reshape(n * 2048, n_ch))
        assert np.array_equal(got[:n * 2048 * 2].reshape(n * 2048, 2), want), planes_h.dtype


SCALE_CASES = [(1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (3, "downmix"), (4, "downmix"), (5, "downmix"),
               (6, "downmix"), (2, "mono"), (2, "mono_dup"), (1, "dup")]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("n_ch,kind", SCALE_CASES)
def test_limiter_off_hand_off_equals_scale_adjust_round16_and_the_twin(ctx, n_ch, kind, n):
    """xaac_pcm16_scale_adjust_map_batch: planar and interleaved WORD32 with qshift_adj 0, 1 and differing per channel, against
    ixheaacd_scale_adjust (a wrapping shift) + ixheaac_round16 in numpy and the CPU twin behind it"""
    import libxaac_amd
    import torch
    rng = np.random.default_rng(13 * n_ch + n + (len(kind) if kind else 0))
    L = 1024
    x = rng.integers(-(1 << 31), 1 << 31, (n, L, n_ch)).astype(np.int64)
    x[:, :200] >>= 12                                                       # quiet words too
    x[:, 0], x[:, 1], x[:, 2] = 0x7fffffff, -0x80000000, 0x7fff8000         # round16's saturating add
    m = libxaac_amd.out_map(kind, n_ch) if kind else None
    out_ch = libxaac_amd.out_map_channels(m, n_ch) if kind else n_ch
    for q in (np.zeros((n, n_ch), np.int8), np.ones((n, n_ch), np.int8), rng.integers(0, 6, (n, n_ch)).astype(np.int8)):
        v = (x << q[:, None, :].astype(np.int64)).astype(np.int32).astype(np.int64)      # wraps
        plain = (np.minimum(v + 0x8000, 0x7fffffff) >> 16).astype(np.int16).reshape(n * L, n_ch)
        want = _twin(kind, n_ch, plain) if kind else plain
        for planar in (False, True):
            xs = x.astype(np.int32)
            xs = np.ascontiguousarray(xs.transpose(0, 2, 1)) if planar else xs
            xd = torch.from_numpy(xs.reshape(-1).copy()).cuda()
            pcm = torch.full((n * L * out_ch + 64,), 0x1234, dtype=torch.int16, device="cuda")
            ctx.pcm16_scale_adjust_map_batch(xd, torch.from_numpy(q.reshape(-1).copy()).cuda(), n_ch, pcm[:n * L * out_ch], m, planar=planar)
            assert ctx.last_launch() == {"grid": (n * L + 255) // 256, "block": 256, "lds_bytes": 0}  # a lane per (stream, sample)
            ctx.sync()
            got = pcm.cpu().numpy()
            assert (got[n * L * out_ch:] == 0x1234).all()
            assert np.array_equal(got[:n * L * out_ch].reshape(n * L, out_ch), want), (planar, q[0].tolist())
            assert np.array_equal(xd.cpu().numpy(), xs.reshape(-1))                 # the samples are read only


# ---- end to end ---------------------------------------------------------------------------------------------------------------

_ours = {}


def _decode(name, *flags):
    """the bytes libxaac_amd/xaacdec_amd writes for stream `name` with `flags`, decoded once per test run"""
    key = (name,) + flags
    if key not in _ours:
        assert os.path.exists(CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
        out = os.path.join(mc._tmp(), "ours_%d.wav" % len(_ours))
        p = subprocess.run([CLI, "-ifile:" + oc.stream_path(name), "-ofile:" + out, "-quiet", *flags], capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, (key, p.stderr[-500:])
        _ours[key] = open(out, "rb").read()
    return _ours[key]


def _mcsbr(name):
    return ("-mcsbr:1",) if name == "mc6_aot5" else ()


@pytest.mark.parametrize("name,flags", [
    ("lc_aot2_16k_mono", ("-tostereo:1",)),
    ("mix_aot2_64k", ("-peak_limiter_off:1",)),
    ("lc_aot2_16k_mono", ("-peak_limiter_off:1",)),
    ("mc6_aot2", ("-peak_limiter_off:1",)),
    ("lc_aot2_16k_mono", ("-peak_limiter_off:1", "-tostereo:1")),
    ("mix_aot2_64k", ("-tostereo:1",)),
    ("mc6_aot2", ("-tostereo:1",)),
    ("mix_aot5_48k", ("-tostereo:1",)),
    ("mix_aot5_48k", ("-peak_limiter_off:1",)),
    ("mc6_aot5", ("-peak_limiter_off:1",)),
    ("mc6_aot5", ("-tostereo:1",)),
    ("lc_aot2_16k_mono", ("-dmix:1",)),
])
def test_files_equal_the_reference_where_its_file_is_self_consistent(name, flags):
    """-tostereo:1, -peak_limiter_off:1 and the no-op cases: the reference's bytes"""
    assert _decode(name, *_mcsbr(name), *flags) == mcs.reference_wav(oc.stream_path(name), *flags)


@pytest.mark.parametrize("lim_off", [False, True], ids=["limiter", "limiter_off"])
@pytest.mark.parametrize("name", oc.MC_STREAMS)
def test_downmix_file(name, lim_off):
    """-downmix:1: a 44-byte stereo header, as many samples as the unflagged decode, every one of them the restatement of our own
    unflagged payload; and the reference's -downmix:1 payload where that is mixed data (6 samples early, up to the flush)"""
    off = ("-peak_limiter_off:1",) if lim_off else ()
    hdr, ch, rate, pay = oc.wav_parts(_decode(name, *_mcsbr(name), "-downmix:1", *off))
    phdr, pch, prate, plain = oc.wav_parts(_decode(name, *_mcsbr(name), *off))
    assert (hdr, ch, rate) == (44, 2, prate) and (phdr, pch) == (68, len(mc.LAYOUT[pch][1]))
    assert np.array_equal(pay, oc.restate(plain, "downmix", pch))
    span, n = oc.check_reference_downmix(name, lim_off, mixed=pay)
    assert n == len(pay) and span >= 0.99 * n


@pytest.mark.parametrize("tostereo", [False, True], ids=["dmix", "dmix_tostereo"])
def test_mono_mix_file(tostereo):
    flags = ("-dmix:1",) + (("-tostereo:1",) if tostereo else ())
    hdr, ch, rate, pay = oc.wav_parts(_decode("mix_aot2_64k", *flags))
    _, _, prate, plain = oc.wav_parts(_decode("mix_aot2_64k"))
    assert (hdr, ch, rate) == (44, 2 if tostereo else 1, prate)
    assert np.array_equal(pay, oc.restate(plain, "mono_dup" if tostereo else "mono"))
    assert oc.check_reference_dmix(tostereo, mixed=pay) == (76560, 76800)


def test_copies_verify_list_and_two_shards(tmp_path):
    """-copies:3 -verify compares mapped blocks; a two-file -ilist of 5.1 streams; -gpus:2 -wrap_devices: the same files"""
    want = _decode("mc6_aot2", "-downmix:1")
    assert _decode("mc6_aot2", "-downmix:1", "-copies:3", "-verify") == want
    assert _decode("mc6_aot2", "-downmix:1", "-copies:4", "-verify", "-gpus:2", "-wrap_devices") == want
    assert _decode("mc6_aot2", "-downmix:1", "-peak_limiter_off:1", "-copies:3", "-verify") == _decode("mc6_aot2", "-downmix:1", "-peak_limiter_off:1")
    data = mc.stream("mc6_aot2")
    frames = mcs.adts_frames(data)
    short = str(tmp_path / "short.aac")
    open(short, "wb").write(data[:frames[len(frames) // 2][1]])         # a stream that ends first
    lst, odir = str(tmp_path / "list.txt"), str(tmp_path / "out")
    os.mkdir(odir)
    open(lst, "w").write(mc.stream_path("mc6_aot2") + "\n" + short + "\n")
    p = subprocess.run([CLI, "-ilist:" + lst, "-odir:" + odir, "-quiet", "-downmix:1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-500:]
    assert open(os.path.join(odir, "mc6_aot2.wav"), "rb").read() == want
    p = subprocess.run([CLI, "-ifile:" + short, "-ofile:" + str(tmp_path / "s.wav"), "-quiet"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-500:]
    _, _, _, plain = oc.wav_parts(open(str(tmp_path / "s.wav"), "rb").read())
    hdr, ch, _, pay = oc.wav_parts(open(os.path.join(odir, "short.wav"), "rb").read())
    assert (hdr, ch) == (44, 2) and np.array_equal(pay, oc.restate(plain, "downmix", 6))


@pytest.mark.parametrize("name,out_map,limiter,flags", [
    ("mc6_aot2", "downmix", True, ("-downmix:1",)),
    ("mc4_32k", "downmix", False, ("-downmix:1", "-peak_limiter_off:1")),
    ("mc6_aot5", "downmix", True, ("-mcsbr:1", "-downmix:1")),
    ("mix_aot2_64k", "mono", True, ("-dmix:1",)),
    ("mix_aot2_64k", "mono_dup", False, ("-dmix:1", "-tostereo:1", "-peak_limiter_off:1")),
    ("lc_aot2_16k_mono", "dup", True, ("-tostereo:1",)),
    ("lc_aot2_16k_mono", "dup", False, ("-tostereo:1", "-peak_limiter_off:1")),
    ("mix_aot2_64k", None, False, ("-peak_limiter_off:1",)),
    ("mc6_aot2", None, False, ("-peak_limiter_off:1",)),
    ("mix_aot5_48k", "dup", False, ("-tostereo:1", "-peak_limiter_off:1")),
])
def test_decode_streams_equals_the_command_line_decoder(name, out_map, limiter, flags):
    from libxaac_amd import decoder
    data = open(oc.stream_path(name), "rb").read()
    sbr = name in ("mc6_aot5", "mix_aot5_48k")
    pcm, rate = decoder.decode_streams([data, data], out_map=out_map, limiter=limiter, esbr=sbr, mc_sbr=name == "mc6_aot5")
    _, ch, wrate, pay = oc.wav_parts(_decode(name, *flags))
    assert rate == wrate
    for x in pcm:
        assert x.shape[1] == ch and np.array_equal(x, pay)


def test_decode_streams_refusals():
    from libxaac_amd import decoder
    st = open(oc.stream_path("mix_aot2_64k"), "rb").read()
    he = open(oc.stream_path("mix_aot5_48k"), "rb").read()
    for data, kw in ((st, dict(out_map="downmix")), (he, dict(out_map="mono", esbr=True)), (mc.stream("mc6_aot2"), dict(out_map="mono_dup")),
                     (st, dict(out_map="stereo"))):
        with pytest.raises(ValueError):
            decoder.decode_streams([data], **kw)


@pytest.mark.parametrize("name,flags", [("mix_aot2_64k", ("-downmix:1",)), ("mc6_aot2", ("-dmix:1",)), ("mix_aot5_48k", ("-dmix:1",)),
                                        ("mc6_aot2", ("-downmix:1", "-dmix:1"))])
def test_refusals_leave_no_file_on_a_gpu_box_either(tmp_path, name, flags):
    out = str(tmp_path / "o.wav")
    p = subprocess.run([CLI, "-ifile:" + oc.stream_path(name), "-ofile:" + out, "-quiet", *flags], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "is not supported" in p.stderr and not os.path.exists(out)
