"""MPEG-4 dynamic range control on the GPU: xaac_drc_apply_batch (libxaac_amd/csrc/drc_kernel.hip) against the numpy int64 model
and the host twin on made-up rows, and on the reference-made records of tests/golden/drc_spec.npz; libxaac_amd/xaacdec_amd with
the reference's -drc_* flags against `oracle/_ref/xaacdec` with the same flags, byte for byte, on every committed DRC stream
(tests/golden/streams_drc), also with -gputools:1, with -copies:3 -verify and in a mixed -ilist; decode_streams(drc=...) and
decode_mixed(drc=...) against the same files.  Every comparison with the reference first asserts that its flagged output has the
full length and differs from its unflagged one."""
import json
import os
import subprocess
import wave

import numpy as np
import pytest
import torch

import drc_cases as dc
import libxaac_amd
from libxaac_amd import decoder

pytestmark = pytest.mark.gpu
PLAIN = os.path.join(dc.ROOT, "tests", "golden", "streams")
FLAG_IDS = ["cut1_boost1", "cut.5_boost.25_t96", "t96", "t124"]
FRAMES = 24


@pytest.fixture(scope="module")
def ctx():
    c = libxaac_amd.XaacContext(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _run_kernel(ctx, sides, specs, stride):
    """rows through xaac_drc_apply_batch at `stride` words per row (the words between the rows hold a sentinel) -> (spec rows,
    status, the words between the rows)"""
    n = len(sides)
    buf = np.full((n, stride), 0x5a5a5a5a, np.int32)
    buf[:, :1024] = specs
    d_spec = torch.from_numpy(buf).cuda()
    d_side = torch.from_numpy(np.ascontiguousarray(sides)).cuda()
    d_status = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    ctx.drc_apply_batch(d_spec, d_side, d_status, spec_stride=stride)
    torch.cuda.synchronize()
    out = d_spec.cpu().numpy()
    return out[:, :1024], d_status.cpu().numpy(), out[:, 1024:]


@pytest.mark.parametrize("stride", [1024, 2048])
@pytest.mark.parametrize("n", [1, 3, 130])
def test_kernel_equals_model_and_twin(ctx, n, stride):
    cases = dc.rows(n)
    sides, specs = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    got, status, between = _run_kernel(ctx, sides, specs, stride)
    assert np.all(between == 0x5a5a5a5a)
    assert ctx.last_launch() == {"grid": (n + 3) // 4, "block": 256, "lds_bytes": 0}
    for i, (what, row, spec) in enumerate(cases):
        twin = spec.copy()
        rc = decoder.drc_apply_host(row, twin)
        assert status[i] == rc == (0 if dc.row_ok(row) else -1), (i, what)
        assert np.array_equal(got[i], dc.model(row, spec)), (i, what, "kernel against the model")
        assert np.array_equal(got[i], twin), (i, what, "kernel against the twin")
        if rc or "identity" in what:
            assert np.array_equal(got[i], spec), (i, what, "left as it was")
    if n >= 13:
        assert (status == -1).sum() == 3


def test_kernel_argument_checks(ctx):
    side = torch.zeros((2, dc.WORDS), dtype=torch.int32, device="cuda")
    spec = torch.zeros(2 * 1024 + 8, dtype=torch.int32, device="cuda")
    for stride in (1020, 1026):   # below a row; no multiple of four
        with pytest.raises(libxaac_amd.XaacError):
            ctx.drc_apply_batch(spec, side, spec_stride=stride)
    with pytest.raises(libxaac_amd.XaacError):   # not 16-byte aligned
        ctx.drc_apply_batch(spec[1:], side, spec_stride=1024)
    ctx.drc_apply_batch(spec, side[:0])          # no rows: nothing to do


@pytest.mark.parametrize("k", range(len(dc.FLAG_SETS)), ids=FLAG_IDS)
def test_kernel_on_the_reference_records(ctx, k):
    """every stream's records of one flag set in one batch: the parser's rows and the reference's unflagged spectra in, the
    reference's flagged spectra out"""
    g = dc.gold()
    sides, specs, want = [], [], []
    for name in dc.NAMES:
        p = decoder.StreamParser(dc.stream(name), drc=dc.DRC_ARGS[k])
        for f in range(len(g[name + "_in"])):
            assert p.next()
            sides.append(p.drc_side())
            specs.append(g[name + "_in"][f])
            want.append(g["%s_out%d" % (name, k)][f])
        p.close()
    sides, specs, want = np.concatenate(sides), np.concatenate(specs), np.concatenate(want)
    assert len(sides) == len(specs) == 72 and not np.array_equal(specs, want)
    got, status, _ = _run_kernel(ctx, sides, specs, 1024)
    assert not status.any() and np.array_equal(got, want)


_ref_cache = {}


def reference(path, flags):
    """(PCM bytes, channels, rate) of `oracle/_ref/xaacdec` for one file and flag set, made once"""
    key = (path, tuple(flags))
    if key not in _ref_cache:
        dc.need("xaacdec")
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "ref.wav")
            subprocess.run([os.path.join(dc.REF, "xaacdec"), "-ifile:" + path, "-ofile:" + out, *flags], check=True, capture_output=True,
                           timeout=120)
            with wave.open(out) as w:
                _ref_cache[key] = (w.readframes(w.getnframes()), w.getnchannels(), w.getframerate())
    return _ref_cache[key]


def flagged_reference(name, flags):
    """the reference's output with the flags, after the check every case makes first: full length, and not the unflagged bytes"""
    path = os.path.join(dc.STREAMS, name + ".aac")
    plain, channels, _ = reference(path, ())
    want, ch, rate = reference(path, flags)
    assert ch == channels and len(plain) == FRAMES * 1024 * 2 * channels
    assert len(want) == len(plain) and want != plain
    return want, ch, rate


def run_cli(path, tmp_path, *flags):
    assert os.path.exists(dc.CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
    out = str(tmp_path / "ours.wav")
    p = subprocess.run([dc.CLI, "-ifile:" + path, "-ofile:" + out, *flags], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-500:]
    with wave.open(out) as w:
        return w.readframes(w.getnframes()), w.getnchannels(), w.getframerate(), json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("k", range(len(dc.FLAG_SETS)), ids=FLAG_IDS)
@pytest.mark.parametrize("name", dc.NAMES)
def test_wav_equals_the_reference_decoders(name, k, tmp_path):
    flags = dc.FLAG_SETS[k]
    want = flagged_reference(name, flags)
    path = os.path.join(dc.STREAMS, name + ".aac")
    assert run_cli(path, tmp_path, *flags)[:3] == want
    assert run_cli(path, tmp_path, "-gputools:1", *flags)[:3] == want
    pcm, ch, rate, info = run_cli(path, tmp_path, "-copies:3", "-verify", *flags)
    assert (pcm, ch, rate) == want and info["streams"] == 3 and info["mismatched_copies"] == 0


@pytest.mark.parametrize("name", dc.NAMES)
def test_without_a_flag_the_elements_change_nothing(name, tmp_path):
    path = os.path.join(dc.STREAMS, name + ".aac")
    want = reference(path, ())
    assert len(want[0]) == FRAMES * 1024 * 2 * want[1]
    assert run_cli(path, tmp_path)[:3] == want


def test_output_stage_flags_compose(tmp_path):
    """the limiter-off hand-off and the mono mix behind the DRC launch, against the reference with the same flags"""
    flags = dc.FLAG_SETS[1]
    flagged_reference("drc_stereo_2band", flags)
    path = os.path.join(dc.STREAMS, "drc_stereo_2band.aac")
    assert run_cli(path, tmp_path, "-peak_limiter_off:1", *flags)[:3] == reference(path, ("-peak_limiter_off:1",) + flags)
    mono = os.path.join(dc.STREAMS, "drc_mono_1band.aac")
    assert run_cli(mono, tmp_path, "-tostereo:1", *flags)[:3] == reference(mono, ("-tostereo:1",) + flags)


@pytest.mark.parametrize("gpus", [(), ("-gpus:2", "-wrap_devices")], ids=["one", "two_shards"])
def test_a_list_of_a_drc_stream_beside_plain_streams_of_other_kinds(gpus, tmp_path):
    """-ilist: DRC streams (stereo and mono at 48 kHz) beside a plain AAC-LC stream of another rate -- three groups side by side,
    the flags act on each; every WAV equals the reference's for that file alone with the same flags"""
    flags = dc.FLAG_SETS[1]
    files = [os.path.join(dc.STREAMS, "drc_stereo_excl.aac"), os.path.join(PLAIN, "lc_aot2_16k_mono.aac"),
             os.path.join(dc.STREAMS, "drc_mono_1band.aac"), os.path.join(dc.STREAMS, "drc_stereo_nonmono.aac")]
    flagged_reference("drc_stereo_excl", flags), flagged_reference("drc_mono_1band", flags)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(files) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([dc.CLI, "-ilist:" + str(lst), "-odir:" + str(out), *gpus, *flags], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-500:]
    for f in files:
        with wave.open(str(out / (os.path.basename(f)[:-4] + ".wav"))) as w:
            assert (w.readframes(w.getnframes()), w.getnchannels(), w.getframerate()) == reference(f, flags), f


def test_a_doubly_covered_channel_ends_that_stream_of_a_list_alone(tmp_path):
    good = os.path.join(dc.STREAMS, "drc_stereo_2band.aac")
    bad = tmp_path / "covered_twice.aac"
    bad.write_bytes(dc.with_two_elements_on_one_channel(dc.stream("drc_stereo_2band"), 5))
    flags = dc.FLAG_SETS[0]
    want = flagged_reference("drc_stereo_2band", flags)
    lst = tmp_path / "list.txt"
    lst.write_text(good + "\n" + str(bad) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([dc.CLI, "-ilist:" + str(lst), "-odir:" + str(out), *flags], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "the stream ends here" in p.stderr, p.stderr[-500:]
    with wave.open(str(out / "drc_stereo_2band.wav")) as w:
        assert w.readframes(w.getnframes()) == want[0]
    with wave.open(str(out / "covered_twice.wav")) as w:
        assert w.getnframes() == 5 * 1024


def _pcm_bytes(x):
    return np.ascontiguousarray(x).tobytes()


@pytest.mark.parametrize("gpu_tools", [False, True], ids=["host_tools", "gpu_tools"])
def test_decode_streams_gives_the_same_pcm(gpu_tools):
    k = 1
    names = ("drc_stereo_2band", "drc_stereo_16band", "drc_stereo_excl", "drc_stereo_nonmono")
    want = [flagged_reference(n, dc.FLAG_SETS[k]) for n in names]
    pcm, rate = decoder.decode_streams([dc.stream(n) for n in names], drc=dc.DRC_ARGS[k], gpu_tools=gpu_tools)
    for x, w, n in zip(pcm, want, names):
        assert (_pcm_bytes(x), x.shape[1], rate) == w, n
    mono = flagged_reference("drc_mono_1band", dc.FLAG_SETS[k])
    pcm, rate = decoder.decode_streams([dc.stream("drc_mono_1band")], drc=dc.DRC_ARGS[k], gpu_tools=gpu_tools, limiter=True)
    assert (_pcm_bytes(pcm[0]), pcm[0].shape[1], rate) == mono


def test_decode_streams_without_drc_is_unchanged():
    path = os.path.join(dc.STREAMS, "drc_stereo_2band.aac")
    pcm, rate = decoder.decode_streams([dc.stream("drc_stereo_2band")])
    assert (_pcm_bytes(pcm[0]), 2, rate) == reference(path, ())


def test_decode_mixed_applies_drc_to_every_lc_group():
    flags, arg = dc.FLAG_SETS[3], dc.DRC_ARGS[3]
    names = ("drc_mono_1band", "drc_stereo_2band")
    want = [flagged_reference(n, flags) for n in names]
    plain = os.path.join(PLAIN, "lc_aot2_16k_mono.aac")
    pcm, rates = decoder.decode_mixed([dc.stream(names[0]), open(plain, "rb").read(), dc.stream(names[1])], drc=arg)
    assert (_pcm_bytes(pcm[0]), pcm[0].shape[1], rates[0]) == want[0] and (_pcm_bytes(pcm[2]), pcm[2].shape[1], rates[2]) == want[1]
    assert (_pcm_bytes(pcm[1]), pcm[1].shape[1], rates[1]) == reference(plain, flags)


def test_refusals_leave_no_file(tmp_path):
    out = tmp_path / "o.wav"
    for src, flags in ((os.path.join(PLAIN, "mix_aot5_48k.aac"), ("-drc_cut_fac:1",)),
                       (os.path.join(dc.ROOT, "tests", "golden", "streams_wide", "mc6_aot2.aac"), ("-drc_boost_fac:1",)),
                       (os.path.join(dc.STREAMS, "drc_stereo_2band.aac"), ("-drc_heavy_comp:1",)),
                       (os.path.join(dc.STREAMS, "drc_stereo_2band.aac"), ("-drc_target_level:200",))):
        p = subprocess.run([dc.CLI, "-ifile:" + src, "-ofile:" + str(out), *flags], capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and not out.exists(), (src, flags)
    with pytest.raises(ValueError):
        decoder.decode_streams([open(os.path.join(PLAIN, "mix_aot5_48k.aac"), "rb").read()], drc=dict(cut=1))
