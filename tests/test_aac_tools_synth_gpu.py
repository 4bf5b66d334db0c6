"""The generator-made streams of tests/golden/streams_synth (tools/make_synth_streams.py; tests/test_aac_tools_synth_cpu.py says
what they are and pins the host side to the reference) on the GPU.

Kernel: xaac_aac_tools_process_batch over the stage-1 spectra, one batch per frame step over all mono and stereo streams (every
sampling frequency index, half of them loud) and one launch per element index over the multichannel ones, the noise generator
states on the device from what a new stream starts with (xaac_parse_core_tools_state) -- against the reference decoder's type-2
XAAC_SPEC_DUMP records word for word, status 0, sentinel words behind every array, the final states equal to the host twin's.

End to end: xaacdec_amd with and without -gputools:1, and decode_streams with gpu_tools both ways, against the samples
oracle/_ref/xaacdec writes -- which a stream with a right-only correlated noise band in its first frame (st_sr03, _05, _07,
_08, _09) reaches only with the corrected initial seeds."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aac_tools_cases as tc  # noqa: E402
from libxaac_amd import decoder  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL, TAIL = 0x5a5a5a5a, 64
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
REF = os.path.join(ROOT, "oracle", "_ref", "xaacdec")
ROWS = tc.synth_rows()
DECODED = [r for r in ROWS if r[5] <= 2 or r[6]]
REFUSED = [r for r in ROWS if r[5] > 2 and not r[6]]
_wavs = {}


@pytest.fixture(scope="module")
def ctx():
    import libxaac_amd
    c = libxaac_amd.XaacContext(0, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("synth_gpu"))


def launch(ctx, spec, side, t_state):
    """one call on int32[n, 2, 1024] / uint8[n, side bytes] and the device states uint8[n, state bytes] (updated in place), with
    sentinel words behind every array -> the spectra; status 0 asserted"""
    import torch
    n = side.shape[0]

    def padded(a, dtype):
        mark = np.full(TAIL, SENTINEL & (0xff if dtype == np.uint8 else 0xffffffff), np.int64).astype(dtype)
        return torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1).view(dtype), mark])).cuda()

    t_spec, t_side = padded(spec, np.int32), padded(side, np.uint8)
    t_status = padded(np.full(n, 77, np.int32), np.int32)
    state_bytes = n * decoder.CORE_TOOLS_STATE_BYTES
    t_st = torch.cat([t_state.reshape(-1), torch.full((TAIL,), SENTINEL & 0xff, dtype=torch.uint8, device="cuda")])
    ctx.aac_tools_process_batch(t_spec[:n * 2048], t_side[:side.size].view(n, -1), t_st[:state_bytes], t_status[:n], spec_stride=2048)
    torch.cuda.synchronize()
    for t, size in ((t_spec, n * 2048), (t_side, side.size), (t_st, state_bytes), (t_status, n)):
        back = t.cpu().numpy()
        mark = SENTINEL & (0xff if back.dtype == np.uint8 else 0xffffffff)
        assert len(back) == size + TAIL and np.all(back[size:].astype(np.int64) == mark), "written behind the batch"
    assert np.array_equal(t_side.cpu().numpy()[:side.size], side.reshape(-1)), "the side info was written"
    assert not t_status.cpu().numpy()[:n].any()
    t_state.copy_(t_st[:state_bytes].view(n, -1))
    return t_spec.cpu().numpy()[:n * 2048].reshape(n, 2, 1024)


def run_streams(ctx, rows, tmp):
    """the streams' elements in one batch per frame step and element index; -> launches made"""
    import torch
    walks, refs, starts = [], [], []
    for name, _, _, frames, _, kind, _ in rows:
        before, _ = tc.synth_walk(name)
        ref = tc.reference_spectra(tc.synth_path(name), tmp, tc.synth_channels(kind))
        assert len(before) == len(ref) == frames, name
        walks.append(before), refs.append(ref)
        starts.append(tc.new_states(open(tc.synth_path(name), "rb").read()))
    n = len(rows)
    n_els = [len(w[0][3]) for w in walks]
    # a state row per (element index, stream), on the device for the whole walk
    t_state = [torch.from_numpy(np.stack([starts[i][k] if k < n_els[i] else np.zeros_like(starts[i][0]) for i in range(n)])).cuda()
               for k in range(max(n_els))]
    host = [[s.copy() for s in st] for st in starts]
    launches = 0
    for step in range(max(len(w) for w in walks)):
        for k in range(max(n_els)):
            live = [i for i in range(n) if step < len(walks[i]) and k < n_els[i]]
            if not live:
                continue
            spec = np.zeros((len(live), 2, 1024), np.int32)
            side = np.zeros((len(live), decoder.CORE_TOOLS_SIDE_BYTES), np.uint8)
            where = []
            for j, i in enumerate(live):
                s1, _, _, ids, sides = walks[i][step]
                row, m = tc.element_rows(ids)[k]
                spec[j, :m] = s1[row:row + m]
                side[j] = np.frombuffer(sides[k], np.uint8)
                where.append((row, m))
            idx = torch.tensor(live, device="cuda")
            st = t_state[k][idx].contiguous()
            got = launch(ctx, spec, side, st)
            t_state[k][idx] = st
            launches += 1
            for j, i in enumerate(live):
                row, m = where[j]
                for c in range(m):
                    bad = np.nonzero(got[j, c] != refs[i][step, row + c])[0]
                    assert not len(bad), (rows[i][0], step, k, c, bad[:8])
                if m == 1:
                    assert not got[j, 1].any()
                rc, _, host[i][k] = tc.apply_host(spec[j], side[j], host[i][k])
                assert rc == 0
    for k in range(max(n_els)):
        final = t_state[k].cpu().numpy()
        for i in range(n):
            if k < n_els[i]:
                assert np.array_equal(final[i], host[i][k]), (rows[i][0], k)
    return launches


def test_mono_and_stereo_streams_equal_the_references_spectra(ctx, tmp):
    rows = [r for r in DECODED if r[5] <= 2]
    assert len(rows) == 24
    assert run_streams(ctx, rows, tmp) <= 24


def test_multichannel_streams_equal_the_references_spectra(ctx, tmp):
    rows = [r for r in DECODED if r[5] > 2]
    assert len(rows) == 6
    assert run_streams(ctx, rows, tmp) == 24 * 4      # one launch per step and element index


def samples(path, kind):
    """the payload of a WAV file: mono / stereo through the wave module (the two programs lay their RIFF chunks out differently),
    more channels behind the 68 bytes of the WAVE_FORMAT_EXTENSIBLE header both write"""
    if kind > 2:
        data = open(path, "rb").read()
        assert data[60:64] == b"data" and int.from_bytes(data[22:24], "little") == tc.synth_channels(kind)
        return data[68:]
    with wave.open(path) as w:
        assert w.getnchannels() == kind and w.getsampwidth() == 2
        return w.readframes(w.getnframes())


def reference_pcm(name, kind, frames, tmp):
    """the samples oracle/_ref/xaacdec writes for a stream (default flags), at full length"""
    if name not in _wavs:
        tc.need("xaacdec")
        out = os.path.join(tmp, "ref_%s.wav" % name)
        subprocess.run([REF, "-ifile:" + tc.synth_path(name), "-ofile:" + out], check=True, capture_output=True, timeout=300)
        _wavs[name] = samples(out, kind)
        assert len(_wavs[name]) == 2 * tc.synth_channels(kind) * 1024 * frames, name
    return _wavs[name]


def cli_pcm(name, kind, tmp, tag, *flags):
    assert os.path.exists(CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
    out = os.path.join(tmp, "%s_%s.wav" % (name, tag))
    p = subprocess.run([CLI, "-ifile:" + tc.synth_path(name), "-ofile:" + out, *flags], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (name, tag, p.stderr[-500:])
    return open(out, "rb").read(), samples(out, kind)


@pytest.mark.parametrize("row", DECODED, ids=[r[0] for r in DECODED])
def test_xaacdec_amd_writes_the_references_samples_with_and_without_gputools(row, tmp):
    name, _, _, frames, _, kind, _ = row
    want = reference_pcm(name, kind, frames, tmp)
    plain, plain_pcm = cli_pcm(name, kind, tmp, "plain")
    tools, tools_pcm = cli_pcm(name, kind, tmp, "tools", "-gputools:1")
    assert plain == tools and len(plain_pcm) == len(want)
    # (the two programs write their own RIFF headers: the samples are the payload)
    assert plain_pcm == want and tools_pcm == want


@pytest.mark.parametrize("flags", [(), ("-gputools:1",)], ids=["plain", "gputools"])
def test_xaacdec_amd_refuses_the_stream_the_parser_refuses(flags, tmp):
    name = REFUSED[0][0]
    out = os.path.join(tmp, "refused.wav")
    p = subprocess.run([CLI, "-ifile:" + tc.synth_path(name), "-ofile:" + out, *flags], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "does not parse" in p.stderr, (p.returncode, p.stderr[-300:])


@pytest.mark.parametrize("flags", [(), ("-gputools:1",)], ids=["plain", "gputools"])
def test_a_list_with_a_frame_0_stream_beside_an_encoder_made_one(flags, tmp_path, tmp):
    """-ilist: streams of different kinds in one run, two of them streams whose first frame needs the corrected seeds"""
    names = [("st_sr05", tc.synth_path("st_sr05")), ("mix_aot2_64k", os.path.join(tc.STREAMS, "mix_aot2_64k.aac")),
             ("st_sr08", tc.synth_path("st_sr08"))]
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(p for _, p in names) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([CLI, "-ilist:" + str(lst), "-odir:" + str(out), *flags], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-500:]
    for name, path in names:
        with wave.open(str(out / (name + ".wav"))) as w:
            got = w.readframes(w.getnframes())
        if name.startswith("st_"):
            assert got == reference_pcm(name, 2, 24, tmp), name
        else:
            ref = str(tmp_path / "ref.wav")
            subprocess.run([REF, "-ifile:" + path, "-ofile:" + ref], check=True, capture_output=True, timeout=300)
            with wave.open(ref) as w:
                assert w.getnframes() > 10000 and got == w.readframes(w.getnframes()), name


E2E = [r for r in DECODED if r[5] >= 2]     # a stereo stream per sampling frequency index, and the multichannel ones


@pytest.mark.parametrize("row", E2E, ids=[r[0] for r in E2E])
def test_decode_streams_gives_the_references_samples_with_gpu_tools_both_ways(row, tmp):
    name, _, _, frames, _, kind, _ = row
    n_ch = tc.synth_channels(kind)
    want = np.frombuffer(reference_pcm(name, kind, frames, tmp), np.int16).reshape(-1, n_ch)
    data = open(tc.synth_path(name), "rb").read()
    for gpu_tools in (False, True):
        got, _ = decoder.decode_streams([data, data], gpu_tools=gpu_tools)
        assert len(got) == 2
        for pcm in got:
            assert pcm.shape == want.shape and np.array_equal(pcm, want), (name, gpu_tools)
