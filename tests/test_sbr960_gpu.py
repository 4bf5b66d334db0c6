"""Low-power SBR of the 960-sample cores (DAB+ / DRM HE-AAC: 15 time slots, 30 QMF slots a frame) on the GPU through
xaac_sbr_lp960_process_batch, bit-exact against the real reference: the records oracle/_ref/xaacdec_capture writes while it
decodes 960-line streams with -esbr:0 (the committed streams_wide/he960_aot5 and streams the reference encoder makes on the
spot with -framesize:960).  Needs the prebuilt oracle/_ref binaries next to the repo."""
import ctypes
import os
import subprocess
import wave

import numpy as np
import pytest

import sbr_capture as cap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
WIDE = os.path.join(ROOT, "tests", "golden", "streams_wide")
N_IN, N_OUT = 960, 1920
SENTINEL = 0x5A5A
BAD_ARG = 0xFFFF8001


def _need(binary):
    if not os.path.exists(os.path.join(REF, binary)):
        pytest.fail("oracle/_ref/%s missing: the reference binaries (built by oracle/Makefile.ref where the reference tree "
                    "exists, git-ignored) did not travel with the snapshot -- the 960-line SBR evidence must not vanish silently"
                    % binary)


def capture(aac, tmp_path, meta=None):
    """the reference's ixheaacd_sbr_dec records of one stream (fixed-point branch: -esbr:0)"""
    _need("xaacdec_capture")
    out = str(tmp_path / (os.path.basename(aac) + ".cap"))
    meta = meta or aac[:-4] + ".txt"
    subprocess.run([os.path.join(REF, "xaacdec_capture"), "-ifile:" + aac, "-ofile:" + out + ".wav", "-esbr:0", "-mp4:1",
                    "-imeta:" + meta], env=dict(os.environ, XAAC_CAPTURE_FILE=out), stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=600, check=True)
    return cap.read_records(out) if os.path.exists(out) else []


@pytest.fixture(scope="module")
def ctx():
    import libxaac_amd
    c = libxaac_amd.XaacContext(0, 0)
    yield c
    c.close()


def rows(objs):
    import torch
    return torch.from_numpy(np.stack([np.frombuffer(bytes(o), np.uint8) for o in objs])).cuda()


def run960(ctx, recs, states=None, entry="sbr_lp960_process_batch", n_in=N_IN, n_out=N_OUT, **kw):
    """one batch, every record from its own st0 (or from `states`, uint8 rows on the device): -> pcm rows, states, status.
    The output buffer carries 256 sentinel words behind the batch's n * n_out samples."""
    import torch
    n = len(recs)
    t_s = rows([r["st0"] for r in recs]) if states is None else states
    pcm_in = torch.from_numpy(np.concatenate([r["pcm_in"][:n_in] for r in recs])).cuda()
    out = torch.full((n * n_out + 256,), SENTINEL, dtype=torch.int16, device="cuda")
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ctx.sbr_lp_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    getattr(ctx, entry)(pcm_in, rows([r["header"] for r in recs]), rows([r["frame"] for r in recs]), t_s, out[:n * n_out], ws,
                        status, **kw)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[n * n_out:] == SENTINEL).all(), "written past the batch's output"
    return o[:n * n_out].reshape(n, n_out), t_s, status.cpu().numpy()


def check_records(ctx, recs, tag):
    out, t_s, status = run960(ctx, recs)
    st = t_s.cpu().numpy()
    for i, r in enumerate(recs):
        assert status[i] == r["ret"], (tag, i, r["call"], status[i], r["ret"])
        assert np.array_equal(out[i], r["pcm_out"][0][:N_OUT]), (tag, "pcm", i, r["call"])
        got = cap.State.from_buffer_copy(st[i].tobytes())
        assert not cap.diff_state(got, r["st1"]), (tag, i, r["call"], cap.diff_state(got, r["st1"])[:3])


def he960_records(tmp_path):
    recs = capture(os.path.join(WIDE, "he960_aot5.aac"), tmp_path)
    assert len(recs) >= 80 and all(r["low_pow"] == 1 and not r["ps"] for r in recs), len(recs)
    for r in recs:    # what the capture hands over for these streams (and what the entry point asks for)
        assert (r["header"].num_time_slots, r["header"].time_step, r["header"].num_columns) == (15, 2, 30)
        assert (r["pcm_out"][0][N_OUT:] == 0).all()
    return recs


def test_every_call_of_the_committed_stream(ctx, tmp_path):
    """each reference call of streams_wide/he960_aot5 from its own captured state, all in one batch"""
    recs = he960_records(tmp_path)
    assert sum(r["frame"].border_vec[r["frame"].num_env] > 15 for r in recs) >= 10   # envelopes past QMF slot 30
    check_records(ctx, recs, "he960_aot5")


def test_chains_with_the_state_on_the_device(ctx, tmp_path):
    """each channel's calls in order, the state carried on the device from call to call (a channel's calls are told apart by
    state continuity: a call's st0 is the st1 of that channel's previous call)"""
    recs = he960_records(tmp_path)
    chains = []
    for r in recs:
        for c in chains:
            if bytes(c[-1]["st1"]) == bytes(r["st0"]):
                c.append(r)
                break
        else:
            chains.append([r])
    # (the stream opens with two mono frames; the first stereo frame's channels start from states the host handed over)
    assert sorted(len(c) for c in chains)[-2] >= 40, [len(c) for c in chains]
    t_s = rows([c[0]["st0"] for c in chains])
    for step in range(max(len(c) for c in chains)):
        live = [k for k, c in enumerate(chains) if step < len(c)]
        batch = [chains[k][step] for k in live]
        states = t_s[live].clone()
        for j, r in enumerate(batch):
            assert bytes(states[j].cpu().numpy()) == bytes(r["st0"]), ("carried state", live[j], step)
        out, states, status = run960(ctx, batch, states=states)
        t_s[live] = states
        for j, r in enumerate(batch):
            assert status[j] == r["ret"] and np.array_equal(out[j], r["pcm_out"][0][:N_OUT]), ("chain", live[j], step)
    for k, c in enumerate(chains):
        assert bytes(t_s[k].cpu().numpy()) == bytes(c[-1]["st1"]), ("final state", k)


def _wav(path, fs, ch, seconds=1.6):
    t = np.arange(int(fs * seconds)) / fs
    rng = np.random.default_rng(fs + ch)
    x = 0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t * (1 + 0.3 * t))
    x = x + 0.15 * rng.standard_normal(t.size) * (np.sin(2 * np.pi * 1.5 * t) > 0)
    x[(np.arange(t.size) % (fs // 4)) < 40] += 0.6      # clicks: transient envelopes
    pcm = np.stack([x, np.roll(x, 97)][:ch], 1)
    with wave.open(path, "wb") as w:
        w.setnchannels(ch)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.clip(np.round(pcm * 32767), -32768, 32767).astype(np.int16).tobytes())


@pytest.mark.parametrize("fs", [32000, 44100, 48000])
@pytest.mark.parametrize("br", [32000, 96000])
def test_streams_made_by_the_reference_encoder(ctx, tmp_path, fs, br):
    """HE-AAC stereo with 960-line frames from oracle/_ref/xaacenc -framesize:960 at the rates and stereo bit rates of
    tools/sweep_usac.py's LD profile: every SBR call.  (The reference decodes mono HE-AAC and HE-AACv2 in HQ mode, which the
    960 entry does not cover; the channel pairs of HE-AAC stereo take the low-power branch.)"""
    _need("xaacenc")
    ch = 2
    wav, aac = str(tmp_path / "in.wav"), str(tmp_path / "he960.aac")
    _wav(wav, fs, ch, seconds=3.0)
    subprocess.run([os.path.join(REF, "xaacenc"), "-ifile:" + wav, "-ofile:" + aac, "-br:%d" % br, "-aot:5", "-framesize:960"],
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert os.path.exists(aac) and os.path.exists(aac[:-4] + ".txt"), "the encoder refused the configuration"
    recs = capture(aac, tmp_path)
    assert len(recs) >= 90, len(recs)      # an encoder or decoder that gives up cannot empty the test
    assert all(r["low_pow"] == 1 and r["header"].num_columns == 30 for r in recs)
    # envelopes that run past time slot 15 (QMF slot 30): the adjuster's exponent change at the frame's end is exercised
    assert any(r["frame"].apply_processing and r["frame"].border_vec[r["frame"].num_env] > 15 for r in recs)
    check_records(ctx, recs, "%d/%d/%d" % (fs, ch, br))


def test_refusals(ctx, tmp_path):
    import libxaac_amd
    recs960 = he960_records(tmp_path)[:4]
    recs1024 = cap.read_records(os.path.join(ROOT, "tests", "golden", "sbr_lp_records.bin.gz"), limit=4)
    # a 16-slot channel sent to the 960 entry, beside 15-slot ones: refused -- status -1, its state and its output samples
    # left as they are --, its neighbours decoded as if it were not there
    mixed = [recs960[0], recs1024[0], recs960[1]]
    out, t_s, status = run960(ctx, mixed)
    st = t_s.cpu().numpy()
    assert list(status) == [0, -1, 0], status
    assert bytes(st[1]) == bytes(mixed[1]["st0"]), cap.diff_state(cap.State.from_buffer_copy(st[1].tobytes()), mixed[1]["st0"])[:3]
    assert (out[1] == SENTINEL).all()
    for j in (0, 2):
        assert np.array_equal(out[j], mixed[j]["pcm_out"][0][:N_OUT]) and bytes(st[j]) == bytes(mixed[j]["st1"])
    # a 15-slot channel whose side info is outside the structs' capacity (nine envelopes): the same
    broken = cap.Frame.from_buffer_copy(bytes(recs960[2]["frame"]))
    broken.num_env = 9
    bad = dict(recs960[2], frame=broken)
    out, t_s, status = run960(ctx, [recs960[0], bad])
    assert list(status) == [0, -1] and bytes(t_s[1].cpu().numpy()) == bytes(bad["st0"]) and (out[1] == SENTINEL).all()
    assert np.array_equal(out[0], recs960[0]["pcm_out"][0][:N_OUT])
    # 15-slot channels sent to the 1024-sample entry: still refused there, beside a 16-slot one it decodes
    mixed = [recs960[0], recs1024[1], recs960[1]]
    out, t_s, status = run960(ctx, mixed, entry="sbr_lp_process_batch", n_in=1024, n_out=2048)
    assert list(status) == [-1, 0, -1], status
    assert np.array_equal(out[1], mixed[1]["pcm_out"][0]) and bytes(t_s[1].cpu().numpy()) == bytes(mixed[1]["st1"])
    # the down-sampled bank is out of scope at 30 slots
    with pytest.raises(libxaac_amd.XaacError) as e:
        run960(ctx, recs960[:2], down_sample=True, n_out=N_IN)
    assert e.value.code == BAD_ARG
    # a workspace below xaac_sbr_lp_workspace_bytes
    import torch
    n = 2
    with pytest.raises(libxaac_amd.XaacError) as e:
        ctx.sbr_lp960_process_batch(torch.zeros(n * N_IN, dtype=torch.int16, device="cuda"), rows([r["header"] for r in recs960[:n]]),
                                    rows([r["frame"] for r in recs960[:n]]), rows([r["st0"] for r in recs960[:n]]),
                                    torch.zeros(n * N_OUT, dtype=torch.int16, device="cuda"),
                                    torch.zeros(ctx.sbr_lp_workspace_bytes(n) - 1, dtype=torch.uint8, device="cuda"))
    assert e.value.code == BAD_ARG
