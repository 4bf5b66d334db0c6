"""HQ SBR and parametric stereo of the 960-sample cores (DAB+ / DRM HE-AAC mono and HE-AACv2: 15 time slots, 30 QMF slots a
frame) on the GPU through xaac_sbr_hq960_process_batch, bit-exact against the real reference: the records
oracle/_ref/xaacdec_capture writes while it decodes 960-line streams with -esbr:0 (the committed streams_wide/he960_aot29 and
streams the reference encoder makes on the spot with -framesize:960).  Needs the prebuilt oracle/_ref binaries next to the
repo."""
import os
import subprocess

import numpy as np
import pytest

import sbr_capture as cap
from test_sbr960_gpu import _wav

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
                    "exists, git-ignored) did not travel with the snapshot -- the 960-line HQ SBR evidence must not vanish "
                    "silently" % binary)


def capture(aac, tmp_path):
    """the reference's ixheaacd_sbr_dec records of one stream (fixed-point branch: -esbr:0)"""
    _need("xaacdec_capture")
    out = str(tmp_path / (os.path.basename(aac) + ".cap"))
    subprocess.run([os.path.join(REF, "xaacdec_capture"), "-ifile:" + aac, "-ofile:" + out + ".wav", "-esbr:0", "-mp4:1",
                    "-imeta:" + aac[:-4] + ".txt"], env=dict(os.environ, XAAC_CAPTURE_FILE=out), stdout=subprocess.DEVNULL,
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


def run(ctx, recs, states=None, ps_states=None, entry="sbr_hq960_process_batch", n_in=N_IN, n_out=N_OUT, fill=0,
        ws_bytes=None, **kw):
    """one batch, every record from its own st0 / ps0 (or from `states` / `ps_states`, uint8 rows on the device); PS records go
    through the entry with their PS side info, the others without.  The batch's output is filled with `fill`, 256 sentinel
    words sit behind it.  -> pcm [n, n_out] or [n, n_out, 2] (L,R), SBR states, PS states (or None), status"""
    import torch
    n, with_ps = len(recs), bool(recs[0]["ps"])
    assert all(bool(r["ps"]) == with_ps for r in recs)
    m = n * n_out * (2 if with_ps else 1)
    t_s = rows([r["st0"] for r in recs]) if states is None else states
    t_ps = (rows([r["ps0"] for r in recs]) if ps_states is None else ps_states) if with_ps else None
    pcm_in = torch.from_numpy(np.concatenate([r["pcm_in"][:n_in] for r in recs])).cuda()
    out = torch.full((m + 256,), SENTINEL, dtype=torch.int16, device="cuda")
    out[:m] = fill
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ctx.sbr_hq_workspace_bytes(n, with_ps) if ws_bytes is None else ws_bytes, dtype=torch.uint8, device="cuda")
    getattr(ctx, entry)(pcm_in, rows([r["header"] for r in recs]), rows([r["frame"] for r in recs]), t_s, out[:m], ws,
                        rows([r["ps_frame"] for r in recs]) if with_ps else None, t_ps, status, **kw)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[m:] == SENTINEL).all(), "written past the batch's output"
    o = o[:m].reshape(n, n_out, 2) if with_ps else o[:m].reshape(n, n_out)
    return o, t_s, t_ps, status.cpu().numpy()


def same_pcm(o, r, n_out=N_OUT):
    if r["ps"]:
        return np.array_equal(o[:, 0], r["pcm_out"][0][:n_out]) and np.array_equal(o[:, 1], r["pcm_out"][1][:n_out])
    return np.array_equal(o, r["pcm_out"][0][:n_out])


def check_records(ctx, recs, tag):
    out, t_s, t_ps, status = run(ctx, recs)
    st = t_s.cpu().numpy()
    ps = t_ps.cpu().numpy() if t_ps is not None else None
    for i, r in enumerate(recs):
        assert status[i] == r["ret"], (tag, i, r["call"], status[i], r["ret"])
        assert same_pcm(out[i], r), (tag, "pcm", i, r["call"])
        got = cap.State.from_buffer_copy(st[i].tobytes())
        assert not cap.diff_state(got, r["st1"]), (tag, i, r["call"], cap.diff_state(got, r["st1"])[:3])
        if ps is not None:
            gps = cap.PsState.from_buffer_copy(ps[i].tobytes())
            assert not cap.diff_state(gps, r["ps1"]), (tag, "ps", i, r["call"], cap.diff_state(gps, r["ps1"])[:3])


def he960_v2_records(tmp_path):
    recs = capture(os.path.join(WIDE, "he960_aot29.aac"), tmp_path)
    assert len(recs) >= 40, len(recs)
    for r in recs:    # HQ + PS at 15 / 30 (and what the entry point asks for)
        assert r["low_pow"] == 0 and r["ps"] == 1, (r["call"], r["low_pow"], r["ps"])
        assert (r["header"].num_time_slots, r["header"].time_step, r["header"].num_columns) == (15, 2, 30)
        assert (r["pcm_out"][:, N_OUT:] == 0).all()
    return recs


def test_every_call_of_the_committed_stream(ctx, tmp_path):
    """each reference call of streams_wide/he960_aot29 from its own captured SBR and PS state, all in one batch"""
    recs = he960_v2_records(tmp_path)
    assert sum(r["frame"].border_vec[r["frame"].num_env] > 15 for r in recs) >= 10   # envelopes past QMF slot 30
    check_records(ctx, recs, "he960_aot29")


def test_chains_with_the_states_on_the_device(ctx, tmp_path):
    """the stream's calls in order, the SBR and the PS state carried on the device from call to call (calls of one stream are
    told apart by state continuity: a call's st0 is the st1 of that stream's previous call)"""
    recs = he960_v2_records(tmp_path)
    chains = []
    for r in recs:
        for c in chains:
            if bytes(c[-1]["st1"]) == bytes(r["st0"]) and bytes(c[-1]["ps1"]) == bytes(r["ps0"]):
                c.append(r)
                break
        else:
            chains.append([r])
    assert max(len(c) for c in chains) >= 35, [len(c) for c in chains]
    t_s = rows([c[0]["st0"] for c in chains])
    t_ps = rows([c[0]["ps0"] for c in chains])
    for step in range(max(len(c) for c in chains)):
        live = [k for k, c in enumerate(chains) if step < len(c)]
        batch = [chains[k][step] for k in live]
        states, ps_states = t_s[live].clone(), t_ps[live].clone()
        out, states, ps_states, status = run(ctx, batch, states=states, ps_states=ps_states)
        t_s[live], t_ps[live] = states, ps_states
        for j, r in enumerate(batch):
            assert status[j] == r["ret"] and same_pcm(out[j], r), ("chain", live[j], step)
    for k, c in enumerate(chains):
        assert bytes(t_s[k].cpu().numpy()) == bytes(c[-1]["st1"]), ("final state", k)
        assert bytes(t_ps[k].cpu().numpy()) == bytes(c[-1]["ps1"]), ("final PS state", k)


@pytest.mark.parametrize("fs", [32000, 44100, 48000])
@pytest.mark.parametrize("aot,ch,brs", [(29, 2, (24000, 40000)), (5, 1, (24000, 40000))], ids=["aot29", "aot5mono"])
@pytest.mark.parametrize("k", [0, 1], ids=["lo", "hi"])
def test_streams_made_by_the_reference_encoder(ctx, tmp_path, fs, aot, ch, brs, k):
    """HE-AACv2 (stereo input) and mono HE-AAC with 960-line frames from oracle/_ref/xaacenc -framesize:960: every SBR call,
    HQ mode at 30 QMF slots; the mono streams go through the entry without PS side info"""
    _need("xaacenc")
    br = brs[k]
    wav, aac = str(tmp_path / "in.wav"), str(tmp_path / "hq960.aac")
    _wav(wav, fs, ch, seconds=3.0)
    subprocess.run([os.path.join(REF, "xaacenc"), "-ifile:" + wav, "-ofile:" + aac, "-br:%d" % br, "-aot:%d" % aot,
                    "-framesize:960"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert os.path.exists(aac) and os.path.exists(aac[:-4] + ".txt"), "the encoder refused the configuration"
    recs = capture(aac, tmp_path)
    assert len(recs) >= 45, len(recs)      # an encoder or decoder that gives up cannot empty the test
    assert all(r["low_pow"] == 0 and r["ps"] == (aot == 29) and r["header"].num_columns == 30 for r in recs)
    assert any(r["frame"].apply_processing and r["frame"].border_vec[r["frame"].num_env] > 15 for r in recs)
    check_records(ctx, recs, "%d/%d/%d" % (aot, fs, br))


def test_refusals(ctx, tmp_path):
    import libxaac_amd
    recs960 = he960_v2_records(tmp_path)[:4]
    recs1024 = cap.read_records(os.path.join(ROOT, "tests", "golden", "sbr_hq_ps_records.bin.gz"), limit=4)
    # a 16-slot HQ record sent to the 960 entry, between 15-slot ones: refused -- status -1, its SBR and PS states and its
    # output samples left as they are --, its neighbours decoded as if it were not there
    mixed = [recs960[0], recs1024[0], recs960[1]]
    out, t_s, t_ps, status = run(ctx, mixed, fill=SENTINEL)
    st, ps = t_s.cpu().numpy(), t_ps.cpu().numpy()
    assert list(status) == [0, -1, 0], status
    assert bytes(st[1]) == bytes(mixed[1]["st0"]), cap.diff_state(cap.State.from_buffer_copy(st[1].tobytes()), mixed[1]["st0"])[:3]
    assert bytes(ps[1]) == bytes(mixed[1]["ps0"])
    assert (out[1] == SENTINEL).all()
    for j in (0, 2):
        assert same_pcm(out[j], mixed[j]) and bytes(st[j]) == bytes(mixed[j]["st1"]) and bytes(ps[j]) == bytes(mixed[j]["ps1"]), j
    # a 15-slot record whose side info is outside the structs' capacity (nine envelopes): the same
    broken = cap.Frame.from_buffer_copy(bytes(recs960[2]["frame"]))
    broken.num_env = 9
    bad = dict(recs960[2], frame=broken)
    out, t_s, t_ps, status = run(ctx, [recs960[0], bad], fill=SENTINEL)
    assert list(status) == [0, -1], status
    assert bytes(t_s[1].cpu().numpy()) == bytes(bad["st0"]) and bytes(t_ps[1].cpu().numpy()) == bytes(bad["ps0"])
    assert (out[1] == SENTINEL).all() and same_pcm(out[0], recs960[0])
    # 15-slot records sent to the 1024-sample entry: still refused there, beside a 16-slot one it decodes
    mixed = [recs960[0], recs1024[1], recs960[1]]
    out, t_s, t_ps, status = run(ctx, mixed, entry="sbr_hq_process_batch", n_in=1024, n_out=2048)
    assert list(status) == [-1, 0, -1], status
    assert same_pcm(out[1], mixed[1], 2048) and bytes(t_s[1].cpu().numpy()) == bytes(mixed[1]["st1"])
    # the down-sampled bank is out of scope at 30 slots (mono streams: with PS the 1024 entry refuses it as well)
    mono = [dict(r, ps=0) for r in recs960[:2]]
    with pytest.raises(libxaac_amd.XaacError) as e:
        run(ctx, mono, down_sample=True, n_out=N_IN)
    assert e.value.code == BAD_ARG
    # a workspace below xaac_sbr_hq_workspace_bytes
    with pytest.raises(libxaac_amd.XaacError) as e:
        run(ctx, recs960[:2], ws_bytes=ctx.sbr_hq_workspace_bytes(2, True) - 1)
    assert e.value.code == BAD_ARG


def test_max_band_hint(ctx, tmp_path):
    """max_band_hint = 48 keeps its meaning at 30 slots: the committed stream (sub_band_end 45) decodes to the same words with and
    without it; a stream that reaches above band 48 (a synthesis bank limit at band 52) is refused with XAAC_FATAL_BAD_ARG, the
    streams beside it untouched by that"""
    recs = he960_v2_records(tmp_path)[:12]
    assert all(r["header"].sub_band_end <= 48 for r in recs)
    plain = run(ctx, recs)
    hinted = run(ctx, recs, max_band_hint=48)
    for a, b in zip(plain, hinted):
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        b = b.cpu().numpy() if hasattr(b, "cpu") else b
        assert np.array_equal(a, b)
    for i, r in enumerate(recs):
        assert plain[3][i] == r["ret"] and same_pcm(plain[0][i], r)
    states = [cap.State.from_buffer_copy(bytes(r["st0"])) for r in recs]
    states[3].syn_usb = 52
    wide = run(ctx, recs, states=rows(states))
    out, t_s, t_ps, status = run(ctx, recs, states=rows(states), max_band_hint=48)
    assert np.uint32(status[3]) == BAD_ARG and wide[3][3] == recs[3]["ret"]
    ws, wps = wide[1].cpu().numpy(), wide[2].cpu().numpy()
    st, ps = t_s.cpu().numpy(), t_ps.cpu().numpy()
    for i in range(len(recs)):
        if i == 3:
            continue
        assert status[i] == recs[i]["ret"] and np.array_equal(out[i], wide[0][i]), i
        assert np.array_equal(st[i], ws[i]) and np.array_equal(ps[i], wps[i]), i


def test_nothing_written_past_the_batch(ctx, tmp_path):
    """sentinel words behind n x 1920 (x 2 with PS) stay as they are, with PS and without (run() checks them), and every sample
    of the batch is written"""
    recs = he960_v2_records(tmp_path)[:5]
    out, _, _, _ = run(ctx, recs, fill=SENTINEL)
    for i, r in enumerate(recs):
        assert same_pcm(out[i], r)
    mono = [dict(r, ps=0) for r in recs]
    out, _, _, status = run(ctx, mono, fill=SENTINEL)
    assert out.shape == (5, N_OUT) and (status != 7).all()
