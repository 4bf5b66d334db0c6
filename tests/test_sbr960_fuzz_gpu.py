"""The 30-slot instantiations of the SBR and PS kernels (xaac_sbr_lp960_process_batch, xaac_sbr_hq960_process_batch: the
narrow and the list-driven HQ core, xaac_ps_kernel<30>, the pair synthesis bank, the 30-slot analysis and mono synthesis
banks) against the 30-slot host oracle on the fuzzed cases of tests/sbr960_fuzz_cases.py, word for word: status, PCM, SBR
state and PS state after every frame of every chain, the states carried on the device.

What the cases cover is asserted in tests/test_sbr960_fuzz_cpu.py; the oracle is pinned to the reference on captured 960-line
calls in tests/test_sbr960_oracle_vs_reference.py.  The oracle shares sbr_core.h, sbr_ps.h and sbr_ps_frame.h with the
kernels, so what these tests can catch is what differs between one lane walking slot after slot through its own banks and
the kernels' arrangement at 30 slots: indices 30 slots on, the PS ring's step of 30 mod 14, the unrolled delay lines,
borders held to 0..30, the list launch, partly filled workgroups.  Needs no reference binaries."""
import numpy as np
import pytest

import sbr960_fuzz_cases as fz
import sbr_capture as cap
import test_sbr_hq960_gpu as hq960
from test_sbr_hq960_gpu import rows

pytestmark = pytest.mark.gpu
SENTINEL, BAD_ARG = hq960.SENTINEL, hq960.BAD_ARG


@pytest.fixture(scope="module")
def ctx():
    import libxaac_amd
    c = libxaac_amd.XaacContext(0, 0)
    yield c
    c.close()


def _recs(headers, frames, ps_frames, pcm, st_in, ps_in):
    """the cases of one step in the shape test_sbr_hq960_gpu.run takes its records in"""
    return [dict(header=h, frame=f, ps_frame=pf, ps=int(pf is not None), pcm_in=p, st0=s, ps0=q)
            for h, f, pf, p, s, q in zip(headers, frames, ps_frames, pcm, st_in, ps_in)]


def _same(tag, rc, out, t_s, t_ps, want):
    """one step of a batch against the oracle's (rc, pcm, state, ps state) per stream"""
    gs = t_s.cpu().numpy()
    gp = t_ps.cpu().numpy() if t_ps is not None else None
    for i, w in enumerate(want):
        assert rc[i] == w[0], (tag, i, "status", int(rc[i]), w[0])
        bad = np.nonzero(out[i].reshape(-1) != w[1])[0]
        assert bad.size == 0, (tag, i, "pcm", int(bad.size), "first", int(bad[0]), int(out[i].reshape(-1)[bad[0]]), int(w[1][bad[0]]))
        s = cap.State.from_buffer_copy(gs[i].tobytes())
        assert not cap.diff_state(s, w[2]), (tag, i, cap.diff_state(s, w[2])[:3])
        if gp is not None:
            p = cap.PsState.from_buffer_copy(gp[i].tobytes())
            assert not cap.diff_state(p, w[3]), (tag, i, cap.diff_state(p, w[3])[:3])


@pytest.mark.parametrize("batch", range(fz.PS_CASES // fz.BATCH))
def test_ps_case_table_at_30_slots(ctx, oracle, batch):
    """xaac_ps_kernel<30> on the case table of tests/test_ps_prep_gpu.py forced at 30 slots: ring phases 0..13, 1..5 PS envelopes
    with borders anywhere in 0..30, a band limit that drops and rises, every sign of common_shift, detector states"""
    import torch
    cs = fz.ps_cases(oracle)[fz.BATCH * batch:fz.BATCH * (batch + 1)]
    n = len(cs)
    assert n == fz.BATCH
    t_s, t_ps = rows([c["steps"][0]["st_in"] for c in cs]), rows([c["steps"][0]["ps_in"] for c in cs])
    st_off, usb_off = cap.State.st_syn_scale.offset, cap.State.syn_usb.offset
    for k in range(fz.PS_FRAMES):
        d = [c["steps"][k] for c in cs]
        if k:   # what the chain changes in the carried SBR state in front of a frame; the PS state stays on the device
            host = t_s.cpu().numpy()
            for i in range(n):
                now = d[i]["st_in"]
                host[i, st_off:st_off + 2] = np.frombuffer(np.int16(now.st_syn_scale).tobytes(), np.uint8)
                host[i, usb_off:usb_off + 2] = np.frombuffer(np.int16(now.syn_usb).tobytes(), np.uint8)
                assert not cap.diff_state(cap.State.from_buffer_copy(host[i].tobytes()), now), (batch, k, i)
            t_s = torch.from_numpy(host).cuda()
        recs = _recs([c["rec"]["header"] for c in cs], [s["frame"] for s in d], [s["ps_frame"] for s in d], [s["pcm"] for s in d],
                     [s["st_in"] for s in d], [s["ps_in"] for s in d])
        out, t_s, t_ps, rc = hq960.run(ctx, recs, states=t_s, ps_states=t_ps)
        _same(("ps", batch, k, [(c["mode"], c["det"], s["common_shift"]) for c, s in zip(cs, d)]), rc, out, t_s, t_ps,
              [s["want"] for s in d])


@pytest.mark.parametrize("with_ps", [True, False], ids=["ps", "mono"])
def test_fuzzed_grids_and_moving_band_limit_hq(ctx, oracle, with_ps):
    """the HQ core, the banks and the pair synthesis at 30 slots: 10 streams x 6 frames of legal grids at 15 time slots (fixed
    and variable, 1..5 envelopes, last borders 12..18), header switches, harmonics, a moving band limit, core PCM from full
    scale down to +-9 -- with PS, and as mono HQ without PS buffers"""
    steps = fz.hq_chain(oracle, with_ps)
    t_s = rows(steps[0]["st_in"])
    t_ps = rows(steps[0]["ps_in"]) if with_ps else None
    for k, d in enumerate(steps):
        recs = _recs(d["headers"], d["frames"], d["ps_frames"], d["pcm"], d["st_in"], d["ps_in"])
        out, t_s, t_ps, rc = hq960.run(ctx, recs, states=t_s, ps_states=t_ps)
        _same(("hq", with_ps, k), rc, out, t_s, t_ps, d["want"])


@pytest.mark.parametrize("stereo", [True, False], ids=["pairs", "mono"])
def test_fuzzed_grids_and_moving_band_limit_lp(ctx, oracle, stereo):
    """xaac_sbr_lp960_process_batch: five interleaved channel pairs (in_ch_fac = out_ch_fac = 2) and five mono channels over 6
    frames of the same grid fuzz, core PCM at full scale, +-3000 and +-9"""
    import torch
    steps = fz.lp_chain(oracle, stereo)
    n, fac = len(steps[0]["st_in"]), 2 if stereo else 1
    t_s = rows(steps[0]["st_in"])
    ws = torch.zeros(ctx.sbr_lp_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    for k, d in enumerate(steps):
        pcm = np.stack(d["pcm"]).reshape(n // fac, fac, fz.N_IN).transpose(0, 2, 1).reshape(-1)       # L R L R ...
        out = torch.full((n * fz.N_OUT + 256,), SENTINEL, dtype=torch.int16, device="cuda")
        status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        ctx.sbr_lp960_process_batch(torch.from_numpy(np.ascontiguousarray(pcm)).cuda(), rows(d["headers"]), rows(d["frames"]), t_s,
                                    out[:n * fz.N_OUT], ws, status, in_ch_fac=fac, out_ch_fac=fac)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[n * fz.N_OUT:] == SENTINEL).all(), "written past the batch's output"
        planar = o[:n * fz.N_OUT].reshape(n // fac, fz.N_OUT, fac).transpose(0, 2, 1).reshape(n, fz.N_OUT)
        _same(("lp", stereo, k), status.cpu().numpy(), planar, t_s, None, d["want"])


def test_streams_above_band_48_take_the_list_launch(ctx, oracle):
    """a batch of five in which two streams need the 64-band rows (a synthesis bank limit at band 52; overlap words above band
    48): every stream equals the oracle over two frames; with max_band_hint = 48 those two are refused with
    XAAC_FATAL_BAD_ARG and the other three come out as without the hint"""
    steps = fz.list_case(oracle)
    t_s, t_ps = rows(steps[0]["st_in"]), rows(steps[0]["ps_in"])
    first = None
    for k, d in enumerate(steps):
        recs = [dict(r, pcm_in=p) for r, p in zip(d["recs"], d["pcm"])]
        out, t_s, t_ps, rc = hq960.run(ctx, recs, states=t_s, ps_states=t_ps)
        _same(("list", k), rc, out, t_s, t_ps, d["want"])
        if first is None:
            first = (recs, out, t_s.cpu().numpy(), t_ps.cpu().numpy())
    recs, wide_out, wide_s, wide_ps = first
    d = steps[0]
    out, t_s, t_ps, rc = hq960.run(ctx, recs, states=rows(d["st_in"]), ps_states=rows(d["ps_in"]), max_band_hint=48, fill=SENTINEL)
    gs, gp = t_s.cpu().numpy(), t_ps.cpu().numpy()
    for i in range(fz.BATCH):
        if i in fz.WIDE_STREAMS:
            assert np.uint32(rc[i]) == BAD_ARG, (i, rc[i])
        else:
            assert rc[i] == 0 and np.array_equal(out[i], wide_out[i]), i
            assert np.array_equal(gs[i], wide_s[i]) and np.array_equal(gp[i], wide_ps[i]), i


def test_malformed_side_info_does_not_disturb_the_batch_at_30_slots(ctx, oracle):
    """one stream's SBR frame and another's PS frame filled with random bytes, in a batch of five: the SBR one is refused --
    status -1, its states and its output samples left as they were --; the PS one has its indices clamped into the tables and
    its borders into 0..30, is reported with status -1 and decodes exactly as the oracle does; the neighbours are exact"""
    m = fz.malformed(oracle)
    recs = [dict(r, frame=f, ps_frame=pf) for r, f, pf in zip(m["recs"], m["frames"], m["ps_frames"])]
    out, t_s, t_ps, rc = hq960.run(ctx, recs, fill=SENTINEL)
    gs, gp = t_s.cpu().numpy(), t_ps.cpu().numpy()
    b = fz.BAD_SBR
    assert rc[b] == -1 and (out[b] == SENTINEL).all()
    assert bytes(gs[b]) == bytes(recs[b]["st0"]) and bytes(gp[b]) == bytes(recs[b]["ps0"])
    keep = [i for i in range(fz.BATCH) if i != b]
    _same("malformed", rc[keep], out[keep], t_s[keep], t_ps[keep], [m["want"][i] for i in keep])
    assert rc[fz.BAD_PS] == -1
    for i in keep:
        if i != fz.BAD_PS:      # ... and the reference's own record
            assert hq960.same_pcm(out[i], recs[i]) and not cap.diff_state(cap.PsState.from_buffer_copy(gp[i].tobytes()), recs[i]["ps1"]), i
