"""The PS kernel's group sums (P3: a running sum over the band lanes, differences at the group borders, one clamp) and its
hybrid-domain rotation (P6: one (slot, re | im) per lane) on the GPU against the oracle's slot loop: 24 streams, four carried
frames through xaac_sbr_hq_process_batch, full-scale noise cores (+-32767), on the golden HE-AACv2 records with content above
band 48 in every third stream's overlap and one synthesis limit at band 52 (the wide rows of the core's list launch), then
with borders off slot 0 and a band limit that moves between frames (so that the limit the group sums read switches inside a
frame); and one batch of 960-line HE-AACv2 records (30 slots) through xaac_sbr_hq960_process_batch against the reference's
capture.  PCM, SBR state, PS state and status word for word: the PS state's energy_prev and peak_decay_diff* of bins 14..19
carry the group sums directly.

How close these chains get to the clamp of the group sums: tests/ps_phases_shim.cpp: xpt_hq_group_sums follows the oracle up
to the tool and adds each (slot, group)'s addends in 64 bits.  The largest sum of these chains is 2^28.8 = 0.22 x
0x7fffffff (asserted below: some reach 2^28); none saturates and none lies within a factor of two of the clamp.  That is the
tool's own scaling, not the inputs': below the band limit every word the sums read has been shifted right by at least one
bit (ps_scale is one below the smallest of the core's scales), which bounds a band's power by 2^29 and the six sums by 2^30,
reached only if every band of a group were at full scale in one slot.  Also tried on the CPU and no closer: +-32767 square
waves, and a band limit that drops in mid-frame over full-scale overlap words above it (2^28.5).  So saturation, the
sums exactly at 0x7fffffff and the largest possible addends are left to the host test of the shared helper
(tests/test_ps_phases_cpu.py); no test-only entry point was added to reach them on the device."""
import ctypes
import os

import numpy as np
import pytest

import ps_phases_lib as ppl
import ps_walk_cases as pw
import sbr_capture as cap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, AMP, SEED = 4, 32767, 11


@pytest.fixture(scope="module")
def ctx():
    import libxaac_amd
    c = libxaac_amd.XaacContext(0, 0)
    yield c
    c.close()


def _chain(oracle, variant):
    """like ps_walk_cases.chain, with full-scale cores and no raised synthesis scale; per stream-frame also the exact group
    sums the oracle's path meets ([32][6], int64)"""
    shim = ppl.load(os.path.join(ROOT, "oracle", "liboracle.so"))
    recs = pw.records()
    rng = np.random.default_rng(SEED)
    states = [cap.State.from_buffer_copy(bytes(r["st0"])) for r in recs]
    pstates = [cap.PsState.from_buffer_copy(bytes(r["ps0"])) for r in recs]
    if variant == "wide":
        for i in range(0, len(recs), 3):
            ov = np.frombuffer(states[i], dtype=np.int32, count=6 * 128, offset=cap.State.overlap.offset).reshape(6, 2, 64)
            ov[:, :, 48 + (i % 16):] = rng.integers(-2000, 2000, ov[:, :, 48 + (i % 16):].shape)
        states[1].syn_usb = 52
    steps = []
    for step in range(FRAMES):
        d = dict(frames=[], ps_frames=[], pcm=[], st_in=[], ps_in=[], want=[], sums=[])
        for i, r in enumerate(recs):
            f = cap.Frame.from_buffer_copy(bytes(r["frame"]))
            pf = cap.PsFrame.from_buffer_copy(bytes(r["ps_frame"]))
            pw._fuzz_ps(rng, pf)
            st = cap.State.from_buffer_copy(bytes(states[i]))
            if variant == "moving":
                pw._borders_off_zero(rng, pf)
                if step in (1, 3):
                    f.max_qmf_subband_aac = int(np.clip(f.max_qmf_subband_aac + rng.integers(-6, 7), r["header"].sub_band_start, 32))
                if step == 2:
                    st.syn_usb = int(rng.integers(8, 23))
                if step == 3:
                    st.syn_usb = r["st0"].syn_usb
            pcm = rng.integers(-AMP, AMP + 1, 1024).astype(np.int16)
            ex = np.zeros(32 * 6, np.int64)
            rc = shim.xpt_hq_group_sums(ctypes.byref(r["header"]), ctypes.byref(f), ctypes.byref(st), ctypes.byref(pf),
                                        ctypes.byref(pstates[i]), pcm.ctypes.data_as(ppl.P16), ex.ctypes.data_as(ppl.P64))
            assert rc == 0, (variant, step, i, rc)
            want = pw.run(oracle.lib.xo_sbr_dec_hq, r["header"], f, st, pf, pstates[i], pcm)
            d["frames"].append(f); d["ps_frames"].append(pf); d["pcm"].append(pcm); d["sums"].append(ex)
            d["st_in"].append(st); d["ps_in"].append(pstates[i]); d["want"].append(want)
            states[i], pstates[i] = want[2], want[3]
        steps.append(d)
    return steps


def _loud(steps, variant):
    """from the oracle's side: how large the group sums of the chain get (see the module's docstring)"""
    a = np.array([s for d in steps for s in d["sums"]])
    print("%s: largest group sum 2^%.2f, %d of %d (slot, group) sums >= 2^28, %d above the clamp" %
          (variant, np.log2(float(a.max()) + 1), int((a >= 2 ** 28).sum()), a.size, int((a > 0x7fffffff).sum())))
    assert (a >= 2 ** 28).sum() >= 3, variant


def _compare(ctx, oracle, variant):
    import torch
    recs = pw.records()
    n = len(recs)
    steps = _chain(oracle, variant)
    _loud(steps, variant)
    t = lambda objs: torch.from_numpy(np.frombuffer(b"".join(bytes(o) for o in objs), np.uint8).reshape(n, -1).copy()).cuda()
    t_h = t([r["header"] for r in recs])
    t_s, t_ps = t(steps[0]["st_in"]), t(steps[0]["ps_in"])
    ws = torch.zeros(ctx.sbr_hq_workspace_bytes(n, True), dtype=torch.uint8, device="cuda")
    usb_off = cap.State.syn_usb.offset
    for k, d in enumerate(steps):
        if k:   # what the chain changes in the carried state in front of a frame, applied to the device's copy
            host = t_s.cpu().numpy()
            for i in range(n):
                host[i, usb_off:usb_off + 2] = np.frombuffer(np.int16(d["st_in"][i].syn_usb).tobytes(), np.uint8)
                assert not cap.diff_state(cap.State.from_buffer_copy(host[i].tobytes()), d["st_in"][i]), (variant, k, i)
            t_s = torch.from_numpy(host).cuda()
        out = torch.zeros(n * 4096, dtype=torch.int16, device="cuda")
        status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        ctx.sbr_hq_process_batch(torch.from_numpy(np.concatenate(d["pcm"])).cuda(), t_h, t(d["frames"]), t_s, out, ws,
                                 t(d["ps_frames"]), t_ps, status)
        torch.cuda.synchronize()
        o, gs, gp, rc = out.cpu().numpy(), t_s.cpu().numpy(), t_ps.cpu().numpy(), status.cpu().numpy()
        for i in range(n):
            want = d["want"][i]
            tag = (variant, k, i)
            assert rc[i] == want[0], tag
            assert np.array_equal(o[4096 * i:4096 * (i + 1)], want[1]), (tag, "pcm", int(np.sum(o[4096 * i:4096 * (i + 1)] != want[1])))
            s, p = cap.State.from_buffer_copy(gs[i].tobytes()), cap.PsState.from_buffer_copy(gp[i].tobytes())
            assert not cap.diff_state(s, want[2]), (tag, cap.diff_state(s, want[2])[:3])
            assert not cap.diff_state(p, want[3]), (tag, cap.diff_state(p, want[3])[:3])


def test_full_scale_noise_on_the_wide_range_records(ctx, oracle):
    _compare(ctx, oracle, "wide")


def test_full_scale_noise_with_a_moving_band_limit(ctx, oracle):
    _compare(ctx, oracle, "moving")


def test_one_batch_of_30_slot_frames(ctx, tmp_path):
    """xaac_ps_kernel<30>: 24 calls of the reference on a 960-line HE-AACv2 stream, each from its own captured state"""
    import test_sbr_hq960_gpu as hq960
    recs = [r for r in hq960.he960_v2_records(tmp_path) if r["ps"]][:24]
    assert len(recs) == 24
    hq960.check_records(ctx, recs, "he960_aot29, 24 PS calls")
