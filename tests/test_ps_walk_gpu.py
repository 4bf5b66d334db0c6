"""The PS kernel's slot walk on the GPU (xaac_sbr_hq_process_batch) against the oracle's slot loop on the chains of
tests/ps_walk_cases.py: 24 streams, five frames, the state carried on the device, the shift in front of the left synthesis
bank negative, zero and positive; then the same with a moving band limit, borders off slot 0 and a synthesis limit below
the all-pass bands.  PCM, SBR state, PS state and status word for word.

The chains raise the carried synthesis scale above 4, where the left bank's last shift (shl32_sat by 4 - st_syn_scale,
generic:1638) has a negative count that the reference and the oracle take modulo 32: the synthesis pair kernel's clamp-then-
shift short cut holds for counts 0..16 only, so these frames also pin its exact form for the counts beyond (before it had
one, every such frame came out with 0x7e00-like maxima instead of 0x7fff in the ring: one LSB off in ~890 of 2048 left
samples)."""
import numpy as np
import pytest

import ps_walk_cases as pw
import sbr_capture as cap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import libxaac_amd
    c = libxaac_amd.XaacContext(0, 0)
    yield c
    c.close()


def _compare(ctx, oracle, variant):
    import torch
    recs = pw.records()
    n = len(recs)
    steps = pw.chain(oracle, variant)
    t = lambda objs: torch.from_numpy(np.frombuffer(b"".join(bytes(o) for o in objs), np.uint8).reshape(n, -1).copy()).cuda()
    t_h = t([r["header"] for r in recs])
    t_s, t_ps = t(steps[0]["st_in"]), t(steps[0]["ps_in"])
    ws = torch.zeros(ctx.sbr_hq_workspace_bytes(n, True), dtype=torch.uint8, device="cuda")
    st_off, usb_off = cap.State.st_syn_scale.offset, cap.State.syn_usb.offset
    for k, d in enumerate(steps):
        if k:   # what the chain changes in the carried state in front of a frame, applied to the device's copy
            host = t_s.cpu().numpy()
            for i in range(n):
                now = d["st_in"][i]
                host[i, st_off:st_off + 2] = np.frombuffer(np.int16(now.st_syn_scale).tobytes(), np.uint8)
                host[i, usb_off:usb_off + 2] = np.frombuffer(np.int16(now.syn_usb).tobytes(), np.uint8)
                assert not cap.diff_state(cap.State.from_buffer_copy(host[i].tobytes()), now), (variant, k, i)
            t_s = torch.from_numpy(host).cuda()
        out = torch.zeros(n * 4096, dtype=torch.int16, device="cuda")
        status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        ctx.sbr_hq_process_batch(torch.from_numpy(np.concatenate(d["pcm"])).cuda(), t_h, t(d["frames"]), t_s, out, ws,
                                 t(d["ps_frames"]), t_ps, status)
        torch.cuda.synchronize()
        o, gs, gp, rc = out.cpu().numpy(), t_s.cpu().numpy(), t_ps.cpu().numpy(), status.cpu().numpy()
        for i in range(n):
            want = d["want"][i]
            tag = (variant, k, i, d["common_shift"][i])
            assert rc[i] == want[0], tag
            assert np.array_equal(o[4096 * i:4096 * (i + 1)], want[1]), (tag, "pcm", int(np.sum(o[4096 * i:4096 * (i + 1)] != want[1])))
            s, p = cap.State.from_buffer_copy(gs[i].tobytes()), cap.PsState.from_buffer_copy(gp[i].tobytes())
            assert not cap.diff_state(s, want[2]), (tag, cap.diff_state(s, want[2])[:3])
            assert not cap.diff_state(p, want[3]), (tag, cap.diff_state(p, want[3])[:3])
    return steps


def test_every_sign_of_the_common_shift(ctx, oracle):
    pw.check_signs(_compare(ctx, oracle, "plain"))


def test_moving_band_limit_and_borders_off_slot_zero(ctx, oracle):
    pw.check_range(_compare(ctx, oracle, "moving"))
