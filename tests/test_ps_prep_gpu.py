"""The PS kernel (libxaac_amd/csrc/sbr_ps_kernel.hip) behind the changes to the phases around its all-pass arithmetic -- the
14-slot delay lines unrolled over the frame in LDS, the group sums' lane-constant shifts, the detector on two lanes per bin
and the short division -- against the host oracle's slot loop, word for word: PCM of both channels, SBR state, the carried
PS state and the status.

Batches of five streams: the kernel's workgroup holds four stream-frames, so the second workgroup is partly filled.  Every
case is a chain of three frames with the PS state carried on the device, so that the 14-slot ring and the detector's three
values written by one frame are read by the next.  The cases are built from the golden records and the generators of
tests/ps_walk_cases.py; what they cover is asserted on the oracle's side (test_the_cases_cover_what_they_claim):

  ring phase        ps.idx_long = 0..13 in front of the first frame (every phase in at least two cases)
  band limit        dropped below the all-pass bands in front of frame 1 and back up in front of frame 2, with the first
                    border at slot 0 / at slot 3, 9 or 17 (the new limit takes over there, and that slot + 14 lies inside the
                    frame too) / not moved at all
  common_shift      negative, zero and positive (the carried synthesis scale raised as in ps_walk_cases)
  lsb, usb          0 < lsb < usb < 64: bands of all three shift classes
  ov_lb vs lb       overlap slots scaled differently from the rest
  detector          carried values zeroed with the band limit at 20 (energy stays 0 in the bins of the bands above it), at
                    0x7fffffff (the smoothed sums saturate), and as recorded (ratios of 0x7fff, peak <= energy, and below)
Bin powers that saturate cannot be had through the whole chain (the tool's own scaling keeps a band's power below 2^29, see
tests/test_ps_phases_gpu.py); they are in tests/test_ps_prep_cpu.py on the host build of the same function.

30 slots (xaac_ps_kernel<30>): here, five chains of three consecutive calls of the reference's own capture of a 960-line
HE-AACv2 stream, states carried on the device, against the reference's PCM and PS states.  Their ring phases and band
limits are the stream's.  The case table above forced at 30 slots, against the host oracle's 30-slot chain
(xo_sbr_dec_hq960), is in tests/test_sbr960_fuzz_gpu.py; the host build of xp_ps_frame<30> runs the moving-limit chains in
tests/test_ps_phases_cpu.py."""
import numpy as np
import pytest

import ps_walk_cases as pw
import sbr_capture as cap

pytestmark = pytest.mark.gpu
BATCH = 4 + 1            # one workgroup of the PS kernel (four waves, a stream-frame each) and one stream more
CASES, FRAMES, SEED = 30, 3, 77
MID = [3, 9, 17]         # first borders inside the frame with border + 14 < 32
MAX = 0x7fffffff


@pytest.fixture(scope="module")
def ctx():
    import libxaac_amd
    c = libxaac_amd.XaacContext(0, 0)
    yield c
    c.close()


_built = {}


def cases(oracle):
    """-> list over cases of dict(rec, mode, det, steps): steps = list over frames of dict(frame, ps_frame, pcm, st_in,
    ps_in, want, common_shift, usb_prev); built once"""
    if "cases" in _built:
        return _built["cases"]
    recs = pw.records()
    rng = np.random.default_rng(SEED)
    out = []
    for k in range(CASES):
        r = recs[(5 * k) % len(recs)]
        mode = ["zero", "mid", "never"][k % 3]
        det = {0: "zeroed", 3: "full"}.get(k % 7, "recorded")
        st = cap.State.from_buffer_copy(bytes(r["st0"]))
        ps = cap.PsState.from_buffer_copy(bytes(r["ps0"]))
        ps.idx_long = k % 14
        for name in ("peak_decay_diff", "energy_prev", "peak_decay_diff_prev"):
            if det != "recorded":
                for b in range(20):
                    getattr(ps, name)[b] = 0 if det == "zeroed" else MAX
        limit = 20 if det == "zeroed" else int(r["st0"].syn_usb)   # zeroed: nothing above band 20, bins 18 and 19 stay silent
        st.syn_usb = limit
        steps = []
        for step in range(FRAMES):
            f = cap.Frame.from_buffer_copy(bytes(r["frame"]))
            pf = cap.PsFrame.from_buffer_copy(bytes(r["ps_frame"]))
            pw._fuzz_ps(rng, pf)
            st = cap.State.from_buffer_copy(bytes(st))
            st.st_syn_scale += pw.RAISE[step]
            if mode == "mid":
                pw._borders_off_zero(rng, pf)
                rest = sorted(int(pf.border_position[e]) for e in range(1, 7) if int(pf.border_position[e]) > MID[k % 3])
                first = [MID[k % 3]] + rest
                for e in range(7):
                    pf.border_position[e] = first[e] if e < len(first) else 0
            if mode != "never":
                if step == 1:
                    st.syn_usb = int(rng.integers(8, min(23, limit)))
                if step == 2:
                    st.syn_usb = limit
            pcm = rng.integers(-pw.AMP, pw.AMP + 1, 1024).astype(np.int16)
            want = pw.run(oracle.lib.xo_sbr_dec_hq, r["header"], f, st, pf, ps, pcm)
            steps.append(dict(frame=f, ps_frame=pf, pcm=pcm, st_in=st, ps_in=ps, want=want, usb_prev=int(ps.usb),
                              common_shift=int(st.st_syn_scale) - int(want[2].ps_scale) - 8))
            st, ps = want[2], want[3]
        out.append(dict(rec=r, mode=mode, det=det, steps=steps))
    _built["cases"] = out
    return out


def test_the_cases_cover_what_they_claim(oracle):
    cs = cases(oracle)
    assert all(sum(1 for k in range(CASES) if k % 14 == p) >= 2 for p in range(14))
    assert all(c["steps"][0]["ps_in"].idx_long == k % 14 for k, c in enumerate(cs))
    shifts = np.array([s["common_shift"] for c in cs for s in c["steps"]])
    assert (shifts < 0).sum() >= 3 and (shifts == 0).sum() >= 3 and (shifts > 0).sum() >= 3, shifts
    assert shifts.min() >= -31 and shifts.max() <= 31
    rising = {"zero": 0, "mid": 0}
    for c in cs:
        for s in c["steps"]:
            assert s["want"][0] == 0
            st_in, st_out = s["st_in"], s["want"][2]
            assert 0 < st_in.syn_lsb < st_in.syn_usb < 64 or st_in.syn_usb < 23, (st_in.syn_lsb, st_in.syn_usb)
            b0 = int(s["ps_frame"].border_position[0])
            if c["mode"] != "never" and st_in.syn_usb > s["usb_prev"] > 0:
                assert (b0 == 0 if c["mode"] == "zero" else b0 in MID) and b0 + 14 < 32
                rising[c["mode"]] += 1
            if c["mode"] == "never":
                assert st_in.syn_usb == c["steps"][0]["st_in"].syn_usb
    assert rising["zero"] >= 5 and rising["mid"] >= 5, rising
    assert sum(1 for c in cs for s in c["steps"] if 0 < s["st_in"].syn_lsb < s["st_in"].syn_usb < 64) >= 2 * CASES
    assert sum(1 for c in cs for s in c["steps"] if s["st_in"].ov_lb_scale != s["want"][2].lb_scale) >= CASES // 2
    zeroed = [c for c in cs if c["det"] == "zeroed"]
    full = [c for c in cs if c["det"] == "full"]
    assert len(zeroed) >= 3 and len(full) >= 3
    for c in zeroed:    # energy = 0 survives in the bins above the band limit (from the first border on), the others have moved
        e = np.array([s["want"][3].energy_prev[:] for s in c["steps"]])
        assert (e[:, 18:] == 0).all(axis=1).any() and (e[:, :14] > 0).all(), e
    for c in full:      # went in at the top of the range; a rescale and 32 slots of decay by 0.766 later every bin still shows it
        assert all(v == MAX for v in c["steps"][0]["ps_in"].energy_prev[:])
        e = np.array(c["steps"][0]["want"][3].peak_decay_diff[:])
        assert e.min() > 2 ** 12, e


def _rows(objs):
    import torch
    return torch.from_numpy(np.stack([np.frombuffer(bytes(o), np.uint8) for o in objs])).cuda()


@pytest.mark.parametrize("batch", range(CASES // BATCH))
def test_32_slots_against_the_slot_loop(ctx, oracle, batch):
    import torch
    cs = cases(oracle)[BATCH * batch:BATCH * (batch + 1)]
    n = len(cs)
    assert n == BATCH
    t_h = _rows([c["rec"]["header"] for c in cs])
    t_s, t_ps = _rows([c["steps"][0]["st_in"] for c in cs]), _rows([c["steps"][0]["ps_in"] for c in cs])
    ws = torch.zeros(ctx.sbr_hq_workspace_bytes(n, True), dtype=torch.uint8, device="cuda")
    st_off, usb_off = cap.State.st_syn_scale.offset, cap.State.syn_usb.offset
    for k in range(FRAMES):
        d = [c["steps"][k] for c in cs]
        if k:   # what the chain changes in the carried SBR state in front of a frame; the PS state stays on the device
            host = t_s.cpu().numpy()
            for i in range(n):
                now = d[i]["st_in"]
                host[i, st_off:st_off + 2] = np.frombuffer(np.int16(now.st_syn_scale).tobytes(), np.uint8)
                host[i, usb_off:usb_off + 2] = np.frombuffer(np.int16(now.syn_usb).tobytes(), np.uint8)
                assert not cap.diff_state(cap.State.from_buffer_copy(host[i].tobytes()), now), (batch, k, i)
            t_s = torch.from_numpy(host).cuda()
        out = torch.zeros(n * 4096, dtype=torch.int16, device="cuda")
        status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        ctx.sbr_hq_process_batch(torch.from_numpy(np.concatenate([s["pcm"] for s in d])).cuda(), t_h,
                                 _rows([s["frame"] for s in d]), t_s, out, ws, _rows([s["ps_frame"] for s in d]), t_ps, status)
        torch.cuda.synchronize()
        o, gs, gp, rc = out.cpu().numpy(), t_s.cpu().numpy(), t_ps.cpu().numpy(), status.cpu().numpy()
        for i in range(n):
            want = d[i]["want"]
            tag = (batch, k, i, cs[i]["mode"], cs[i]["det"], d[i]["common_shift"])
            assert rc[i] == want[0], tag
            assert np.array_equal(o[4096 * i:4096 * (i + 1)], want[1]), (tag, "pcm", int(np.sum(o[4096 * i:4096 * (i + 1)] != want[1])))
            s, p = cap.State.from_buffer_copy(gs[i].tobytes()), cap.PsState.from_buffer_copy(gp[i].tobytes())
            assert not cap.diff_state(p, want[3]), (tag, cap.diff_state(p, want[3])[:3])
            assert not cap.diff_state(s, want[2]), (tag, cap.diff_state(s, want[2])[:3])


def test_30_slots_chained_against_the_reference_capture(ctx, tmp_path):
    import test_sbr_hq960_gpu as hq960
    recs = hq960.he960_v2_records(tmp_path)
    chains = []             # calls of one stream in order: a call's states are the previous call's outputs
    for r in recs:
        for c in chains:
            if bytes(c[-1]["st1"]) == bytes(r["st0"]) and bytes(c[-1]["ps1"]) == bytes(r["ps0"]):
                c.append(r)
                break
        else:
            chains.append([r])
    long = max(chains, key=len)
    assert len(long) >= BATCH * 2 + FRAMES
    starts = [2 * j for j in range(BATCH)]      # five runs of three calls, two calls apart: five ring phases
    t_s, t_ps = hq960.rows([long[a]["st0"] for a in starts]), hq960.rows([long[a]["ps0"] for a in starts])
    assert len({long[a]["ps0"].idx_long for a in starts}) >= 3
    for k in range(FRAMES):
        batch = [long[a + k] for a in starts]
        out, t_s, t_ps, status = hq960.run(ctx, batch, states=t_s, ps_states=t_ps)
        gp = t_ps.cpu().numpy()
        for j, r in enumerate(batch):
            assert status[j] == r["ret"] and hq960.same_pcm(out[j], r), ("pcm", k, j)
            p = cap.PsState.from_buffer_copy(gp[j].tobytes())
            assert not cap.diff_state(p, r["ps1"]), (k, j, cap.diff_state(p, r["ps1"])[:3])
    for j, a in enumerate(starts):
        assert bytes(t_s[j].cpu().numpy()) == bytes(long[a + FRAMES - 1]["st1"]), ("final state", j)
