"""tests/golden/sbr_grid_chains.npz: 384 + 384 calls of the REAL ixheaacd_sbr_dec (low-power; HQ + parametric stereo) on
FUZZED LEGAL ENVELOPE GRIDS, made by tools/make_golden_sbr_grid_chains.py as 16 + 16 chains of 24 steps with the state carried
by the reference itself.  tests/golden/sbr_chains.npz keeps the grids of its captured streams; here every step's grid comes
from tests/sbr_grid_cases.py: legal_grid_frame (the legal halves of test_env_pairs_cpu._fuzz_frame): 1-5 envelopes, borders
off 0 and 16, freq_res that changes inside a frame and at the noise border, transient_env at every position -- so the
envelope adjuster meets the reference, not only other compilations of libxaac_amd/csrc/sbr_core.h, on such grids.
(profiles/sbr_grid_chains_coverage.txt: the grids of both files side by side.)
  * the committed file covers what it says (the generator asserts the same before it writes);
  * CPU: the oracle's paired build and its one-envelope build (_seq) each walk every chain, own state carried, and must
    reproduce every return code and CRC;
  * GPU (-m gpu): the kernels walk all chains of a kind as one batch, state resident on the device, same CRCs; the low-power
    chains a second time as interleaved stereo (chain 2k with chain 2k+1).
Not pinned to the reference by this file: grids no bitstream can say (_fuzz_frame's wild 2: the reference's process ends
without a result on them) and a band limit that moves inside a chain (the reference-side loop did not finish within a time
limit); those still meet only the shared source."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

import sbr_capture as cap
from sbr_grid_cases import grid_coverage_gaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_sbr_chains import chain_pcm  # noqa: E402  (the generator's own PCM function: data, not reference code)

P16 = ctypes.POINTER(ctypes.c_int16)
CH = np.load(os.path.join(ROOT, "tests", "golden", "sbr_grid_chains.npz"))
PCM_KIND = {"lp": 4, "hq": 5}      # tools/make_golden_sbr_grid_chains.py: PCM_KIND


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("kind", ["lp", "hq"])
def test_fixture_covers_the_grids_it_says(kind):
    frm, hdr, ret = CH[kind + "_frame"], CH[kind + "_header"], CH[kind + "_ret"]
    assert ret.shape == (16, 24)
    frames = [cap.Frame.from_buffer_copy(np.ascontiguousarray(x).tobytes()) for x in frm.reshape(-1, frm.shape[-1])]
    headers = [cap.Header.from_buffer_copy(np.ascontiguousarray(x).tobytes()) for x in hdr.reshape(-1, hdr.shape[-1])]
    assert grid_coverage_gaps(frames, headers, ret, min_late=20) == []
    for f in frames:      # and every grid is one a bitstream can say
        b = [f.border_vec[e] for e in range(f.num_env + 1)]
        assert 1 <= f.num_env <= 5 and all(x < y for x, y in zip(b, b[1:])) and 0 <= b[0] <= 3 and 13 <= b[-1] <= 19, b
        mid = b[-1] if f.num_env == 1 else b[(f.num_env + 1) // 2]
        assert [f.noise_border_vec[i] for i in range(f.num_noise_env + 1)] == ([b[0], b[-1]] if f.num_env == 1 else [b[0], mid, b[-1]])


@pytest.mark.parametrize("build", ["", "_seq"])
@pytest.mark.parametrize("kind", ["lp", "hq"])
def test_oracle_walks_the_reference_chains(oracle, kind, build):
    """build "": two envelopes per pass; "_seq": the one-envelope chain (oracle/oracle_sbr_seq.cpp)"""
    hq = kind == "hq"
    hdr, frm, ret = CH[kind + "_header"], CH[kind + "_frame"], CH[kind + "_ret"]
    fn = getattr(oracle.lib, "xo_sbr_dec_" + kind + build)
    n_chains, steps = ret.shape
    for c in range(n_chains):
        st = np.ascontiguousarray(CH[kind + "_st0"][c]).copy()
        ps = np.ascontiguousarray(CH["hq_ps0"][c]).copy() if hq else None
        for s in range(steps):
            pin = np.ascontiguousarray(chain_pcm(PCM_KIND[kind], c, s))
            h, f = np.ascontiguousarray(hdr[c, s]), np.ascontiguousarray(frm[c, s])
            if hq:
                out = np.zeros(4096, np.int16)
                pf = np.ascontiguousarray(CH["hq_ps_frame"][c, s])
                rc = fn(vp(h), vp(f), vp(st), vp(pf), vp(ps), pin.ctypes.data_as(P16), 1, out.ctypes.data_as(P16), 2)
            else:
                out = np.zeros(2048, np.int16)
                rc = fn(vp(h), vp(f), vp(st), pin.ctypes.data_as(P16), 1, out.ctypes.data_as(P16), 1)
            assert rc == ret[c, s], (c, s)
            assert crc(out) == CH[kind + "_crc_pcm"][c, s], ("pcm", c, s)
            assert crc(st) == CH[kind + "_crc_state"][c, s], ("state", c, s)
            if hq:
                assert crc(ps) == CH["hq_crc_ps"][c, s], ("ps state", c, s)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lp", "hq", "lp_stereo"])
def test_gpu_walks_the_reference_chains(kind):
    """lp_stereo: the low-power chains as eight interleaved stereo pairs (in_ch_fac = out_ch_fac = 2), chain 2k left,
    chain 2k+1 right: same CRCs per channel"""
    import torch
    import libxaac_amd
    stereo = kind == "lp_stereo"
    kind = kind[:2]
    hq = kind == "hq"
    ctx = libxaac_amd.XaacContext(0, 0)
    hdr, frm, ret = CH[kind + "_header"], CH[kind + "_frame"], CH[kind + "_ret"]
    n, steps = ret.shape
    fac = 2 if stereo else 1
    t_st = torch.from_numpy(np.ascontiguousarray(CH[kind + "_st0"])).cuda()
    t_ps = torch.from_numpy(np.ascontiguousarray(CH["hq_ps0"])).cuda() if hq else None
    ws = torch.zeros(ctx.sbr_hq_workspace_bytes(n, True) if hq else ctx.sbr_lp_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    for s in range(steps):
        pcm = np.stack([chain_pcm(PCM_KIND[kind], c, s) for c in range(n)])
        if stereo:
            pcm = pcm.reshape(n // 2, 2, 1024).transpose(0, 2, 1)      # L R L R ...
        pin = torch.from_numpy(np.ascontiguousarray(pcm).reshape(-1)).cuda()
        status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        th = torch.from_numpy(np.ascontiguousarray(hdr[:, s])).cuda()
        tf = torch.from_numpy(np.ascontiguousarray(frm[:, s])).cuda()
        if hq:
            out = torch.zeros(n * 4096, dtype=torch.int16, device="cuda")
            tpf = torch.from_numpy(np.ascontiguousarray(CH["hq_ps_frame"][:, s])).cuda()
            ctx.sbr_hq_process_batch(pin, th, tf, t_st, out, ws, tpf, t_ps, status)
        else:
            out = torch.zeros(n * 2048, dtype=torch.int16, device="cuda")
            ctx.sbr_lp_process_batch(pin, th, tf, t_st, out, ws, status, fac, fac)
        torch.cuda.synchronize()
        assert np.array_equal(status.cpu().numpy(), ret[:, s]), s
        o = out.cpu().numpy()
        o = o.reshape(n // 2, 2048, 2).transpose(0, 2, 1).reshape(n, 2048) if stereo else o.reshape(n, -1)
        stn = t_st.cpu().numpy()
        for c in range(n):
            assert crc(o[c]) == CH[kind + "_crc_pcm"][c, s], ("pcm", c, s)
            assert crc(stn[c]) == CH[kind + "_crc_state"][c, s], ("state", c, s)
        if hq:
            psn = t_ps.cpu().numpy()
            for c in range(n):
                assert crc(psn[c]) == CH["hq_crc_ps"][c, s], ("ps state", c, s)
    ctx.close()
