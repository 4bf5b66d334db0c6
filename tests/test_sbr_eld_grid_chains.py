"""tests/golden/sbr_eld_grid_chains.npz: 1152 calls of the REAL ixheaacd_sbr_dec run as an AAC-ELD channel's (low-delay SBR:
LD analysis bank, block floating point, HF generator, envelope adjuster, LD synthesis bank on 16 or 15 QMF slots), made by
tools/make_golden_sbr_eld_grid_chains.py as 12 chains of 96 steps -- one per (stream, channel) of the eight layout streams of
tests/golden/streams_ld (eight SBR band layouts, mono and stereo, six channels per frame length) -- with the state carried by
the reference itself.  tests/golden/sbr_eld_chains.npz keeps the grids and the one band layout of its two streams; here three
steps of four take a grid from tests/sbr_grid_cases.py: legal_ld_grid_frame, every grid a low-delay bitstream can say: FIXFIX
with 1, 2, 4 or 8 envelopes (4 and 8: all envelopes but the last empty, and an empty noise envelope) and LD_TRAN at every
transient position, the noise border at envelope 1, free freq_res per envelope.
(profiles/sbr_eld_grid_chains_coverage.txt: grids and layouts of both files side by side.)
  * the committed file covers what it says (the generator asserts the same before it writes), and every grid in it is one the
    rules of the low-delay grid produce;
  * CPU: the oracle (xo_sbr_dec_eld) walks every chain with its own state carried: every return code, and the CRC32s of the PCM,
    of the state and of the rows the synthesis bank hands on; a refused channel of a batch is left as include/xaac_amd.h says;
  * GPU (-m gpu), states resident on the device: xaac_sbr_eld_process_batch walks (a) all chains of a frame length as one batch
    (six channels: the banks take four to a workgroup, so the tail workgroup runs), (b) the same chains as interleaved stereo
    pairs without status and handed-on rows, (c) step 0 as batches of 1, 3 and 5 channels, (d) two steps with a refused channel
    among good ones: the neighbours as if it were not there, the refused one as the oracle leaves it."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

import sbr_capture as cap
from sbr_grid_cases import ld_grid_coverage_gaps, ld_grid_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_sbr_chains import chain_pcm  # noqa: E402  (the generator's own input function: data, not reference code)

CH = np.load(os.path.join(ROOT, "tests", "golden", "sbr_eld_grid_chains.npz"))
P16, P32 = ctypes.POINTER(ctypes.c_int16), ctypes.POINTER(ctypes.c_int32)
PCM_CHAIN0 = 16      # tools/make_golden_sbr_eld_grid_chains.py: PCM_CHAIN0
N_CHAINS = len(CH["n_slots"])
ROWS = [np.nonzero(CH["step_chain"] == c)[0] for c in range(N_CHAINS)]
FILL16, FILL32 = 0x5a5a, 0x5a5a5a5a      # what the output arrays hold before a call: what a refused channel must leave


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pcm_of(c, s, n):
    return np.ascontiguousarray(chain_pcm(3, PCM_CHAIN0 + c, s)[:32 * n])


def chains_of(n_slots):
    return [c for c in range(N_CHAINS) if int(CH["n_slots"][c]) == n_slots]


def structs():
    return ([cap.Frame.from_buffer_copy(np.ascontiguousarray(x).tobytes()) for x in CH["frame"]],
            [cap.Header.from_buffer_copy(np.ascontiguousarray(x).tobytes()) for x in CH["header"]])


def oracle_eld(oracle):
    fn = oracle.lib.xo_sbr_dec_eld
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 3 + [P16, ctypes.c_int, P16, ctypes.c_int, P32]
    fs = oracle.lib.xo_sbr_dec_eld_slots
    fs.restype = ctypes.c_int
    fs.argtypes = fn.argtypes + [ctypes.c_int]
    return fn, fs


def refused_cases(n_slots):
    """(step, victim's position in the batch of chains_of(n_slots), header, frame) of the two refused channels: at step 0 a
    header of the other frame length, at step 1 a frame whose last border lies above num_time_slots"""
    mine, other = chains_of(n_slots), chains_of(31 - n_slots)
    j = 2
    h0 = np.ascontiguousarray(CH["header"][ROWS[other[0]][0]]).copy()
    f0 = np.ascontiguousarray(CH["frame"][ROWS[mine[j]][0]]).copy()
    h1 = np.ascontiguousarray(CH["header"][ROWS[mine[j]][1]]).copy()
    f1 = cap.Frame.from_buffer_copy(np.ascontiguousarray(CH["frame"][ROWS[mine[j]][1]]).tobytes())
    f1.border_vec[f1.num_env] = n_slots + 1
    return [(0, j, h0, f0), (1, j, h1, np.frombuffer(bytes(f1), np.uint8).copy())]


def test_fixture_covers_what_it_says():
    frames, headers = structs()
    assert CH["ret"].size >= 1000 and CH["st0"].shape[1] == ctypes.sizeof(cap.EldState)
    assert ld_grid_coverage_gaps(frames, headers, CH["ret"], slots=(16, 15), step_chain=CH["step_chain"]) == []
    for c in range(N_CHAINS):       # a chain keeps its frame length
        assert {int(headers[r].num_time_slots) for r in ROWS[c]} == {int(CH["n_slots"][c])}


def test_every_grid_is_one_a_low_delay_bitstream_can_say():
    frames, headers = structs()
    for f, h in zip(frames, headers):
        n = int(h.num_time_slots)
        assert ld_grid_kind(f, n) is not None, ([f.border_vec[e] for e in range(9)], f.num_env, f.transient_env)
        assert h.time_step == 1 and h.num_columns == n and f.frame_class == 0


def test_oracle_walks_the_reference_chains(oracle):
    fn, _ = oracle_eld(oracle)
    for c, rows in enumerate(ROWS):
        n = int(CH["n_slots"][c])
        st = CH["st0"][c].copy()
        for s, r in enumerate(rows):
            pin = pcm_of(c, s, n)
            po, hand = np.zeros(64 * n, np.int16), np.zeros(16 * 128, np.int32)
            h, f = np.ascontiguousarray(CH["header"][r]), np.ascontiguousarray(CH["frame"][r])
            rc = fn(vp(h), vp(f), vp(st), pin.ctypes.data_as(P16), 1, po.ctypes.data_as(P16), 1, hand.ctypes.data_as(P32))
            want = CH["crc"][r]
            assert rc == CH["ret"][r], (c, s)
            assert crc(po) == want[0], ("pcm", c, s)
            assert crc(st) == want[1], ("state", c, s)
            assert crc(hand[:128 * n]) == want[2], ("handed-on rows", c, s)


def _oracle_refused(fs, n_slots):
    """the oracle's result for the refused channel of refused_cases(n_slots), its state carried over the two steps:
    [(rc, state, pcm_out, handed-on rows)]"""
    mine = chains_of(n_slots)
    out = []
    st = None
    for s, j, h, f in refused_cases(n_slots):
        c = mine[j]
        st = CH["st0"][c].copy() if st is None else st.copy()
        pin = pcm_of(c, s, n_slots)
        po, hand = np.full(64 * n_slots, FILL16, np.int16), np.full(n_slots * 128, FILL32, np.int32)
        rc = fs(vp(h), vp(f), vp(st), pin.ctypes.data_as(P16), 1, po.ctypes.data_as(P16), 1, hand.ctypes.data_as(P32), n_slots)
        out.append((rc, st.copy(), po, hand))
    return out


@pytest.mark.parametrize("n_slots", [16, 15])
def test_oracle_leaves_a_refused_channel_as_the_header_says(oracle, n_slots):
    """include/xaac_amd.h, xaac_sbr_eld_batch.status: -1; the analysis bank's state has moved on by the frame -- to where the
    good call on the same samples takes it --, nothing else of the state, no sample and no handed-on row has changed"""
    fn, fs = oracle_eld(oracle)
    mine = chains_of(n_slots)
    ana = slice(0, ctypes.sizeof(cap.EldAna))
    prev = None
    for (s, j, _, _), (rc, st, po, hand) in zip(refused_cases(n_slots), _oracle_refused(fs, n_slots)):
        c = mine[j]
        before = CH["st0"][c] if prev is None else prev
        assert rc == -1
        assert np.array_equal(st[ana.stop:], before[ana.stop:]) and np.all(po == FILL16) and np.all(hand == FILL32)
        good = before.copy()        # the fixture's own header and frame of step 0 on this state and these samples: the bank's state alone is compared
        r = ROWS[c][0]
        h, f = np.ascontiguousarray(CH["header"][r]), np.ascontiguousarray(CH["frame"][r])
        o2, h2 = np.zeros(64 * n_slots, np.int16), np.zeros(16 * 128, np.int32)
        pin = pcm_of(c, s, n_slots)
        assert fn(vp(h), vp(f), vp(good), pin.ctypes.data_as(P16), 1, o2.ctypes.data_as(P16), 1, h2.ctypes.data_as(P32)) == 0
        assert np.array_equal(st[ana], good[ana]) and not np.array_equal(st[ana], before[ana])
        prev = st


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
class _Gpu:
    """a batch of chains with their states resident on the device"""

    def __init__(self, chains, n_slots, stereo=False):
        import torch
        import libxaac_amd
        self.torch, self.chains, self.n, self.m, self.fac = torch, chains, n_slots, len(chains), 2 if stereo else 1
        self.ctx = libxaac_amd.XaacContext(0, 0)
        assert CH["st0"].shape[1] == libxaac_amd.SBR_ELD_STATE_BYTES
        self.st = torch.from_numpy(np.ascontiguousarray(CH["st0"][chains])).cuda()
        self.ws = torch.zeros(self.ctx.sbr_eld_workspace_bytes(self.m), dtype=torch.uint8, device="cuda")

    def step(self, s, replace=None, with_status=True):
        """one call on step s of every chain (replace: {position: (header, frame)}) -> status, PCM [m, 64 n], states,
        handed-on rows [m, 128 n] as numpy (status and rows None without with_status)"""
        torch, m, n, fac = self.torch, self.m, self.n, self.fac
        rows = [ROWS[c][s] for c in self.chains]
        hd, fr = np.ascontiguousarray(CH["header"][rows]), np.ascontiguousarray(CH["frame"][rows])
        for j, (h, f) in (replace or {}).items():
            hd[j], fr[j] = h, f
        pcm = np.stack([pcm_of(c, s, n) for c in self.chains])
        if fac == 2:
            pcm = pcm.reshape(m // 2, 2, 32 * n).transpose(0, 2, 1)      # L R L R ...
        pin = torch.from_numpy(np.ascontiguousarray(pcm).reshape(-1)).cuda()
        out = torch.full((m * 64 * n,), FILL16, dtype=torch.int16, device="cuda")
        hand = torch.full((m * n * 128,), FILL32, dtype=torch.int32, device="cuda") if with_status else None
        status = torch.full((m,), 7, dtype=torch.int32, device="cuda") if with_status else None
        self.ctx.sbr_eld_process_batch(pin, torch.from_numpy(hd).cuda(), torch.from_numpy(fr).cuda(), self.st, out, self.ws, n,
                                       status=status, in_ch_fac=fac, out_ch_fac=fac, qmf_handed_on=hand)
        assert self.ctx.last_launch() == {"grid": m, "block": 64, "lds_bytes": 0}
        self.ctx.sync()
        o = out.cpu().numpy()
        o = o.reshape(m // 2, 64 * n, 2).transpose(0, 2, 1).reshape(m, 64 * n) if fac == 2 else o.reshape(m, -1)
        return (status.cpu().numpy() if with_status else None, o, self.st.cpu().numpy(),
                hand.cpu().numpy().reshape(m, -1) if with_status else None)

    def check(self, s, got, skip=()):
        status, o, stn, hd = got
        rows = [ROWS[c][s] for c in self.chains]
        for j, r in enumerate(rows):
            if j in skip:
                continue
            want = CH["crc"][r]
            if status is not None:
                assert status[j] == CH["ret"][r], ("status", self.chains[j], s)
            assert crc(o[j]) == want[0], ("pcm", self.chains[j], s)
            assert crc(stn[j]) == want[1], ("state", self.chains[j], s)
            if hd is not None:
                assert crc(hd[j]) == want[2], ("handed-on rows", self.chains[j], s)


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [16, 15])
def test_gpu_walks_the_reference_chains_as_one_batch(n_slots):
    """(a): six channels -- a workgroup of four and a tail workgroup of two in both bank launches"""
    mine = chains_of(n_slots)
    assert len(mine) % 2 == 0 and len(mine) % 4 != 0
    g = _Gpu(mine, n_slots)
    for s in range(len(ROWS[mine[0]])):
        g.check(s, g.step(s))
    g.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [16, 15])
def test_gpu_walks_the_reference_chains_as_interleaved_stereo(n_slots):
    """(b): chain 2k left, chain 2k+1 right (in_ch_fac = out_ch_fac = 2), no status and no handed-on rows asked for"""
    mine = chains_of(n_slots)
    g = _Gpu(mine, n_slots, stereo=True)
    for s in range(len(ROWS[mine[0]])):
        g.check(s, g.step(s, with_status=False))
    g.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 3, 5])
@pytest.mark.parametrize("n_slots", [16, 15])
def test_gpu_small_batches(n_slots, m):
    """(c): step 0 from fresh states: the tail workgroups of both bank launches with 1, 3 and 1 (behind four) channels"""
    g = _Gpu(chains_of(n_slots)[-m:], n_slots)
    g.check(0, g.step(0))
    g.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [16, 15])
def test_gpu_refused_channel_among_good_ones(oracle, n_slots):
    """(d): the neighbours produce the fixture's CRCs as if the refused channel were not there; the refused channel has status -1
    and the state, samples and handed-on rows xo_sbr_dec_eld_slots leaves for the same call (include/xaac_amd.h:
    xaac_sbr_eld_batch.status: the analysis bank's state moved on, nothing else touched)"""
    _, fs = oracle_eld(oracle)
    g = _Gpu(chains_of(n_slots), n_slots)
    for (s, j, h, f), (rc, st, po, hand) in zip(refused_cases(n_slots), _oracle_refused(fs, n_slots)):
        assert 0 < j < g.m - 1 and rc == -1
        got = g.step(s, replace={j: (h, f)})
        g.check(s, got, skip=(j,))
        status, o, stn, hd = got
        assert status[j] == -1, s
        assert np.array_equal(stn[j], st), ("state of the refused channel", s, np.nonzero(stn[j] != st)[0][:8])
        assert np.array_equal(o[j], po) and np.array_equal(hd[j], hand), ("output of the refused channel", s)
    g.ctx.close()
