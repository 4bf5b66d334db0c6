"""What the 30-slot fuzz cases of tests/sbr960_fuzz_cases.py cover, asserted on the oracle's side with no GPU and no
reference binaries: tests/test_sbr960_fuzz_gpu.py holds the kernels against exactly these cases, so a condition that stops
holding here is a hole in what the 30-slot instantiations are tested on.  Also: the generators shared with the 32-slot tests
and the committed reference-made chains still make, by default, the draws they made before they took a slot count."""
import zlib

import numpy as np

import ps_walk_cases as pw
import sbr960_fuzz_cases as fz
import sbr_capture as cap
import sbr_grid_cases as gc


def test_default_draws_of_the_shared_generators_are_unchanged():
    """CRCs taken before legal_grid_frame, _fuzz_ps and _borders_off_zero had a slot-count parameter"""
    r = pw.records()[0]
    rng = np.random.default_rng(960)
    h = cap.Header.from_buffer_copy(bytes(r["header"]))
    b = b""
    for kind in (0, 1, 0, 1, 1, 0):
        f = cap.Frame.from_buffer_copy(bytes(r["frame"]))
        gc.legal_grid_frame(rng, h, f, kind)
        b += bytes(f)
    assert zlib.crc32(b) & 0xffffffff == 0x5771966f
    b = b""
    for _ in range(4):
        pf = cap.PsFrame.from_buffer_copy(bytes(r["ps_frame"]))
        pw._fuzz_ps(rng, pf)
        b += bytes(pf)
        pw._borders_off_zero(rng, pf)
        b += bytes(pf)
    assert zlib.crc32(b) & 0xffffffff == 0x391876b9


def test_the_golden_records_are_30_slot_calls():
    for recs, low_pow, ps in ((fz.lp_records(), 1, 0), (fz.hq_records(), 0, 1)):
        assert 10 <= len(recs) <= 24
        for r in recs:
            assert (r["low_pow"], r["ps"], r["ret"]) == (low_pow, ps, 0)
            assert (r["header"].num_time_slots, r["header"].time_step, r["header"].num_columns) == (15, 2, 30)
            assert (r["pcm_out"][:, fz.N_OUT:] == 0).all() and (r["pcm_in"][fz.N_IN:] == 0).all()


def test_the_oracle_reproduces_the_golden_records(oracle):
    """the committed records through the 30-slot oracle (the whole streams: tests/test_sbr960_oracle_vs_reference.py)"""
    for r in fz.hq_records():
        rc, out, st, ps = fz.run_hq(oracle, r["header"], r["frame"], r["st0"], r["ps_frame"], r["ps0"],
                                    np.ascontiguousarray(r["pcm_in"][:fz.N_IN]))
        assert rc == 0 and np.array_equal(out[0::2], r["pcm_out"][0][:fz.N_OUT]) and np.array_equal(out[1::2], r["pcm_out"][1][:fz.N_OUT])
        assert not cap.diff_state(st, r["st1"]) and not cap.diff_state(ps, r["ps1"]), r["call"]
    for r in fz.lp_records():
        rc, out, st = fz.run_lp(oracle, r["header"], r["frame"], r["st0"], np.ascontiguousarray(r["pcm_in"][:fz.N_IN]))
        assert rc == 0 and np.array_equal(out, r["pcm_out"][0][:fz.N_OUT]) and not cap.diff_state(st, r["st1"]), r["call"]


def test_ps_cases_cover_what_they_claim(oracle):
    cs = fz.ps_cases(oracle)
    assert len(cs) == fz.PS_CASES == 6 * fz.BATCH and all(len(c["steps"]) == fz.PS_FRAMES == 3 for c in cs)
    # ring phase: every idx_long in front of the first frame of at least two cases
    assert all(sum(1 for c in cs if c["steps"][0]["ps_in"].idx_long == p) >= 2 for p in range(14))
    # return codes: a frame the oracle refuses is a generator bug, not a case
    assert all(s["want"][0] == 0 for c in cs for s in c["steps"])
    # PS envelopes: 1..5 of them, borders inside 0..30, first border at 0 and off 0, a border at 29, unused entries in 0..30
    grids = [fz.ps_borders(s["ps_frame"]) for c in cs for s in c["steps"]]
    assert {len(g) - 1 for g in grids if g[-1] == fz.NQ} >= {1, 2, 3, 4, 5}
    assert all(g[-1] == fz.NQ for g in grids), "every grid ends at the frame's end"
    assert any(g[0] == 0 for g in grids) and any(g[0] > 0 for g in grids)
    assert sum(fz.LATE_BORDER in g for g in grids) >= 2
    assert all(0 <= int(s["ps_frame"].border_position[e]) <= fz.NQ for c in cs for s in c["steps"] for e in range(7))
    assert {int(s["ps_frame"].iid_quant) for c in cs for s in c["steps"]} == {0, 1}
    # common_shift: all three signs, inside fx_shl_sat's range
    shifts = np.array([s["common_shift"] for c in cs for s in c["steps"]])
    assert (shifts < 0).sum() >= 3 and (shifts == 0).sum() >= 3 and (shifts > 0).sum() >= 3, shifts
    assert shifts.min() >= -31 and shifts.max() <= 31
    # band limit: dropped below the all-pass bands in front of frame 1, back up in front of frame 2
    rising = {"zero": 0, "mid": 0}
    for c in cs:
        for k, s in enumerate(c["steps"]):
            st_in = s["st_in"]
            assert 0 < st_in.syn_lsb < st_in.syn_usb < 64 or st_in.syn_usb < 23, (st_in.syn_lsb, st_in.syn_usb)
            b0 = int(s["ps_frame"].border_position[0])
            if c["mode"] != "never":
                if k == 1:
                    assert st_in.syn_usb < 23 and st_in.syn_usb < s["usb_prev"]
                if st_in.syn_usb > s["usb_prev"] > 0:
                    assert k == 2 and (b0 == 0 if c["mode"] == "zero" else b0 in fz.MID) and b0 + 14 < fz.NQ
                    rising[c["mode"]] += 1
            else:
                assert st_in.syn_usb == c["steps"][0]["st_in"].syn_usb
    assert rising["zero"] >= 5 and rising["mid"] >= 5, rising
    assert sum(1 for c in cs if any(s["st_in"].ov_lb_scale != s["want"][2].lb_scale for s in c["steps"])) >= fz.PS_CASES // 2
    # detector state
    zeroed = [c for c in cs if c["det"] == "zeroed"]
    full = [c for c in cs if c["det"] == "full"]
    recorded = [c for c in cs if c["det"] == "recorded"]
    assert len(zeroed) >= 3 and len(full) >= 3 and len(recorded) >= 3
    for c in zeroed:    # the limit at 20: energy = 0 survives in bins 18..19, the others have moved
        assert c["steps"][0]["st_in"].syn_usb == 20
        e = np.array([s["want"][3].energy_prev[:] for s in c["steps"]])
        assert (e[:, 18:] == 0).all(axis=1).any() and (e[:, :14] > 0).all(), e
    for c in full:      # went in at the top of the range; a rescale and 30 slots of decay later every bin still shows it
        assert all(v == fz.MAX for v in c["steps"][0]["ps_in"].energy_prev[:])
        e = np.array(c["steps"][0]["want"][3].peak_decay_diff[:])
        assert e.min() > 2 ** 12, e


def _grid_gaps(steps, min_late):
    frames = [f for d in steps for f in d["frames"]]
    headers = [h for d in steps for h in d["headers"]]
    rets = [w[0] for d in steps for w in d["want"]]
    # (a last border below 15 is in the cases wherever the boundary's screen, xs_side_info_bad, lets it through: it does)
    return gc.grid_coverage_gaps(frames, headers, rets, min_late=min_late, early_end=True, slots=fz.NTS)


def _common(steps, n):
    assert len(steps) == fz.FRAMES == 6 and all(len(d["frames"]) == n for d in steps)
    frames = [f for d in steps for f in d["frames"]]
    for f in frames:
        b = [int(f.border_vec[e]) for e in range(f.num_env + 1)]
        assert f.apply_processing and 1 <= f.num_env <= 5 and all(x < y for x, y in zip(b, b[1:]))
        assert 0 <= b[0] <= 3 and 12 <= b[-1] <= 18
    assert sum(f.border_vec[0] == 0 and f.border_vec[f.num_env] == fz.NTS for f in frames) >= n, "fixed grids: 0 = b0 < .. < b_n = 15"
    assert {int(f.sbr_invf_mode[0]) for f in frames} == {0, 1, 2, 3}
    assert {int(f.freq_res[0]) for f in frames} == {0, 1}
    moved = sum(int(f.max_qmf_subband_aac) != int(h.sub_band_start) for d in steps for f, h in zip(d["frames"], d["headers"]))
    assert moved >= 5, moved
    return frames


def test_hq_chains_cover_what_they_claim(oracle):
    for with_ps in (True, False):
        steps = fz.hq_chain(oracle, with_ps)
        _common(steps, fz.STREAMS)
        assert not _grid_gaps(steps, 15), _grid_gaps(steps, 15)
        assert all((h.channel_mode == 3) == with_ps for d in steps for h in d["headers"])
        amps = {int(np.abs(p).max()) for d in steps for p in d["pcm"]}
        assert max(amps) > 30000 and min(amps) <= 9
        if with_ps:
            assert {len(fz.ps_borders(pf)) - 1 for d in steps for pf in d["ps_frames"]} >= {1, 2, 3, 4, 5}
        else:       # the mono chain is the same streams without the tool, not the same output
            assert all(w[3] is None and w[1].shape == (fz.N_OUT,) for d in steps for w in d["want"])


def test_lp_chains_cover_what_they_claim(oracle):
    for stereo in (True, False):
        steps = fz.lp_chain(oracle, stereo)
        _common(steps, 2 * fz.BATCH if stereo else fz.BATCH)
        gaps = _grid_gaps(steps, 15 if stereo else 5)
        assert not gaps, gaps
        amps = sorted({int(np.abs(p).max()) for d in steps for p in d["pcm"]})
        assert amps[0] <= 9 and any(2000 < a <= 3000 for a in amps) and amps[-1] > 32000, amps


def test_list_case_reaches_above_band_48(oracle):
    steps = fz.list_case(oracle)
    assert len(steps[0]["recs"]) == fz.BATCH
    for d in steps:
        assert all(w[0] == 0 for w in d["want"])
        assert all(r["header"].sub_band_end <= 48 for r in d["recs"])
    st = steps[0]["st_in"]
    assert st[fz.WIDE_STREAMS[0]].syn_usb == 52
    ov = np.ctypeslib.as_array(st[fz.WIDE_STREAMS[1]].overlap).reshape(6, 2, 64)
    assert np.any(ov[:, :, 50:])
    for i in set(range(fz.BATCH)) - set(fz.WIDE_STREAMS):
        assert st[i].syn_usb <= 48 and st[i].codec_usb <= 48 and not np.any(np.ctypeslib.as_array(st[i].overlap).reshape(6, 2, 64)[:, :, 48:])


def test_malformed_case_is_refused_and_clamped(oracle):
    m = fz.malformed(oracle)
    assert len(m["recs"]) == fz.BATCH
    assert m["want"][fz.BAD_SBR][0] == -1 and m["want"][fz.BAD_PS][0] == -1
    # a border behind the 30-slot frame but inside 0..32, right behind borders the slot walk meets: where it is held to shows
    bp = [int(m["ps_frames"][fz.BAD_PS].border_position[e]) for e in range(7)]
    assert bp[0] == 0 and 0 < bp[1] < fz.NQ < bp[2] <= 32, bp
    assert any(not -32 <= v <= 32 for v in bp[3:]), bp
    # the refused SBR frame: the oracle has touched nothing either
    assert bytes(m["want"][fz.BAD_SBR][2]) == bytes(m["recs"][fz.BAD_SBR]["st0"])
    for i, r in enumerate(m["recs"]):
        if i not in (fz.BAD_SBR, fz.BAD_PS):
            w = m["want"][i]
            assert w[0] == 0 and np.array_equal(w[1][0::2], r["pcm_out"][0][:fz.N_OUT]) and not cap.diff_state(w[3], r["ps1"])
