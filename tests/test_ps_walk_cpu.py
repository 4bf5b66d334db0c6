"""The slot walk of the frame-at-once parametric-stereo arrangement (sbr_ps_frame.h, compiled for the host:
xo_sbr_dec_hq_phased) against the slot loop (xo_sbr_dec_hq) on chains whose shift in front of the left synthesis bank takes
every sign: the walk has one arrangement for common_shift <= 0 and one for > 0, and real chains only reach the first.
Inputs: tests/ps_walk_cases.py."""
import numpy as np

import ps_walk_cases as pw
import sbr_capture as cap


def _compare(oracle, variant):
    recs = pw.records()
    steps = pw.chain(oracle, variant)
    for k, d in enumerate(steps):
        for i, r in enumerate(recs):
            want = d["want"][i]
            got = pw.run(oracle.lib.xo_sbr_dec_hq_phased, r["header"], d["frames"][i], d["st_in"][i], d["ps_frames"][i],
                         d["ps_in"][i], d["pcm"][i])
            tag = (variant, k, i, d["common_shift"][i])
            assert got[0] == want[0], tag
            assert np.array_equal(got[1], want[1]), (tag, "pcm", int(np.sum(got[1] != want[1])))
            assert not cap.diff_state(got[2], want[2]), (tag, cap.diff_state(got[2], want[2])[:3])
            assert not cap.diff_state(got[3], want[3]), (tag, cap.diff_state(got[3], want[3])[:3])
    return steps


def test_every_sign_of_the_common_shift(oracle):
    pw.check_signs(_compare(oracle, "plain"))


def test_moving_band_limit_and_borders_off_slot_zero(oracle):
    pw.check_range(_compare(oracle, "moving"))
