"""Envelope grids a bitstream can say, for the SBR frame side info of include/xaac_sbr.h (tests/sbr_capture.py: Frame):
the legal halves of the grid fuzz of tests/test_env_pairs_cpu.py (_fuzz_frame draws them through legal_grid_frame, number
for number), shared with the generators of the reference-made chains (tools/make_golden_sbr_grid_chains.py,
tests/test_esbr_core_oracle_vs_reference.py) -- and what a set of such frames has to cover before it is worth committing.
Data only: nothing here knows the reference or the oracle."""
import numpy as np


def set_grid(rng, h, f, n_env, borders):
    """writes a grid (n_env envelopes between the given borders) into the frame and draws everything that hangs on it:
    freq_res per envelope, the noise borders (1 noise envelope for 1 envelope, else 2, split at border (n_env + 1) / 2),
    transient_env in -1..n_env, inverse-filter modes, harmonics, packed envelope and noise-floor words"""
    f.num_env = n_env
    for e in range(9):
        f.border_vec[e] = int(borders[e]) if e < len(borders) else 0
    for e in range(8):
        f.freq_res[e] = int(rng.integers(0, 2))
    f.num_noise_env = 1 if n_env == 1 else 2
    f.noise_border_vec[0] = f.border_vec[0]
    f.noise_border_vec[1] = f.border_vec[(n_env + 1) // 2] if n_env > 1 else f.border_vec[n_env]
    f.noise_border_vec[2] = f.border_vec[n_env]
    f.transient_env = int(rng.integers(-1, n_env + 1))
    for i in range(h.num_if_bands):
        f.sbr_invf_mode[i] = int(rng.integers(0, 4))
    nsf = h.num_sf_bands[1]
    for i in range(nsf):
        f.add_harmonics[i] = int(rng.integers(0, 5) == 0)
    for i in range(len(f.int_env_sf_arr)):
        f.int_env_sf_arr[i] = int((int(rng.integers(0, 512)) << 6) | int(rng.integers(0, 40)))
    for i in range(len(f.int_noise_floor)):
        f.int_noise_floor[i] = int((int(rng.integers(0, 512)) << 6) | int(rng.integers(20, 50)))


def legal_grid_frame(rng, h, f, kind, slots=16):
    """1..5 envelopes on a grid a parser can produce.  kind 0: a fixed frame's, 0 = b0 < .. < b_n = 16;  kind 1: a variable
    frame's, first border 0..3, last border 13..19, strictly rising between.  slots: the frame's time slots, 16 or -- the
    960-sample cores -- 15, where the fixed grid ends at 15 and the variable one at 12..18 (the same draws in the same order)"""
    n_env = int(rng.integers(1, 6))
    if kind == 0:
        inner = sorted(rng.choice(np.arange(1, slots), n_env - 1, replace=False).tolist())
        borders = [0] + inner + [slots]
    else:
        assert kind == 1, kind
        lo, hi = int(rng.integers(0, 4)), int(rng.integers(slots - 3, slots + 4))
        inner = sorted(rng.choice(np.arange(lo + 1, hi), n_env - 1, replace=False).tolist())
        borders = [lo] + inner + [hi]
    set_grid(rng, h, f, n_env, borders)


# ---- what a fixture of such frames covers ----------------------------------------------------------------------------------
def transient_position(f):
    """where transient_env points: "none" (-1), "first" (0), "inner", "end" (num_env)"""
    t, n = int(f.transient_env), int(f.num_env)
    return "none" if t < 0 else "first" if t == 0 else "end" if t >= n else "inner"


def grid_key(f):
    """(num_env, first border, last border, transient position) of a frame"""
    return int(f.num_env), int(f.border_vec[0]), int(f.border_vec[f.num_env]), transient_position(f)


def grid_coverage_gaps(frames, headers=None, rets=None, min_late=20, early_end=True, slots=16):
    """the coverage conditions of a grid fixture that the given frames (sbr_capture.Frame), their headers
    (sbr_capture.Header) and return codes do NOT meet: a list of plain words, empty when all are met.  Without headers the
    conditions on limiter gains, interpolation and smoothing are left out (the eSBR chains keep them elsewhere); early_end
    False leaves out the last border below 16 (no bitstream says one, and the whole-frame eSBR boundary refuses it).  slots: the
    frame's time slots (16, or 15 for the 960-sample cores), which stand where 16 does in these words."""
    gaps = []
    need = lambda ok, what: None if ok else gaps.append(what)
    n_envs = {int(f.num_env) for f in frames}
    need(n_envs >= {1, 2, 3, 4, 5}, "num_env 1..5 (has %s)" % sorted(n_envs))
    need(any(f.freq_res[e] != f.freq_res[e + 1] for f in frames for e in range(f.num_env - 1)), "adjacent envelopes of different freq_res")
    need(any(f.num_env > 1 and f.freq_res[(f.num_env + 1) // 2 - 1] != f.freq_res[(f.num_env + 1) // 2] for f in frames),
         "a freq_res change at the noise border")
    pos = {transient_position(f) for f in frames}
    need(pos >= {"none", "first", "inner", "end"}, "transient_env -1 / 0 / inner / num_env (has %s)" % sorted(pos))
    first = [int(f.border_vec[0]) for f in frames]
    last = [int(f.border_vec[f.num_env]) for f in frames]
    need(any(b == 0 for b in first) and any(b > 0 for b in first), "first border 0 and > 0")
    need(any(b == slots for b in last) and (not early_end or any(b < slots for b in last)),
         "last border = %d%s" % (slots, " and < %d" % slots if early_end else ""))
    need(sum(b > slots for b in last) >= min_late, "%d steps with the last border > %d (has %d)" % (min_late, slots, sum(b > slots for b in last)))
    harm = [any(f.add_harmonics[i] for i in range(56)) for f in frames]
    need(any(harm) and not all(harm), "steps with and without add_harmonics")
    if headers is not None:
        need({int(h.limiter_gains) for h in headers} >= {0, 1, 2, 3}, "all four limiter_gains")
        need({int(h.interpol_freq) for h in headers} >= {0, 1}, "both interpol_freq")
        need({int(h.smoothing_mode) for h in headers} >= {0, 1}, "both smoothing_mode")
    if rets is not None:
        need(not np.any(np.asarray(rets)), "return code 0 on every step")
    return gaps
