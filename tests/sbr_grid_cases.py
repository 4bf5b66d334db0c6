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


# ---- low-delay SBR (AAC-ELD): the grids of sbr_ld_grid(), ISO/IEC 14496-3 ---------------------------------------------------
# bs_transient_position -> (num_env, border 1, border 2 or -1, transient_env): tables 4.A.89 (512-sample frames, 16 time slots)
# and 4.A.90 (480, 15 time slots) of the standard
LD_TRAN_512 = [(2, 4, -1, 0), (2, 5, -1, 0), (3, 2, 6, 1), (3, 3, 7, 1), (3, 4, 8, 1), (3, 5, 9, 1), (3, 6, 10, 1), (3, 7, 11, 1),
               (3, 8, 12, 1), (3, 9, 13, 1), (3, 10, 14, 1), (2, 11, -1, 1), (2, 12, -1, 1), (2, 13, -1, 1), (2, 14, -1, 1),
               (2, 15, -1, 1)]
LD_TRAN_480 = [(2, 4, -1, 0), (2, 5, -1, 0), (3, 2, 6, 1), (3, 3, 7, 1), (3, 4, 8, 1), (3, 5, 9, 1), (3, 6, 10, 1), (3, 7, 11, 1),
               (3, 8, 12, 1), (3, 9, 13, 1), (2, 10, -1, 1), (2, 11, -1, 1), (2, 12, -1, 1), (2, 13, -1, 1), (2, 14, -1, 1)]
LD_FIXFIX_NUM_ENV = (1, 2, 4, 8)
LD_FIXFIX_REL_BORDER = {1: 0, 2: 8, 4: 0, 8: 0}     # the relative border a FIXFIX frame of that many envelopes adds per envelope


def ld_tran_table(slots):
    assert slots in (16, 15), slots
    return LD_TRAN_512 if slots == 16 else LD_TRAN_480


def ld_grid(kind, slots):
    """the low-delay grid a bitstream says with kind ("fixfix", num_env) or ("ld_tran", bs_transient_position):
    (borders, noise borders, transient_env).  FIXFIX: borders 0, r, 2r, .., slots with the relative border r above -- 4 and 8
    envelopes are all empty but the last, and their noise border (envelope num_env / 2) is slot 0: an empty noise envelope.
    LD_TRAN: borders and transient_env from the table, the noise border always at envelope 1."""
    cls, v = kind
    if cls == "fixfix":
        assert v in LD_FIXFIX_NUM_ENV, v
        borders = [LD_FIXFIX_REL_BORDER[v] * e for e in range(v)] + [slots]
        mid, tran = v // 2, -1
    else:
        assert cls == "ld_tran", cls
        n_env, b1, b2, tran = ld_tran_table(slots)[v]
        borders = [0, b1] + ([b2] if n_env == 3 else []) + [slots]
        mid = 1
    noise = [0, slots] if len(borders) == 2 else [0, borders[mid], slots]
    return borders, noise, tran


def ld_grid_kinds(slots):
    return [("fixfix", n) for n in LD_FIXFIX_NUM_ENV] + [("ld_tran", p) for p in range(len(ld_tran_table(slots)))]


def ld_grid_kind(f, slots):
    """which grid of ld_grid_kinds(slots) a frame holds, freq_res included (one bit for all envelopes of a FIXFIX frame, one
    per envelope of an LD_TRAN frame); None when it is none of them"""
    if not 1 <= f.num_env <= 8:
        return None
    got = ([int(f.border_vec[e]) for e in range(f.num_env + 1)], [int(f.noise_border_vec[e]) for e in range(f.num_noise_env + 1)],
           int(f.transient_env))
    for kind in ld_grid_kinds(slots):
        if got == ld_grid(kind, slots):
            if kind[0] == "fixfix" and len({int(f.freq_res[e]) for e in range(f.num_env)}) != 1:
                return None
            return kind
    return None


def legal_ld_grid_frame(rng, h, f, slots):
    """a grid drawn uniformly from ld_grid_kinds(slots): FIXFIX with 1, 2, 4 or 8 envelopes or LD_TRAN at one of the 16 (15)
    transient positions.  Everything else is set_grid's draws; of those the noise borders and transient_env give way to the
    grid's own, and a FIXFIX frame keeps the first envelope's freq_res for all."""
    kinds = ld_grid_kinds(slots)
    kind = kinds[int(rng.integers(0, len(kinds)))]
    borders, noise, tran = ld_grid(kind, slots)
    set_grid(rng, h, f, len(borders) - 1, borders)
    f.frame_class = 0
    f.num_noise_env = len(noise) - 1
    for e in range(3):
        f.noise_border_vec[e] = noise[e] if e < len(noise) else 0
    f.transient_env = tran
    if kind[0] == "fixfix":
        for e in range(1, 8):
            f.freq_res[e] = f.freq_res[0]
    return kind


def band_layout(h):
    """what of a header's frequency tables tells one band layout from another"""
    return (int(h.sub_band_start), int(h.sub_band_end), (int(h.num_sf_bands[0]), int(h.num_sf_bands[1])), int(h.num_nf_bands),
            int(h.num_patches))


def ld_grid_coverage_gaps(frames, headers, rets, slots=(16, 15), step_chain=None, min_each=3, min_layouts=8):
    """the coverage conditions of a low-delay grid fixture that the given frames, their headers and return codes do NOT meet,
    as plain words (empty: all met).  slots: the frame lengths in time slots that have to be there; a step's own is its header's
    num_time_slots.  step_chain (optional): the chain each step belongs to, for the condition on the chain count."""
    gaps = []
    need = lambda ok, what: None if ok else gaps.append(what)
    need(not np.any(np.asarray(rets)), "return code 0 on every step")
    for n in slots:
        mine = [f for f, h in zip(frames, headers) if h.num_time_slots == n]
        seen = {}
        for f in mine:
            k = ld_grid_kind(f, n)
            seen[k] = seen.get(k, 0) + 1
        need(None not in seen, "%d slots: only grids a low-delay bitstream can say (%d others)" % (n, seen.get(None, 0)))
        for kind in ld_grid_kinds(n):
            need(seen.get(kind, 0) >= min_each, "%d slots: %s %d at least %d times (has %d)" % (n, kind[0], kind[1], min_each, seen.get(kind, 0)))
        if step_chain is not None:
            n_chains = len({int(c) for c, h in zip(step_chain, headers) if h.num_time_slots == n})
            need(n_chains % 2 == 0 and n_chains % 4 != 0, "%d slots: a chain count that is even and no multiple of 4 (has %d)" % (n, n_chains))
    need(any(f.freq_res[e] != f.freq_res[e + 1] for f in frames for e in range(f.num_env - 1)), "a freq_res change inside a frame")
    harm = [any(f.add_harmonics[i] for i in range(56)) for f in frames]
    need(any(harm) and not all(harm), "steps with and without add_harmonics")
    need({int(h.limiter_gains) for h in headers} >= {0, 1, 2, 3}, "all four limiter_gains")
    need({int(h.interpol_freq) for h in headers} >= {0, 1}, "both interpol_freq")
    need({int(h.smoothing_mode) for h in headers} >= {0, 1}, "both smoothing_mode")
    need({int(h.channel_mode) for h in headers} >= {1, 2}, "channel_mode 1 and 2")
    layouts = {band_layout(h) for h in headers}
    need(len(layouts) >= min_layouts, "%d band layouts (has %d)" % (min_layouts, len(layouts)))
    for n in slots:
        need(len({band_layout(h) for h in headers if h.num_time_slots == n}) >= 2, "%d slots: more than one band layout" % n)
    need({l[2] for l in layouts} >= {(6, 12), (7, 14), (8, 16)}, "num_sf_bands (6, 12), (7, 14) and (8, 16) (has %s)" % sorted({l[2] for l in layouts}))
    need({l[4] for l in layouts} >= {2, 3, 4}, "num_patches 2, 3 and 4 (has %s)" % sorted({l[4] for l in layouts}))
    need(any(l[1] == 64 for l in layouts), "a sub_band_end of 64")
    return gaps


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
