"""Two phases of the frame-at-once parametric-stereo arrangement (libxaac_amd/csrc/sbr_ps_frame.h) on the host.

P3, the group sums of transient-detector bins 14..19: the helper (xp_gsum_addend / xp_gsum_scan / xp_gsum_sum: a running sum
modulo 2^32 over the bands, the difference at a group's borders, one unsigned clamp) against the sequential fx_add_sat loop of
sbr_ps.h: xp_bin_power, and the bound the wrapping sums rest on (xp_gsum_fits) on the tables the library is built with.

P6 (and everything else): whole frames of xp_ps_frame<32> and <30> against the slot loop, on the side info and PS states of
the chains of tests/ps_walk_cases.py (both variants) and full-scale noise matrices.

tests/ps_phases_shim.cpp holds the host entry points; tests/ps_phases_lib.py compiles it with g++."""
import ctypes
import os

import numpy as np
import pytest

import ps_phases_lib as ppl
import ps_walk_cases as pw
import sbr_capture as cap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P32 = ctypes.POINTER(ctypes.c_int32)
BORDERS = [9, 11, 14, 18, 23, 35, 64]      # tables_ps.inc: borders_group[16..22]
SHIFTS = [0, 1, 1, 2, 3, 4]                # group_shift
MAX = 0x7fffffff
USBS = [9, 10, 11, 12, 14, 16, 18, 20, 23, 29, 35, 50, 64]


@pytest.fixture(scope="module")
def shim(oracle):
    return ppl.load(os.path.join(ROOT, "oracle", "liboracle.so"))


def sums(shim, pw64, usb):
    pw64 = np.ascontiguousarray(pw64, np.int32)
    new, ref = np.zeros(6, np.int32), np.zeros(6, np.int32)
    shim.xpt_group_sums(pw64.ctypes.data_as(P32), int(usb), new.ctypes.data_as(P32), ref.ctypes.data_as(P32))
    return new, ref


def exact(pw64, usb):
    """the sums in unbounded integers, clamped: what both must give"""
    return np.array([min(MAX, sum(int(pw64[sb]) >> SHIFTS[g] for sb in range(BORDERS[g], min(BORDERS[g + 1], usb))))
                     for g in range(6)], np.int64)


def check(shim, pw64, usb, tag):
    new, ref = sums(shim, pw64, usb)
    assert np.array_equal(new, ref), (tag, usb, new, ref)
    assert np.array_equal(new.astype(np.int64), exact(pw64, usb)), (tag, usb, new)
    return new


def test_the_bound_holds_for_the_tables(shim):
    assert shim.xpt_gsum_fits() == 1
    # ... and the borders and shifts this file works with are the tables' (tools/gen_tables_ps.py writes them)
    txt = open(os.path.join(ROOT, "libxaac_amd", "csrc", "tables_ps.inc")).read()
    nums = lambda name: [int(v) for v in txt.split("/* %s */ {" % name)[1].split("}")[0].replace("\n", " ").split(",") if v.strip()]
    assert nums("borders_group")[16:23] == BORDERS and nums("group_shift") == SHIFTS
    assert all((BORDERS[g + 1] - BORDERS[g]) * (MAX >> SHIFTS[g]) < 2 ** 32 for g in range(6))


def test_random_powers(shim):
    rng = np.random.default_rng(31)
    saturated = 0
    for k in range(400):
        top = int(rng.integers(8, 32))
        pw64 = rng.integers(0, 2 ** top, 64, dtype=np.int64).clip(0, MAX)
        usb = 64 if k % 2 == 0 else int(rng.integers(0, 65))
        saturated += int((check(shim, pw64, usb, ("random", k)) == MAX).sum())
    assert saturated >= 10         # some of the draws reach the clamp


def test_every_addend_at_its_maximum(shim):
    """(2^31 - 1) >> shift in every band: the bound case of every group, the largest sums a group can have"""
    pw64 = np.full(64, MAX, np.int64)
    for usb in USBS:
        new = check(shim, pw64, usb, "max")
        for g in range(6):
            n = min(BORDERS[g + 1], usb) - BORDERS[g]
            assert new[g] == (0 if n <= 0 else min(MAX, n * (MAX >> SHIFTS[g])))
    pw64[:9] = MAX                  # bands below 9 belong to no group
    assert np.array_equal(check(shim, pw64, 64, "max"), np.full(6, MAX))


def _fill(g, total):
    """addends of group g (each at most MAX >> shift) that add up to total, as powers (addend << shift)"""
    pw64 = np.zeros(64, np.int64)
    left = total
    for sb in range(BORDERS[g], BORDERS[g + 1]):
        a = min(left, MAX >> SHIFTS[g])
        pw64[sb] = a << SHIFTS[g]
        left -= a
    assert left == 0
    return pw64


def test_sums_at_the_clamp_and_one_above(shim):
    for g in range(6):
        for total, want in ((MAX - 1, MAX - 1), (MAX, MAX), (MAX + 1, MAX), (MAX + 2, MAX)):
            pw64 = _fill(g, total)
            new = check(shim, pw64, 64, ("clamp", g, total))
            assert new[g] == want and (np.delete(new, g) == 0).all()
            # the low bits the group's shift drops change nothing
            pw64[BORDERS[g]:BORDERS[g + 1]] |= (1 << SHIFTS[g]) - 1
            assert check(shim, pw64, 64, ("clamp+", g, total))[g] == want
            # the same sum with the neighbours full: the differences of the running sum stay apart
            pw64[9:BORDERS[g]] = MAX
            pw64[BORDERS[g + 1]:] = MAX
            assert check(shim, pw64, 64, ("clamp, full neighbours", g, total))[g] == want


def test_band_limit_at_every_border_and_inside_every_group(shim):
    rng = np.random.default_rng(32)
    for usb in USBS:
        for k in range(20):
            pw64 = rng.integers(0, 2 ** int(rng.integers(20, 32)), 64, dtype=np.int64).clip(0, MAX)
            new = check(shim, pw64, usb, ("usb", k))
            assert all(new[g] == 0 for g in range(6) if BORDERS[g] >= usb)


# ---- whole frames ----------------------------------------------------------------------------------------------------

def _frame(shim, ns, phased, ps, pf, x, sc):
    p = cap.PsState.from_buffer_copy(bytes(ps))
    f = cap.PsFrame.from_buffer_copy(bytes(pf))
    xl, xr = np.zeros(ns * 128, np.int32), np.zeros(ns * 128, np.int32)
    ps_scale = shim.xpt_ps_frame(ns, phased, ctypes.byref(p), ctypes.byref(f), x.ctypes.data_as(P32), *sc,
                                 xl.ctypes.data_as(P32), xr.ctypes.data_as(P32))
    return ps_scale, xl, xr, p


def _noise_matrix(rng, step, i):
    """38 rows of 64 re | 64 im: noise whose level falls with the band, full scale in every third stream-frame"""
    top = [31, 27, 22][(step + i) % 3]
    x = rng.integers(-2 ** (top - 1), 2 ** (top - 1), (38, 2, 64), dtype=np.int64)
    x >>= (np.arange(64) // 8)[None, None, :] * ((step + i) % 2)
    return np.ascontiguousarray(x.reshape(38 * 128).astype(np.int32))


def _whole_frames(shim, oracle, ns, variant):
    steps = pw.chain(oracle, variant)
    rng = np.random.default_rng(33 + ns)
    states = [cap.PsState.from_buffer_copy(bytes(p)) for p in steps[0]["ps_in"]]
    mid_frame = 0
    for k, d in enumerate(steps):
        for i in range(0, pw.STREAMS, 2):
            pf = cap.PsFrame.from_buffer_copy(bytes(d["ps_frames"][i]))
            for e in range(7):      # a 30-slot grid ends at border 30 (the kernel clamps the same way)
                pf.border_position[e] = min(int(pf.border_position[e]), ns)
            st_in, st_out = d["st_in"][i], d["want"][i][2]
            sc = (int(st_out.lb_scale), int(st_in.ov_lb_scale), int(st_out.hb_scale), int(st_in.st_syn_scale),
                  int(st_in.syn_lsb), int(st_in.syn_usb))
            x = _noise_matrix(rng, k, i)
            mid_frame += int(states[i].usb != sc[5] and 0 < pf.border_position[0] < ns)
            a = _frame(shim, ns, 0, states[i], pf, x, sc)
            b = _frame(shim, ns, 1, states[i], pf, x, sc)
            tag = (ns, variant, k, i)
            assert a[0] == b[0], tag
            assert np.array_equal(a[1], b[1]), (tag, "left", int(np.sum(a[1] != b[1])))
            assert np.array_equal(a[2], b[2]), (tag, "right", int(np.sum(a[2] != b[2])))
            assert not cap.diff_state(a[3], b[3]), (tag, cap.diff_state(a[3], b[3])[:3])
            states[i] = a[3]
    return mid_frame


@pytest.mark.parametrize("ns", [32, 30])
def test_whole_frames_plain(shim, oracle, ns):
    _whole_frames(shim, oracle, ns, "plain")


@pytest.mark.parametrize("ns", [32, 30])
def test_whole_frames_with_the_band_limit_switching_in_mid_frame(shim, oracle, ns):
    """usb_prev != usb and the first border inside the frame: the group sums read the old limit up to that slot"""
    assert _whole_frames(shim, oracle, ns, "moving") >= 3
