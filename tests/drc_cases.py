"""Shared by tests/test_drc_cpu.py and tests/test_drc_gpu.py: the committed DRC streams (tests/golden/streams_drc,
tools/make_drc_streams.py), the reference-made spectra in front of and behind ixheaacd_drc_apply (tests/golden/drc_spec.npz,
tools/make_golden_drc.py), the flag sets as the two decoders take them, a numpy int64 model of the application and the side rows
the kernel and its twin are walked over."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_drc_streams import FLAG_SETS, NAMES  # noqa: E402

STREAMS = os.path.join(ROOT, "tests", "golden", "streams_drc")
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
REF = os.path.join(ROOT, "oracle", "_ref")
# FLAG_SETS as decode_streams' drc argument
DRC_ARGS = (dict(cut=1, boost=1), dict(cut=0.5, boost=0.25, target_level=96), dict(target_level=96), dict(target_level=124))
ONE = 1 << 25
WORDS = 33   # int32 words of xaac_drc_side: n_bands, end[16], fac[16]

_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "drc_spec.npz")))
        assert tuple(_gold["names"]) == NAMES and tuple(_gold["flag_sets"]) == tuple(" ".join(f) for f in FLAG_SETS)
    return _gold


def stream(name):
    return open(os.path.join(STREAMS, name + ".aac"), "rb").read()


def need(binary):
    import pytest
    if not os.path.exists(os.path.join(REF, binary)):
        pytest.fail("oracle/_ref/%s missing: the reference binaries did not travel with the snapshot" % binary)


def side_row(ends, facs):
    row = np.zeros(WORDS, np.int32)
    row[0] = len(ends)
    row[1:1 + min(len(ends), 16)] = ends[:16]
    row[17:17 + min(len(facs), 16)] = facs[:16]
    return row


def row_ok(row):
    n = int(row[0])
    return 1 <= n <= 16 and all(0 <= int(e) <= 1024 and int(e) % 4 == 0 for e in row[1:1 + n])


def model(row, spec):
    """ixheaacd_drc_apply's spectral branch in numpy int64 (drc_freq_dec.c:956-1017, :1098; :103-118 per line): a new array"""
    x = spec.astype(np.int64)
    if not row_ok(row):
        return spec.copy()
    start = 0
    for k in range(int(row[0])):
        end, fac = int(row[1 + k]), int(row[17 + k])
        if end > start:
            x[start:end] = np.clip((x[start:end] * fac) >> 25, -(1 << 31), (1 << 31) - 1)   # (>> on int64: a floor)
        start = end
    return x.astype(np.int32)


def fixed_rows():
    """the rows every size of the kernel test starts with: (side row, spectrum) pairs that name their case"""
    rng = np.random.default_rng(7)
    spec = lambda mag=1 << 27: rng.integers(-mag, mag, 1024, dtype=np.int64).astype(np.int32)
    fac = lambda n: rng.integers(1 << 20, 1 << 28, n)
    sat = spec(1 << 31)
    sat[:8] = [0x7fffffff, -0x80000000, 0x7fffffff, -0x80000000, 1 << 30, -(1 << 30), -1, 1]
    neg = -np.abs(spec(1 << 12)) - 1     # small negative lines: a floor, not a rounding toward zero
    return [
        ("one band of 1024", side_row([1024], fac(1)), spec()),
        ("sixteen bands", side_row(list(range(64, 1025, 64)), fac(16)), spec()),
        ("a first end of 4", side_row([4, 512, 1024], fac(3)), spec()),
        ("a last end below 1024", side_row([256, 700], fac(2)), spec()),
        ("non-monotonic ends", side_row([512, 128, 640, 64, 1024], fac(5)), spec()),
        ("identity", side_row([512, 1024], [ONE, ONE]), spec()),
        ("saturating factors", side_row([512, 1024], [(1 << 30) + 12345, 0x7fffffff]), sat),
        ("negative lines", side_row([1024], [ONE - 1]), neg),
        ("identity again", side_row([1024], [ONE]), spec()),
        ("refused: 17 bands", side_row([1024] * 17, fac(17)), spec()),
        ("refused: an end of 1028", side_row([512, 1028], fac(2)), spec()),
        ("refused: an end of 510", side_row([510, 1024], fac(2)), spec()),
        ("a zero factor", side_row([1024], [0]), spec()),
    ]


def random_rows(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        nb = int(rng.integers(1, 17))
        ends = (rng.integers(0, 257, nb) * 4).tolist()
        if rng.integers(0, 3) == 0:
            ends = sorted(ends)
        facs = np.where(rng.integers(0, 4, nb) == 0, ONE, rng.integers(0, 1 << 31, nb)).tolist()
        if rng.integers(0, 6) == 0:
            facs = [ONE] * nb
        mag = 1 << int(rng.integers(4, 32))
        out.append(("random", side_row(ends, facs), rng.integers(-mag, mag, 1024, dtype=np.int64).astype(np.int32)))
    return out


def rows(n):
    """n rows: the fixed ones in front (as many as fit), random ones behind"""
    return (fixed_rows() + random_rows(max(0, n - 13), 100 + n))[:n]


def with_two_elements_on_one_channel(data, at_frame):
    """the ADTS stream `data` (one of the committed stereo streams) with frame `at_frame` replaced by a frame of the same generator
    whose two dynamic_range_info elements both cover channel 0"""
    import make_drc_streams as m
    t, books = m.tables()
    wl = [w for w in t["sfb_48_1024"] if w > 0]
    ws = [w for w in t["sfb_48_128"] if w > 0]
    g = m.DrcGen(900, 3, wl, ws, books, 60)
    bad = g.frame_with(2, [dict(gains=[-20], excluded=[0, 1]), dict(gains=[30], prog_ref_level=100)])
    frames, pos = [], 0
    while pos + 7 <= len(data):
        n = ((data[pos + 3] & 3) << 11) | (data[pos + 4] << 3) | (data[pos + 5] >> 5)
        frames.append(data[pos:pos + n])
        pos += n
    frames[at_frame] = bad
    return b"".join(frames)
