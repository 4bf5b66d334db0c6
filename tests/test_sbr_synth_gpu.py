"""The generator-made HE-AAC / HE-AACv2 streams of tests/golden/streams_synth_sbr (tools/make_synth_sbr_streams.py;
tests/test_sbr_synth_cpu.py says what they cover and pins the host front end to the reference) end to end on the GPU.

libxaac_amd/xaacdec_amd with -esbr:0 and with the default flags writes, for every committed stream, the file `oracle/_ref/xaacdec`
writes with the same flags, byte for byte, header included: against the committed CRC of that file (tests/golden/sbr_synth_ref.npz)
and, where oracle/_ref is built, against a fresh run -- after the check that the reference's file has its full length and is not
its decode of the core frames alone (tests/sbr_synth_cases.py: checked_reference_wav).  The whole set goes through one -ilist per
flag set (18 streams of 18 kinds: two GPU processes), three single files through -copies:3 -verify.  decode_streams and
decode_mixed give the same samples on six streams (a stereo, a mono and a PS one, each quiet and loud).  The stream whose output
rate would ask for the down-sampled bank is refused up front by all three, and nothing is written.  -esbr_hq:1 (the tolerance
path) is not part of this."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sbr_synth_cases as cs  # noqa: E402
from libxaac_amd import decoder  # noqa: E402

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
FLAG_IDS = ["esbr0", "default"]
SINGLE = ["st_sr08", "mono_sr07", "ps_sr09"]
SIX = ["st_sr06", "st_sr07", "mono_sr06", "mono_sr07", "ps_sr06", "ps_sr07"]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("sbr_synth_gpu"))


@pytest.fixture(scope="module")
def gold():
    return np.load(cs.GOLD)


def expected(row, k, gold, tmp):
    """(CRC32, size) of the reference's file for flag set k -- committed, and made again where the reference is built"""
    want = tuple(int(v) for v in gold[row[0] + "_wav"][3 * k:3 * k + 2])
    if cs.have_reference("xaacdec"):
        blob = cs.checked_reference_wav(row, cs.FLAG_SETS[k], tmp)
        assert (cs.crc(blob), len(blob)) == want, (row[0], "the committed CRC is not the reference's file")
    return want


@pytest.mark.parametrize("k", [0, 1], ids=FLAG_IDS)
def test_xaacdec_amd_writes_the_references_files_for_the_whole_set_in_one_list(k, gold, tmp):
    assert os.path.exists(CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
    out = os.path.join(tmp, "list_%d" % k)
    os.mkdir(out)
    lst = os.path.join(tmp, "list_%d.txt" % k)
    open(lst, "w").write("\n".join(cs.path(r[0]) for r in cs.DECODED) + "\n")
    p = subprocess.run([CLI, "-ilist:" + lst, "-odir:" + out, *cs.FLAG_SETS[k]], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-800:]
    bad = []
    for row in cs.DECODED:
        got = open(os.path.join(out, row[0] + ".wav"), "rb").read()
        want = expected(row, k, gold, tmp)
        if (cs.crc(got), len(got)) != want:
            detail = ""
            if cs.have_reference("xaacdec"):
                ref = cs.reference_wav(cs.path(row[0]), cs.FLAG_SETS[k], tmp)
                a, b = np.frombuffer(got[44:], np.int16), np.frombuffer(ref[44:], np.int16)
                n = min(len(a), len(b))
                at = np.nonzero(a[:n] != b[:n])[0]
                detail = "header %s, %d of %d samples differ, first in frame %s" % (
                    "equal" if got[:44] == ref[:44] else "differs", len(at), n, int(at[0]) // 4096 if len(at) else "-")
            bad.append((row[0], len(got), want[1], detail))
    assert not bad, bad


@pytest.mark.parametrize("k", [0, 1], ids=FLAG_IDS)
@pytest.mark.parametrize("name", SINGLE)
def test_three_copies_of_a_single_file_verify_and_equal_the_references_file(name, k, gold, tmp):
    row = [r for r in cs.DECODED if r[0] == name][0]
    out = os.path.join(tmp, "%s_%d.wav" % (name, k))
    p = subprocess.run([CLI, "-ifile:" + cs.path(name), "-ofile:" + out, "-copies:3", "-verify", *cs.FLAG_SETS[k]], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-800:]
    got = open(out, "rb").read()
    assert (cs.crc(got), len(got)) == expected(row, k, gold, tmp), name


@pytest.mark.parametrize("esbr", [False, True], ids=FLAG_IDS)
def test_decode_streams_and_decode_mixed_give_the_references_samples(esbr, gold, tmp):
    rows = [[r for r in cs.DECODED if r[0] == name][0] for name in SIX]
    assert sorted((r[3], r[5]) for r in rows) == sorted((kind, level) for kind in ("st", "mono", "ps") for level in (cs.gen.core.QUIET, cs.gen.core.LOUD))
    k = 1 if esbr else 0
    datas = [open(cs.path(r[0]), "rb").read() for r in rows]
    want = []
    for r in rows:
        expected(r, k, gold, tmp)
        want.append(int(gold[r[0] + "_wav"][3 * k + 2]))
    mixed, rates = decoder.decode_mixed(datas, esbr=esbr)
    for r, data, pcm, rate, crc in zip(rows, datas, mixed, rates, want):
        assert rate == 2 * cs.gen.RATES[r[2]] and pcm.shape[1] == 2
        assert cs.crc(np.ascontiguousarray(pcm).tobytes()) == crc, ("decode_mixed", r[0])
        alone, rate = decoder.decode_streams([data, data], esbr=esbr)
        assert rate == 2 * cs.gen.RATES[r[2]] and len(alone) == 2
        for pcm in alone:
            assert cs.crc(np.ascontiguousarray(pcm).tobytes()) == crc, ("decode_streams", r[0])


@pytest.mark.parametrize("k", [0, 1], ids=FLAG_IDS)
def test_the_stream_that_needs_the_down_sampled_bank_is_refused_and_nothing_is_written(k, tmp):
    name = cs.REFUSED[0][0]
    out = os.path.join(tmp, "refused_%d.wav" % k)
    p = subprocess.run([CLI, "-ifile:" + cs.path(name), "-ofile:" + out, *cs.FLAG_SETS[k]], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "down-sampled bank" in p.stderr, (p.returncode, p.stderr[-300:])
    assert not os.path.exists(out)
    data = open(cs.path(name), "rb").read()
    with pytest.raises(ValueError, match="down-sampled"):
        decoder.decode_streams([data], esbr=bool(k))
    with pytest.raises(ValueError, match="down-sampled"):
        decoder.decode_mixed([data, open(cs.path("mono_sr06"), "rb").read()], esbr=bool(k))
