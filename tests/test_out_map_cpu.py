"""The output stage (downmix to stereo, mono mix, mono twice, limiter off) without a GPU: the CPU twin against the numpy
restatement, the restatement against the reference decoder's own files, the table against the reference's ROM, what the sums can
reach, the command line decoder's -plan and refusals, the new descriptors' layouts."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import libxaac_amd
from libxaac_amd import decoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import aac_tools_cases as tc  # noqa: E402
import multichannel_cases as mc  # noqa: E402
import out_map_cases as oc  # noqa: E402

CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
WIDE = mc.WIDE


def _block(rng, n, n_ch):
    """full-range words; rows of -32768 and of other negative values, where a floor per term differs from a floor of the sum"""
    x = rng.integers(-32768, 32768, (n, n_ch)).astype(np.int16)
    x[0], x[1], x[2], x[3] = -32768, 32767, -1, -32767
    x[4:40] = -rng.integers(1, 32769, (36, n_ch))
    x[40:60, ::2] = -32768
    return x


@pytest.mark.parametrize("n_ch", [1, 2, 3, 4, 5, 6])
def test_host_twin_equals_the_restatement(n_ch):
    rng = np.random.default_rng(100 + n_ch)
    x = _block(rng, 4099, n_ch)
    kinds = {1: ["dup"], 2: ["mono", "mono_dup"]}.get(n_ch, ["downmix"])
    for kind in kinds:
        got = decoder.out_map_apply_host(libxaac_amd.out_map(kind, n_ch), x)
        assert np.array_equal(got, oc.restate(x, kind, n_ch)), kind
    assert np.array_equal(decoder.out_map_apply_host(libxaac_amd.out_map(libxaac_amd.OUT_MAP_NONE), x), x)
    # in place, as the command line decoder mixes the limiter's flushed delay line
    for kind in kinds:
        buf = np.zeros((len(x), max(2, n_ch)), np.int16).reshape(-1)
        buf[:x.size] = x.reshape(-1)
        m = libxaac_amd.out_map(kind, n_ch)
        out_ch = decoder.load_host_library().xaac_out_map_apply_host(ctypes.byref(m), n_ch, buf.ctypes.data, len(x), buf.ctypes.data)
        assert np.array_equal(buf[:len(x) * out_ch].reshape(len(x), out_ch), oc.restate(x, kind, n_ch)), kind


def test_host_twin_refuses_what_no_map_takes():
    lib = decoder.load_host_library()
    x = np.zeros((8, 6), np.int16)
    for kind, n_ch in (("downmix", 2), ("downmix", 1), ("mono", 1), ("mono", 3), ("mono_dup", 6), ("dup", 2)):
        m = libxaac_amd.out_map(kind, 6)
        assert lib.xaac_out_map_apply_host(ctypes.byref(m), n_ch, x.ctypes.data, 8, x.ctypes.data) == -1, (kind, n_ch)
    m = libxaac_amd.out_map("downmix", 5)       # an element list that does not cover six channels
    assert lib.xaac_out_map_apply_host(ctypes.byref(m), 6, x.ctypes.data, 8, x.ctypes.data) == -1
    m = libxaac_amd.out_map("downmix", 6)
    m.element_slot[3] = 4                       # two elements on one slot
    assert lib.xaac_out_map_apply_host(ctypes.byref(m), 6, x.ctypes.data, 8, x.ctypes.data) == -1


def test_what_the_downmix_sums_can_reach():
    """xaac_out_map_row_bound over the generated table.  No row sums to 2^30, so no sum passes +32767.  The floors round a negative
    term away from zero: the 5.0 rows stay inside WORD16 all the same, the 5.1 rows reach -32769 when the four channels of a side all
    sit at -32768 -- there the reference's WORD16 sum wraps to +32767, and so do the twin and the restatement (the sums are kept in
    32 bits and cut to 16 at the end, which is the same word)."""
    m = oc.matrix()
    for k in range(2):
        bound, row_sum = decoder.out_map_row_bound(k)
        assert row_sum == int(m[k].sum(axis=1).max()) and row_sum < 1 << 30
        assert bound == int(((m[k] + 32767) >> 15).sum(axis=1).max())
    assert decoder.out_map_row_bound(0)[0] <= 32767
    assert decoder.out_map_row_bound(1)[0] == 32769
    assert decoder.out_map_row_bound(2)[0] < 0
    worst = np.full((1, 6), -32768, np.int16)
    assert oc.restate(worst, "downmix", 6).tolist() == [[32767, 32767]]
    assert decoder.out_map_apply_host(libxaac_amd.out_map("downmix", 6), worst).tolist() == [[32767, 32767]]
    assert decoder.out_map_apply_host(libxaac_amd.out_map("downmix", 5), worst[:, :5]).tolist() == [[-31596, -31596]]
    # every coefficient the element walk of a configuration never reads is zero: the walk is the matrix product
    for cc in (3, 4, 5, 6):
        x = _block(np.random.default_rng(cc), 512, cc).astype(np.int64)
        mk = m[1 if cc == 6 else 0]
        full = np.stack([sum(((mk[side][s] * x[:, s]) >> 16) >> 14 for s in range(cc)) for side in range(2)], 1).astype(np.int16)
        assert np.array_equal(full, oc.restate(x.astype(np.int16), "downmix", cc))


def test_table_matches_the_reference_rom():
    """libxaac_amd/csrc/tables_out_map.inc regenerated from the compiled reference's ROM equals the committed file"""
    tc.need("libref_harness.so")
    import gen_tables_out_map as g
    assert g.render(g.reference_matrix()) == open(oc.INC).read()


@pytest.mark.parametrize("lim_off", [False, True], ids=["limiter", "limiter_off"])
@pytest.mark.parametrize("name", oc.MC_STREAMS)
def test_restatement_equals_the_reference_downmix(name, lim_off):
    """the reference's -downmix:1 file is the restatement of its own unflagged file, 6 stereo samples early, up to the unmixed
    flush data; the compared share of the file is 0.99 at least"""
    span, n = oc.check_reference_downmix(name, lim_off)
    assert span >= 0.99 * n, (span, n)


@pytest.mark.parametrize("tostereo", [False, True], ids=["dmix", "dmix_tostereo"])
def test_restatement_equals_the_reference_mono_mix(tostereo):
    span, n = oc.check_reference_dmix(tostereo)
    assert (span, n) == (76560, 76800)


def _plan(*args):
    p = subprocess.run([CLI, "-plan"] + list(args), capture_output=True, text=True, timeout=60)
    return p.returncode, (json.loads(p.stdout) if p.returncode == 0 else None), p.stderr


MC6, MC6_HE = os.path.join(WIDE, "mc6_aot2.aac"), os.path.join(WIDE, "mc6_aot5.aac")
STEREO, MONO, HE = (os.path.join(oc.STREAMS, n + ".aac") for n in ("mix_aot2_64k", "lc_aot2_16k_mono", "mix_aot5_48k"))


@pytest.mark.parametrize("path,flags,want", [
    (MC6, (), (6, "none", 1, "extensible68")),
    (MC6, ("-downmix:1",), (2, "downmix", 1, "pcm44")),
    (MC6, ("-downmix:1", "-peak_limiter_off:1"), (2, "downmix", 0, "pcm44")),
    (MC6, ("-tostereo:1",), (6, "none", 1, "extensible68")),
    (MC6_HE, ("-mcsbr:1", "-downmix:1"), (2, "downmix", 0, "pcm44")),
    (MC6_HE, ("-mcsbr:1", "-peak_limiter_off:1"), (6, "none", 0, "extensible68")),
    (STEREO, ("-dmix:1",), (1, "mono", 1, "pcm44")),
    (STEREO, ("-dmix:1", "-tostereo:1"), (2, "mono_dup", 1, "pcm44")),
    (STEREO, ("-tostereo:1",), (2, "none", 1, "pcm44")),
    (STEREO, ("-peak_limiter_off:1",), (2, "none", 0, "pcm44")),
    (STEREO, ("-downmix:0", "-dmix:0", "-tostereo:0", "-peak_limiter_off:0"), (2, "none", 1, "pcm44")),
    (MONO, ("-tostereo:1",), (2, "dup", 1, "pcm44")),
    (MONO, ("-dmix:1",), (1, "none", 1, "pcm44")),
    (MONO, ("-tostereo:1", "-peak_limiter_off:1"), (2, "dup", 0, "pcm44")),
    (HE, ("-tostereo:1", "-peak_limiter_off:1"), (2, "none", 0, "pcm44")),
])
def test_plan_names_the_output_layout(path, flags, want):
    """-plan prints the output channel count, the map, whether a limiter runs and the header kind -- before any HIP call (this
    box has no GPU)"""
    rc, d, err = _plan("-ifile:" + path, *flags)
    assert rc == 0, err
    assert (d["out_channels"], d["out_map"], d["limiter"], d["wav_header"]) == want
    assert d["channels"] == {MC6: 6, MC6_HE: 6, STEREO: 2, MONO: 1, HE: 2}[path]


@pytest.mark.parametrize("path,flags,message", [
    (STEREO, ("-downmix:1",), "-downmix:1 on a stream of one or two channels"),
    (MONO, ("-downmix:1",), "-downmix:1 on a stream of one or two channels"),
    (HE, ("-downmix:1",), "-downmix:1 on a stream of one or two channels"),
    (HE, ("-dmix:1",), "-dmix:1 on a stream with SBR or with more than two channels"),
    (MC6, ("-dmix:1",), "-dmix:1 on a stream with SBR or with more than two channels"),
    (MC6_HE, ("-mcsbr:1", "-dmix:1"), "-dmix:1 on a stream with SBR or with more than two channels"),
    (MC6, ("-downmix:1", "-dmix:1"), "-downmix:1 together with -dmix:1"),
    (MONO, ("-dmix:1", "-tostereo:1"), "-dmix:1 together with -tostereo:1 on a mono stream"),
    (MC6, ("-downmix:2",), "-downmix:0 or -downmix:1"),
    (STEREO, ("-peak_limiter_off:on",), "-peak_limiter_off:0 or -peak_limiter_off:1"),
])
@pytest.mark.parametrize("plan", [True, False], ids=["plan", "decode"])
def test_refusals_have_their_own_message_and_leave_no_file(tmp_path, path, flags, message, plan):
    """what the decoder does not take is refused before a device is looked at: a message of its own, a non-zero exit, no file"""
    out = str(tmp_path / "o.wav")
    p = subprocess.run([CLI, "-ifile:" + path, "-ofile:" + out, *flags] + (["-plan"] if plan else []), capture_output=True, text=True,
                       timeout=60)
    assert p.returncode != 0 and message in p.stderr and p.stderr.startswith("xaacdec_amd: ")
    assert not os.path.exists(out) and p.stdout == ""


def test_usage_lists_the_flags():
    p = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    for flag in ("-downmix:0|1", "-dmix:0|1", "-tostereo:0|1", "-peak_limiter_off:0|1"):
        assert flag in p.stderr


def test_decode_streams_rules():
    """decode_streams' out_map follows the command line decoder: a map, a no-op (None), or a ValueError"""
    pick = decoder._pick_out_map
    assert pick(None, 6, False, 6) is None
    m = pick("downmix", 6, False, 6)
    assert (m.kind, m.matrix, m.n_elements, list(m.element_type), list(m.element_slot)) == (1, 1, 4, [0, 1, 1, 3], [2, 0, 4, 3])
    m = pick("downmix", 4, True, 4)
    assert (m.kind, m.matrix, m.n_elements, list(m.element_type)[:3], list(m.element_slot)[:3]) == (1, 0, 3, [0, 1, 0], [2, 0, 3])
    assert pick("mono", 2, False, 0).kind == libxaac_amd.OUT_MAP_MONO_MIX
    assert pick("mono_dup", 2, False, 0).kind == libxaac_amd.OUT_MAP_MONO_MIX_DUP
    assert pick("dup", 1, False, 0).kind == libxaac_amd.OUT_MAP_DUP_STEREO
    assert pick("mono", 1, False, 0) is None and pick("dup", 2, False, 0) is None and pick("dup", 1, True, 0) is None
    assert pick("dup", 6, False, 6) is None and pick("dup", 2, True, 0) is None
    for bad in (("downmix", 2, False, 0), ("downmix", 1, True, 0), ("mono", 2, True, 0), ("mono", 6, False, 6), ("mono_dup", 6, True, 6),
                ("mono_dup", 1, False, 0), ("stereo", 2, False, 0)):
        with pytest.raises(ValueError):
            pick(*bad)
    # the element lists are those of the layout table the multichannel tests use
    for cc in (3, 4, 5, 6):
        elements, route, _ = mc.LAYOUT[cc]
        m, ch = pick("downmix", cc, False, cc), 0
        for k, e in enumerate(elements):
            assert (m.element_type[k], m.element_slot[k]) == (e, route[ch])
            ch += 2 if e == 1 else 1


def test_descriptor_layouts_match_the_headers(tmp_path):
    """the ctypes mirrors of the new descriptors against what a C compiler makes of include/xaac_amd.h and include/xaac_esbr.h"""
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xaac_esbr.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(xaac_out_map), '
                   'offsetof(xaac_out_map, n_elements), offsetof(xaac_out_map, element_type), offsetof(xaac_out_map, element_slot), '
                   'sizeof(xaac_limiter_map_batch), offsetof(xaac_limiter_map_batch, map), sizeof(xaac_scale_adjust_map_batch), '
                   'offsetof(xaac_scale_adjust_map_batch, samples), offsetof(xaac_scale_adjust_map_batch, stride), '
                   'offsetof(xaac_scale_adjust_map_batch, pcm16), offsetof(xaac_scale_adjust_map_batch, map), '
                   'sizeof(xaac_mc_pcm_out_map_batch), offsetof(xaac_mc_pcm_out_map_batch, map), XAAC_OUT_MAP_NONE, '
                   'XAAC_OUT_MAP_DOWNMIX_STEREO, XAAC_OUT_MAP_MONO_MIX, XAAC_OUT_MAP_MONO_MIX_DUP, XAAC_OUT_MAP_DUP_STEREO); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    M, L, S, P = libxaac_amd.OutMap, libxaac_amd.abi.LimiterMapBatch, libxaac_amd.abi.ScaleAdjustMapBatch, libxaac_amd.abi.McPcmOutMapBatch
    assert got == [ctypes.sizeof(M), M.n_elements.offset, M.element_type.offset, M.element_slot.offset, ctypes.sizeof(L), L.map.offset,
                   ctypes.sizeof(S), S.samples.offset, S.stride.offset, S.pcm16.offset, S.map.offset, ctypes.sizeof(P), P.map.offset,
                   libxaac_amd.OUT_MAP_NONE, libxaac_amd.OUT_MAP_DOWNMIX_STEREO, libxaac_amd.OUT_MAP_MONO_MIX,
                   libxaac_amd.OUT_MAP_MONO_MIX_DUP, libxaac_amd.OUT_MAP_DUP_STEREO]


def test_mapped_entry_points_check_their_arguments():
    """the new batch entry points refuse a missing context or descriptor (no GPU needed for that)"""
    lib = libxaac_amd.load_library()
    for name in ("xaac_peak_limiter_process_map_batch", "xaac_pcm16_scale_adjust_map_batch", "xaac_mc_pcm16_from_float_map_batch",
                 "xaac_mc_pcm16_from_planes_map_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p]
        assert fn(None, None) & 0x80000000, name
