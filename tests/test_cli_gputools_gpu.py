"""`xaacdec_amd -gputools:1` and `decode_streams(..., gpu_tools=True)`: the M/S, intensity, PNS and TNS tools on the GPU
(stage-1 parse, side rows up beside the spectra, xaac_aac_tools_process_batch in front of the IMDCT) must give the WAV bytes the
decoder writes without the flag and the reference decoder (oracle/_ref/xaacdec) writes: AAC-LC, HE-AAC and HE-AACv2 streams,
with -esbr:0 and with default flags, one stream, a batch of copies (-copies:N -verify) and an -ilist batch of streams of
different lengths.  (The -ilist handling of a stream the tools kernel refuses is code the parser's own output cannot reach --
its side info always passes the kernel's checks -- so it is not exercised here; the kernel's refusals are in
tests/test_aac_tools_gpu.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")
REF = os.path.join(ROOT, "oracle", "_ref", "xaacdec")
NAMES = ["mix_aot2_64k", "mix_aot5_48k", "mono_aot5_32k", "harm_aot5_48k", "mix_aot29_32k", "synth_lc_a", "synth_lc_b",
         "synth_lc_mono", "lc_aot2_16k_mono", "he_aot5_44k"]

pytestmark = pytest.mark.gpu


def cli(tmp_path, tag, *args):
    assert os.path.exists(CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
    p = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (tag, p.stderr[-500:])
    return p


def wav_bytes(name, tmp_path, tag, *flags):
    out = str(tmp_path / ("%s_%s.wav" % (name, tag)))
    p = cli(tmp_path, tag, "-ifile:" + os.path.join(STREAMS, name + ".aac"), "-ofile:" + out, *flags)
    return open(out, "rb").read(), json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("flags", [(), ("-esbr:0",)], ids=["default", "esbr0"])
@pytest.mark.parametrize("name", NAMES)
def test_wav_equals_the_decoder_without_the_flag_and_the_reference(name, flags, tmp_path):
    if not os.path.exists(REF):
        pytest.fail("oracle/_ref/xaacdec missing: the reference binary did not travel with the snapshot")
    with_tools, _ = wav_bytes(name, tmp_path, "tools", "-gputools:1", *flags)
    plain, _ = wav_bytes(name, tmp_path, "plain", *flags)
    want = str(tmp_path / "ref.wav")
    subprocess.run([REF, "-ifile:" + os.path.join(STREAMS, name + ".aac"), "-ofile:" + want, *flags], check=True, capture_output=True)
    assert len(with_tools) > 10000 and with_tools == plain
    # (the two programs write their own RIFF headers: the reference's differs in its chunk layout, the samples are the payload)
    import wave
    with wave.open(want) as w:
        ref_pcm = w.readframes(w.getnframes())
    with wave.open(str(tmp_path / ("%s_tools.wav" % name))) as w:
        assert w.readframes(w.getnframes()) == ref_pcm


@pytest.mark.parametrize("flags", [(), ("-esbr:0",)], ids=["default", "esbr0"])
@pytest.mark.parametrize("name", ["mix_aot2_64k", "synth_lc_a", "mix_aot5_48k", "mix_aot29_32k"])
def test_a_batch_of_copies(name, flags, tmp_path):
    one, _ = wav_bytes(name, tmp_path, "one", *flags)
    many, info = wav_bytes(name, tmp_path, "many", "-gputools:1", "-copies:48", "-verify", *flags)
    assert many == one and info["streams"] == 48 and info["mismatched_copies"] == 0


@pytest.mark.parametrize("flags", [(), ("-esbr:0",)], ids=["default", "esbr0"])
@pytest.mark.parametrize("names", [("synth_lc_a", "mix_aot2_64k", "synth_lc_b"), ("mix_aot5_48k", "harm_aot5_48k"),
                                   ("mix_aot29_32k",)], ids=["lc", "he", "hev2"])
def test_a_list_of_different_streams_in_one_batch(names, flags, tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(os.path.join(STREAMS, n + ".aac") for n in names) + "\n")
    outs = {}
    for tag, extra in (("tools", ("-gputools:1",)), ("plain", ())):
        out = tmp_path / tag
        out.mkdir()
        cli(tmp_path, tag, "-ilist:" + str(lst), "-odir:" + str(out), *extra, *flags)
        outs[tag] = {n: open(str(out / (n + ".wav")), "rb").read() for n in set(names)}
    for n in set(names):
        assert len(outs["tools"][n]) > 10000 and outs["tools"][n] == outs["plain"][n], n
        single, _ = wav_bytes(n, tmp_path, "single", *flags)
        assert outs["tools"][n] == single, n


@pytest.mark.parametrize("esbr", [False, True])
@pytest.mark.parametrize("name", ["synth_lc_a", "mix_aot2_64k", "mix_aot5_48k", "mix_aot29_32k", "synth_lc_mono"])
def test_decode_streams_with_gpu_tools(name, esbr):
    from libxaac_amd import decoder
    data = open(os.path.join(STREAMS, name + ".aac"), "rb").read()
    other = open(os.path.join(STREAMS, {"synth_lc_a": "synth_lc_b"}.get(name, name) + ".aac"), "rb").read()
    want, rate = decoder.decode_streams([data, other, data], esbr=esbr)
    got, rate2 = decoder.decode_streams([data, other, data], esbr=esbr, gpu_tools=True)
    assert rate == rate2 and len(got) == 3
    for a, b in zip(got, want):
        assert len(a) > 1000 and np.array_equal(a, b)
