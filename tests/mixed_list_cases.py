"""Shared by tests/test_mixed_list_cpu.py and tests/test_mixed_list_gpu.py: the committed mono / stereo ADTS streams sorted by
kind -- (core sampling rate, channels, SBR payload in the first frame), what a lock-step batch needs to be one for all its
streams --, the reference decoder's WAV files for them (oracle/_ref/xaacdec, one decode per file and flag set for the whole test
run) and the ADTS frame splitter (test infrastructure)."""
import atexit
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aac_tools_cases as tc  # noqa: E402  (need)

REF = os.path.join(ROOT, "oracle", "_ref")
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
WIDE = os.path.join(ROOT, "tests", "golden", "streams_wide")
CLI = os.path.join(ROOT, "libxaac_amd", "xaacdec_amd")

# (core rate, channels, SBR) -> the committed streams of that kind
KINDS = {
    (48000, 2, 0): ["mix_aot2_64k", "synth_lc_a", "synth_lc_b"],
    (48000, 1, 0): ["synth_lc_mono"],
    (16000, 1, 0): ["lc_aot2_16k_mono"],
    (24000, 2, 1): ["mix_aot5_48k", "harm_aot5_48k"],
    (22050, 2, 1): ["he_aot5_44k"],
    (24000, 1, 1): ["mono_aot5_32k", "mix_aot29_32k"],
}
# the ten streams as one list: no two neighbours of one kind, so that every group has to be gathered from all over the list
NAMES = ["mix_aot2_64k", "mix_aot5_48k", "mono_aot5_32k", "harm_aot5_48k", "mix_aot29_32k", "synth_lc_a", "synth_lc_b",
         "synth_lc_mono", "lc_aot2_16k_mono", "he_aot5_44k"]
KIND_OF = {n: k for k, names in KINDS.items() for n in names}
assert sorted(KIND_OF) == sorted(NAMES)


def groups_of(names):
    """[(kind, [places in `names`])] in the order in which `names` first holds each kind: what the decoder has to make of the list"""
    out = {}
    for i, n in enumerate(names):
        out.setdefault(KIND_OF[n], []).append(i)
    return list(out.items())


def out_kind(kind):
    """what the reference writes for a stream of that kind with default flags or -esbr:0: (output rate, output channels)"""
    rate, n_ch, sbr = kind
    return (2 * rate, 2) if sbr else (rate, n_ch)


def path(name):
    return os.path.join(STREAMS, name + ".aac")


def stream(name):
    return open(path(name), "rb").read()


def write_list(tmp_path, paths, name="list.txt"):
    lst = tmp_path / name
    lst.write_text("".join(str(p) + "\n" for p in paths))
    return str(lst)


def adts_frames(data):
    pos, out = 0, []
    while pos + 7 <= len(data):
        n = ((data[pos + 3] & 3) << 11) | (data[pos + 4] << 3) | (data[pos + 5] >> 5)
        out.append(data[pos:pos + n])
        pos += n
    return out


_dir = None
_cache = {}


def reference_wav(path, *flags):
    """the bytes oracle/_ref/xaacdec writes for the ADTS file at `path` with `flags`: one decode per (file, flags) and test run"""
    global _dir
    key = (str(path),) + tuple(flags)
    if key not in _cache:
        tc.need("xaacdec")
        if _dir is None:
            _dir = tempfile.mkdtemp(prefix="xaac_mixed_")
            atexit.register(shutil.rmtree, _dir, True)
        out = os.path.join(_dir, "ref_%d.wav" % len(_cache))
        subprocess.run([os.path.join(REF, "xaacdec"), "-ifile:" + str(path), "-ofile:" + out, *flags], check=True, capture_output=True,
                       timeout=600)
        _cache[key] = open(out, "rb").read()
    return _cache[key]


def esbr_flags(flags):
    """the flags of a run that the reference decoder knows too (its -esbr switch; the rest is this decoder's own)"""
    return tuple(f for f in flags if f.startswith("-esbr:"))
