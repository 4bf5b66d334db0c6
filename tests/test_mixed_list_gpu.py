"""A list that mixes kinds of stream, on the GPU: xaacdec_amd -ilist with all ten committed mono / stereo streams -- six kinds, six
groups side by side (or one after the other with -serialgroups:1) -- and libxaac_amd.decode_mixed on the same streams.  Every
stream alone is already pinned to the reference decoder by tests/test_cli_gpu.py, so whatever differs here belongs to the
grouping: every file must equal, header included, what `oracle/_ref/xaacdec` writes for that stream alone."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import mixed_list_cases as mx

pytestmark = pytest.mark.gpu


def decode_list(tmp_path, paths, *flags, out="out"):
    """-> (the finished process, {file name: bytes} of what it wrote)"""
    assert os.path.exists(mx.CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
    lst = mx.write_list(tmp_path, paths, out + ".txt")
    odir = tmp_path / out
    odir.mkdir()
    p = subprocess.run([mx.CLI, "-ilist:" + lst, "-odir:" + str(odir), *flags], capture_output=True, text=True, timeout=300)
    return p, {f: open(str(odir / f), "rb").read() for f in sorted(os.listdir(str(odir)))}


@pytest.mark.parametrize("flags", [(), ("-esbr:0",), ("-gputools:1",), ("-gpus:2", "-wrap_devices"), ("-serialgroups:1",)],
                         ids=["default", "esbr0", "gputools", "gpus2", "serial"])
def test_all_ten_streams_in_one_list(flags, tmp_path):
    p, got = decode_list(tmp_path, [mx.path(n) for n in mx.NAMES], *flags)
    assert p.returncode == 0, p.stderr[-500:]
    assert sorted(got) == sorted(n + ".wav" for n in mx.NAMES)
    for n in mx.NAMES:
        assert got[n + ".wav"] == mx.reference_wav(mx.path(n), *mx.esbr_flags(flags)), (n, flags)
    info = json.loads(p.stdout.strip().splitlines()[-1])
    want = mx.groups_of(mx.NAMES)
    assert info["streams"] == 10 and info["mismatched_copies"] == 0 and len(info["groups"]) == len(want) == 6
    for g, (kind, places) in zip(info["groups"], want):
        assert (g["rate"], g["channels"], g["sbr"], g["streams"]) == (mx.out_kind(kind)[0], kind[1], kind[2], len(places))
        assert g["esbr"] == (kind[2] if "-esbr:0" not in flags else 0)
        assert g["frames"] == sum(len(mx.adts_frames(mx.stream(mx.NAMES[i]))) for i in places)
    assert sum(g["frames"] for g in info["groups"]) == info["frames"]
    first = info["groups"][0]      # the run's own keys: the first listed stream's group
    assert (info["rate"], info["channels"], info["sbr"], info["esbr"]) == (first["rate"], first["channels"], first["sbr"], first["esbr"])


def test_the_order_of_the_list_does_not_matter(tmp_path):
    shuffled = list(mx.NAMES)
    random.Random(7).shuffle(shuffled)
    assert shuffled != mx.NAMES and shuffled != mx.NAMES[::-1]
    for k, names in enumerate((mx.NAMES[::-1], shuffled)):
        p, got = decode_list(tmp_path, [mx.path(n) for n in names], "-quiet", out="out%d" % k)
        assert p.returncode == 0, p.stderr[-500:]
        assert got == {n + ".wav": mx.reference_wav(mx.path(n)) for n in mx.NAMES}, names


def test_groups_whose_streams_end_at_different_frames(tmp_path):
    """two groups of several streams, each with a stream cut short: it drops out of its group's steps, the others go on"""
    a, b = mx.adts_frames(mx.stream("mix_aot5_48k")), mx.adts_frames(mx.stream("mono_aot5_32k"))
    (tmp_path / "stereo_cut.aac").write_bytes(b"".join(a[:12]))
    (tmp_path / "mono_cut.aac").write_bytes(b"".join(b[:20]))
    paths = [mx.path("mix_aot5_48k"), mx.path("mono_aot5_32k"), str(tmp_path / "stereo_cut.aac"), mx.path("mix_aot2_64k"),
             str(tmp_path / "mono_cut.aac")]
    p, got = decode_list(tmp_path, paths)
    assert p.returncode == 0, p.stderr[-500:]
    assert len(got) == 5
    for path in paths:
        name = os.path.basename(path)[:-4] + ".wav"
        assert got[name] == mx.reference_wav(path), name
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert [(g["streams"], g["frames"]) for g in info["groups"]] == [(2, len(a) + 12), (2, len(b) + 20), (1, len(mx.adts_frames(mx.stream("mix_aot2_64k"))))]


def test_a_damaged_stream_ends_alone_in_a_mixed_list(tmp_path):
    """mix_aot29_32k with the payload of frame 10 zeroed (the ADTS header stays, so the next frame would still be found: the host
    parser refuses the frame) beside three intact streams of other kinds.  What a list of one kind does with a stream that stops
    parsing (tests/test_cli_gpu.py: test_a_damaged_stream_of_a_list_ends_alone, -esbr:0): exit code 0, "the stream ends here" for
    that stream on stderr, its frames up to there written -- ten here --, the other streams as if it had not been in the list."""
    frames = mx.adts_frames(mx.stream("mix_aot29_32k"))
    head = 7 if frames[10][1] & 1 else 9       # (protection_absent: no CRC behind the header)
    frames[10] = frames[10][:head] + bytes(len(frames[10]) - head)
    bad = tmp_path / "damaged.aac"
    bad.write_bytes(b"".join(frames))
    intact = ["synth_lc_mono", "mix_aot5_48k", "mix_aot2_64k"]
    paths = [mx.path(intact[0]), mx.path(intact[1]), str(bad), mx.path(intact[2])]
    p, got = decode_list(tmp_path, paths, "-esbr:0")
    assert p.returncode == 0, p.stderr[-500:]
    assert "xaacdec_amd: stream 2: a frame does not parse" in p.stderr and p.stderr.count("the stream ends here") == 1
    for n in intact:
        assert got[n + ".wav"] == mx.reference_wav(mx.path(n), "-esbr:0"), n
    whole = mx.reference_wav(mx.path("mix_aot29_32k"), "-esbr:0")
    part = got["damaged.wav"]
    assert len(part) == 44 + 10 * 2048 * 2 * 2 and part[44:] == whole[44:len(part)]
    assert part[:4] == b"RIFF" and part[20:36] == whole[20:36]        # the same fmt chunk: PCM, stereo, 48 kHz


@pytest.fixture(scope="module")
def ten_streams():
    return [mx.stream(n) for n in mx.NAMES]


@pytest.mark.parametrize("kwargs", [{"esbr": True}, {"esbr": False}, {"esbr": True, "serial": True}], ids=["esbr", "esbr0", "serial"])
def test_decode_mixed(kwargs, ten_streams):
    import libxaac_amd
    pcm, rates = libxaac_amd.decode_mixed(ten_streams, **kwargs)
    assert len(pcm) == len(rates) == len(mx.NAMES)
    flags = () if kwargs["esbr"] else ("-esbr:0",)
    for n, x, rate in zip(mx.NAMES, pcm, rates):
        want = mx.reference_wav(mx.path(n), *flags)
        assert rate == int.from_bytes(want[24:28], "little"), n
        assert x.dtype == np.int16 and x.shape[1] == int.from_bytes(want[22:24], "little"), n
        assert np.ascontiguousarray(x).tobytes() == want[44:], n


def test_verify_on_a_mixed_list(tmp_path):
    """-verify compares the copies of one input; the streams of a list are no copies of each other, so every group of a list runs as
    -copies:1 does: nothing to compare, nothing mismatched"""
    p, got = decode_list(tmp_path, [mx.path(n) for n in mx.NAMES], "-verify")
    assert p.returncode == 0, p.stderr[-500:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert info["mismatched_copies"] == 0 and len(info["groups"]) == 6
    assert sum(g["frames"] for g in info["groups"]) == info["frames"] == sum(len(mx.adts_frames(mx.stream(n))) for n in mx.NAMES)
    assert got == {n + ".wav": mx.reference_wav(mx.path(n)) for n in mx.NAMES}
