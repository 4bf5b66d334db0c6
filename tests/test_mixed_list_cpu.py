"""A list that mixes kinds of stream -- xaacdec_amd -ilist and libxaac_amd.decode_mixed --, as far as it can be checked without a
GPU: the sorting of the list into groups of one kind (-plan prints it and exits before the first HIP call), the refusals that
come before a device is looked at, and the Python function that maps streams to groups and results back to list order."""
import json
import os
import random
import subprocess

import pytest

import mixed_list_cases as mx
from libxaac_amd import decoder, dist


def cli(*args):
    assert os.path.exists(mx.CLI), "libxaac_amd/xaacdec_amd is not built (make -C libxaac_amd/host)"
    return subprocess.run([mx.CLI] + list(args), capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("gpus", [1, 2])
def test_plan_of_a_mixed_list(gpus, tmp_path):
    """all ten committed streams in one list: six groups in the order of their first files, each with its own rate, channels, header
    and split over the devices (shard_range over the group's own streams)"""
    lst = mx.write_list(tmp_path, [mx.path(n) for n in mx.NAMES])
    p = cli("-plan", "-ilist:" + lst, "-odir:" + str(tmp_path), "-gpus:%d" % gpus)
    assert p.returncode == 0, p.stderr[-500:]
    d = json.loads(p.stdout)
    want = mx.groups_of(mx.NAMES)
    assert d["streams"] == len(mx.NAMES) and len(want) == 6 and len(d["groups"]) == 6
    assert d["gpus"] == gpus
    for g, (kind, places) in zip(d["groups"], want):
        rate, n_ch, sbr = kind
        out_rate, out_ch = mx.out_kind(kind)
        assert (g["rate"], g["core_rate"], g["channels"], g["sbr"]) == (out_rate, rate, n_ch, sbr), kind
        assert (g["out_channels"], g["wav_header"], g["out_map"]) == (out_ch, "pcm44", "none"), kind
        assert g["esbr"] == sbr and g["limiter"] == 1 - sbr, kind     # the default -esbr:1 where there is SBR; the limiter where not
        assert g["streams"] == len(places) and g["list_index"] == places, kind
        assert g["threads"] >= 1
        used = min(gpus, len(places))         # a device that gets no stream of a group starts nothing for it
        assert len(g["shards"]) == used
        for r, s in enumerate(g["shards"]):
            lo, hi = dist.shard_range(len(places), r, used)
            assert (s["device"], s["lo"], s["n"]) == (r, lo, hi - lo), kind
        assert sum(s["n"] for s in g["shards"]) == g["streams"]
    # the run's own keys: the first listed stream's group; the flat list of shards names every group's
    first = d["groups"][0]
    assert all(d[k] == first[k] for k in ("channels", "sbr", "esbr", "out_channels", "out_map", "limiter", "wav_header"))
    assert [(s["group"], s["device"], s["lo"], s["n"]) for s in d["shards"]] == \
        [(k, s["device"], s["lo"], s["n"]) for k, g in enumerate(d["groups"]) for s in g["shards"]]


def test_threads_are_shared_out_over_the_groups(tmp_path):
    lst = mx.write_list(tmp_path, [mx.path(n) for n in mx.NAMES])
    p = cli("-plan", "-ilist:" + lst, "-odir:" + str(tmp_path), "-threads:20")
    assert p.returncode == 0, p.stderr[-500:]
    groups = json.loads(p.stdout)["groups"]
    assert [g["threads"] for g in groups] == [max(1, 20 * g["streams"] // 10) for g in groups] == [6, 4, 4, 2, 2, 2]
    p = cli("-plan", "-ilist:" + lst, "-odir:" + str(tmp_path), "-threads:3")
    assert [g["threads"] for g in json.loads(p.stdout)["groups"]] == [1] * 6      # at least one each


def test_plan_of_a_list_of_one_kind_is_what_it_was(tmp_path):
    """one kind, one group: no "groups" key, and stdout byte for byte what the decoder printed before it took mixed lists"""
    lst = mx.write_list(tmp_path, [mx.path(n) for n in ("mix_aot2_64k", "synth_lc_a", "synth_lc_b")])
    p = cli("-plan", "-ilist:" + lst, "-odir:" + str(tmp_path))
    assert p.returncode == 0, p.stderr[-500:]
    assert p.stdout == ('{"streams": 3, "gpus": 1, "channels": 2, "sbr": 0, "esbr": 0, "out_channels": 2, "out_map": "none", '
                        '"limiter": 1, "wav_header": "pcm44", "shards": [{"device": 0, "lo": 0, "n": 3}]}\n')
    p = cli("-plan", "-ilist:" + lst, "-odir:" + str(tmp_path), "-gpus:2", "-serialgroups:1", "-dmix:1")
    assert p.stdout == ('{"streams": 3, "gpus": 2, "channels": 2, "sbr": 0, "esbr": 0, "out_channels": 1, "out_map": "mono", '
                        '"limiter": 1, "wav_header": "pcm44", "shards": [{"device": 0, "lo": 0, "n": 2}, {"device": 1, "lo": 2, "n": 1}]}\n')


@pytest.mark.parametrize("plan", [("-plan",), ()], ids=["plan", "run"])
def test_refusals_come_before_any_device_or_file(plan, tmp_path):
    lst = mx.write_list(tmp_path, [mx.path(n) for n in mx.NAMES])
    out = tmp_path / "out"
    out.mkdir()
    # -dmix:1 is fine for the AAC-LC groups and refused for the SBR ones: the whole run is refused, with the first SBR file's name
    p = cli(*plan, "-ilist:" + lst, "-odir:" + str(out), "-dmix:1")
    first_sbr = next(n for n in mx.NAMES if mx.KIND_OF[n][2])
    assert p.returncode != 0 and p.stdout == ""
    assert p.stderr == "xaacdec_amd: %s: -dmix:1 on a stream with SBR or with more than two channels is not supported\n" % mx.path(first_sbr)
    # -downmix:1 has nothing to mix down in any of them: the first file's name
    p = cli(*plan, "-ilist:" + lst, "-odir:" + str(out), "-downmix:1")
    assert p.returncode != 0 and p.stdout == ""
    assert mx.path(mx.NAMES[0]) + ": -downmix:1 on a stream of one or two channels is not supported" in p.stderr
    # a stream of more than two channels beside another kind: refused up front, as it was
    mc = mx.write_list(tmp_path, [os.path.join(mx.WIDE, "mc6_aot2.aac"), mx.path("mix_aot2_64k")], "mc.txt")
    p = cli(*plan, "-ilist:" + mc, "-odir:" + str(out))
    assert p.returncode != 0 and p.stdout == "" and "different kinds" in p.stderr
    # -serialgroups takes 0 or 1
    p = cli(*plan, "-ilist:" + lst, "-odir:" + str(out), "-serialgroups:2")
    assert p.returncode == 1 and p.stdout == "" and "usage" in p.stderr and "-serialgroups" in p.stderr
    assert os.listdir(str(out)) == []


def test_the_usage_text_no_longer_asks_for_one_kind():
    p = cli()
    assert p.returncode == 1 and "-serialgroups" in p.stderr and "of the same kind" not in p.stderr
    assert "more than two channels only beside streams of its own kind" in " ".join(p.stderr.split())


def test_decode_mixed_sorts_the_list_into_groups_and_back():
    """libxaac_amd.decoder.plan_mixed / restore_list_order, the two halves of decode_mixed around its pipelines"""
    names = list(mx.NAMES)
    random.Random(20240607).shuffle(names)
    streams = [mx.stream(n) for n in names]
    groups = decoder.plan_mixed(streams)
    want = mx.groups_of(names)
    assert [(g.kind[:3], g.index) for g in groups] == [((r, c, bool(s)), places) for (r, c, s), places in want]
    assert all(g.kind[3] == 0 and g.threads >= 1 for g in groups)
    # every group hands back one result per stream, in its own order: the list's order comes back
    results = [[names[i] for i in g.index] for g in groups]
    assert decoder.restore_list_order(groups, results, len(names)) == names
    with pytest.raises(ValueError):
        decoder.restore_list_order(groups, results[:-1] + [results[-1][:-1]], len(names))
    assert [g.threads for g in decoder.plan_mixed([mx.stream(n) for n in mx.NAMES], threads=20)] == [6, 4, 4, 2, 2, 2]
    one = decoder.plan_mixed([mx.stream("synth_lc_a"), mx.stream("mix_aot2_64k")], threads=0)
    assert len(one) == 1 and one[0].index == [0, 1] and one[0].threads == 0      # one kind: decode_streams' own default


def test_decode_mixed_refuses_before_any_gpu_work():
    """(no GPU in this test: the refusals are plan_mixed's, which decode_mixed calls first; and decode_mixed itself raises them
    before it imports torch)"""
    import libxaac_amd
    lc, sbr = mx.stream("synth_lc_a"), mx.stream("mono_aot5_32k")
    streams = [lc, mx.stream("synth_lc_mono"), lc, sbr, mx.stream("mix_aot5_48k")]
    with pytest.raises(ValueError, match=r'^stream 3: out_map="mono" on a stream with SBR'):
        decoder.plan_mixed(streams, out_map="mono")
    with pytest.raises(ValueError, match=r'^stream 0: out_map="downmix" on a stream of one or two channels'):
        decoder.plan_mixed(streams, out_map="downmix")
    with pytest.raises(ValueError, match=r"^stream 1: out_map=\"mono_dup\" on a mono stream"):
        decoder.plan_mixed(streams, out_map="mono_dup")
    assert len(decoder.plan_mixed(streams, out_map="dup")) == 4          # a no-op where it means nothing
    with pytest.raises(ValueError, match="out_map is None"):
        decoder.plan_mixed(streams, out_map="stereo")
    mc = open(os.path.join(mx.WIDE, "mc6_aot2.aac"), "rb").read()
    for both in ([lc, mc], [mc, sbr]):
        with pytest.raises(ValueError, match="channel configurations"):
            decoder.plan_mixed(both)
    assert [g.index for g in decoder.plan_mixed([mc, mc])] == [[0, 1]] and decoder.plan_mixed([mc])[0].kind == (48000, 6, False, 6)
    with pytest.raises(ValueError, match=r"^stream 3: "):
        libxaac_amd.decode_mixed(streams, out_map="mono", device="cuda:0")
