"""Shared by tests/test_out_map_cpu.py and tests/test_out_map_gpu.py: the numpy restatement of the reference's output stage
(ixheaacd_dec_downmix_to_stereo, the mono mix, the mono channel twice), the way the reference's own -downmix:1 / -dmix:1 files
relate to its unflagged ones, and the streams the tests decode (test infrastructure)."""
import os
import re
import struct

import numpy as np

import aac_tools_cases as tc
import mc_sbr_cases as mcs
import multichannel_cases as mc

ROOT = mc.ROOT
STREAMS = tc.STREAMS
INC = os.path.join(ROOT, "libxaac_amd", "csrc", "tables_out_map.inc")
LAG = 6                 # stereo samples the reference's -downmix:1 file starts early (its header / skip arithmetic keeps the stream's count)
MAPS = ("downmix", "mono", "mono_dup", "dup")
MC_STREAMS = ["mc3_48k", "mc4_32k", "mc5_48k", "mc6_aot2", "mc6_aot5"]     # the last one with SBR


def matrix():
    """[k][side][slot] of the committed table (tests/test_out_map_cpu.py holds it against the reference's ROM)"""
    body = re.search(r"xo_down_mix_matrix\[2\]\[2\]\[8\] = \{(.*)\};", open(INC).read(), re.S).group(1)
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], np.int64).reshape(2, 2, 8)


def restate(pcm, kind, channel_config=0):
    """what the reference's output stage makes of an interleaved PCM16 block int16[samples, channels]"""
    x = np.asarray(pcm, np.int16).astype(np.int64)
    if kind == "downmix":           # decoder/ixheaacd_multichannel.c:364-422, in element order
        elements, route, _ = mc.LAYOUT[channel_config]
        m = matrix()[1 if channel_config == 6 else 0]
        left, right, ch = np.zeros(len(x), np.int64), np.zeros(len(x), np.int64), 0
        for e in elements:
            s = route[ch]
            left += ((m[0][s] * x[:, s]) >> 16) >> 14                                 # mult32x16in32, then >> 14: a floor per term
            r = s + 1 if e == 1 else s                                               # a pair's right sum takes its second channel
            right += ((m[1][r] * x[:, r]) >> 16) >> 14
            ch += 2 if e == 1 else 1
        return np.stack([left, right], 1).astype(np.int16)                           # WORD16 sums: they wrap
    if kind in ("mono", "mono_dup"):                                                 # api.c:3749
        v = ((x[:, 0] >> 1) + (x[:, 1] >> 1)).astype(np.int16)
        return np.stack([v, v], 1) if kind == "mono_dup" else v[:, None]
    if kind == "dup":
        return np.repeat(np.asarray(pcm, np.int16), 2, axis=1)
    raise ValueError(kind)


def wav_parts(data):
    """-> (header bytes, channels, rate, payload int16[samples, channels])"""
    assert data[:4] == b"RIFF" and data[8:16] == b"WAVEfmt "
    fmt = struct.unpack("<I", data[16:20])[0]
    ch, rate = struct.unpack("<HI", data[22:28])
    at = 20 + fmt
    assert data[at:at + 4] == b"data"
    pay = np.frombuffer(data[at + 8:], np.int16)
    return at + 8, ch, rate, pay[:len(pay) // ch * ch].reshape(-1, ch)


def stream_path(name):
    if name.startswith("mc6_aot5"):
        return mcs.stream_path(name)
    if name.startswith("mc"):
        return mc.stream_path(name)
    return os.path.join(STREAMS, name + ".aac")


def attack(rate):
    return int(5.0 * rate / 1000)      # attack_time_samples of the limiter (peak_limiter.c:46-77)


def check_reference_downmix(name, lim_off, mixed=None):
    """The reference's own -downmix:1 file of stream `name` against the restatement of an unflagged decode (`mixed`: the stereo
    payload to hold it against; default the restatement of the reference's own unflagged file): ref[i] == mixed[i + LAG] on the
    span that is mixed data -- n - LAG samples, less the limiter's flushed delay line where there is a limiter.  -> (span, n)"""
    path = stream_path(name)
    flags = ("-downmix:1",) + (("-peak_limiter_off:1",) if lim_off else ())
    hdr, ch, rate, plain = wav_parts(mcs.reference_wav(path) if not lim_off else mcs.reference_wav(path, "-peak_limiter_off:1"))
    assert hdr == 68 and ch == mc.channel_config(open(path, "rb").read())
    rhdr, rch, _, _ = wav_parts(mcs.reference_wav(path, *flags))
    assert (rhdr, rch) == (68, ch)                       # the reference's header still claims the stream's channels
    ref = np.frombuffer(mcs.reference_wav(path, *flags)[68:], np.int16)
    ref = ref[:len(ref) // 2 * 2].reshape(-1, 2)
    if mixed is None:
        mixed = restate(plain, "downmix", ch)
    n = len(plain)
    sbr = name == "mc6_aot5"
    span = n - LAG - (0 if lim_off or sbr else attack(rate))
    assert len(ref) >= span and len(mixed) >= span + LAG
    assert np.array_equal(ref[:span], mixed[LAG:LAG + span]), (name, lim_off)
    return span, n


def check_reference_dmix(tostereo, mixed=None):
    """the same for -dmix:1 [-tostereo:1] on the stereo AAC-LC stream: the first n - attack samples; no lag.  -> (span, n)"""
    path = stream_path("mix_aot2_64k")
    flags = ("-dmix:1",) + (("-tostereo:1",) if tostereo else ())
    _, ch, rate, plain = wav_parts(mcs.reference_wav(path))
    rhdr, rch, _, ref = wav_parts(mcs.reference_wav(path, *flags))
    assert ch == 2 and (rhdr, rch) == (44, 2 if tostereo else 1)
    if mixed is None:
        mixed = restate(plain, "mono_dup" if tostereo else "mono")
    n = len(plain)
    span = n - attack(rate)
    assert len(ref) >= span and len(mixed) >= span
    assert np.array_equal(ref[:span], mixed[:span]), tostereo
    return span, n
