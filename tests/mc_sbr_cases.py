"""Shared by tests/test_mc_sbr_cpu.py and tests/test_mc_sbr_gpu.py: the multichannel HE-AAC streams (the committed 5.1 stream plus
streams of channel_config 3, 4 and 5 that oracle/_ref/xaacenc -aot:5 makes on the spot, once per test run) and the reference
decoder's WAV files for them (test infrastructure)."""
import os
import subprocess
import wave

import numpy as np

import aac_tools_cases as tc
import multichannel_cases as mc

REF = mc.REF
# name -> (channels, core sampling rate of the encoder's input, bit rate): one stream per channel_config 3, 4, 5
ENCODED = {"mc3_he_48k": (3, 48000, 96000), "mc4_he_32k": (4, 32000, 96000), "mc5_he_48k": (5, 48000, 128000)}
NAMES = ["mc6_aot5"] + sorted(ENCODED)

_cache = {}


def stream_path(name):
    """the ADTS file of stream `name` (encoded on first use)"""
    if name == "mc6_aot5":
        return mc.stream_path(name)
    if ("aac", name) not in _cache:
        tc.need("xaacenc")
        ch, rate, br = ENCODED[name]
        wav, aac = os.path.join(mc._tmp(), name + ".wav"), os.path.join(mc._tmp(), name + ".aac")
        pcm = np.round(mc.signal(rate, ch) * 32767.0).astype(np.int16)
        with wave.open(wav, "wb") as w:
            w.setnchannels(ch), w.setsampwidth(2), w.setframerate(rate)
            w.writeframes(pcm.tobytes())
        subprocess.run([os.path.join(REF, "xaacenc"), "-ifile:" + wav, "-ofile:" + aac, "-aot:5", "-adts:1", "-br:%d" % br],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=600)
        _cache[("aac", name)] = aac
    return _cache[("aac", name)]


def stream(name):
    return open(stream_path(name), "rb").read()


def adts_frames(data):
    """the byte ranges of the ADTS frames of a stream"""
    at, out = 0, []
    while at + 7 <= len(data):
        n = ((data[at + 3] & 3) << 11) | (data[at + 4] << 3) | (data[at + 5] >> 5)
        out.append((at, at + n))
        at += n
    return out


def reference_wav(path, *flags):
    """the bytes oracle/_ref/xaacdec writes for an ADTS file with `flags`, decoded once per test run"""
    key = ("wav", path) + flags
    if key not in _cache:
        tc.need("xaacdec")
        out = os.path.join(mc._tmp(), "ref_he_%d.wav" % len(_cache))
        subprocess.run([os.path.join(REF, "xaacdec"), "-ifile:" + path, "-ofile:" + out] + list(flags), check=True, capture_output=True,
                       timeout=600)
        _cache[key] = open(out, "rb").read()
    return _cache[key]
