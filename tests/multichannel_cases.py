"""Shared by tests/test_multichannel_cpu.py and tests/test_multichannel_gpu.py: the multichannel AAC-LC streams (the committed
5.1 stream plus streams of channel_config 3, 4 and 5 that oracle/_ref/xaacenc makes on the spot, once per test run), the
reference decoder's WAV files for them, and the layout table of the four configurations (test infrastructure)."""
import atexit
import os
import shutil
import subprocess
import sys
import tempfile
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aac_tools_cases as tc  # noqa: E402  (transient_signal, need)

REF = os.path.join(ROOT, "oracle", "_ref")
WIDE = os.path.join(ROOT, "tests", "golden", "streams_wide")
# name -> (channels, sampling rate, bit rate): one stream per channel_config 3, 4, 5; the 4-channel one at 32 kHz
ENCODED = {"mc3_48k": (3, 48000, 160000), "mc4_32k": (4, 32000, 160000), "mc5_48k": (5, 48000, 240000)}
NAMES = ["mc6_aot2"] + sorted(ENCODED)
# channel_config -> (element ids in bitstream order: 0 SCE, 1 CPE, 3 LFE; output channel of every bitstream channel; WAV mask)
LAYOUT = {3: ((0, 1), (2, 0, 1), 0x7), 4: ((0, 1, 0), (2, 0, 1, 3), 0x107), 5: ((0, 1, 1), (2, 0, 1, 3, 4), 0x37),
          6: ((0, 1, 1, 3), (2, 0, 1, 4, 5, 3), 0x3f)}
WAV_HEADER_BYTES = 68   # WAVE_FORMAT_EXTENSIBLE as the reference's command line decoder writes it (44 for mono / stereo)

_dir = None
_cache = {}


def _tmp():
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="xaac_mc_")
        atexit.register(shutil.rmtree, _dir, True)
    return _dir


def signal(rate, channels, seconds=1.0):
    """distinct content per channel (a tone of its own over the shared transient bed) and a click train in channels 1 and 2 --
    the first channel pair of every configuration -- so that short windows occur there"""
    x = tc.transient_signal(rate, channels, seconds=seconds, seed=channels)
    t = np.arange(len(x)) / rate
    for c in range(channels):
        x[:, c] += 0.1 * np.sin(2 * np.pi * (300.0 + 170.0 * c) * t)
    for at in range(1500, len(x) - 64, 4100):
        x[at:at + 24, 1] += 0.7 * np.hanning(24)
        x[at + 3:at + 27, 2] -= 0.6 * np.hanning(24)
    return np.clip(x, -0.98, 0.98)


def stream_path(name):
    """the ADTS file of stream `name` (encoded on first use)"""
    if name == "mc6_aot2" or name == "mc6_aot5":
        return os.path.join(WIDE, name + ".aac")
    if ("aac", name) not in _cache:
        tc.need("xaacenc")
        ch, rate, br = ENCODED[name]
        wav, aac = os.path.join(_tmp(), name + ".wav"), os.path.join(_tmp(), name + ".aac")
        pcm = np.round(signal(rate, ch) * 32767.0).astype(np.int16)
        with wave.open(wav, "wb") as w:
            w.setnchannels(ch), w.setsampwidth(2), w.setframerate(rate)
            w.writeframes(pcm.tobytes())
        subprocess.run([os.path.join(REF, "xaacenc"), "-ifile:" + wav, "-ofile:" + aac, "-aot:2", "-adts:1", "-br:%d" % br],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=600)
        _cache[("aac", name)] = aac
    return _cache[("aac", name)]


def stream(name):
    return open(stream_path(name), "rb").read()


def channel_config(data):
    return ((data[2] & 1) << 2) | (data[3] >> 6)


def reference_wav(path):
    """the bytes oracle/_ref/xaacdec writes for an ADTS file (default flags), decoded once per test run"""
    if ("wav", path) not in _cache:
        tc.need("xaacdec")
        out = os.path.join(_tmp(), "ref_%d.wav" % len(_cache))
        subprocess.run([os.path.join(REF, "xaacdec"), "-ifile:" + path, "-ofile:" + out], check=True, capture_output=True, timeout=600)
        _cache[("wav", path)] = open(out, "rb").read()
    return _cache[("wav", path)]
