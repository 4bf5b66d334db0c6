#!/usr/bin/env python3
"""Write tests/golden/streams_drc/drc_*.aac: ADTS AAC-LC streams of tools/make_synth_streams.py's syntax generator with
dynamic_range_info in fill elements (extension type 0xB) behind the channel element of a frame, in front of ID_END -- what the
reference reads with ixheaacd_drc_element_read (decoder/ixheaacd_drc_freq_dec.c:609-672) once a -drc_* flag is given:

  drc_mono_1band     mono, one band over the whole frame (no drc_bands), gain words that change per frame
  drc_stereo_2band   stereo, two bands (band_top 63 and 255), prog_ref_level moving 80 .. 82
  drc_stereo_16band  stereo, sixteen bands, long and short window frames
  drc_stereo_excl    stereo, one channel excluded (either one; some frames with one element per channel), and frames with no
                     element between frames with one
  drc_stereo_nonmono stereo, band tops that do not rise: empty bands and lines that two bands cover

Every stream starts with a frame that has an element.  The tool ends with an error unless the reference decoder
(oracle/_ref/xaacdec) decodes each stream to its full length and its output with each flag set differs from its unflagged one."""
import os
import subprocess
import sys
import tempfile
import wave

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_synth_streams import Bits, Gen, adts, tables  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "streams_drc")
NAMES = ("drc_mono_1band", "drc_stereo_2band", "drc_stereo_16band", "drc_stereo_excl", "drc_stereo_nonmono")
FRAMES = 24
# (the generator's seeds.  A seed whose first frame substitutes correlated noise in a right-channel band that the left channel codes
# is avoided: the reference's two passes over the first frame leave it a seed that one pass does not, host/xaac_parse.cpp)
SEEDS = {"drc_mono_1band": 100, "drc_stereo_2band": 101, "drc_stereo_16band": 102, "drc_stereo_excl": 103, "drc_stereo_nonmono": 205}
FLAG_SETS = (("-drc_cut_fac:1", "-drc_boost_fac:1"), ("-drc_cut_fac:0.5", "-drc_boost_fac:0.25", "-drc_target_level:96"),
             ("-drc_target_level:96",), ("-drc_target_level:124",))


def drc_fill(b, gains, tops=None, prog_ref_level=None, excluded=None):
    """one fill element with one dynamic_range_info: gains = the bands' words (-127 .. 127), tops = their band_top bytes (None: a
    single band without drc_bands), excluded = the first seven channels' exclusion bits (None: no mask)"""
    e = Bits()
    e.put(0xB, 4)                       # EXT_DYNAMIC_RANGE
    e.put(0, 1)                         # pce_tag_present
    e.put(int(excluded is not None), 1)
    if excluded is not None:
        for ch in range(7):
            e.put(int(excluded[ch]) if ch < len(excluded) else 0, 1)
        e.put(0, 1)                     # additional_excluded_chns
    e.put(int(tops is not None), 1)
    if tops is not None:
        assert len(tops) == len(gains) and 1 <= len(tops) <= 16
        e.put(len(tops) - 1, 4), e.put(0, 4)   # drc_band_incr, drc_interpolation_scheme
        for t in tops:
            e.put(t, 8)
    else:
        assert len(gains) == 1
    e.put(int(prog_ref_level is not None), 1)
    if prog_ref_level is not None:
        e.put(prog_ref_level, 7), e.put(0, 1)
    for g in gains:
        e.put(int(g < 0), 1), e.put(abs(g), 7)
    assert e.n % 8 == 0
    cnt = e.n // 8
    b.put(6, 3)
    if cnt < 15:
        b.put(cnt, 4)
    else:
        b.put(15, 4), b.put(cnt - 14, 8)
    b.put(e.v, e.n)


class DrcGen(Gen):
    def frame_with(self, channels, elements):
        """a frame of one channel element, the fill elements `elements` (keyword sets of drc_fill) behind it, ID_END"""
        b = Bits()
        if channels == 1:
            b.put(0, 3), b.put(0, 4)
            self.channel_with_gain(b, None, False, False, 0)
        else:
            b.put(1, 3), b.put(0, 4)
            common = self.r(0, 3) != 0
            b.put(int(common), 1)
            if common:
                ics = self.ics(b, 0)
                self.seq[1] = self.seq[0]
                mask = self.r(0, 2)
                b.put(mask, 2)
                if mask == 1:
                    for g in range(len(ics["groups"])):
                        for _ in range(ics["max_sfb"]):
                            b.put(self.r(0, 1), 1)
                for ch in range(2):
                    self.channel_with_gain(b, ics, ch == 1, True, ch)
            else:
                for ch in range(2):
                    self.channel_with_gain(b, None, False, False, ch)
        for kw in elements:
            drc_fill(b, **kw)
        b.put(7, 3)
        return adts(b.bytes(), self.sr_index, channels)


def elements_of(name, g, f):
    """the dynamic_range_info elements of frame f of stream `name` (g: the stream's generator, for its random numbers)"""
    gain = lambda: g.r(-127, 127) if g.r(0, 3) else g.r(-12, 12)
    if name == "drc_mono_1band":
        return [dict(gains=[gain()], prog_ref_level=80 + f % 3 if f % 4 != 3 else None)]
    if name == "drc_stereo_2band":
        return [dict(gains=[gain(), gain()], tops=[63, 255], prog_ref_level=80 + f % 3)]
    if name == "drc_stereo_16band":
        tops = sorted(set(g.r(0, 254) for _ in range(15)))
        while len(tops) < 15:
            tops = sorted(set(tops + [g.r(0, 254)]))
        tops.append(255 if f % 3 else g.r(tops[-1] + 1, 255))
        return [dict(gains=[gain() for _ in range(16)], tops=tops, prog_ref_level=100 + f % 20)]
    if name == "drc_stereo_excl":
        if f and f % 5 in (2, 3):
            return []                                       # no element: the channels keep what they had
        if f % 5 == 4:                                      # one element per channel
            return [dict(gains=[gain(), gain()], tops=[g.r(10, 200), 255], prog_ref_level=90, excluded=[0, 1]),
                    dict(gains=[gain()], excluded=[1, 0])]
        return [dict(gains=[gain(), gain(), gain()], tops=[31, g.r(40, 200), 255], prog_ref_level=100 + f,
                     excluded=[f % 2, 1 - f % 2])]
    if name == "drc_stereo_nonmono":
        n = g.r(3, 8)
        tops = [g.r(0, 255) for _ in range(n)]
        if f % 2:
            tops[1] = max(0, tops[0] - g.r(1, 40))           # a band that ends below its start
        return [dict(gains=[gain() for _ in range(n)], tops=tops, prog_ref_level=108 + f % 5 - 2)]
    raise KeyError(name)


def stream(name, books, wl, ws):
    channels = 1 if "mono_" in name else 2
    g = DrcGen(SEEDS[name], 3, wl, ws, books, 60)
    frames = [g.frame_with(channels, elements_of(name, g, f)) for f in range(FRAMES)]
    return b"".join(frames), channels


def reference_pcm(path, flags, ref=os.path.join(ROOT, "oracle", "_ref", "xaacdec")):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "o.wav")
        subprocess.run([ref, "-ifile:" + path, "-ofile:" + out, *flags], check=True, capture_output=True)
        with wave.open(out) as w:
            return w.readframes(w.getnframes()), w.getnchannels()


def main():
    t, books = tables()
    wl = [w for w in t["sfb_48_1024"] if w > 0]
    ws = [w for w in t["sfb_48_128"] if w > 0]
    os.makedirs(OUT, exist_ok=True)
    for name in NAMES:
        data, channels = stream(name, books, wl, ws)
        path = os.path.join(OUT, name + ".aac")
        open(path, "wb").write(data)
        plain, nch = reference_pcm(path, ())
        assert nch == channels and len(plain) == FRAMES * 1024 * 2 * channels, (name, nch, len(plain))
        for flags in FLAG_SETS:
            pcm, _ = reference_pcm(path, flags)
            assert len(pcm) == len(plain), (name, flags, len(pcm))
            assert pcm != plain, (name, flags, "the reference's output does not change with the flags")
        print(name, FRAMES, "frames", len(data), "bytes")


if __name__ == "__main__":
    main()
