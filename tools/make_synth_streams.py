#!/usr/bin/env python3
"""Write tests/golden/streams/synth_*.aac: ADTS AAC-LC streams made by a syntax generator instead of an encoder, so that
the tools the reference's encoder never uses reach the parser tests -- pulse data, intensity stereo (both signs, with and
without M/S on the band), perceptual noise substitution (alone, correlated through M/S, in short blocks), every code book
with escapes up to 13 bits, TNS filters of every order in both directions on long and short windows, all window sequences
with random grouping, M/S mask modes 0 / 1 / 2, separate and common windows, fill and data stream elements in between.
The frames are random but legal; the code words come from libxaac_amd/host/tables_aac.inc (the books read out of the
reference's ROM).  Test infrastructure: the reference decoder itself (oracle/_ref) supplies the expected spectra / PCM
for these streams through tools/make_golden_parser.py like for the encoder-made ones.

And tests/golden/streams_synth/*.aac (synth_set below): every sampling frequency index 0 .. 11 with its own scale factor band
tables, mono and stereo, quiet and loud; ADTS channel_configuration 3 and 6 (SCE CPE [CPE LFE]); a stream the multichannel
entry points refuse.  tests/test_aac_tools_synth_cpu.py / _gpu.py compare them with the reference decoder run on the spot and
check that this script writes every committed file byte for byte."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "streams")
SYNTH = os.path.join(ROOT, "tests", "golden", "streams_synth")
ZERO, ESC, NOISE, IS2, IS = 0, 11, 13, 14, 15
# sampling frequency index -> width tables, as tools/gen_tables_aac_tools.py and xh_core_init choose them
LONG = ["96_1024", "96_1024", "64_1024", "48_1024", "48_1024", "32_1024", "24_1024", "24_1024", "16_1024", "16_1024",
        "16_1024", "8_1024"]
SHORT = ["96_128", "96_128", "96_128", "48_128", "48_128", "48_128", "24_128", "24_128", "16_128", "16_128", "16_128",
         "8_128"]
MC_ELEMENTS = {3: (0, 1), 6: (0, 1, 1, 3)}   # channel_configuration -> element ids in bitstream order (0 SCE, 1 CPE, 3 LFE)
QUIET, LOUD = 60, 150                         # Gen's level


def tables():
    txt = open(os.path.join(ROOT, "libxaac_amd", "host", "tables_aac.inc")).read()
    t = {}
    for m in re.finditer(r"xh_(\w+)\[(\d+)\] = \{([^}]*)\}", txt):
        t[m.group(1)] = [int(v.replace("u", ""), 0) for v in m.group(3).replace("\n", " ").split(",") if v.strip()]
    books = []
    for cb in range(12):
        enc = {}
        for code, ln, idx in zip(t["hcb%d_code" % cb], t["hcb%d_len" % cb], t["hcb%d_idx" % cb]):
            enc[idx] = (code >> (32 - ln), ln)
        books.append(enc)
    return t, books


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0, (value, bits)
        self.v = (self.v << bits) | value
        self.n += bits

    def align(self):
        self.put(0, (8 - self.n % 8) % 8)

    def bytes(self):
        self.align()
        return self.v.to_bytes(self.n // 8, "big")


def adts(payload, sr_index, channels):
    n = len(payload) + 7
    assert n < 8192, "the frame does not fit an ADTS frame_length"
    h = Bits()
    h.put(0xfff, 12), h.put(0, 1), h.put(0, 2), h.put(1, 1)       # sync, MPEG-4, layer, no CRC
    h.put(1, 2), h.put(sr_index, 4), h.put(0, 1), h.put(channels, 3)  # AAC-LC
    h.put(0, 4), h.put(n, 13), h.put(0x7ff, 11), h.put(0, 2)
    return h.bytes() + payload


class Gen:
    def __init__(self, seed, sr_index, widths_long, widths_short, books, level, avoid=False, busy=False):
        """level: the global gains are drawn from 100 .. 100 + level (LOUD: stage-1 spectra of 31 to 32 magnitude bits occur);
        avoid: no noise band in the right channel of a common-window pair where the band's ms_used bit is set and the left
        channel has no noise -- the one pattern whose noise depends on a seed an earlier frame (or another element) left;
        busy: block switching in every second frame, so that a stream of two dozen frames has enough EIGHT_SHORT ones; and a
        pair takes a common window only where both channels' window sequences of the frame before allow the same next one
        (the first form takes the left channel's word for both: the right channel may then go from EIGHT_SHORT straight to
        ONLY_LONG, which is no legal stream, and the reference's overlap-add treats it one way in a stereo stream and
        another way in a stream of more channels)"""
        self.rng = np.random.default_rng(seed)
        self.sr_index, self.wl, self.ws, self.books, self.level = sr_index, widths_long, widths_short, books, level
        self.avoid, self.busy = avoid, busy
        self.seq = [0, 0]
        self.history = {}   # multichannel frames: the window sequences of every channel element's channels
        self.window_cb, self.window_pos = None, 0   # fits()
        self.frames = 0     # frames made so far
        self.right_only = set()   # the frames with the pattern `avoid` keeps out, as written

    def r(self, lo, hi):
        return int(self.rng.integers(lo, hi + 1))

    def next_sequence(self, prev):
        if self.busy:   # a quarter of the frames EIGHT_SHORT instead of one in eleven
            return self.r(0, 1) if prev in (0, 3) else 2 + self.r(0, 1)
        if prev in (0, 3):
            return 0 if self.r(0, 3) else 1
        return 2 if self.r(0, 2) == 0 else 3

    def ics(self, b, ch, forced=None):
        seq = self.next_sequence(self.seq[ch]) if forced is None else forced
        self.seq[ch] = seq
        shape = self.r(0, 1)
        b.put(0, 1), b.put(seq, 2), b.put(shape, 1)
        if forced is not None:     # (the LFE)
            max_sfb = self.r(1, 12)
            b.put(max_sfb, 6), b.put(0, 1)
            return dict(seq=seq, max_sfb=max_sfb, groups=[1])
        if seq != 2:
            max_sfb = self.r(0, len(self.wl)) if self.r(0, 9) == 0 else self.r(len(self.wl) // 2, len(self.wl))
            b.put(max_sfb, 6), b.put(0, 1)
            return dict(seq=seq, max_sfb=max_sfb, groups=[1])
        max_sfb = self.r(0, len(self.ws))
        grouping = self.r(0, 127)
        b.put(max_sfb, 4), b.put(grouping, 7)
        groups = [1]
        for i in range(7):
            if grouping & (0x40 >> i):
                groups[-1] += 1
            else:
                groups.append(1)
        return dict(seq=seq, max_sfb=max_sfb, groups=groups)

    def channel(self, b, ics, intensity, lfe=False):
        """what follows global_gain and ics_info in an individual_channel_stream"""
        long_block = ics["seq"] != 2
        widths = self.wl if long_block else self.ws
        max_sfb, groups = ics["max_sfb"], ics["groups"]
        # sections
        sect_bits, esc = (5, 31) if long_block else (3, 7)
        choices = [ZERO] + list(range(1, 12)) * 2 + [NOISE, NOISE] + ([IS, IS2, IS] if intensity else [])
        cbs = []
        for g in range(len(groups)):
            row, sfb = [], 0
            while sfb < max_sfb:
                cb = choices[self.r(0, len(choices) - 1)]
                ln = min(self.r(1, 8), max_sfb - sfb)
                if self.avoid and intensity and cb == NOISE and any(
                        ics["ms"][g][k] and ics["left"][g][k] != NOISE for k in range(sfb, sfb + ln)):
                    cb = self.r(1, 11)
                b.put(cb, 4)
                left = ln
                while left >= esc:
                    b.put(esc, sect_bits)
                    left -= esc
                b.put(left, sect_bits)
                row += [cb] * ln
                sfb += ln
            cbs.append(row)
        # scale factors
        noise_seen = False
        for g in range(len(groups)):
            for cb in cbs[g]:
                if cb == ZERO:
                    continue
                if cb == NOISE and not noise_seen:
                    b.put(self.r(200, 330), 9)
                    noise_seen = True
                else:
                    d = self.r(-6, 6) if cb < NOISE else self.r(-4, 4)
                    code, ln = self.books[0][d + 60]
                    b.put(code, ln)
        # pulse data
        pulse = long_block and max_sfb > 0 and self.r(0, 2) == 0
        b.put(int(pulse), 1)
        if pulse:
            number = self.r(0, 3)
            start = self.r(0, min(max_sfb - 1, 30))
            b.put(number, 2), b.put(start, 6)
            for _ in range(number + 1):
                b.put(self.r(0, 31), 5), b.put(self.r(1, 15), 4)
        # TNS
        tns = max_sfb > 0 and self.r(0, 1) == 0 and not lfe
        b.put(int(tns), 1)
        if tns:
            for w in range(1 if long_block else 8):
                n_filt = self.r(0, 3 if long_block else 1) if self.r(0, 2) else 0
                b.put(n_filt, 2 if long_block else 1)
                if not n_filt:
                    continue
                res = self.r(0, 1)
                b.put(res, 1)
                for _ in range(n_filt):
                    b.put(self.r(0, (len(widths) if long_block else 8)), 6 if long_block else 4)   # length in bands
                    order = self.r(0, 12 if long_block else 7)
                    b.put(order, 5 if long_block else 3)
                    if order:
                        b.put(self.r(0, 1), 1)
                        compress = self.r(0, 1)
                        b.put(compress, 1)
                        bits = res + 3 - compress
                        for _ in range(order):
                            b.put(self.r(0, (1 << bits) - 1), bits)
        b.put(0, 1)  # gain_control_data_present
        # spectral data
        self.window_cb = None
        for g, glen in enumerate(groups):
            sfb = 0
            while sfb < max_sfb:
                cb = cbs[g][sfb]
                if cb == ZERO or cb >= NOISE:
                    sfb += 1
                    continue
                for _ in range(glen if not long_block else 1):
                    self.spectral(b, cb, widths[sfb])
                sfb += 1
        return cbs

    def fits(self, b, cb, length, signs):
        """The reference reads the code words of a section from a 32-bit window that it refills by one byte behind a code
        word and one byte behind its sign bits (block.c:504-604, :643-779, ixheaacd_aac_read_byte_corr): a code word with
        signs of more than 16 bits -- book 3 has 16 + 4, book 9 15 + 2 -- leaves the window shorter than it found it, and a
        run of them starves it: the next long code word is then read with zero bits at its end, as another one.  No encoder
        writes such runs; this generator would, every few dozen streams.  Follows the window's read position through
        neighbouring bands of one book (the reference starts every section afresh, so it is never behind this count) and
        says whether the next code word still lies inside the window; the caller draws again if not."""
        if cb != self.window_cb:
            self.window_cb, self.window_pos = cb, b.n % 8
        if self.window_pos + length > 32:
            return False
        pos = self.window_pos + length
        pos -= 8 if pos >= 8 else 0
        pos += signs
        pos -= 8 if pos >= 8 else 0
        self.window_pos = pos
        return True

    def spectral(self, b, cb, width):
        book = self.books[cb]
        if cb != self.window_cb:
            self.window_cb = None
        if cb <= 4:
            for _ in range(width // 4):
                if cb <= 2:
                    v = [self.r(-1, 1) for _ in range(4)]
                    idx = 27 * (v[0] + 1) + 9 * (v[1] + 1) + 3 * (v[2] + 1) + v[3] + 1
                    b.put(*book[idx])
                else:
                    while True:
                        v = [self.r(-2, 2) for _ in range(4)]
                        idx = 27 * abs(v[0]) + 9 * abs(v[1]) + 3 * abs(v[2]) + abs(v[3])
                        if self.fits(b, cb, book[idx][1], sum(x != 0 for x in v)):
                            break
                    b.put(*book[idx])
                    for x in v:
                        if x:
                            b.put(int(x < 0), 1)
        elif cb <= 10:
            lav = {5: 4, 6: 4, 7: 7, 8: 7, 9: 12, 10: 12}[cb]
            for _ in range(width // 2):
                v = [self.r(-lav, lav) if self.r(0, 3) else 0 for _ in range(2)]
                if cb <= 6:
                    b.put(*book[9 * (v[0] + 4) + v[1] + 4])
                else:
                    mod = 8 if cb <= 8 else 13
                    while not self.fits(b, cb, book[mod * abs(v[0]) + abs(v[1])][1], sum(x != 0 for x in v)):
                        v = [self.r(-lav, lav) if self.r(0, 3) else 0 for _ in range(2)]
                    b.put(*book[mod * abs(v[0]) + abs(v[1])])
                    for x in v:
                        if x:
                            b.put(int(x < 0), 1)
        else:
            for _ in range(width // 2):
                v = []
                for _ in range(2):
                    k = self.r(0, 9)
                    m = self.r(0, 15) if k < 7 else (self.r(16, 200) if k < 9 else self.r(201, 8191))
                    v.append(-m if self.r(0, 1) else m)
                b.put(*book[17 * min(abs(v[0]), 16) + min(abs(v[1]), 16)])
                for x in v:
                    if x:
                        b.put(int(x < 0), 1)
                for x in v:
                    m = abs(x)
                    if m >= 16:
                        n = m.bit_length() - 5
                        b.put((1 << n) - 1, n), b.put(0, 1), b.put(m - (1 << (n + 4)), n + 4)

    def frame(self, channels, behind=None):
        """behind(b): called right behind the channel element (tools/make_synth_sbr_streams.py hangs the SBR fill element there)"""
        b = Bits()
        if self.r(0, 5) == 0:                       # a data stream element in front
            cnt, flag = self.r(0, 6), self.r(0, 1)
            b.put(4, 3), b.put(0, 4), b.put(flag, 1), b.put(cnt, 8)
            if flag:
                b.align()
            for _ in range(cnt):
                b.put(self.r(0, 255) if self.r(0, 3) else 0x12, 8)
        if channels == 1:
            b.put(0, 3), b.put(0, 4)
            self.channel_with_gain(b, None, False, False, 0)
            if behind:
                behind(b)
            b.put(7, 3)
            return adts(b.bytes(), self.sr_index, 1)
        self.pair(b, 0)
        if behind:
            behind(b)
        if self.r(0, 3) == 0:                       # a fill element (not SBR)
            cnt = self.r(1, 10)
            b.put(6, 3), b.put(cnt, 4), b.put(0, 4), b.put(0, 4)
            for _ in range(cnt - 1):
                b.put(0xa5, 8)
        b.put(7, 3)
        return adts(b.bytes(), self.sr_index, 2)

    def pair(self, b, tag):
        """a channel_pair_element"""
        b.put(1, 3), b.put(tag, 4)
        common = self.r(0, 3) != 0
        if self.busy and (self.seq[0] in (0, 3)) != (self.seq[1] in (0, 3)):
            common = False   # (the channels' histories allow no common next sequence)
        b.put(int(common), 1)
        if common:
            ics = self.ics(b, 0)
            self.seq[1] = self.seq[0]
            mask = self.r(0, 2)
            b.put(mask, 2)
            ics["ms"] = [[int(mask == 2)] * ics["max_sfb"] for _ in ics["groups"]]
            if mask == 1:
                for g in range(len(ics["groups"])):
                    for sfb in range(ics["max_sfb"]):
                        ics["ms"][g][sfb] = self.r(0, 1)
                        b.put(ics["ms"][g][sfb], 1)
            for ch in range(2):   # intensity stereo needs the common window (its sign rides on the M/S mask)
                cbs = self.channel_with_gain(b, ics, ch == 1, True, ch)
                if ch == 0:
                    ics["left"] = cbs
            if any(m and r == NOISE and l != NOISE for g in range(len(cbs)) for m, l, r in zip(ics["ms"][g], ics["left"][g], cbs[g])):
                self.right_only.add(self.frames)
        else:
            for ch in range(2):
                self.channel_with_gain(b, None, False, False, ch)

    def channel_with_gain(self, b, ics, right, common, ch, forced=None):
        """individual_channel_stream: global_gain, (ics_info), then the rest; -> the code book of every band"""
        gain = self.r(100, 100 + self.level)
        b.put(gain, 8)
        if not common:
            ics = self.ics(b, ch, forced)
        return self.channel(b, ics, right, lfe=forced is not None)

    def frame_mc(self, config):
        """a frame of ADTS channel_configuration 3 (SCE CPE) or 6 (SCE CPE CPE LFE), element instance tags counted per kind
        of element; every element keeps its own window sequence history.  The reference reads an LFE as it reads an SCE
        (aacdecoder.c:388-401) and puts no restriction of its own on it; this one keeps to ISO/IEC 14496-3 4.6.10: long
        windows only (ONLY_LONG_SEQUENCE), no TNS, a low max_sfb"""
        b = Bits()
        tags = {0: 0, 1: 0, 3: 0}
        for k, kind in enumerate(MC_ELEMENTS[config]):
            self.seq = self.history.setdefault(k, [0, 0])
            if kind == 1:
                self.pair(b, tags[kind])
            else:
                b.put(kind, 3), b.put(tags[kind], 4)
                self.channel_with_gain(b, None, False, False, 0, forced=0 if kind == 3 else None)
            tags[kind] += 1
            if kind != 3 and self.r(0, 5) == 0:     # a fill element (not SBR) behind the element
                cnt = self.r(1, 6)
                b.put(6, 3), b.put(cnt, 4), b.put(0, 4), b.put(0, 4)
                for _ in range(cnt - 1):
                    b.put(0xa5, 8)
        b.put(7, 3)
        return adts(b.bytes(), self.sr_index, config)


_tables = None


def make(seed, sr_index, frames, level, kind, avoid=False, busy=True):
    """-> the bytes of a stream; kind: 1 mono, 2 stereo, or channel_configuration 3 / 6"""
    return make_with_notes(seed, sr_index, frames, level, kind, avoid, busy)[0]


def make_with_notes(seed, sr_index, frames, level, kind, avoid=False, busy=True):
    """-> (the bytes, the frames the generator wrote a right-only correlated noise band into -- see Gen's `avoid`)"""
    global _tables
    if _tables is None:
        _tables = tables()
    t, books = _tables
    wl = [w for w in t["sfb_" + LONG[sr_index]] if w > 0]
    ws = [w for w in t["sfb_" + SHORT[sr_index]] if w > 0]
    assert sum(wl) == 1024 and sum(ws) == 128
    g = Gen(seed, sr_index, wl, ws, books, level, avoid, busy)
    out = []
    for g.frames in range(frames):
        out.append(g.frame(kind) if kind <= 2 else g.frame_mc(kind))
    return b"".join(out), sorted(g.right_only)


# tests/golden/streams: (name, seed, sampling frequency index, frames, level, kind, avoid)
FIRST = [("synth_lc_a", 11, 3, 96, 40, 2, False), ("synth_lc_b", 12, 3, 96, 90, 2, False), ("synth_lc_mono", 13, 3, 64, 60, 1, False)]
# the stereo streams' seeds: 100 + index unless listed (picked so that every index meets the coverage floors of
# tests/test_aac_tools_synth_cpu.py and five streams at five indices (3, 5, 7, 8, 9) have a right-only correlated noise band in frame 0)
STEREO_SEED = {0: 112, 7: 131, 8: 180, 9: 121}
MONO_SEED = {1: 225, 2: 214, 3: 263, 4: 216, 6: 242, 10: 234}


def synth_set():
    """tests/golden/streams_synth, the same rows: a stereo stream of 24 frames and a mono stream of 12 per sampling frequency
    index (the stereo one LOUD at the odd indices, the mono one at the even ones); channel_configuration 3 and 6 with the
    avoidance switch on; one short configuration-6 stream with it off, which the multichannel entry points refuse"""
    rows = []
    for sr in range(12):
        rows.append(("st_sr%02d" % sr, STEREO_SEED.get(sr, 100 + sr), sr, 24, LOUD if sr & 1 else QUIET, 2, False))
        rows.append(("mono_sr%02d" % sr, MONO_SEED.get(sr, 200 + sr), sr, 12, QUIET if sr & 1 else LOUD, 1, False))
    rows += [("mc3_sr03", 14303, 3, 24, QUIET, 3, True), ("mc3_sr08", 15308, 8, 24, QUIET, 3, True),
             ("mc6_sr03", 603, 3, 24, QUIET, 6, True), ("mc6_sr05", 1605, 5, 24, QUIET, 6, True),
             ("mc6_sr11", 1611, 11, 24, QUIET, 6, True), ("mc6_sr03_loud", 633, 3, 24, LOUD, 6, True),
             ("mc6_sr03_refused", 663, 3, 8, QUIET, 6, False)]
    return rows


def write(rows, out, busy):
    os.makedirs(out, exist_ok=True)
    for name, seed, sr, frames, level, kind, avoid in rows:
        data = make(seed, sr, frames, level, kind, avoid, busy)
        open(os.path.join(out, name + ".aac"), "wb").write(data)
        print(name, frames, "frames", len(data), "bytes")


def main():
    write(FIRST, OUT, False)
    write(synth_set(), SYNTH, True)


if __name__ == "__main__":
    main()
