#!/usr/bin/env python3
"""Write tests/golden/streams_synth_sbr/*.aac: ADTS HE-AAC and HE-AACv2 streams (implicit signalling) whose SBR and PS payloads
come from a syntax generator instead of an encoder, so that the side info the reference's encoder never writes reaches the host
front end (libxaac_amd/host/sbr_side.cpp) and the kernels behind it: every bs_freq_scale / bs_alter_scale / bs_noise_bands /
bs_limiter_bands / bs_limiter_gains / bs_interpol_freq / bs_smoothing_mode, start and stop frequencies and cross-over bands all over
their ranges (dozens of band layouts, one to four patches), headers sent again unchanged, changed in the fields that cause no reset
and changed in those that do, the four frame classes with every envelope count, both delta directions, both amplitude resolutions,
inverse filtering modes 0 .. 3, additional harmonics, coupling switched on and off inside a stream, EXT_SBR_DATA_CRC payloads, and
parametric stereo with 10 / 20 / 34 bands, coarse and fine IID, 0 .. 4 envelopes, explicit borders, enable flags off, an IPD/OPD
extension element to skip and frames without a PS element.  A stream carries CRCs in every frame or in none; one with CRCs has one wrong.

The AAC-LC core frames are make_synth_streams.Gen's; the SBR fill element goes right behind the channel element.  The code words
come from libxaac_amd/host/tables_sbr_side.inc (the books read out of the reference's ROM).  The payload is a seeded draw over the
syntax of ISO/IEC 14496-3 4.4.2.8 / 8.6.4: what is legal is decided here, from the standard's rules (band tables of 4.6.18.3.2,
grids of 4.6.18.3.3, delta coding of 4.6.18.3.5 and 8.6.4.6.2), never by asking the project's parser.  Test infrastructure: the
reference decoder (oracle/_ref) supplies the expected side info and PCM through tools/make_golden_sbr_synth.py.

Kept out, because the standard rules them out or the reference does not decode them as a stream: grids whose
borders do not strictly rise or whose start does not meet the end of the frame before; a delta in time across a change of band
tables, amplitude resolution, coupling or PS band count; band tables the standard's limits refuse (k2 - k0, kx > 32, more than
five noise bands); payloads of more than 269 bytes; a frame without its fill element (the reference switches SBR off for it,
api.c:3344-3349, and with its default flags writes a file without samples); a change of extension type inside a stream."""
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_synth_streams as core  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "streams_synth_sbr")
RATES = [96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000]
FIXFIX, FIXVAR, VARFIX, VARVAR = 0, 1, 2, 3
EXT_SBR_DATA, EXT_SBR_DATA_CRC = 13, 14
MAX_PAYLOAD = 269   # the bytes a fill element holds (count 15 + esc_count 255 - 1)
# bs_start_freq -> offset from the lowest start band, by output rate (ISO/IEC 14496-3 table 4.6.18.3.2.1)
OFFSET = {16000: [-8, -7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7],
          22050: [-5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 13],
          24000: [-5, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 13, 16],
          32000: [-6, -4, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 13, 16],
          48000: [-4, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 13, 16, 20],
          96000: [-2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 13, 16, 20, 24]}
PS_BANDS = [10, 20, 34]


def nint(x):
    return int(math.floor(x + 0.5))


_books = None


def books():
    """-> {name: {value: (code, length)}} for the xh_sbr_* and xh_ps_* triples"""
    global _books
    if _books is None:
        txt = open(os.path.join(ROOT, "libxaac_amd", "host", "tables_sbr_side.inc")).read()
        t = {}
        for m in re.finditer(r"xh_(\w+)\[(\d+)\] = \{([^}]*)\}", txt):
            t[m.group(1)] = [int(v.replace("u", ""), 0) for v in m.group(3).replace("\n", " ").split(",") if v.strip()]
        _books = {}
        for name in [k[:-5] for k in t if k.endswith("_code")]:
            _books[name] = {val: (code >> (32 - ln), ln) for code, ln, val in zip(t[name + "_code"], t[name + "_len"], t[name + "_val"])}
    return _books


# ---- the band tables of a header: ISO/IEC 14496-3 4.6.18.3.2 --------------------------------------------------------------------
def band_tables(fs, h):
    """h: the header's fields -> dict(master, high, low, n_q, kx, k2) or None where the standard refuses the combination"""
    start_min = nint((3000 if fs < 32000 else 4000 if fs < 64000 else 5000) * 128.0 / fs)
    stop_min = nint((6000 if fs < 32000 else 8000 if fs < 64000 else 10000) * 128.0 / fs)
    off = OFFSET[fs] if fs in OFFSET and fs < 44100 else OFFSET[48000] if fs <= 64000 else OFFSET[96000]
    k0 = start_min + off[h["start_freq"]]
    if h["stop_freq"] < 14:
        edges = [nint(stop_min * (64.0 / stop_min) ** (p / 13.0)) for p in range(14)]
        k2 = stop_min + sum(sorted(edges[p + 1] - edges[p] for p in range(13))[:h["stop_freq"]])
    else:
        k2 = (2 if h["stop_freq"] == 14 else 3) * k0
    k2 = min(k2, 64)
    limit = 48 if fs <= 32000 else 35 if fs == 44100 else 32
    if k2 <= k0 or k2 - k0 > limit or k0 < 5:
        return None
    if h["freq_scale"] == 0:
        if h["alter_scale"] == 0:
            dk, n = 1, 2 * ((k2 - k0) // 2)
        else:
            dk, n = 2, 2 * nint((k2 - k0) / 4.0)
        if n < 1:
            return None
        d = [dk] * n
        diff = k2 - (k0 + n * dk)
        incr, k = (1, 0) if diff < 0 else (-1, n - 1)
        while diff != 0:
            d[k] -= incr
            k += incr
            diff += incr
        master = list(np.cumsum([k0] + d))
    else:
        bands = 14 - 2 * h["freq_scale"]
        warp = 1.3 if h["alter_scale"] else 1.0
        two = k2 / float(k0) > 2.2449
        k1 = 2 * k0 if two else k2

        def region(a, b, n):
            edges = [nint(a * (b / float(a)) ** (k / float(n))) for k in range(n + 1)]
            return sorted(edges[k + 1] - edges[k] for k in range(n))
        n0 = 2 * nint(bands * math.log(k1 / float(k0)) / (2.0 * math.log(2.0)))
        if n0 < 1:
            return None
        d0 = region(k0, k1, n0)
        if d0[0] <= 0:
            return None
        master = list(np.cumsum([k0] + d0))
        if two:
            n1 = 2 * nint(bands * math.log(k2 / float(k1)) / (2.0 * math.log(2.0) * warp))
            if n1 < 1:
                return None
            d1 = region(k1, k2, n1)
            if d1[0] < d0[-1]:
                change = min(d0[-1] - d1[0], (d1[-1] - d1[0]) // 2)
                d1[0] += change
                d1[-1] -= change
                d1.sort()
            if d1[0] <= 0:
                return None
            master += list(np.cumsum([k1] + d1))[1:]
    master = [int(v) for v in master]
    n_master = len(master) - 1
    if h["xover_band"] >= n_master or n_master > 48:
        return None
    high = master[h["xover_band"]:]
    n_high = len(high) - 1
    low = [high[0]] + [high[i] for i in range(2 - (n_high & 1), n_high + 1, 2)] if n_high & 1 else high[::2]
    kx = high[0]
    if kx > 32 or len(low) - 1 < 1:
        return None
    n_q = max(1, nint(h["noise_bands"] * math.log(k2 / float(kx)) / math.log(2.0))) if h["noise_bands"] else 1
    if n_q > 5 or n_q > len(low) - 1:
        return None
    return dict(master=master, high=high, low=low, n_q=n_q, kx=kx, k2=k2)


class Channel:
    """what the delta coding of one channel looks back at"""

    def __init__(self):
        self.env = None      # the last envelope's values on the high resolution bands (None: nothing to delta against)
        self.noise = None
        self.amp_res = None


class SbrGen:
    """kind: "st" (channel pair, with and without coupling), "mono", "ps" (mono with a PS element)"""

    def __init__(self, seed, sr_index, kind, frames, level, crc=False):
        """crc: every payload is an EXT_SBR_DATA_CRC one, and one frame's CRC is wrong.  A stream is of one extension type throughout:
        with its default flags the reference decodes a payload one frame late but looks at the extension type of the frame
        that has just come in (sbrdecoder.c:474-500), so a change of type makes it read a CRC word as data or the other way round."""
        self.crc = crc
        self.rng = np.random.default_rng(seed)
        self.kind, self.frames, self.fs = kind, frames, 2 * RATES[sr_index]
        self.stereo = kind == "st"
        t, aac_books = core._tables if core._tables else core.tables()
        core._tables = (t, aac_books)
        wl = [w for w in t["sfb_" + core.LONG[sr_index]] if w > 0]
        ws = [w for w in t["sfb_" + core.SHORT[sr_index]] if w > 0]
        self.core = core.Gen(seed, sr_index, wl, ws, aac_books, level, busy=True)
        self.books = books()
        self.ch = [Channel(), Channel()]
        self.prev_end = [16, 16]         # per channel: where the last grid ended
        self.header = None
        self.tables = None
        self.coupling = None
        self.must_freq = True            # the next frame's first envelopes are coded along frequency (nothing valid to look back at)
        self.ps = dict(iid=None, icc=None, header=None)
        self.notes = []                  # per frame: what was written (the tests' coverage assertions read the reference's records, not this)
        self.plan()

    def r(self, lo, hi):
        return int(self.rng.integers(lo, hi + 1))

    # ---- which frames carry what ---------------------------------------------------------------------------------------------
    def plan(self):
        n = self.frames
        body = list(range(2, n))
        self.rng.shuffle(body)
        self.resend, self.tweak, self.reset = body[0], body[1], body[2]
        self.bad_crc = body[5]
        self.no_ps = set(body[6:8]) if self.kind == "ps" else set()
        self.clamp = set(body[8:10])     # frames whose deltas run below zero (the reference clamps)

    # ---- header ------------------------------------------------------------------------------------------------------------------
    def draw_header(self, keep=None):
        """a header the standard accepts; keep: the fields of the old one that stay (the extra_2 change)"""
        while True:
            h = dict(amp_res=self.r(0, 1), start_freq=self.r(0, 15), stop_freq=self.r(0, 15), xover_band=self.r(0, 7) if self.r(0, 2) == 0 else 0,
                     extra_1=self.r(0, 3) != 0, extra_2=self.r(0, 3) != 0)
            h.update(freq_scale=self.r(0, 3), alter_scale=self.r(0, 1), noise_bands=self.r(0, 3)) if h["extra_1"] else \
                h.update(freq_scale=2, alter_scale=1, noise_bands=2)
            h.update(limiter_bands=self.r(0, 3), limiter_gains=self.r(0, 3), interpol_freq=self.r(0, 1), smoothing_mode=self.r(0, 1)) \
                if h["extra_2"] else h.update(limiter_bands=2, limiter_gains=2, interpol_freq=1, smoothing_mode=1)
            if keep is not None:
                new = dict(keep)
                for k in ("extra_2", "limiter_bands", "limiter_gains", "interpol_freq", "smoothing_mode"):
                    new[k] = h[k]
                if all(new[k] == keep[k] for k in ("limiter_bands", "limiter_gains", "interpol_freq", "smoothing_mode")):
                    continue
                return new
            t = band_tables(self.fs, h)
            if t is None:
                continue
            if self.header is not None and all(h[k] == self.header[k] for k in ("start_freq", "stop_freq", "xover_band", "freq_scale",
                                                                                   "alter_scale", "noise_bands")):
                continue
            return h

    def put_header(self, b, h):
        b.put(h["amp_res"], 1), b.put(h["start_freq"], 4), b.put(h["stop_freq"], 4), b.put(h["xover_band"], 3), b.put(0, 2)
        b.put(int(h["extra_1"]), 1), b.put(int(h["extra_2"]), 1)
        if h["extra_1"]:
            b.put(h["freq_scale"], 2), b.put(h["alter_scale"], 1), b.put(h["noise_bands"], 2)
        if h["extra_2"]:
            b.put(h["limiter_bands"], 2), b.put(h["limiter_gains"], 2), b.put(h["interpol_freq"], 1), b.put(h["smoothing_mode"], 1)

    # ---- grid --------------------------------------------------------------------------------------------------------------------
    def draw_grid(self, b, start):
        """-> (frame class, borders, freq_res per envelope); the start border meets the end of the channel's grid before"""
        while True:
            cls = self.r(0, 3)
            if start != 0 and cls in (FIXFIX, FIXVAR):
                continue
            if cls == FIXFIX:
                e = self.r(0, 2)
                n, res = 1 << e, self.r(0, 1)
                b.put(cls, 2), b.put(e, 2), b.put(res, 1)
                return cls, [16 * i // n for i in range(n + 1)], [res] * n
            if cls == FIXVAR:
                end, n_rel = 16 + self.r(0, 3), self.r(0, 3)
                rel = [self.r(0, 3) for _ in range(n_rel)]
                borders, at = [end], end
                for v in rel:
                    at -= 2 * v + 2
                    borders.insert(0, at)
                if borders[0] <= 0:
                    continue
                borders.insert(0, 0)
                n = n_rel + 1
                ptr, res = self.r(0, n), [self.r(0, 1) for _ in range(n)]
                b.put(cls, 2), b.put(end - 16, 2), b.put(n_rel, 2)
                for v in rel:
                    b.put(v, 2)
                b.put(ptr, (n + 1 - 1).bit_length() if n > 1 else 1)
                for v in reversed(res):     # (the envelopes' bits run from the last one back)
                    b.put(v, 1)
                return cls, borders, res
            if cls == VARFIX:
                n_rel = self.r(0, 3)
                rel = [self.r(0, 3) for _ in range(n_rel)]
                borders, at = [start], start
                for v in rel:
                    at += 2 * v + 2
                    borders.append(at)
                if borders[-1] >= 16:
                    continue
                borders.append(16)
                n = n_rel + 1
                ptr, res = self.r(0, n), [self.r(0, 1) for _ in range(n)]
                b.put(cls, 2), b.put(start, 2), b.put(n_rel, 2)
                for v in rel:
                    b.put(v, 2)
                b.put(ptr, (n + 1 - 1).bit_length() if n > 1 else 1)
                for v in res:
                    b.put(v, 1)
                return cls, borders, res
            end, n0, n1 = 16 + self.r(0, 3), self.r(0, 3), self.r(0, 3)
            if n0 + n1 + 1 > 5:
                continue
            rel0, rel1 = [self.r(0, 3) for _ in range(n0)], [self.r(0, 3) for _ in range(n1)]
            lead, at = [start], start
            for v in rel0:
                at += 2 * v + 2
                lead.append(at)
            trail, at = [end], end
            for v in rel1:
                at -= 2 * v + 2
                trail.insert(0, at)
            if lead[-1] >= trail[0]:
                continue
            borders = lead + trail
            n = n0 + n1 + 1
            ptr, res = self.r(0, n), [self.r(0, 1) for _ in range(n)]
            b.put(cls, 2), b.put(start, 2), b.put(end - 16, 2), b.put(n0, 2), b.put(n1, 2)
            for v in rel0 + rel1:
                b.put(v, 2)
            b.put(ptr, (n + 1 - 1).bit_length() if n > 1 else 1)
            for v in res:
                b.put(v, 1)
            return cls, borders, res

    # ---- envelopes and noise floors ------------------------------------------------------------------------------------------------
    def envelopes(self, b, c, grid, dirs, bal, amp_res, clamp):
        """the envelope scale factors of channel c: start values and code words; keeps Channel.env"""
        ch, t = self.ch[c], self.tables
        high, low = t["high"], t["low"]
        n_high = len(high) - 1
        top = (24 if amp_res else 48) if bal else (35 if amp_res else 70)   # what the reference takes without concealing
        step = 2 if bal else 1
        lav = (12 if amp_res else 24) if bal else (31 if amp_res else 60)
        name = ("bal" if bal else "env") + "_%s_" + ("30" if amp_res else "15")
        book_t, book_f = self.books["sbr_" + name % "t"], self.books["sbr_" + name % "f"]
        start_bits = (5 if amp_res else 6) if bal else (6 if amp_res else 7)
        floor = -3 * step if clamp else 0
        for e, res in enumerate(grid[2]):
            bands = high if res else low
            n = len(bands) - 1
            cover = [[k for k in range(n_high) if bands[i] <= high[k] < bands[i + 1]] for i in range(n)]
            vals = []
            if dirs[e] == 0:
                v = step * self.r(0, top // step)
                b.put(v // step, start_bits)
                vals.append(v)
                for i in range(1, n):
                    d = self.small_delta(vals[-1], step, lav, floor, top)
                    b.put(*book_f[d // step + lav])
                    vals.append(vals[-1] + d)
            else:
                for i in range(n):
                    was = ch.env[cover[i][0]]
                    d = self.small_delta(was, step, lav, floor, top)
                    b.put(*book_t[d // step + lav])
                    vals.append(was + d)
            new = [0] * n_high
            for i in range(n):
                for k in cover[i]:
                    new[k] = vals[i]
            ch.env = new
        ch.env = [min(max(v, 0), 70 >> amp_res) for v in ch.env]     # what the reference keeps behind the frame
        ch.amp_res = amp_res

    def small_delta(self, was, step, lav, floor, top):
        """a delta that keeps was + delta in floor .. top: mostly small, now and then the whole range"""
        lo, hi = max(floor - was, -lav * step), min(top - was, lav * step)
        if lo > hi:                      # (was lies outside the range: the nearest step back into it)
            return lo if was < floor else hi
        lo, hi = -((-lo) // step), hi // step
        if self.r(0, 7):
            lo, hi = max(lo, -2), min(hi, 2)
            if lo > hi:
                lo = hi = (lo if lo > 2 else hi)
        return step * self.r(lo, hi)

    def noise(self, b, c, n_env, dirs, bal, clamp):
        ch, n_q = self.ch[c], self.tables["n_q"]
        step, lav, top = (2, 12, 24) if bal else (1, 31, 30)
        book_t = self.books["sbr_noise_bal_t_30" if bal else "sbr_noise_t_30"]
        book_f = self.books["sbr_bal_f_30" if bal else "sbr_env_f_30"]
        floor, top = (-2 * step, top + 8) if clamp else (0, top)    # the reference limits the level to 0 .. 35
        for e in range(n_env):
            vals = []
            if dirs[e] == 0:
                v = step * self.r(0, min(top, 31 * step if bal else 31) // step)
                b.put(v // step, 5)
                vals.append(v)
                for i in range(1, n_q):
                    d = self.small_delta(vals[-1], step, lav, floor, top)
                    b.put(*book_f[d // step + lav])
                    vals.append(vals[-1] + d)
            else:
                for i in range(n_q):
                    d = self.small_delta(ch.noise[i], step, lav, floor, top)
                    b.put(*book_t[d // step + lav])
                    vals.append(ch.noise[i] + d)
            ch.noise = vals
        ch.noise = [min(max(v, 0), 35) for v in ch.noise]     # limited behind the frame's last noise floor

    def directions(self, n, may_time):
        d = [self.r(0, 1) for _ in range(n)]
        if not may_time:
            d[0] = 0
        return d

    # ---- parametric stereo -------------------------------------------------------------------------------------------------------
    def ps_element(self, first):
        """-> the bits of an EXTENSION_ID_PS element (ISO/IEC 14496-3 8.6.4.2)"""
        b, ps = core.Bits(), self.ps
        header = first or self.r(0, 2) == 0
        b.put(int(header), 1)
        if header:
            hd = dict(enable_iid=int(self.r(0, 5) != 0), iid_mode=self.r(0, 5), enable_icc=int(self.r(0, 5) != 0), icc_mode=self.r(0, 5),
                      enable_ext=int(self.r(0, 3) == 0))
            old = ps["header"]
            if old is None or (old["enable_iid"], old["iid_mode"]) != (hd["enable_iid"], hd["iid_mode"]):
                ps["iid"] = None
            if old is None or (old["enable_icc"], old["icc_mode"] % 3) != (hd["enable_icc"], hd["icc_mode"] % 3):
                ps["icc"] = None
            ps["header"] = hd
            b.put(hd["enable_iid"], 1)
            if hd["enable_iid"]:
                b.put(hd["iid_mode"], 3)
            b.put(hd["enable_icc"], 1)
            if hd["enable_icc"]:
                b.put(hd["icc_mode"], 3)
            b.put(hd["enable_ext"], 1)
        hd = ps["header"]
        cls = self.r(0, 1)
        b.put(cls, 1)
        if cls == 0:
            idx = self.r(0, 3)
            n_env = [0, 1, 2, 4][idx]
            b.put(idx, 2)
        else:
            n_env = self.r(1, 4)
            b.put(n_env - 1, 2)
            for pos in sorted(self.rng.choice(np.arange(1, 33), n_env, replace=False).tolist()):
                b.put(int(pos) - 1, 5)
        if hd["enable_iid"]:
            fine = hd["iid_mode"] > 2
            top = 15 if fine else 7
            df, dt = self.books["ps_iid_df_fine" if fine else "ps_iid_df"], self.books["ps_iid_dt_fine" if fine else "ps_iid_dt"]
            ps["iid"] = self.ps_params(b, n_env, PS_BANDS[hd["iid_mode"] % 3], ps["iid"], df, dt, -top, top)
        if hd["enable_icc"]:
            ps["icc"] = self.ps_params(b, n_env, PS_BANDS[hd["icc_mode"] % 3], ps["icc"], self.books["ps_icc_df"], self.books["ps_icc_dt"], 0, 7)
        if hd["enable_ext"]:
            cnt = self.r(1, 4)
            b.put(cnt, 4), b.put(0, 2)                      # ps_extension_id 0: IPD/OPD, which the reference skips
            for k in range(cnt):
                b.put(self.r(0, 255) if k else self.r(0, 31), 8 if k else 6)    # (enable_ipdopd 0)
        self.notes[-1]["ps"] = dict(hd, n_env=n_env, cls=cls)
        return b

    def ps_params(self, b, n_env, bands, prev, df, dt, lo, hi):
        for _ in range(n_env):
            time = int(prev is not None and self.r(0, 1))
            b.put(time, 1)
            vals = []
            for i in range(bands):
                was = prev[i] if time else (vals[-1] if vals else 0)
                span = 2 if self.r(0, 5) else hi - lo
                d = self.r(max(lo - was, -span), min(hi - was, span))
                b.put(*(dt if time else df)[d])
                vals.append(was + d)
            prev = vals
        return prev

    # ---- one frame's sbr_extension_data ----------------------------------------------------------------------------------------------
    def payload(self, f):
        """-> (extension type, bytes behind the type's nibble as a Bits of whole payload length) """
        note = dict(frame=f)
        self.notes.append(note)
        saved = (list(self.prev_end), self.must_freq, self.coupling, dict(self.ps), [(c.env, c.noise, c.amp_res) for c in self.ch],
                 self.header, self.tables)
        for attempt in range(64):
            b = self.sbr_data(f, note, small=attempt > 8)
            if 4 + b.n + (10 if note["crc"] else 0) <= 8 * MAX_PAYLOAD:
                break
            prev_end, self.must_freq, self.coupling, ps, chans, self.header, self.tables = saved
            self.prev_end, self.ps = list(prev_end), dict(ps)
            for c, (env, noise, amp) in zip(self.ch, chans):
                c.env, c.noise, c.amp_res = env, noise, amp
            for k in [k for k in note if k != "frame"]:
                del note[k]
        else:
            raise AssertionError("no payload of this frame fits a fill element")
        out = core.Bits()
        kind = EXT_SBR_DATA_CRC if note["crc"] else EXT_SBR_DATA
        total = -(-(4 + (10 if note["crc"] else 0) + b.n) // 8) * 8
        body = core.Bits()
        body.put(b.v, b.n)
        body.put(0, total - 4 - (10 if note["crc"] else 0) - b.n)     # bs_fill_bits
        if note["crc"]:
            crc = 0
            for i in range(body.n - 1, -1, -1):                      # x^10 + x^9 + x^5 + x^4 + x + 1 over everything behind the word
                bit = ((body.v >> i) & 1) ^ ((crc >> 9) & 1)
                crc = (crc << 1) & 0x3ff
                if bit:
                    crc ^= 0x233
            if f == self.bad_crc and self.crc:
                crc ^= 1 << self.r(0, 9)
                # the reference drops the frame and conceals, nothing of it counts
                self.prev_end, self.must_freq, self.coupling, self.ps = [16, 16], True, saved[2], dict(saved[3])
                note["bad_crc"] = True
            out.put(crc, 10)
        out.put(body.v, body.n)
        return kind, out

    def sbr_data(self, f, note, small):
        b = core.Bits()
        with_header = f == 0 or f in (self.resend, self.tweak, self.reset)
        note["crc"] = self.crc
        note["header"] = with_header
        b.put(int(with_header), 1)
        if with_header:
            if f == 0 or f == self.reset:
                self.header = self.draw_header()
                self.tables = band_tables(self.fs, self.header)
                self.must_freq = True
                for c in self.ch:
                    c.env = c.noise = None
                note["reset"] = True
            elif f == self.tweak:
                self.header = self.draw_header(keep=self.header)
            self.put_header(b, self.header)
        h, t = self.header, self.tables
        n_high, n_q = len(t["high"]) - 1, t["n_q"]
        clamp = f in self.clamp
        b.put(0, 1) if self.r(0, 4) else (b.put(1, 1), b.put(0, 8 if self.stereo else 4))     # bs_data_extra + reserved bits
        coupling = 0
        if self.stereo:
            coupling = self.r(0, 1) if self.coupling is None or self.r(0, 3) == 0 else self.coupling
            if self.prev_end[0] != self.prev_end[1]:     # the one grid of a coupled pair has one start border
                coupling = 0
            b.put(coupling, 1)
        n_ch = 2 if self.stereo else 1
        grids = []
        together = self.r(0, 1)          # a pair's grids end together in half the frames, so that the next one may be coupled
        for c in range(1 if coupling else n_ch):
            while True:
                gb = core.Bits()
                g = self.draw_grid(gb, self.prev_end[c] - 16)
                if small and len(g[2]) > 2:
                    continue
                if c == 1 and together and g[1][-1] != grids[0][1][-1]:
                    continue
                break
            b.put(gb.v, gb.n)
            grids.append(g)
        if coupling:
            grids.append(grids[0])
        may_time = not self.must_freq and (not self.stereo or coupling == self.coupling)
        amp = [0 if (g[0] == FIXFIX and len(g[2]) == 1) else h["amp_res"] for g in grids]
        dirs_e, dirs_n = [], []
        for c in range(n_ch):
            ok = may_time and self.ch[c].env is not None and self.ch[c].amp_res == amp[c]
            dirs_e.append(self.directions(len(grids[c][2]), ok))
            dirs_n.append(self.directions(1 if len(grids[c][2]) == 1 else 2, may_time and self.ch[c].noise is not None))
            for d in dirs_e[-1] + dirs_n[-1]:
                b.put(d, 1)
        invf = [[self.r(0, 3) for _ in range(n_q)] for _ in range(1 if coupling else n_ch)]
        for row in invf:
            for v in row:
                b.put(v, 2)
        if coupling:
            self.envelopes(b, 0, grids[0], dirs_e[0], False, amp[0], clamp)
            self.noise(b, 0, len(dirs_n[0]), dirs_n[0], False, clamp)
            self.envelopes(b, 1, grids[1], dirs_e[1], True, amp[1], clamp)
            self.noise(b, 1, len(dirs_n[1]), dirs_n[1], True, clamp)
        else:
            for c in range(n_ch):
                self.envelopes(b, c, grids[c], dirs_e[c], False, amp[c], clamp)
            for c in range(n_ch):
                self.noise(b, c, len(dirs_n[c]), dirs_n[c], False, clamp)
        harm = []
        for c in range(n_ch):
            on = self.r(0, 2) == 0
            harm.append(on)
            b.put(int(on), 1)
            if on:
                for _ in range(n_high):
                    b.put(int(self.r(0, 5) == 0), 1)
        ext = None
        if self.kind == "ps" and f not in self.no_ps:
            ext = core.Bits()
            ext.put(2, 2)
            e = self.ps_element(f == 0 or self.ps["header"] is None)
            ext.put(e.v, e.n)
        elif self.kind != "ps" and self.r(0, 5) == 0:           # an extension nobody knows: skipped
            ext = core.Bits()
            ext.put(self.r(0, 1), 2)
            for _ in range(self.r(1, 3)):
                ext.put(self.r(0, 255), 8)
        b.put(int(ext is not None), 1)
        if ext is not None:
            cnt = -(-ext.n // 8)
            b.put(min(cnt, 15), 4)
            if cnt >= 15:
                b.put(cnt - 15, 8)
            b.put(ext.v, ext.n)
            b.put(0, 8 * cnt - ext.n)
        self.prev_end = [grids[0][1][-1], grids[-1][1][-1]]
        self.must_freq = False
        self.coupling = coupling if self.stereo else None
        note.update(cls=[g[0] for g in grids], n_env=[len(g[2]) for g in grids], coupling=coupling, amp_res=amp, invf=invf, harm=harm,
                    clamp=clamp, header_fields=dict(h) if with_header else None)
        return b

    def frame(self, f):
        def behind(b):
            kind, bits = self.payload(f)
            cnt = (4 + bits.n) // 8
            assert (4 + bits.n) % 8 == 0 and 0 < cnt <= MAX_PAYLOAD
            b.put(6, 3)
            if cnt < 15:
                b.put(cnt, 4)
            else:
                b.put(15, 4), b.put(cnt - 14, 8)
            b.put(kind, 4), b.put(bits.v, bits.n)
        self.core.frames = f
        return self.core.frame(2 if self.stereo else 1, behind)


def make_with_notes(seed, sr_index, kind, frames, level, crc=False):
    """-> (the bytes of a stream, the generator's notes per frame)"""
    g = SbrGen(seed, sr_index, kind, frames, level, crc)
    out = []
    for f in range(frames):
        out.append(g.frame(f))
    return b"".join(out), g.notes


def make(seed, sr_index, kind, frames, level, crc=False):
    return make_with_notes(seed, sr_index, kind, frames, level, crc)[0]


# core sampling frequency indices whose SBR output rate stays at or below 48 kHz: what xaacdec_amd decodes; above them the
# reference switches to the down-sampled synthesis bank, which xaacdec_amd refuses up front
DECODED = [6, 7, 8, 9, 10, 11]


def synth_set():
    """(name, seed, sampling frequency index, kind, frames, level, decoded, crc): a stereo, a mono and a PS stream per index of
    DECODED (levels alternating so that half of each kind are LOUD, and half of each kind carry CRCs), and one refused stream (PS
    at a 32 kHz core: the down-sampled bank)"""
    rows = []
    for k, sr in enumerate(DECODED):
        for j, (kind, frames) in enumerate((("st", 24), ("mono", 12), ("ps", 24))):
            name = "%s_sr%02d" % (kind, sr)
            rows.append((name, 1000 * (j + 1) + sr, sr, kind, frames, core.LOUD if (k + j) & 1 else core.QUIET, True,
                         (k + j) % 6 in (0, 1, 3)))
    rows.append(("ps_sr05_refused", 3005, 5, "ps", 8, core.QUIET, False, False))
    return rows


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, seed, sr, kind, frames, level, _, crc in synth_set():
        data = make(seed, sr, kind, frames, level, crc)
        open(os.path.join(OUT, name + ".aac"), "wb").write(data)
        print(name, frames, "frames", len(data), "bytes")


if __name__ == "__main__":
    main()
