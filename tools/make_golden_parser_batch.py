#!/usr/bin/env python3
"""Pins what xaac_parse_batch_run_sized writes: tests/golden/parser_batch_pin.json holds, for every run below, the CRC32 of
every output array (chained over the calls of the run, the arrays pre-filled and never cleared in between, so rows a call leaves
alone count too) and of the calls' return values.  The runs walk the committed ADTS streams to their end -- intact, truncated,
with flipped bits, spliced into a stream of another channel count (the refusal behind a delivered frame and its roll-back) and
re-framed as ADTS frames of two raw data blocks -- at stage 1 and 2, in both readings of the SBR payload, one and four frames per
call, and two streams per batch.  tests/test_parser_elements_cpu.py replays the runs against the library as it is.

    python tools/make_golden_parser_batch.py            # writes the file (XAAC_HOST_LIBRARY: another build of the library)
"""
import ctypes
import glob
import json
import os
import random
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libxaac_amd import (CORE_TOOLS_SIDE_BYTES, ESBR_SIDE_BYTES, PS_FRAME_BYTES, SBR_FRAME_BYTES,  # noqa: E402
                         SBR_HEADER_BYTES, decoder)

GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN = os.path.join(GOLDEN, "parser_batch_pin.json")
SEED = 20261019
ARRAYS = ("spec", "ics", "header", "frame", "ps_frame", "flags", "tools", "consumed", "status", "esbr_side", "reset_pitch", "pos",
          "lines", "tools_side")
MAX_CALLS = 4096    # (no committed stream has that many frames: a run that does not end is a bug)


def streams():
    """name -> bytes: the ten mono / stereo streams and the two 5.1 ones"""
    out = {os.path.basename(f)[:-4]: open(f, "rb").read() for f in sorted(glob.glob(os.path.join(GOLDEN, "streams", "*.aac")))}
    for name in ("mc6_aot2", "mc6_aot5"):
        out[name] = open(os.path.join(GOLDEN, "streams_wide", name + ".aac"), "rb").read()
    return out


def frame_offsets(data):
    """the byte offsets of the ADTS frames of an intact stream, and its end"""
    at, out = 0, []
    while at + 7 <= len(data):
        n = ((data[at + 3] & 3) << 11) | (data[at + 4] << 3) | (data[at + 5] >> 5)
        if n < 7 or at + n > len(data):
            break
        out.append(at)
        at += n
    return out + [at]


def two_block_frames(frames):
    """unprotected single-block ADTS frames, two by two as one ADTS frame of two raw data blocks (the first one's header with the
    length of both and number_of_raw_data_blocks_in_frame = 1)"""
    out = []
    for k in range(0, len(frames) - 1, 2):
        a, b = frames[k], frames[k + 1]
        assert a[1] & 1 and b[1] & 1 and not a[6] & 3 and not b[6] & 3
        n = len(a) + len(b) - 7
        h = bytearray(a[:7])
        h[3], h[4], h[5], h[6] = (h[3] & 0xfc) | (n >> 11), (n >> 3) & 0xff, (h[5] & 0x1f) | ((n & 7) << 5), (h[6] & 0xfc) | 1
        out.append(bytes(h) + a[7:] + b[7:])
    return b"".join(out)


def damaged(name, all_streams, kinds):
    """[(label, bytes)]: the deterministic damaged copies of one stream"""
    data = all_streams[name]
    rng = random.Random("%d %s" % (SEED, name))
    at = frame_offsets(data)
    frames = [data[at[k]:at[k + 1]] for k in range(len(at) - 1)]
    out = [("cut%d" % k, data[:rng.randrange(at[1] + 1, len(data))]) for k in range(3)]
    flipped = bytearray(data)
    for _ in range(32):
        flipped[rng.randrange(at[1], len(data))] ^= 1 << rng.randrange(8)
    out.append(("flips", bytes(flipped)))
    half = at[len(frames) // 2]
    wide = kinds[name]["channel_config"] != 0
    # behind the first half: a stream of another channel count (mono -> stereo, stereo -> mono), the 5.1 streams the other 5.1 one
    other_ch = sorted(n for n, k in kinds.items() if not k["channel_config"] and k["n_ch"] != kinds[name]["n_ch"])[0]
    partner = ("mc6_aot5" if name == "mc6_aot2" else "mc6_aot2") if wide else other_ch
    out.append(("splice_" + partner, data[:half] + all_streams[partner]))
    if wide:    # ... and a stereo one: the channel_config refusal
        stereo = sorted(n for n, k in kinds.items() if not k["channel_config"] and k["n_ch"] == 2)[0]
        out.append(("splice_" + stereo, data[:half] + all_streams[stereo]))
    else:       # two raw data blocks per ADTS frame, the last frame's second block the other stream's: refused behind a delivered
        other = all_streams[other_ch]    # block, with the block count to be rolled back
        o = frame_offsets(other)
        odd = frames[:9] + [other[o[0]:o[1]]]
        out.append(("blocks", two_block_frames(frames[:10]) + data[at[10]:at[14]]))
        out.append(("blocks_" + other_ch, two_block_frames(odd) + data[at[10]:at[14]]))
    return out


def stream_kinds(all_streams):
    """name -> the batch settings its first frame asks for"""
    out = {}
    for name, data in all_streams.items():
        n_ch, n_els, sbr, config = decoder.probe_first_frame(data)
        out[name] = {"n_ch": n_ch, "n_els": n_els, "sbr": bool(sbr), "channel_config": config if n_els > 1 else 0}
    return out


def run_batch(lib, datas, kind, stage, esbr, frames):
    """walks the streams to their end with xaac_parse_batch_run_sized -> {array: crc32, "rc": crc32 of the return values}"""
    n, T, n_ch, n_els = len(datas), frames, kind["n_ch"], kind["n_els"]
    sbr, wide = kind["sbr"], kind["channel_config"] != 0
    parsers = (ctypes.c_void_p * n)()
    for i in range(n):
        h = ctypes.c_void_p()
        assert lib.xaac_parser_create(ctypes.byref(h)) == 0
        assert lib.xaac_parser_set_esbr(h, int(esbr)) == 0
        parsers[i] = h
    blobs = [np.frombuffer(d + b"\0" * 16, np.uint8).copy() for d in datas]
    ptrs = np.array([b.ctypes.data for b in blobs], np.uint64)
    size = np.array([len(d) for d in datas], np.uint64)
    fill = lambda shape, dtype: np.frombuffer(b"\xa5" * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()
    a = {"spec": fill((T, n * n_ch, 1024), np.int32), "ics": fill((T, n * n_ch, 2), np.uint8), "tools": fill((T, n), np.int32),
         "consumed": fill((n,), np.uint64), "status": fill((T, n), np.int32), "pos": np.zeros(n, np.uint64),
         "lines": fill((T, n), np.int32), "tools_side": fill((T, n_els * n, CORE_TOOLS_SIDE_BYTES), np.uint8)}
    if sbr:
        a["header"], a["frame"] = fill((T, n * n_ch, SBR_HEADER_BYTES), np.uint8), fill((T, n * n_ch, SBR_FRAME_BYTES), np.uint8)
        a["flags"], a["reset_pitch"] = fill((T, n * n_els, 8), np.int32), fill((T, n * n_els), np.int32)
        if not wide:
            a["ps_frame"] = fill((T, n, PS_FRAME_BYTES), np.uint8)
        if esbr:
            a["esbr_side"] = fill((T, n * n_ch, ESBR_SIDE_BYTES), np.uint8)
    b = decoder._ParseBatch()
    b.n_streams, b.n_ch, b.with_sbr, b.ps_enable, b.stage, b.threads = n, n_ch, int(sbr), 1, stage, 1
    b.parser, b.data, b.bytes = ctypes.addressof(parsers), ptrs.ctypes.data, size.ctypes.data
    for name, arr in a.items():
        setattr(b, name, arr.ctypes.data)
    b.frames, b.channel_config, b.mc_sbr = T, kind["channel_config"], int(wide and sbr)
    crc, rcs = dict.fromkeys(a, 0), []
    while len(rcs) < MAX_CALLS:
        rcs.append(lib.xaac_parse_batch_run_sized(ctypes.byref(b), ctypes.sizeof(b)))
        for name, arr in a.items():
            crc[name] = zlib.crc32(arr.tobytes(), crc[name])
        if len(rcs) >= 2 and rcs[-1] <= 0 and rcs[-2] <= 0:    # (one call beyond the end: what a refusal left in the parser shows there)
            break
    assert rcs[-1] <= 0, "the run did not end"
    for i in range(n):
        lib.xaac_parser_destroy(parsers[i])
    crc["rc"] = zlib.crc32(np.array(rcs, np.int32).tobytes())
    return crc, sum(r for r in rcs if r > 0)


def runs():
    """yields (label, streams, kind, stage, esbr, frames)"""
    all_streams = streams()
    kinds = stream_kinds(all_streams)
    for name, data in all_streams.items():
        copies = [("intact", data)] + damaged(name, all_streams, kinds)
        for label, blob in copies:
            for stage in (1, 2):
                for esbr in ((0, 1) if kinds[name]["sbr"] else (0,)):
                    for frames in (1, 4):
                        yield "%s/%s/s%de%dT%d" % (name, label, stage, esbr, frames), [blob], kinds[name], stage, esbr, frames
    stereo = [n for n in sorted(kinds) if not kinds[n]["channel_config"] and kinds[n]["n_ch"] == 2]
    pairs = [(a, b) for a in stereo for b in stereo if a < b and kinds[a]["sbr"] == kinds[b]["sbr"]]
    two = [pairs[0], [p for p in pairs if kinds[p[0]]["sbr"] != kinds[pairs[0][0]]["sbr"]][0], ("mc6_aot5", "mc6_aot5")]
    for x, y in two:
        for stage in (1, 2):
            for esbr in ((0, 1) if kinds[x]["sbr"] else (0,)):
                for frames in (1, 4):
                    yield "%s+%s/s%de%dT%d" % (x, y, stage, esbr, frames), [all_streams[x], all_streams[y]], kinds[x], stage, esbr, frames


def replay():
    """-> ({label: the crc32 words of the run's arrays in the order of ARRAYS, then the one of its return values}, frames parsed)"""
    lib = decoder.load_host_library()
    lib.xaac_parse_batch_run_sized.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    out, total = {}, 0
    for label, datas, kind, stage, esbr, frames in runs():
        crc, parsed = run_batch(lib, datas, kind, stage, esbr, frames)
        out[label] = " ".join("%08x" % crc[k] for k in ARRAYS + ("rc",) if k in crc)
        total += parsed
    return out, total


def main():
    pin, total = replay()
    with open(PIN, "w") as f:
        json.dump({"seed": SEED, "runs": pin}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d runs, %d frames -> %s (%d bytes)" % (len(pin), total, PIN, os.path.getsize(PIN)))


if __name__ == "__main__":
    main()
