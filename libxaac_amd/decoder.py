"""libxaac_amd.decoder -- whole-stream decoding with no reference code in the process: the host-side bitstream front end
(libxaac_amd/libxaac_host.so, include/xaac_parse.h: ADTS, AAC-LC syntax, SBR / PS side info, all on the CPU) feeding the
GPU entry points of include/xaac_amd.h (IMDCT, low-power / HQ SBR with parametric stereo, peak limiter), with every stream's
state resident in device memory.  Mirrors what the reference's command line decoder does for `xaacdec -esbr:0` on ADTS
AAC-LC / HE-AAC / HE-AACv2 streams of one or two channels (decoder/ixheaacd_api.c:2624-3788: frame loop, core -> SBR
hand-off :353-366, peak limiter and its delay :3666-3692, the flush of its delay line :2824-2866, mono duplicated to
stereo :3639-3660), so the PCM equals the reference's byte for byte (tests/test_decoder_gpu.py).

`parse_stream` is the CPU half alone (used by the CPU tests and the parser-rate measurement); `decode_streams` decodes
N streams in lock step, one batch of frames per GPU call.  There is no CPU fallback for the GPU half.
"""
import collections
import ctypes
import os
import time

import numpy as np

from . import (CORE_TOOLS_SIDE_BYTES, CORE_TOOLS_STATE_BYTES, DRC_SIDE_WORDS, ESBR_PS_STATE_BYTES, ESBR_SIDE_BYTES, ESBR_STATE_BYTES,
               HANDOVER_PS_START, HBE_STATE_BYTES, LIMITER_STATE_BYTES, PCM_LC, PCM_SBR, PS_FRAME_BYTES, PS_STATE_BYTES,
               SBR_FRAME_BYTES, SBR_HEADER_BYTES, SBR_STATE_BYTES, LimiterState, XaacContext, out_map_channels, peak_limiter_init)
from . import out_map as make_out_map
from . import abi
from .abi import (AdtsHeader, CoreFrame, CoreToolsChannel, CoreToolsSide, CoreToolsState, DrcConfig, SbrSide,  # noqa: F401
                  TnsFilterSide)
from .abi import (F_APPLY, F_FRAME_OK, F_PS, F_PS_START, F_RESET, F_RESET_CHANNELS, F_STEREO,  # noqa: F401  (the flag row's positions)
                  F_UPSAMPLING)
from .abi import ParseBatch as _ParseBatch   # the descriptor BatchParser fills

_HERE = os.path.dirname(os.path.abspath(__file__))
_host = None
torch = None    # imported by the first decode_streams call: the parser half of this module works without it

TOOL_MS, TOOL_INTENSITY, TOOL_PNS, TOOL_TNS, TOOL_PULSE, TOOL_SHORT, TOOL_ESCAPE = 1, 2, 4, 8, 16, 32, 64


def host_library_path():
    return os.environ.get("XAAC_HOST_LIBRARY") or os.path.join(_HERE, "libxaac_host.so")


def load_host_library():
    """the CPU front end; raises when it has not been built (make -C libxaac_amd/host)"""
    global _host
    if _host is None:
        path = host_library_path()
        if not os.path.exists(path):
            raise RuntimeError("libxaac_host.so is not built: make -C libxaac_amd/host")
        _host = abi.bind_host(ctypes.CDLL(path))
    return _host


def out_map_apply_host(m, pcm):
    """xaac_out_map_apply_host, the CPU twin of the mapped GPU calls: pcm int16[samples, channels] through the OutMap m (None:
    as it is) -> int16[samples, mapped channels]"""
    pcm = np.ascontiguousarray(pcm, np.int16)
    if m is None:
        return pcm.copy()
    samples, n_ch = pcm.shape
    out = np.zeros((samples, max(1, n_ch, 2)), np.int16)
    oc = load_host_library().xaac_out_map_apply_host(ctypes.byref(m), n_ch, pcm.ctypes.data, samples, out.ctypes.data)
    if oc <= 0:
        raise ValueError("the output map does not take %d channels" % n_ch)
    return out.reshape(-1)[:samples * oc].reshape(samples, oc).copy()


def drc_config(drc):
    """decode_streams' drc argument -> the DrcConfig the parsers take (xaac_drc_config), or None for None.  drc: a dict of
    cut=, boost= (0 .. 1: -drc_cut_fac, -drc_boost_fac) and target_level= (0 .. 127: -drc_target_level), any of them left out
    keeps the reference's 1, 1 and 108 (api.c:477-481).  The reference keeps (WORD32)(factor * 100) of a float (api.c:629-653).  ValueError for
    anything else: a value out of range, heavy_comp (-drc_heavy_comp:1: DVB ancillary data, not supported), an unknown key."""
    if drc is None:
        return None
    if not isinstance(drc, dict):
        raise ValueError("drc is None or a dict of cut=, boost=, target_level=")
    unknown = set(drc) - {"cut", "boost", "target_level", "heavy_comp"}
    if unknown:
        raise ValueError("drc: unknown key %s" % sorted(unknown)[0])
    if drc.get("heavy_comp"):
        raise ValueError("drc heavy_comp (-drc_heavy_comp:1, DVB ancillary data) is not supported")
    cfg = DrcConfig(100, 100, 108)
    for key in ("cut", "boost"):
        v = np.float32(drc.get(key, 1.0))
        if not 0.0 <= v <= 1.0:
            raise ValueError("drc %s is outside 0 .. 1" % key)
        setattr(cfg, key, int(v * np.float32(100)))
    level = drc.get("target_level", 108)
    if int(level) != level or not 0 <= level <= 127:
        raise ValueError("drc target_level is outside 0 .. 127")
    cfg.target_level = int(level)
    return cfg


def _refuse_drc(n_ch, sbr, channel_config):
    """what dynamic range control does not cover, as decode_streams and the command line decoder refuse it"""
    if sbr:
        raise ValueError("drc on a stream with SBR (the QMF-domain branch of dynamic range control) is not supported")
    if channel_config:
        raise ValueError("drc on a stream of more than two channels is not supported")


def drc_apply_host(side, spec):
    """xaac_drc_apply_host, the CPU twin of xaac_drc_apply_batch: side int32[DRC_SIDE_WORDS] (one xaac_drc_side), spec int32[1024]
    in place -> the call's return value (0, or -1 for a row it refuses)"""
    side = np.ascontiguousarray(side, np.int32)
    assert side.size == DRC_SIDE_WORDS and spec.dtype == np.int32 and spec.size == 1024 and spec.flags["C_CONTIGUOUS"]
    return int(load_host_library().xaac_drc_apply_host(side.ctypes.data, spec.ctypes.data))


def out_map_row_bound(matrix):
    """xaac_out_map_row_bound -> (what a downmix sum of matrix k can reach, the largest plain sum of a row)"""
    row_sum = ctypes.c_int64(0)
    return int(load_host_library().xaac_out_map_row_bound(int(matrix), ctypes.byref(row_sum))), int(row_sum.value)


class ParseError(RuntimeError):
    def __init__(self, code, frame):
        RuntimeError.__init__(self, "host parser: error %d in frame %d" % (code, frame))
        self.code, self.frame = code, frame


class StreamParser:
    """One ADTS stream through the host front end, frame by frame.  (The reference decodes the first frame twice, once
    while it initialises -- ixheaacd_dec_init, api.c:2097 -- and again as the first output frame; every state is set up
    afresh in between, api.c:2141-2170, but for the seeds of correlated noise bands, which lie in scratch memory: the parser
    starts its noise generator from them (xaac_parse_core_tools_state), so one pass is all that is needed here.)"""

    def __init__(self, data, with_sbr=None, stage=2, esbr=False, drc=None):
        self.lib = load_host_library()
        self.esbr = bool(esbr)     # the reference's default -esbr:1 reading of the SBR payload (xaac_parser_set_esbr)
        self.data = bytes(data)
        self.buf = (ctypes.c_uint8 * len(self.data)).from_buffer_copy(self.data)
        self.h = ctypes.c_void_p()
        if self.lib.xaac_parser_create(ctypes.byref(self.h)):
            raise RuntimeError("xaac_parser_create failed")
        if self.esbr and self.lib.xaac_parser_set_esbr(self.h, 1):
            raise RuntimeError("xaac_parser_set_esbr failed")
        self.drc = drc_config(drc)   # dynamic range control on (xaac_parse_drc_config): drc_side() answers for every frame
        if self.drc is not None and self.lib.xaac_parse_drc_config(self.h, ctypes.byref(self.drc)):
            raise RuntimeError("xaac_parse_drc_config failed")
        self.pos, self.frame_no, self.stage = 0, 0, stage
        self.core, self.side, self.used = CoreFrame(), SbrSide(), ctypes.c_size_t()
        self.esbr_side = [(ctypes.c_uint8 * ESBR_SIDE_BYTES)(), (ctypes.c_uint8 * ESBR_SIDE_BYTES)()]
        hdr = AdtsHeader()
        rc = self.lib.xaac_adts_parse_header(self.buf, len(self.data), ctypes.byref(hdr))
        if rc:
            raise ParseError(rc, 0)
        self.core_rate = hdr.sampling_rate
        self.n_ch, n_elems, sbr, _ = probe_first_frame(self.data)   # a look at frame 0: channels, SBR payload or not
        if n_elems != 1:
            raise ParseError(-3, 0)         # (several channel elements: parse_stream_mc)
        # the SBR tools run for the frames that carry an SBR payload (api.c:3369-3373: a stream at 24 kHz and below gets an SBR
        # decoder object by implicit signalling, api.c:2160, but without payloads it is never called: plain AAC-LC output)
        self.sbr = bool(sbr) if with_sbr is None else bool(with_sbr)

    def close(self):
        if self.h:
            self.lib.xaac_parser_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def next(self):
        """-> False at the end of the stream, True with self.core (and self.side for SBR streams) filled"""
        left = len(self.data) - self.pos
        if left < 7:
            return False
        rc = self.lib.xaac_parse_adts_frame(self.h, ctypes.byref(self.buf, self.pos), left, self.stage, ctypes.byref(self.core),
                                            ctypes.byref(self.used))
        if rc == 1:      # a truncated last frame
            return False
        if rc:
            raise ParseError(rc, self.frame_no)
        self.pos += self.used.value
        if self.sbr:
            rc = self.lib.xaac_parse_sbr_side(self.h, 1, ctypes.byref(self.side))
            if rc:
                raise ParseError(rc, self.frame_no)
            if self.esbr:
                for c in range(self.core.n_ch):
                    if self.lib.xaac_parse_esbr_side(self.h, c, self.esbr_side[c]):
                        raise ParseError(-2, self.frame_no)
        self.frame_no += 1
        return True

    def drc_side(self):
        """the xaac_drc_side rows of the frame next() delivered last: int32[n_ch, DRC_SIDE_WORDS]"""
        side = np.zeros((self.core.n_ch, DRC_SIDE_WORDS), np.int32)
        rc = self.lib.xaac_parse_drc_side(self.h, side.ctypes.data)
        if rc:
            raise ParseError(rc, self.frame_no - 1)
        return side


def parse_stream(data, stage=2, esbr=False):
    """the CPU half alone: [(spec int32[n_ch, 1024], ics int16[n_ch, 4], tools, side or None)] of every frame; esbr: the
    -esbr:1 reading of the SBR payload, and a fifth member [xaac_esbr_side bytes per channel]"""
    p = StreamParser(data, stage=stage, esbr=esbr)
    out = []
    while p.next():
        n = p.core.n_ch
        spec = np.ctypeslib.as_array(p.core.spec)[:n].copy()
        ics = np.ctypeslib.as_array(p.core.ics)[:n].copy()
        side = None
        if p.sbr:
            side = SbrSide()
            ctypes.memmove(ctypes.byref(side), ctypes.byref(p.side), ctypes.sizeof(SbrSide))
        if esbr:
            out.append((spec, ics, int(p.core.tools), side, [bytes(p.esbr_side[c]) for c in range(n)] if p.sbr else None))
        else:
            out.append((spec, ics, int(p.core.tools), side))
    p.close()
    return out


# ADTS channel_config 3 .. 6: (channel elements in bitstream order -- 0 SCE, 1 CPE, 3 LFE --, the output channel of every
# bitstream channel, the WAV channel mask).  The reference gives the first CPE the first two output channels, then the first
# SCE, the LFE, the second CPE, the second SCE (ixheaacd_get_channel_mask, common_lpfuncs.c:107-173; api.c:3176-3177).
MC_LAYOUT = {3: ((0, 1), (2, 0, 1), 0x7), 4: ((0, 1, 0), (2, 0, 1, 3), 0x107), 5: ((0, 1, 1), (2, 0, 1, 3, 4), 0x37),
             6: ((0, 1, 1, 3), (2, 0, 1, 4, 5, 3), 0x3f)}
MC_MAX_ELEMENTS = 4


def probe_first_frame(data):
    """-> (channels, channel elements, frame 0 carries an SBR payload, channel_config of the header) of an ADTS stream, through
    a parser of its own (xaac_parse_adts_frame_mc: streams of one element as well as channel_config 3 .. 6)"""
    lib = load_host_library()
    data = bytes(data)
    hdr = AdtsHeader()
    rc = lib.xaac_adts_parse_header(data[:16], min(16, len(data)), ctypes.byref(hdr))
    if rc:
        raise ParseError(rc, 0)
    elems, n, used, probe = (CoreFrame * MC_MAX_ELEMENTS)(), ctypes.c_int32(), ctypes.c_size_t(), ctypes.c_void_p()
    lib.xaac_parser_create(ctypes.byref(probe))
    rc = lib.xaac_parse_adts_frame_mc(probe, data, len(data), 1, elems, MC_MAX_ELEMENTS, ctypes.byref(n), ctypes.byref(used))
    lib.xaac_parser_destroy(probe)
    if rc:
        raise ParseError(rc, 0)
    return (sum(elems[k].n_ch for k in range(n.value)), n.value, any(elems[k].sbr_bytes > 0 for k in range(n.value)),
            hdr.channel_config)


def parse_stream_mc(data, stage=2):
    """the CPU half alone for a stream of several channel elements (xaac_parse_adts_frame_mc): per frame
    (spec int32[channels, 1024], ics int16[channels, 4], [XAAC_TOOL_* bits per element], [element_id per element],
    [xaac_core_tools_side bytes per element]), channels in bitstream order"""
    lib = load_host_library()
    data = bytes(data)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    p = ctypes.c_void_p()
    if lib.xaac_parser_create(ctypes.byref(p)):
        raise RuntimeError("xaac_parser_create failed")
    elems, n, used = (CoreFrame * MC_MAX_ELEMENTS)(), ctypes.c_int32(), ctypes.c_size_t()
    out, pos = [], 0
    try:
        while len(data) - pos >= 7:
            rc = lib.xaac_parse_adts_frame_mc(p, ctypes.byref(buf, pos), len(data) - pos, stage, elems, MC_MAX_ELEMENTS,
                                              ctypes.byref(n), ctypes.byref(used))
            if rc == 1:
                break
            if rc:
                raise ParseError(rc, len(out))
            pos += used.value
            spec, ics, sides = [], [], []
            for k in range(n.value):
                m = elems[k].n_ch
                spec.append(np.ctypeslib.as_array(elems[k].spec)[:m].copy())
                ics.append(np.ctypeslib.as_array(elems[k].ics)[:m].copy())
                side = (ctypes.c_uint8 * CORE_TOOLS_SIDE_BYTES)()
                if lib.xaac_parse_core_tools_side_mc(p, k, side):
                    raise ParseError(-2, len(out))
                sides.append(bytes(side))
            out.append((np.concatenate(spec), np.concatenate(ics), [int(elems[k].tools) for k in range(n.value)],
                        [int(elems[k].element_id) for k in range(n.value)], sides))
    finally:
        lib.xaac_parser_destroy(p)
    return out


def usable_cores():
    """host cores this process may really use: the scheduler affinity mask cut by the cgroup CPU quota (v2 cpu.max or v1
    cfs_quota_us / cfs_period_us) when there is one"""
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            quota = None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, per = float(f.read()), float(g.read())
                quota = None if q <= 0 else q / per
        except (OSError, ValueError):
            pass
    return aff if quota is None else max(1, min(aff, int(quota + 0.5)))


def gpu_numa_cpus(device_index):
    """CPUs of the NUMA node the GPU hangs off (hipDeviceGetPCIBusId -> /sys/bus/pci/devices/<id>/numa_node -> the node's
    cpulist), cut by what the process may run on; None where that cannot be read (no sysfs, a single node, node -1)"""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        buf = ctypes.create_string_buffer(64)
        if hip.hipDeviceGetPCIBusId(buf, 64, int(device_index)) != 0:
            return None
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % buf.value.decode().lower()).read())
        if node < 0:
            return None
        cpus = []
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            a, _, b = part.partition("-")
            cpus += range(int(a), int(b or a) + 1)
        cpus = sorted(set(cpus) & os.sched_getaffinity(0))
        return cpus or None
    except (OSError, ValueError, AttributeError):
        return None


class _NearGpu:
    """While pinned staging memory is allocated and first touched: the calling thread on the GPU's NUMA node, so that the
    pages land there.  With the staging on the other socket the bus carries one direction at full rate but both at once
    (a step's spectra going up beside the PCM of the step before coming down) at 38 GiB/s in total instead of 63 (measured
    on a two-socket MI355X host with 64 MiB copies)."""

    def __init__(self, device_index):
        self.cpus = gpu_numa_cpus(device_index)

    def __enter__(self):
        self.before = None
        if self.cpus:
            try:
                self.before = os.sched_getaffinity(0)
                os.sched_setaffinity(0, self.cpus)
            except OSError:
                self.before = None
        return self

    def __exit__(self, *exc):
        if self.before is not None:
            os.sched_setaffinity(0, self.before)
        return False


class _TorchCpuThreads:
    """For the length of a decode: torch's intra-op CPU pool no larger than the cores the process is granted.  torch sizes
    the pool by the CPUs the machine lists; in a container that lists 256 and grants 16, one parallel fill of a staging
    array wakes a pool whose threads then spin through the cgroup's CPU quota, and the parser threads behind it are throttled:
    measured 1.1-1.6 x 10^6 frames/s end to end with the default pool, 3.6 x 10^6 with it capped (same box, same run)."""

    def __enter__(self):
        import torch
        self.torch, self.before = torch, torch.get_num_threads()
        cap = usable_cores()
        if self.before > cap:
            torch.set_num_threads(cap)
        return self

    def __exit__(self, *exc):
        if self.torch.get_num_threads() != self.before:
            self.torch.set_num_threads(self.before)
        return False


class BatchParser:
    """N ADTS streams of one kind through the host front end in lock step: xaac_parse_batch_run parses one frame of every
    stream on a team of CPU threads, straight into the (pinned) staging arrays handed to step()."""

    def __init__(self, streams, threads=0, stage=2, esbr=False, mc_sbr=False, drc=None):
        self.lib = load_host_library()
        self.esbr = bool(esbr)
        self.n = n = len(streams)
        self.length = np.array([len(d) for d in streams], np.uint64)
        self.start = np.concatenate([[0], np.cumsum(self.length)[:-1]]).astype(np.uint64)
        self.blob = np.frombuffer(b"".join(bytes(d) for d in streams) + b"\0" * 16, np.uint8).copy()
        self.base = self.blob.ctypes.data
        self.pos = np.zeros(n, np.uint64)
        self._ptrs = (np.uint64(self.base) + self.start).astype(np.uint64)   # every stream's first byte
        self.parsers = (ctypes.c_void_p * n)()
        for i in range(n):
            h = ctypes.c_void_p()
            if self.lib.xaac_parser_create(ctypes.byref(h)):
                raise RuntimeError("xaac_parser_create failed")
            if self.esbr:
                self.lib.xaac_parser_set_esbr(h, 1)
            if drc is not None and self.lib.xaac_parse_drc_config(h, ctypes.byref(drc)):   # (a DrcConfig: drc_config())
                raise RuntimeError("xaac_parse_drc_config failed")
            self.parsers[i] = h
        self.threads, self.stage = int(threads), int(stage)
        self.consumed, self.status = np.zeros(n, np.uint64), np.zeros(n, np.int32)
        self.frames = np.zeros(n, np.int64)
        hdr = AdtsHeader()
        rc = self.lib.xaac_adts_parse_header(bytes(streams[0][:16]), min(16, len(streams[0])), ctypes.byref(hdr))
        if rc:
            raise ParseError(rc, 0)
        self.core_rate, self.n_ch = hdr.sampling_rate, (2 if hdr.channel_config == 2 else 1)
        channels, n_elems, sbr, config = probe_first_frame(streams[0])
        self.sbr = bool(sbr)
        # several channel elements (channel_config 3 .. 6): the multichannel form of the batch call; with SBR payloads only when
        # the caller asked for per-element SBR (mc_sbr: flags int32[n, n_elems, abi.SBR_FLAG_WORDS] and reset_pitch int32[n, n_elems], a row per
        # channel element; header / frame / eside rows per channel in bitstream order)
        self.channel_config, self.n_elems = (config, n_elems) if n_elems > 1 else (0, 1)
        for d in streams[1:]:   # a multichannel stream only beside streams of its own channel_config, whichever comes first
            other = (((d[2] & 1) << 2) | (d[3] >> 6)) if len(d) >= 4 else -1
            if other != config and (3 <= other <= 6 or 3 <= config <= 6):
                raise ValueError("streams of different channel configurations in one batch")
        if self.channel_config:
            if self.sbr and not mc_sbr:
                raise ValueError("multichannel SBR (an SBR payload in a stream of more than two channels) is not supported")
            self.n_ch = channels
        self.mc_sbr = bool(mc_sbr) and bool(self.channel_config) and self.sbr
        self.reset_pitch = np.zeros(n * (self.n_elems if self.mc_sbr else 1), np.int32)   # at frames with a reset flag: xaac_parse_reset_pitch

    def close(self):
        if getattr(self, "_in_flight", False):   # (a caller that gave up between start_step() and wait_step(): the team must get its batch back)
            self.lib.xaac_parse_batch_wait(None)
            self._in_flight = False
        for i in range(self.n):
            if self.parsers[i]:
                self.lib.xaac_parser_destroy(self.parsers[i])
                self.parsers[i] = None

    def tools_states(self):
        """uint8[n_elems, n, CORE_TOOLS_STATE_BYTES], element-major like the tools' side rows: what every stream's noise generators
        start from (xaac_parse_core_tools_state_mc), for the caller of a stage-1 parse, once the first step has been parsed.  A
        stream that delivered no frame keeps zeros"""
        out = np.zeros((self.n_elems, self.n, CORE_TOOLS_STATE_BYTES), np.uint8)
        for i in range(self.n):
            for k in range(self.n_elems):
                self.lib.xaac_parse_core_tools_state_mc(self.parsers[i], k, out[k, i].ctypes.data)
        return out

    def _descriptor(self, spec, ics, hdr, frm, psf, flags, with_sbr, eside=None, status=None, reset_pitch=None, frames=1, lines=None,
                    tools_side=None, drc_side=None):
        # data / bytes are the whole streams and stay as they are; the library moves self.pos (xaac_parse_batch::pos), so a
        # call costs this thread the filling of the descriptor and nothing per stream
        b = _ParseBatch()
        b.n_streams, b.n_ch, b.with_sbr, b.ps_enable, b.stage, b.threads = self.n, self.n_ch, int(with_sbr), 1, self.stage, self.threads
        b.parser, b.data, b.bytes = ctypes.addressof(self.parsers), self._ptrs.ctypes.data, self.length.ctypes.data
        ptr = lambda t: None if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data)
        b.spec, b.ics, b.header, b.frame, b.ps_frame, b.flags = ptr(spec), ptr(ics), ptr(hdr), ptr(frm), ptr(psf), ptr(flags)
        b.tools, b.consumed = None, self.consumed.ctypes.data   # (which tools a frame used: nobody downstream asks)
        b.status = (self.status if status is None else status).ctypes.data
        b.esbr_side = ptr(eside)
        b.reset_pitch = (self.reset_pitch if reset_pitch is None else reset_pitch).ctypes.data
        b.pos = self.pos.ctypes.data
        b.frames = int(frames)
        b.lines = None if lines is None else lines.ctypes.data
        b.tools_side = ptr(tools_side)   # uint8[frames, n, CORE_TOOLS_SIDE_BYTES]: the tools' side info of a stage-1 parse
        b.channel_config = self.channel_config   # (with it: tools_side is uint8[frames, n_elems, n, ...], element-major)
        b.mc_sbr = int(self.mc_sbr)
        b.drc_side = ptr(drc_side)       # int32[frames, n * n_ch, DRC_SIDE_WORDS]: a row beside every row of spec
        return b

    def _advance(self, ok, status=None):
        """one step's status words -> bool[n] (which streams delivered a frame); ok: the library call's return value, or None"""
        if ok is not None and ok < 0:
            raise RuntimeError("xaac_parse_batch: %d" % ok)
        status = self.status if status is None else status
        good = status == 0
        self.frames += good
        if not good.all():
            bad = ~good & (status != 1)
            if np.any(bad):
                i = int(np.nonzero(bad)[0][0])
                raise ParseError(int(status[i]), int(self.frames[i]))
        return good

    def step(self, spec, ics, hdr=None, frm=None, psf=None, flags=None, eside=None, tools_side=None, drc_side=None):
        """parses the next frame of every stream into the staging arrays; -> bool[n]: which streams delivered a frame
        (the others are at their end: their rows are left as they were)"""
        b = self._descriptor(spec, ics, hdr, frm, psf, flags, self.sbr, eside, tools_side=tools_side, drc_side=drc_side)
        return self._advance(self.lib.xaac_parse_batch_run_sized(ctypes.byref(b), ctypes.sizeof(b)))

    def start_step(self, spec, ics, hdr=None, frm=None, psf=None, flags=None, eside=None, status=None, reset_pitch=None, frames=1,
                   lines=None, tools_side=None, drc_side=None):
        """step() in two halves (xaac_parse_batch_start / _wait): the library's worker team parses while the caller does
        something else; the staging arrays are the team's until wait_step() returns.  status / reset_pitch: the caller's own
        int32[n] arrays for this step's results (a caller that starts the next step before it has looked at this one's).
        frames = T > 1: up to T consecutive frames of every stream in one call (xaac_parse_batch::frames), every array with
        a leading dimension T (status / reset_pitch int32[T, n]); finish_step is then called per step t with status[t].
        lines: int32[T, n] out, xaac_parse_batch::lines."""
        self._status_in_flight = status
        b = self._descriptor(spec, ics, hdr, frm, psf, flags, self.sbr, eside, status, reset_pitch, frames, lines, tools_side, drc_side)
        rc = self.lib.xaac_parse_batch_start_sized(ctypes.byref(b), ctypes.sizeof(b))
        if rc:
            raise RuntimeError("xaac_parse_batch_start: %d" % rc)
        self._in_flight = True

    def wait_step(self, check=True):
        """-> (bool[n] as step(), seconds the team parsed); check False: (parsed-ok count, seconds) -- the caller looks at its
        status array itself (finish_step) after it has started the next step"""
        busy = ctypes.c_double(0.0)
        ok = self.lib.xaac_parse_batch_wait(ctypes.byref(busy))
        self._in_flight = False
        if not check:
            return ok, busy.value
        return self._advance(ok, self._status_in_flight), busy.value

    def finish_step(self, ok, status):
        """what wait_step(check=True) does behind the library call, for a step waited for with check=False (ok: the call's
        return value, or None for one step of a call over several frames: the status words decide)"""
        return self._advance(ok, status)


def _struct_bytes(fn, size):
    raw = (ctypes.c_uint8 * size)()
    fn(raw)
    return np.frombuffer(raw, np.uint8).copy()


_hip = None


def _hip_runtime():
    """the HIP runtime itself, for the one copy torch has no call for: hipMemcpy2DAsync (the leading columns of a matrix)"""
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return _hip


# what the pipeline and the chains see of one step of a staging set: which streams delivered a frame, and that step's rows
_Step = collections.namedtuple("_Step", "sent got spec ics hdr frm psf eside flags flags_pin tside reset_pitch lines dside")


class _Alloc:
    """zeroed device tensors (dz) and zeroed pinned host tensors (pinned) of one decode"""

    def __init__(self, dev):
        self.dev, self.near_gpu = dev, _NearGpu(dev.index or 0)

    def dz(self, *shape, dtype=None):
        return torch.zeros(*shape, dtype=dtype or torch.uint8, device=self.dev)

    def pinned(self, *shape, dtype=None):
        with self.near_gpu:    # allocated and first touched on the GPU's NUMA node
            t = torch.empty(*shape, dtype=dtype or torch.uint8, pin_memory=True)
            t.numpy().fill(0)  # (numpy: one thread; torch.zeros would wake the whole intra-op pool for it)
        return t


class Staging:
    """what one parser call leaves for the GPU: pinned host arrays of T steps (one frame of every stream each).  arrays: the
    side info the chain wants beside the spectra and window info (of "hdr", "frm", "psf", "flags", "eside"); tools: the spectral
    tools' side rows too"""

    def __init__(self, bp, pinned, T, arrays=(), tools=False, drc=False):
        n, nc = bp.n, bp.n * bp.n_ch
        want = lambda name, *shape: pinned(T, *shape) if name in arrays else None
        self.bp, self.T = bp, T
        self.spec, self.ics = pinned(T, nc, 1024, dtype=torch.int32), pinned(T, nc, 2)
        self.tside = pinned(T, n * bp.n_elems, CORE_TOOLS_SIDE_BYTES) if tools else None   # element-major within a step
        self.dside = pinned(T, nc, DRC_SIDE_WORDS, dtype=torch.int32) if drc else None      # a row per channel, beside the spectra
        self.hdr, self.frm = want("hdr", nc, SBR_HEADER_BYTES), want("frm", nc, SBR_FRAME_BYTES)
        self.psf, self.eside = want("psf", n, PS_FRAME_BYTES), want("eside", nc, ESBR_SIDE_BYTES)
        self.flags = self.flags_pin = None
        if "flags" in arrays:
            self.flags = np.zeros((T, n, bp.n_elems, abi.SBR_FLAG_WORDS) if bp.mc_sbr else (T, n, abi.SBR_FLAG_WORDS), np.int32)   # (mc_sbr: a row per channel element)
            self.flags_pin = pinned(T, n, abi.SBR_FLAG_WORDS, dtype=torch.int32)   # the rows as they go up for xaac_sbr_state_apply_side_batch
        self.seconds = 0.0
        self.sent = [torch.cuda.Event() for _ in range(T)]   # step t's copies up are over (sent[T - 1]: the parser may write the set again)
        self.sent_once = False
        self.status = np.zeros((T, n), np.int32)   # this set's own
        self.reset_pitch = np.zeros((T, n, bp.n_elems) if bp.mc_sbr else (T, n), np.int32)
        self.lines = np.zeros((T, n), np.int32)   # leading spectral lines that may be non-zero, per step and stream
        self.steps = None

    def begin(self):    # the library's team parses into this set while the caller queues the steps before on the GPU
        if self.sent_once:
            self.sent[self.T - 1].synchronize()   # (the set's last copies up: long over when its turn comes again)
        self.bp.start_step(self.spec, self.ics, self.hdr, self.frm, self.psf, self.flags, self.eside, status=self.status,
                           reset_pitch=self.reset_pitch, frames=self.T, lines=self.lines, tools_side=self.tside,
                           drc_side=self.dside)
        return self

    def end(self):      # back from the team; the results are looked at in finish(), once the next set is on its way
        self.ok, self.seconds = self.bp.wait_step(check=False)
        return self

    def finish(self):
        rows = (self.spec, self.ics, self.hdr, self.frm, self.psf, self.eside, self.flags, self.flags_pin, self.tside,
                self.reset_pitch, self.lines, self.dside)
        self.steps = [_Step(self.sent[t], self.bp.finish_step(None, self.status[t]), *(a if a is None else a[t] for a in rows))
                      for t in range(self.T)]
        return self


class _ToolsStage:
    """gpu_tools: the M/S, intensity, PNS and TNS tools in front of whichever chain's IMDCT -- the tools' side rows (two device
    sets like the spectra), the noise generators, the kernel's status words: a row per stream and channel element, element-major.
    first_rows: the row of every element's first channel among a stream's n_ch rows on the device"""

    def __init__(self, ctx, n, dz, pinned, n_ch, first_rows=(0,)):
        self.ctx, self.n, self.n_ch, self.first_rows = ctx, n, n_ch, tuple(first_rows)
        rows = n * len(self.first_rows)
        self.side_d2 = [dz(rows, CORE_TOOLS_SIDE_BYTES) for _ in range(2)]
        self.state = dz(rows, CORE_TOOLS_STATE_BYTES)
        self.status2 = [dz(rows, dtype=torch.int32) for _ in range(2)]
        self.status_h2 = [pinned(rows, dtype=torch.int32) for _ in range(2)]

    def begin(self, bp):   # behind the first parsed step, in front of the first run: the streams' generators as they start
        self.state.copy_(torch.from_numpy(bp.tools_states().reshape(self.state.shape)))

    def send_up(self, step, slot):
        self.side_d2[slot].copy_(step.tside, non_blocking=True)

    def run(self, spec_d, slot):   # stage-1 spectra -> the spectra the IMDCT takes, in place (ended streams' rows run idle, unlooked at)
        n = self.n
        for k, row in enumerate(self.first_rows):   # one launch per element index over all streams
            rows = slice(k * n, (k + 1) * n)
            self.ctx.aac_tools_process_batch(spec_d, self.side_d2[slot][rows], self.state[rows], self.status2[slot][rows],
                                             spec_stride=1024 * self.n_ch, first_row=row)

    def refused(self, slot, got):   # a delivered frame's element the kernel did not take
        return int(self.status_h2[slot].numpy().reshape(len(self.first_rows), self.n)[:, got].min(initial=0)) < 0


class _DrcStage:
    """drc: dynamic range control on the spectra in front of the AAC-LC chain's IMDCT (behind the spectral tools where they run on
    the GPU) -- the side rows the parser made beside the spectra, in two device sets like them"""

    def __init__(self, ctx, nc, dz):
        self.ctx = ctx
        self.side_d2 = [dz(nc, DRC_SIDE_WORDS, dtype=torch.int32) for _ in range(2)]

    def send_up(self, step, slot):
        self.side_d2[slot].copy_(step.dside, non_blocking=True)

    def run(self, spec_d, slot):   # in place (ended streams' rows run idle on the rows their last frame left)
        self.ctx.drc_apply_batch(spec_d, self.side_d2[slot])


class _Chain:
    """What _Pipeline knows of a decode chain: host_arrays (the side info a staging set must carry for it), pcm2 / pcm_h2 and
    status2 / status_h2 (two sets on the device and in pinned memory; the status sets or None), out_ch / out_rate, and
    send_up(step, slot, got) -- inside the `up` stream: the chain's own side info into device set `slot`;
    run(step, slot, got, first, spec_d, ics_d) -- on the main stream: the chain's kernels -> (PCM block shape, samples to cut
    from the front of the block, drop the block);
    finish(out, keep_pcm) -- behind the last step.
    A chain owns the device-resident state of its streams and every buffer its kernels use: allocate(dz, pinned) makes them."""
    host_arrays = ()
    status2 = status_h2 = None

    def __init__(self, ctx, lib, dev, n, n_ch, rate, alloc, trace=None, out_map=None, limiter=True):
        self.ctx, self.lib, self.dev, self.dz, self.trace = ctx, lib, dev, alloc.dz, trace
        self.out_map, self.limiter = out_map, limiter   # what the PCM hand-off does to a sample's channels (an OutMap); AAC-LC: limiter on
        self.n, self.n_ch, self.nc, self.rate = n, n_ch, n * n_ch, rate
        self.ovl, self.ovl_state = alloc.dz(self.nc, 512, dtype=torch.int32), alloc.dz(self.nc, 2)   # the IMDCT's overlap halves, window state
        self.allocate(alloc.dz, alloc.pinned)

    def _states(self, init, size, rows):   # `rows` structs as the host library initialises them, on the device
        return torch.from_numpy(np.tile(_struct_bytes(init, size), (rows, 1)).copy()).to(self.dev)

    def send_up(self, step, slot, got):
        pass

    def finish(self, out, keep_pcm):
        pass


class _LcChain(_Chain):
    """AAC-LC: IMDCT -> WORD32 + qshift_adj -> peak limiter -> round16 (api.c:3662-3692), then the limiter's delay line
    behind each stream"""

    def allocate(self, dz, pinned):
        ctx, dev, n, n_ch, rate = self.ctx, self.dev, self.n, self.n_ch, self.rate
        self.out_ch, self.out_rate = n_ch, rate     # as coded
        if self.out_map is not None:                # ... or what the map leaves: only that block exists on the device and comes down
            self.out_ch = out_map_channels(self.out_map, n_ch)
        out_ch = self.out_ch
        self.out32, self.qadj = dz(n * 1024 * n_ch, dtype=torch.int32), dz(n * n_ch, dtype=torch.int8)
        lim0, self.delay = peak_limiter_init(n_ch, rate)
        self.lim = torch.from_numpy(np.tile(np.frombuffer(bytes(lim0), np.uint8), (n, 1)).copy()).to(dev)
        self.lim_at_end, self.lim_taken = {}, np.zeros(n, bool)
        self.ws = dz(max(ctx.peak_limiter_workspace_bytes(n), 16))
        self.pcm2 = [dz(n * 1024 * out_ch, dtype=torch.int16) for _ in range(2)]
        self.pcm_h2 = [pinned(n * 1024 * out_ch, dtype=torch.int16) for _ in range(2)]

    def run(self, step, slot, got, first, spec_d, ics_d):
        shape, cut = (self.n, 1024, self.out_ch), (self.delay if first else 0)   # the limiter's delay is cut from the first frame
        planar = self.n_ch > 2
        if not self.limiter:    # ixheaacd_scale_adjust + round16 in the limiter's place: the IMDCT's own hand-off, or -- with a map, or
            # more than two channels -- the kernel behind it in which a sample's channels meet in one lane
            if self.out_map is None and not planar:
                self.ctx.imdct_process_batch(spec_d, ics_d, self.ovl, self.ovl_state, pcm16=self.pcm2[slot], ch_fac=self.n_ch)
            else:
                self.ctx.imdct_process_batch(spec_d, ics_d, self.ovl, self.ovl_state, out32=self.out32, qshift_adj=self.qadj,
                                             ch_fac=1 if planar else self.n_ch)
                self.ctx.pcm16_scale_adjust_map_batch(self.out32, self.qadj, self.n_ch, self.pcm2[slot], self.out_map, planar=planar)
            return shape, cut, False
        # a stream that ended with the step before: its limiter state as its last frame left it (the rows of ended
        # streams go on running idle through the kernels; the delay line flushed behind a stream is the one it ended on)
        for i in np.nonzero(~got & ~self.lim_taken)[0]:
            self.lim_at_end[int(i)] = self.lim[int(i)].cpu().numpy()     # (waits for the kernels of the step before)
            self.lim_taken[i] = True
        # more than two channels: a row per channel (the pipeline sent them up in output channel order), the limiter reads them planar
        self.ctx.imdct_process_batch(spec_d, ics_d, self.ovl, self.ovl_state, out32=self.out32, qshift_adj=self.qadj,
                                     ch_fac=1 if planar else self.n_ch)
        if self.out_map is not None:    # the map is the limiter's epilogue
            self.ctx.peak_limiter_process_map_batch(self.out32, self.qadj, self.lim, self.n_ch, self.ws, self.pcm2[slot], self.out_map,
                                                    planar=planar)
        else:
            self.ctx.peak_limiter_process_batch(self.out32, self.qadj, self.lim, self.n_ch, self.ws, pcm16=self.pcm2[slot], planar=planar)
        return shape, cut, False

    def finish(self, out, keep_pcm):
        if not keep_pcm:
            return
        # the limiter's delay line holds the last attack_time_samples samples: api.c:2824-2866
        self.ctx.sync()
        lim_h, n_ch = self.lim.cpu().numpy(), self.n_ch
        for i in range(self.n):
            if not self.limiter:    # the reference flushes the delay line all the same, and nothing ever went into it
                out[i].append(np.zeros((self.delay, self.out_ch), np.int16))
                continue
            st = LimiterState.from_buffer_copy((self.lim_at_end[i] if i in self.lim_at_end else lim_h[i]).tobytes())
            att, idx = st.attack_time_samples, st.delayed_input_index
            d = np.ctypeslib.as_array(st.delayed_input)[:att * n_ch].reshape(att, n_ch)
            tail = np.concatenate([d[idx:], d[:idx]]).astype(np.float64)
            inside = (tail > -2147483649.0) & (tail < 2147483648.0)      # (WORD32) of a float as x86 converts it: what does
            v = np.where(inside, np.trunc(np.where(inside, tail, 0.0)), -2147483648.0).astype(np.int64)   # not fit is INT_MIN
            v = np.clip(v + 0x8000, -(1 << 31), (1 << 31) - 1) >> 16   # round16
            out[i].append(out_map_apply_host(self.out_map, v.astype(np.int16)))   # the flushed samples take the map the frames took


class _SbrBase(_Chain):
    """what both SBR chains hold: the core's 16-bit PCM, two device sets of header / frame (and PS frame) rows, status words,
    stereo PCM at twice the core's rate (PS, or the mono column twice)"""

    def allocate(self, dz, pinned):
        n, nc = self.n, self.nc
        self.out_ch, self.out_rate = 2, 2 * self.rate
        self.host_arrays = ("hdr", "frm", "flags") + (("psf",) if self.n_ch == 1 else ())
        self.core16 = dz(nc * 1024, dtype=torch.int16)
        self.hdr_d2, self.frm_d2 = [dz(nc, SBR_HEADER_BYTES) for _ in range(2)], [dz(nc, SBR_FRAME_BYTES) for _ in range(2)]
        self.psf_d2 = [dz(n, PS_FRAME_BYTES) for _ in range(2)] if self.n_ch == 1 else None
        self.status2 = [dz(nc, dtype=torch.int32) for _ in range(2)]
        self.status_h2 = [pinned(nc, dtype=torch.int32) for _ in range(2)]
        self.pcm2 = [dz(n * 2048 * 2, dtype=torch.int16) for _ in range(2)]
        self.pcm_h2 = [pinned(n * 2048 * 2, dtype=torch.int16) for _ in range(2)]
        self.ps_state = None

    def send_up(self, step, slot, got, eside_d=None):
        self.hdr_d2[slot].copy_(step.hdr, non_blocking=True)
        self.frm_d2[slot].copy_(step.frm, non_blocking=True)
        if eside_d is not None:
            eside_d.copy_(step.eside, non_blocking=True)
        if self.n_ch == 1 and (step.flags[got, F_PS] != 0).any():   # the PS frames, when a delivered frame has one
            self.psf_d2[slot].copy_(step.psf, non_blocking=True)


class _SbrChain(_SbrBase):
    """The fixed-point SBR tools (-esbr:0) behind the IMDCT's 16-bit PCM: low power for a channel pair; HQ for mono streams,
    with parametric stereo where the frames carry it, else the mono column twice"""

    def allocate(self, dz, pinned):
        _SbrBase.allocate(self, dz, pinned)
        ctx, lib, n, n_ch = self.ctx, self.lib, self.n, self.n_ch
        self.state = self._states(lib.xaac_sbr_state_init, SBR_STATE_BYTES, self.nc)
        self.flags_d2 = [dz(n, abi.SBR_FLAG_WORDS, dtype=torch.int32) for _ in range(2)]
        self.side_words = False
        if n_ch == 2:
            self.ws = dz(ctx.sbr_lp_workspace_bytes(self.nc))
        else:
            self.ps_state = self._states(lib.xaac_ps_state_init, PS_STATE_BYTES, n)
            self.ws = dz(ctx.sbr_hq_workspace_bytes(n, True))
            self.pcm_mono = dz(n * 2048, dtype=torch.int16)

    def send_up(self, step, slot, got):
        _SbrBase.send_up(self, step, slot, got)
        # frames that reset the SBR decoder or fall back to plain up-sampling change a few words of the resident state: on the
        # device, from xaac_sbr_state_apply_side_batch's flag rows (streams without a frame: zero rows)
        flags = step.flags
        self.side_words = bool((got & ((flags[:, F_RESET] != 0) | (flags[:, F_UPSAMPLING] != 0))).any())
        if self.side_words:
            step.flags_pin.numpy()[:] = flags * got[:, None].astype(np.int32)
            self.flags_d2[slot].copy_(step.flags_pin, non_blocking=True)

    def run(self, step, slot, got, first, spec_d, ics_d):
        ctx, n, n_ch, flags, state = self.ctx, self.n, self.n_ch, step.flags, self.state
        hdr_d, frm_d, pcm, status = self.hdr_d2[slot], self.frm_d2[slot], self.pcm2[slot], self.status2[slot]
        ctx.imdct_process_batch(spec_d, ics_d, self.ovl, self.ovl_state, pcm16=self.core16, ch_fac=n_ch, pcm_mode=PCM_SBR)
        if self.side_words:
            ctx.sbr_state_apply_side_batch(hdr_d, self.flags_d2[slot], state, n_ch, ps_state=self.ps_state)
        if n_ch == 2:
            ctx.sbr_lp_process_batch(self.core16, hdr_d, frm_d, state, pcm, self.ws, status=status, in_ch_fac=2, out_ch_fac=2)
        else:
            with_ps = flags[got, F_PS] != 0
            if with_ps.any():
                starts = np.nonzero(got & (flags[:, F_PS_START] != 0))[0]
                if starts.size:
                    idx = torch.from_numpy(starts.astype(np.int32)).to(self.dev)
                    ctx.sbr_state_handover(HANDOVER_PS_START, idx, idx, state, self.ps_state)
                ctx.sbr_hq_process_batch(self.core16, hdr_d, frm_d, state, pcm, self.ws, ps_frame=self.psf_d2[slot],
                                         ps_state=self.ps_state, status=status)
                if not with_ps.all():
                    # streams with and without parametric stereo in one step (HE-AAC beside HE-AACv2 mono streams): the PS launch
                    # passes a stream without PS through as the mono frame it is and leaves its right samples alone (as the
                    # native decoder runs such a step, host/xaacdec_amd.cpp: SbrChain::run_hq_ps): the left ones go there too
                    rows = torch.from_numpy(np.nonzero(got & (flags[:, F_PS] == 0))[0]).to(self.dev)
                    both = pcm.view(n, 2048, 2)
                    both[rows, :, 1] = both[rows, :, 0]
            else:
                ctx.sbr_hq_process_batch(self.core16, hdr_d, frm_d, state, self.pcm_mono, self.ws, status=status)
                # mono duplicated to stereo (api.c:3639-3660)
                pcm.view(n, 2048, 2).copy_(self.pcm_mono.view(n, 2048, 1).expand(n, 2048, 2))
        return (n, 2048, 2), 0, False


# float offsets of members of struct xaac_esbr_state, from its mirror (tests/test_parser_esbr.py pins the values): qmf_re / qmf_im
# rows, and the transposer's last rows ph_re / ph_im
_ES_QMF_RE, _ES_QMF_IM, _ES_PH_RE, _ES_PH_IM = (getattr(abi.EsbrState, m).offset // 4 for m in ("qmf_re", "qmf_im", "ph_re", "ph_im"))
# struct xaac_hbe_state: the floats of its two delay lines (synth_buf and analy_buf, neighbours), and where its integers begin
_HBE_DELAY_LINES = slice(abi.HbeState.synth_buf.offset // 4, (abi.HbeState.analy_buf.offset + abi.HbeState.analy_buf.size) // 4)
_HBE_TAIL_AT = abi.HbeState.synth_size.offset


class _EsbrChain(_SbrBase):
    """Path A (-esbr:1): IMDCT (16-bit core PCM) -> xaac_esbr_core_from_pcm16_batch -> the eSBR chain -> xaac_esbr_pcm16_from_float_batch
    (saturate / truncate to 16 bit: ixheaacd_samples_sat, decode_main.c:82-107); every state member stays on the device"""

    def allocate(self, dz, pinned):
        _SbrBase.allocate(self, dz, pinned)
        ctx, lib, n, n_ch, nc = self.ctx, self.lib, self.n, self.n_ch, self.nc
        self.host_arrays += ("eside",)
        self.state = self._states(lib.xaac_esbr_state_init, ESBR_STATE_BYTES, nc)
        self.hbe = dz(nc, HBE_STATE_BYTES)
        self.eside_d2 = [dz(nc, ESBR_SIDE_BYTES) for _ in range(2)]
        self.ws = dz(ctx.esbr_workspace_bytes(nc))
        self.out_l, self.out_r = dz(nc, 2048, dtype=torch.float32), None
        self.core = dz(nc, 1024, dtype=torch.float32)
        if n_ch == 1:
            self.ps_state = self._states(lib.xaac_esbr_ps_state_init, ESBR_PS_STATE_BYTES, n)
            self.out_r = dz(n, 2048, dtype=torch.float32)
            self.plain = (self.out_l, 2048)              # without PS: mono twice (api.c:3639-3660)
        else:
            self.plain = (self.out_l[1:], 4096)          # a pair's channels are neighbouring rows
        self.older = dz(nc, 2, 24 * 64, dtype=torch.float32)   # rows 8..31 of the QMF history as the frame before found them
        # the transposers' integers (struct xaac_hbe_state from synth_size on)
        self.hbe_tail = np.zeros((nc, HBE_STATE_BYTES - _HBE_TAIL_AT), np.uint8)

    def hbe_hint(self):   # the largest transposer bank of the batch, as the ABI's LDS hint takes it (8, or 0 = any)
        return 8 if int(self.hbe_tail.view(np.int32)[:, 0].max()) <= 8 else 0

    def send_up(self, step, slot, got):
        _SbrBase.send_up(self, step, slot, got, self.eside_d2[slot])

    def reset_transposers(self, step, touched):
        """ixheaacd_sbr_dec_reset for Path A (sbrdecoder.c:175-236) on the streams `touched`: new transposer parameters from the
        header's band tables (its two delay lines cleared), then two transposer runs over rows 8..39 and 40..71 of the QMF buffer
        as the frame before left it: rows 8..31 are what that frame found as rows 8..31 of its history (`older`), rows 32..71 are
        the state's history (the codec bank's num_time_slots is 32 here).  The second run's last eight output rows become the
        state's ph rows (bands outside the transposer's range keep what they held)."""
        n_ch = self.n_ch
        rows_h = (touched[:, None] * n_ch + np.arange(n_ch)[None, :]).ravel()
        self.reset_rows(step, rows_h, np.repeat(step.reset_pitch[touched], n_ch))

    def reset_rows(self, step, rows_h, pitch_h):
        """... on the channel rows rows_h, with the pitch every row's reset hands its transposer runs"""
        ctx, dev, n_ch, dz = self.ctx, self.dev, self.n_ch, self.dz
        k = len(rows_h)
        rows = torch.from_numpy(rows_h).to(dev)
        hb = self.hbe.index_select(0, rows)
        tails = np.ascontiguousarray(self.hbe_tail[rows_h])            # (one call for all of them: every stream's first
        heads = np.ascontiguousarray(step.hdr.numpy()[rows_h])         #  frame is a reset frame)
        bad = self.lib.xaac_hbe_state_reinit_tails(tails.ctypes.data, heads.ctypes.data, len(rows_h))
        if bad >= 0:
            raise RuntimeError("the QMF transposer refused the SBR band tables of stream %d" % (rows_h[bad] // n_ch))
        self.hbe_tail[rows_h] = tails
        hb[:, _HBE_TAIL_AT:] = torch.from_numpy(tails).to(dev)
        hb32 = hb.view(torch.float32)
        hb32[:, _HBE_DELAY_LINES] = 0.0                # synth_buf, analy_buf
        pitch = torch.from_numpy(np.ascontiguousarray(pitch_h, np.int32)).to(dev)
        st32 = self.state.view(torch.float32)
        hist, old = st32.index_select(0, rows), self.older.index_select(0, rows)
        q_re, q_im = dz(k, 32, 64, dtype=torch.float32), dz(k, 32, 64, dtype=torch.float32)
        pv_re, pv_im = dz(k, 32, 64, dtype=torch.float32), dz(k, 32, 64, dtype=torch.float32)
        rst = dz(k, dtype=torch.int32)
        q_re[:, :24] = old[:, 0].view(k, 24, 64)
        q_im[:, :24] = old[:, 1].view(k, 24, 64)
        q_re[:, 24:] = hist[:, _ES_QMF_RE:_ES_QMF_RE + 8 * 64].view(k, 8, 64)
        q_im[:, 24:] = hist[:, _ES_QMF_IM:_ES_QMF_IM + 8 * 64].view(k, 8, 64)
        ctx.hbe_apply_batch(q_re, q_im, hb, pv_re, pv_im, status=rst, pitch_in_bins=pitch, max_synth_size=self.hbe_hint())
        q_re[:] = hist[:, _ES_QMF_RE + 8 * 64:_ES_QMF_RE + 40 * 64].view(k, 32, 64)
        q_im[:] = hist[:, _ES_QMF_IM + 8 * 64:_ES_QMF_IM + 40 * 64].view(k, 32, 64)
        pv_re[:, 24:] = hist[:, _ES_PH_RE:_ES_PH_RE + 512].view(k, 8, 64)
        pv_im[:, 24:] = hist[:, _ES_PH_IM:_ES_PH_IM + 512].view(k, 8, 64)
        ctx.hbe_apply_batch(q_re, q_im, hb, pv_re, pv_im, status=rst, pitch_in_bins=pitch, max_synth_size=self.hbe_hint())
        hist[:, _ES_PH_RE:_ES_PH_RE + 512] = pv_re[:, 24:].reshape(k, 512)
        hist[:, _ES_PH_IM:_ES_PH_IM + 512] = pv_im[:, 24:].reshape(k, 512)
        st32.index_copy_(0, rows, hist)
        self.hbe.index_copy_(0, rows, hb)

    def keep_older(self):
        """rows 8..31 of the QMF history as this frame finds them: for the reset a later frame may bring"""
        st32 = self.state.view(torch.float32)
        self.older[:, 0] = st32[:, _ES_QMF_RE + 8 * 64:_ES_QMF_RE + 32 * 64]
        self.older[:, 1] = st32[:, _ES_QMF_IM + 8 * 64:_ES_QMF_IM + 32 * 64]

    def run(self, step, slot, got, first, spec_d, ics_d):
        ctx, n_ch, flags, state, out_l = self.ctx, self.n_ch, step.flags, self.state, self.out_l
        hdr_d, frm_d, eside_d = self.hdr_d2[slot], self.frm_d2[slot], self.eside_d2[slot]
        # (interleaved as the reference holds it: its in-place 32 -> 16 bit conversion of a pair leaves traces of channel
        # 0 in channel 1, api.c:353-366, which the IMDCT's PCM_SBR hand-off restates for ch_fac 2)
        ctx.imdct_process_batch(spec_d, ics_d, self.ovl, self.ovl_state, pcm16=self.core16, ch_fac=n_ch, pcm_mode=PCM_SBR)
        touched = np.nonzero(got & (flags[:, F_RESET] != 0))[0]
        if touched.size:
            self.reset_transposers(step, touched)
        self.keep_older()
        ctx.esbr_core_from_pcm16(self.core16, self.core, ch_fac=n_ch)
        if self.trace is not None:   # debugging: the device states in front of the chain call
            self.trace(dict(state=state, hbe=self.hbe, ps_state=self.ps_state, core=self.core, side=eside_d, header=hdr_d, frame=frm_d))
        with_ps = (flags[got, F_PS] != 0) if n_ch == 1 else np.zeros(1, bool)
        ps = with_ps.any()      # float parametric stereo: the chain writes both channels
        psf_d, ps_state, out_r = (self.psf_d2[slot], self.ps_state, self.out_r) if ps else (None, None, None)
        right, stride = (out_r, 2048) if ps else self.plain
        ctx.esbr_sbr_process_batch(self.core, hdr_d, frm_d, eside_d, state, out_l, self.ws, status=self.status2[slot], ps_frame=psf_d,
                                   ps_state=ps_state, out_r=out_r, hbe_state=self.hbe, hbe_max_synth_size=self.hbe_hint())
        if ps and not with_ps.all():
            # streams without PS in a PS step: the float PS launch skips them and leaves their rows of out_r alone
            # (esbr_ps_kernel.hip); they are mono frames, the left channel twice (EsbrChain::run of the native decoder)
            rows = torch.from_numpy(np.nonzero(got & (flags[:, F_PS] == 0))[0]).to(self.dev)
            out_r[rows] = out_l[rows]
        ctx.esbr_pcm16_from_float(out_l, right, self.pcm2[slot], stride=stride)
        return (self.n, 2048, 2), 0, first      # the first frame's output is not written in this mode


class _McEsbrChain(_EsbrChain):
    """Path A for streams of more than two channels (channel_config 3 .. 6): one SBR decoder per channel element as the reference
    keeps them, which here is every channel a row of its own -- in bitstream order -- through the same batch entry points.  The
    IMDCT leaves WORD32 rows (ch_fac 1); xaac_mc_core_from_out32_batch makes the in-place 16-bit conversion of every element in the
    frame's block; xaac_mc_pcm16_from_float_batch puts the planes into the block in output channel order (ixheaacd_samples_sat_mc;
    no limiter: api.c:3381).  No parametric stereo in such a frame.  Flags and reset pitch come per channel element."""

    def allocate(self, dz, pinned):
        _EsbrChain.allocate(self, dz, pinned)
        n, n_ch = self.n, self.n_ch
        elements, self.route, _ = MC_LAYOUT[n_ch]
        self.el_of_ch = np.repeat(np.arange(len(elements)), [2 if e == 1 else 1 for e in elements])
        self.out_ch = out_ch = 2 if self.out_map is not None else n_ch   # (the downmix to stereo on the way out)
        self.out32, self.qadj = dz(self.nc, 1024, dtype=torch.int32), dz(self.nc, dtype=torch.int8)
        self.pcm2 = [dz(n * 2048 * out_ch, dtype=torch.int16) for _ in range(2)]
        self.pcm_h2 = [pinned(n * 2048 * out_ch, dtype=torch.int16) for _ in range(2)]

    def send_up(self, step, slot, got):
        self.hdr_d2[slot].copy_(step.hdr, non_blocking=True)
        self.frm_d2[slot].copy_(step.frm, non_blocking=True)
        self.eside_d2[slot].copy_(step.eside, non_blocking=True)

    def run(self, step, slot, got, first, spec_d, ics_d):
        ctx, n_ch, state = self.ctx, self.n_ch, self.state
        hdr_d, frm_d, eside_d = self.hdr_d2[slot], self.frm_d2[slot], self.eside_d2[slot]
        ctx.imdct_process_batch(spec_d, ics_d, self.ovl, self.ovl_state, out32=self.out32, qshift_adj=self.qadj, ch_fac=1)
        # channel rows whose element resets in this frame (the LFE's never does: it has no header)
        reset = (step.flags[:, self.el_of_ch, F_RESET] != 0) & got[:, None]
        rows_h = np.nonzero(reset.ravel())[0]
        if rows_h.size:
            self.reset_rows(step, rows_h, step.reset_pitch[:, self.el_of_ch].ravel()[rows_h])
        self.keep_older()
        ctx.mc_core_from_out32(self.out32, self.qadj, self.core, n_ch)
        if self.trace is not None:
            self.trace(dict(state=state, hbe=self.hbe, ps_state=None, core=self.core, side=eside_d, header=hdr_d, frame=frm_d))
        ctx.esbr_sbr_process_batch(self.core, hdr_d, frm_d, eside_d, state, self.out_l, self.ws, status=self.status2[slot],
                                   hbe_state=self.hbe, hbe_max_synth_size=self.hbe_hint())
        ctx.mc_pcm16_from_planes(self.out_l, self.pcm2[slot], self.route, out_map=self.out_map)
        return (self.n, 2048, self.out_ch), 0, first


def _pick_out_map(name, n_ch, sbr, channel_config):
    """the OutMap decode_streams' out_map asks for on this kind of stream, None where the reference's flag is a no-op, ValueError
    where the command line decoder refuses the combination"""
    if name is None:
        return None
    if name not in ("downmix", "mono", "mono_dup", "dup"):
        raise ValueError('out_map is None, "downmix", "mono", "mono_dup" or "dup"')
    if name == "downmix":
        if n_ch <= 2 or not channel_config:
            raise ValueError("out_map=\"downmix\" on a stream of one or two channels is not supported (there is nothing to mix down)")
        return make_out_map(name, channel_config)
    if name in ("mono", "mono_dup"):
        if sbr or n_ch > 2:
            raise ValueError("out_map=\"%s\" on a stream with SBR or with more than two channels is not supported" % name)
        if n_ch == 1 and name == "mono_dup":
            raise ValueError("out_map=\"mono_dup\" on a mono stream is not supported")
        return make_out_map(name) if n_ch == 2 else None
    return make_out_map(name) if n_ch == 1 and not sbr else None    # "dup": a mono AAC-LC stream's channel twice, else a no-op


class _Pipeline:
    """The lock-step driver behind decode_streams.  Three staging sets go round: the parse of step k + 1 | the copies up and
    kernels of step k | the copy down of step k - 1.  Copies up have a stream of their own (`up`) into two sets of device
    input arrays, so step k + 1 goes up while step k's kernels read theirs; the copy down of step k runs on a second stream
    (`down`) beside the copies up and kernels of step k + 1 (two PCM / status sets), and the host takes a step's PCM one step
    later.  What runs between the two is the chain's business (_LcChain, _SbrChain or _EsbrChain, picked once in here), with
    the spectral tools in front of it when gpu_tools says so."""

    def __init__(self, streams, ctx, device, threads, keep_pcm, overlap, esbr, trace, frames_per_parse, gpu_tools, mc_sbr=False,
                 out_map=None, limiter=True, drc=None):
        self.dev = dev = torch.device(device)
        alloc, lib = _Alloc(dev), load_host_library()
        self.own = ctx is None
        if self.own:   # the context launches on torch's current stream, so that its kernels and torch's copies stay in order
            ctx = XaacContext(dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
        self.ctx = ctx
        self.bp = bp = BatchParser(streams, threads=threads, esbr=esbr, stage=1 if gpu_tools else 2, mc_sbr=mc_sbr, drc=drc)
        if bp.mc_sbr:   # what per-element SBR does not cover
            try:
                if not esbr:
                    raise ValueError("mc_sbr with esbr=False (the fixed-point SBR tools in a stream of more than two channels) is not supported")
                if 2 * bp.core_rate > 48000:
                    raise ValueError("mc_sbr with a down-sampled bank (an output rate above 48 kHz) is not supported")
            except ValueError:
                bp.close()
                raise
        if bp.sbr and not bp.mc_sbr and 2 * bp.core_rate > 48000:   # the chains below write at twice the core's rate
            bp.close()
            raise ValueError("SBR with a down-sampled bank (an output rate above 48 kHz) is not supported")
        try:
            out_map = _pick_out_map(out_map, bp.n_ch, bool(bp.sbr), bp.channel_config)
            if drc is not None:
                _refuse_drc(bp.n_ch, bool(bp.sbr), bp.channel_config)
        except ValueError:
            bp.close()
            raise
        # more than two channels: bitstream channel c of a stream goes up as row route[c] of its rows (the reference's output order);
        # with SBR the rows stay in bitstream order (the hand-off behind the SBR calls routes them)
        self.route = MC_LAYOUT[bp.channel_config][1] if bp.channel_config and not bp.sbr else None
        self.ics_routed = [alloc.pinned(bp.n * bp.n_ch, 2) for _ in range(4)] if self.route else None
        self.n, self.nc, self.keep_pcm, self.overlap = bp.n, bp.n * bp.n_ch, keep_pcm, overlap
        self.T = T = max(1, int(frames_per_parse))
        kind = _LcChain if not bp.sbr else _McEsbrChain if bp.mc_sbr else _EsbrChain if esbr else _SbrChain
        self.chain = chain = kind(ctx, lib, dev, bp.n, bp.n_ch, bp.core_rate, alloc, trace, out_map, bool(limiter) or bool(bp.sbr))
        first_rows = (0,)
        if bp.channel_config:   # every element's first bitstream channel, where the routed upload puts it
            elements, route, _ = MC_LAYOUT[bp.channel_config]
            starts = np.concatenate([[0], np.cumsum([2 if e == 1 else 1 for e in elements])[:-1]])
            first_rows = tuple(route[int(c)] if self.route else int(c) for c in starts)
        self.tools = _ToolsStage(ctx, bp.n, alloc.dz, alloc.pinned, bp.n_ch, first_rows) if gpu_tools else None
        self.drc = _DrcStage(ctx, bp.n * bp.n_ch, alloc.dz) if drc is not None else None
        # two sets of device input arrays: step k + 1 is copied up (its own stream) while step k's kernels read theirs
        self.spec_d2 = [alloc.dz(self.nc, 1024, dtype=torch.int32) for _ in range(2)]
        self.ics_d2 = [alloc.dz(self.nc, 2) for _ in range(2)]
        self.lines_held = [0, 0]   # per device input set: the leading spectral lines that may be non-zero there
        self.sets = [Staging(bp, alloc.pinned, T, chain.host_arrays, bool(gpu_tools), drc is not None) for _ in range(3 if overlap else 1)]
        self.main_stream, self.down, self.up = torch.cuda.current_stream(dev), torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        self.done = [torch.cuda.Event(), torch.cuda.Event()]
        self.computed = [torch.cuda.Event(), torch.cuda.Event()]
        self.hip = _hip_runtime()
        self.out = [[] for _ in range(bp.n)]
        self.waiting = None    # (slot, got, shape, cut, drop) of the step whose PCM is on its way
        self.t_parse = self.t_gpu = self.t_wait_parse = self.t_wait_down = 0.0

    def consume(self):
        """the host's half of the step whose PCM is on its way, if there is one: wait, look at the status words, keep the PCM"""
        if self.waiting is None:
            return
        slot, got, shape, cut, drop = self.waiting
        self.waiting = None
        t_c = time.perf_counter()
        self.done[slot].synchronize()
        self.t_wait_down += time.perf_counter() - t_c
        # (rows of streams that are over run idle on whatever their staging rows hold -- possibly nothing the kernels accept:
        # what they say about those is not looked at)
        chain, tools = self.chain, self.tools
        if chain.status_h2 is not None and int(chain.status_h2[slot].numpy().reshape(self.n, -1)[got].min(initial=0)) < 0:
            raise RuntimeError("the SBR kernels refused a frame")
        if tools is not None and tools.refused(slot, got):
            raise RuntimeError("the AAC tools kernel refused a frame")
        if self.keep_pcm and not drop:
            block = chain.pcm_h2[slot].numpy().reshape(shape)
            for i in np.nonzero(got)[0]:
                self.out[i].append(block[i, cut:].copy())

    def hand_down(self, slot, got, shape, cut, drop):
        chain, tools, down = self.chain, self.tools, self.down
        ev = self.computed[slot]
        ev.record(self.main_stream)   # this step's kernels are queued: its input set may be refilled, its PCM may go down
        with torch.cuda.stream(down):
            down.wait_event(ev)
            chain.pcm_h2[slot].copy_(chain.pcm2[slot], non_blocking=True)
            if chain.status2 is not None:
                chain.status_h2[slot].copy_(chain.status2[slot], non_blocking=True)
            if tools is not None:
                tools.status_h2[slot].copy_(tools.status2[slot], non_blocking=True)
            self.done[slot].record(down)
        self.consume()
        self.waiting = (slot, got, shape, cut, drop)
        if not self.overlap:   # one staging set: its copies up must be over before the next parse writes it
            self.consume()

    def send_up(self, cur, slot, got, step_no):
        """everything this step sends up, on the `up` stream beside the kernels of the step before"""
        up, spec_d = self.up, self.spec_d2[slot]
        with torch.cuda.stream(up):
            if step_no > 2:
                up.wait_event(self.computed[slot])   # (the kernels that read this input set two steps ago)
            # the spectra: only the leading lines that are not zero in every delivered row (AAC + SBR streams code the lower
            # half of the spectrum or less; 16 of the 26 MB a step of 4096 HE-AACv2 streams sends up are spectra), and
            # what this device set still holds beyond them from two steps ago (the host rows are zero there)
            lines_now = min(1024, (int(cur.lines[got].max()) + 63) & ~63)
            width = max(lines_now, self.lines_held[slot])
            self.lines_held[slot] = lines_now
            if self.route:      # one strided copy per channel, to its output place; the window info through a routed host copy
                n_ch, n = self.bp.n_ch, self.n
                ics_h = self.ics_routed[step_no & 3]
                for c, to in enumerate(self.route):
                    if width > 0:
                        rc = self.hip.hipMemcpy2DAsync(spec_d.data_ptr() + 4096 * to, 4096 * n_ch, cur.spec.data_ptr() + 4096 * c,
                                                       4096 * n_ch, 4 * width, n, 1, up.cuda_stream)
                        if rc != 0:
                            raise RuntimeError("hipMemcpy2DAsync: %d" % rc)
                    ics_h.numpy().reshape(n, n_ch, 2)[:, to] = cur.ics.numpy().reshape(n, n_ch, 2)[:, c]
                self.ics_d2[slot].copy_(ics_h, non_blocking=True)
            elif width >= 1024:
                spec_d.copy_(cur.spec, non_blocking=True)
            elif width > 0:
                rc = self.hip.hipMemcpy2DAsync(spec_d.data_ptr(), 4096, cur.spec.data_ptr(), 4096, 4 * width, self.nc, 1, up.cuda_stream)
                if rc != 0:
                    raise RuntimeError("hipMemcpy2DAsync: %d" % rc)
            if not self.route:
                self.ics_d2[slot].copy_(cur.ics, non_blocking=True)
            if self.tools is not None:
                self.tools.send_up(cur, slot)
            if self.drc is not None:
                self.drc.send_up(cur, slot)
            self.chain.send_up(cur, slot, got)
            cur.sent.record(up)

    def steps(self):
        """the step loop: until every stream is over"""
        T, overlap, sets, chain, tools, main_stream = self.T, self.overlap, self.sets, self.chain, self.tools, self.main_stream
        cur_set, t_in_set, pending, which, step_no, first = None, 0, None, 0, 0, True
        if overlap:
            # (the parse of the next steps runs on the parser library's own threads, xaac_parse_batch_start / _wait: a Python helper
            # thread would have to win the interpreter lock from this one, which gives it up only for microseconds at a time
            # while it queues copies and launches -- measured, its parse began when this thread blocked on the result)
            pending = sets[0].begin()
        while True:
            if t_in_set == T or cur_set is None:   # the next parser call's frames
                t_w = time.perf_counter()
                if not overlap:
                    pending = sets[0].begin()
                cur_set = pending.end()
                self.t_wait_parse += time.perf_counter() - t_w
                if overlap:    # the next T steps' frames are parsed while this thread looks at these and queues them on the GPU
                    which = (which + 1) % 3
                    pending = sets[which].begin()
                cur_set.finish()
                self.t_parse += cur_set.seconds
                t_in_set = 0
            cur = cur_set.steps[t_in_set]
            t_in_set += 1
            got = cur.got
            if not got.any():
                if overlap:
                    pending.end()   # (every stream is over: that call found nothing to parse)
                break
            slot = step_no & 1
            step_no += 1
            t0 = time.perf_counter()
            self.send_up(cur, slot, got, step_no)
            cur_set.sent_once = True
            main_stream.wait_event(cur.sent)
            spec_d = self.spec_d2[slot]
            if tools is not None:
                if first:
                    tools.begin(self.bp)
                tools.run(spec_d, slot)
            if self.drc is not None:
                self.drc.run(spec_d, slot)
            shape, cut, drop = chain.run(cur, slot, got, first, spec_d, self.ics_d2[slot])
            self.hand_down(slot, got, shape, cut, drop)
            self.t_gpu += time.perf_counter() - t0
            first = False

    def run(self, timing):
        """-> decode_streams' return value.  However the steps end, the parser team is taken back (a batch it still holds
        included) and a context of the pipeline's own closed: xaac_destroy frees the host-side handle alone -- the stream is
        torch's, the buffers are this decode's tensors -- so work still queued behind an error is not disturbed"""
        bp, chain = self.bp, self.chain
        try:
            t_steps = time.perf_counter()
            self.steps()
            self.consume()
            t_steps = time.perf_counter() - t_steps
            chain.finish(self.out, self.keep_pcm)
            frames = int(bp.frames.sum())
        finally:
            bp.close()
            if self.own:
                self.ctx.close()
        if timing is not None:
            # parse_s: inside the parser calls; wait_parse_s: what the loop waited for them; gpu_s: the loop's GPU section (enqueue
            # + wait_down_s, the wait for the previous step's PCM)
            timing.update(parse_s=self.t_parse, gpu_s=self.t_gpu, steps_s=t_steps, frames=frames, wait_parse_s=self.t_wait_parse,
                          wait_down_s=self.t_wait_down)
        return [np.concatenate(o) if o else np.zeros((0, chain.out_ch), np.int16) for o in self.out], chain.out_rate


def decode_streams(streams, ctx=None, device="cuda:0", threads=0, keep_pcm=True, timing=None, overlap=True, esbr=False,
                   _trace=None, frames_per_parse=4, gpu_tools=False, mc_sbr=False, out_map=None, limiter=True, drc=None):
    """Decodes N ADTS streams of the same kind (all AAC-LC mono or stereo, all AAC-LC of one channel_config 3 .. 6 -- 3.0 to
    5.1, output channels in the reference's order, MC_LAYOUT --, all HE-AAC stereo, or all HE-AAC / HE-AACv2 mono) in lock step: per step one frame of every stream is parsed on CPU threads into pinned staging arrays, copied to the GPU
    (spectra + window info, SBR / PS side info: nothing else crosses the bus on the way in), run through the GPU entry
    points against the streams' device-resident states, and the PCM copied back.
    -> (list of int16 [samples, channels] arrays, output sampling rate).  keep_pcm False: the PCM still comes back to the host
    every step but is not collected (throughput measurements); timing: a dict that receives seconds per stage.
    overlap: the host parses the next steps (further sets of staging arrays; the parser library's own threads,
    xaac_parse_batch_start / _wait) while this thread queues these on the GPU.
    frames_per_parse: frames of every stream per parser call (xaac_parse_batch::frames): a stream's parser state and bytes are
    fetched once for T frames -- on the GPU box's host the parser ran 15-40 % faster with 2..8 than with 1 -- and the T steps go
    through the GPU one after the other.
    esbr: decode SBR streams the way the reference does with its default flags (-esbr:1, "Path A": the float eSBR tools of
    xaac_esbr_sbr_process_batch with the QMF harmonic transposer and float parametric stereo; the SBR payload runs one
    frame late, and the reference's command line decoder does not write the first frame's output,
    test/decoder/ixheaacd_main.c:2181-2186) instead of -esbr:0.  AAC-LC streams decode
    the same either way.  SBR header changes in the middle of a stream are followed as the reference follows them (the
    reset-time transposer runs, sbrdecoder.c:196-236, read 24 rows of the QMF history of the frame before: kept beside the
    state).
    gpu_tools: the M/S, intensity, PNS and TNS tools run on the GPU (xaac_aac_tools_process_batch in front of the IMDCT) instead of
    in the parser: the streams are parsed at stage 1, the tools' side rows go up beside the spectra and every stream's noise
    generator lives on the device (one per channel element).  Off by default; the PCM is the same either way.
    mc_sbr: take HE-AAC streams of channel_config 3 .. 6 (an SBR payload per channel element; one SBR decoder per element, as the
    reference keeps them; output channels in the reference's order at twice the core's rate, no limiter).  esbr=True only: with
    esbr=False, or with an output rate above 48 kHz (the down-sampled bank), such a stream is a ValueError; without mc_sbr an SBR
    payload in a stream of more than two channels is a ValueError as before.
    out_map: the reference's output stage on the GPU, as an epilogue of the call that writes the PCM (only the mapped block comes down):
    "downmix" (-downmix:1: 3 .. 6 channels -> stereo), "mono" (-dmix:1: a stereo AAC-LC stream -> mono; a no-op on a mono one),
    "mono_dup" (-dmix:1 -tostereo:1: that mix in both channels), "dup" (-tostereo:1: a mono AAC-LC stream's channel twice; a no-op
    on everything else).  What the command line decoder refuses is a ValueError: "downmix" on one or two channels, "mono" /
    "mono_dup" with SBR or more than two channels, "mono_dup" on a mono stream.  Every sample is mapped, the limiter's flushed delay
    line included.
    limiter: False is -peak_limiter_off:1 (AAC-LC: ixheaacd_scale_adjust + round16 in the limiter's place; nothing changes with SBR).
    drc: None, or a dict of cut=, boost= (0 .. 1) and target_level= (0 .. 127) -- the reference's -drc_cut_fac, -drc_boost_fac and
    -drc_target_level (drc_config()): MPEG-4 dynamic range control and level normalisation from the dynamic_range_info of the
    streams' fill elements, on the GPU in front of the IMDCT (xaac_drc_apply_batch; the limiter runs behind as before).  AAC-LC
    mono and stereo streams; with SBR or more than two channels, heavy_comp or a value out of range it is a ValueError."""
    global torch
    drc = drc_config(drc)
    if drc is not None and len(streams):   # (refused before anything touches a GPU; the pipeline checks the batch it builds again)
        _, n_ch, sbr, config = stream_kind(streams[0])
        _refuse_drc(n_ch, sbr, config)
    import torch
    with _TorchCpuThreads():
        return _Pipeline(streams, ctx, device, threads, keep_pcm, overlap, esbr, _trace, frames_per_parse, bool(gpu_tools),
                         bool(mc_sbr), out_map, limiter, drc).run(timing)


def stream_kind(data):
    """the kind of an ADTS stream, as the batch calls need it to be one for all their streams: (core sampling rate, channels, frame
    0 carries an SBR payload, channel_config 3 .. 6 of a stream of several channel elements or else 0).  CPU only."""
    data = bytes(data)
    hdr = AdtsHeader()
    rc = load_host_library().xaac_adts_parse_header(data[:16], min(16, len(data)), ctypes.byref(hdr))
    if rc:
        raise ParseError(rc, 0)
    channels, n_elems, sbr, config = probe_first_frame(data)
    return int(hdr.sampling_rate), int(channels), bool(sbr), int(config) if n_elems > 1 else 0


def _default_parser_threads():
    """the size the parser library's team takes when nobody names one (host/xaac_parse.cpp: batch_threads)"""
    hw = os.cpu_count() or 1
    return min(min(hw // 2, 48) if hw >= 4 else hw, 2 * usable_cores())


# one group of decode_mixed: its kind (stream_kind), the places of its streams in the caller's list, its share of the parser threads
MixedGroup = collections.namedtuple("MixedGroup", "kind index threads")


def plan_mixed(streams, out_map=None, threads=0, drc=None):
    """What decode_mixed does before anything touches a GPU: probes every stream and sorts the list into groups of one kind, in the
    order in which the list first names the kinds, every group's streams in list order.  -> [MixedGroup].
    ValueError: a stream of channel_config 3 .. 6 beside another kind ("channel configurations", as decode_streams says it), or an
    out_map that one of the groups refuses (_pick_out_map's message behind "stream <i>: ", i the first such stream of the list).
    threads: the whole call's parser threads (0: the library's default), shared out over several groups in proportion to their
    streams, one at least; a single group keeps the value as it is."""
    if out_map is not None and out_map not in ("downmix", "mono", "mono_dup", "dup"):
        _pick_out_map(out_map, 0, False, 0)    # (a name that is none of the maps: its own message, no stream's)
    drc = drc_config(drc)                      # (a value out of range: its own message too)
    by_kind = {}
    for i, d in enumerate(streams):
        by_kind.setdefault(stream_kind(d), []).append(i)
    if len(by_kind) > 1 and any(kind[3] for kind in by_kind):
        raise ValueError("streams of different channel configurations in one batch")
    for (_, n_ch, sbr, config), index in by_kind.items():    # (in the order of the groups' first streams)
        try:
            _pick_out_map(out_map, n_ch, sbr, config)
            if drc is not None:
                _refuse_drc(n_ch, sbr, config)
        except ValueError as e:
            raise ValueError("stream %d: %s" % (index[0], e)) from None
    if len(by_kind) == 1:
        return [MixedGroup(kind, index, int(threads)) for kind, index in by_kind.items()]
    team = int(threads) if int(threads) > 0 else _default_parser_threads()
    return [MixedGroup(kind, index, max(1, team * len(index) // len(streams))) for kind, index in by_kind.items()]


def restore_list_order(groups, results, n):
    """results[g][k] belongs to stream groups[g].index[k] of the caller's list -> the n results in list order"""
    out = [None] * n
    for g, per_stream in zip(groups, results):
        if len(per_stream) != len(g.index):
            raise ValueError("a group of %d streams with %d results" % (len(g.index), len(per_stream)))
        for i, r in zip(g.index, per_stream):
            out[i] = r
    if any(r is None for r in out):
        raise ValueError("the groups do not cover the list")
    return out


def decode_mixed(streams, device="cuda:0", serial=False, esbr=False, gpu_tools=False, out_map=None, limiter=True, threads=0,
                 frames_per_parse=4, keep_pcm=True, drc=None):
    """Decodes ADTS streams of several kinds in one call: mono and stereo, any core sampling rate, AAC-LC beside HE-AAC and
    HE-AACv2.  -> (list of int16 [samples, channels] arrays, list of output sampling rates), both in the order of `streams`.

    The kind of a stream is (core sampling rate, channels, SBR payload in the first frame) -- what decode_streams wants to be
    the same for all its streams.  Every stream is probed on the CPU (stream_kind) and the list sorted into groups of one kind
    (plan_mixed); every group is decoded as decode_streams decodes it, by a pipeline of its own on its own torch.cuda.Stream with
    its own XaacContext, driven by one Python thread per group, so that the groups' copies and kernels share the device side by
    side.  The groups share nothing but the parser library's one team of threads: its calls queue, and `threads` (the whole
    call's, 0: the library's default) is shared out over the groups in proportion to their streams.  serial=True runs the
    same groups one after the other on the calling thread (the same PCM: to measure what side by side gains, or to find the
    group an error belongs to).
    esbr, gpu_tools, out_map, limiter, frames_per_parse, keep_pcm: as decode_streams takes them, for every group what they mean
    for a list of that kind alone (AAC-LC groups decode the same with either esbr; "dup" doubles a mono AAC-LC group's channel
    and is a no-op on the others).  An out_map that one group refuses is a ValueError that names the first such stream of the
    list ("stream <i>: ..."), raised before any GPU work, and nothing is decoded.  drc (decode_streams' dict) acts on the AAC-LC
    groups; a list with an SBR stream or one of more than two channels is refused the same way.  A stream of channel_config 3 .. 6 is only
    taken beside streams of its own kind (one group: decode_streams' path); beside another kind it is the ValueError "streams of
    different channel configurations in one batch", also before any GPU work -- its flags (mc_sbr, "downmix") mean nothing
    for the other kinds.  An SBR mono stream comes out in two channels, as decode_streams and the reference write it.
    An error inside one group's pipeline is raised here once every group has ended (the first group's, in list order)."""
    global torch
    groups = plan_mixed(streams, out_map, threads, drc)    # (the refusals: before torch is so much as imported)
    drc = drc_config(drc)
    import threading
    import torch
    dev = torch.device(device)
    results, errors = [None] * len(groups), [None] * len(groups)

    def run_group(k):
        g = groups[k]
        try:
            own = torch.cuda.Stream(dev)
            with torch.cuda.device(dev), torch.cuda.stream(own):   # (the pipeline's context launches on the thread's current stream)
                results[k] = _Pipeline([streams[i] for i in g.index], None, dev, g.threads, keep_pcm, True, esbr, None,
                                       frames_per_parse, bool(gpu_tools), False, out_map, limiter, drc).run(None)
                own.synchronize()
        except BaseException as e:   # (handed to the caller's thread)
            errors[k] = e

    with _TorchCpuThreads():
        if serial or len(groups) == 1:
            for k in range(len(groups)):
                run_group(k)
        else:
            team = [threading.Thread(target=run_group, args=(k,), name="decode_mixed-%d" % k) for k in range(len(groups))]
            for t in team:
                t.start()
            for t in team:
                t.join()
    for e in errors:
        if e is not None:
            raise e
    pcm = restore_list_order(groups, [r[0] for r in results], len(streams))
    rates = restore_list_order(groups, [[r[1]] * len(g.index) for g, r in zip(groups, results)], len(streams))
    return pcm, rates
