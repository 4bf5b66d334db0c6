"""libxaac_amd -- MI355X (gfx950) back-end for the transform hot path of the
libxaac decoder: host-side mirror of the reference's frame-level seam.

The product is ``libxaac_amd/libxaac_amd.so`` (hand-written HIP + a C ABI,
``include/xaac_amd.h``).  This module is the thin Python host layer used by the
tests and ``bench.py``: it binds the C ABI with ctypes (the structs and prototypes: ``abi.py``) and uses PyTorch only to
own device memory and streams.  There is no CPU fallback: importing works
anywhere, but creating a context without the built library or without a HIP
device raises.

Reference seam mirrored (names, argument meaning, error behaviour):
``ixheaacd_imdct_process`` -- decoder/ixheaacd_lpfuncs.c:347 (decl
decoder/ixheaacd_block.h:132), here batched over N channel-frames.
"""
import ctypes
import os

from . import abi
from .abi import (LIM_MAX_ATTACK, LIM_MAX_CH, AacToolsBatch, ApplySideBatch, DrcBatch, DrcConfig, DrcSide, EsbrAnaBatch,  # noqa: F401
                  EsbrAnaNbBatch, EsbrCoreInBatch, EsbrPcmOutBatch, EsbrSbrBatch, EsbrSynBatch, HandoverBatch, HbeAnalBatch,
                  HbeApplyBatch, HbeDftAnalBatch, HbeDftApplyBatch, HbeSynthBatch, ImdctBatch, ImdctLdBatch, LimiterBatch,
                  LimiterMapBatch, LimiterState, McCoreInBatch, McPcmOutMapBatch, OutMap, PvcBatch, QmfAnaBatch, QmfAnaEldBatch,
                  QmfSynBatch, QmfSynEldBatch, SbrEldBatch, SbrHqBatch, SbrLpBatch, ScaleAdjustMapBatch, UsacImdctBatch)

__all__ = [
    "ONLY_LONG_SEQUENCE", "LONG_START_SEQUENCE", "EIGHT_SHORT_SEQUENCE", "LONG_STOP_SEQUENCE",
    "PCM_LC", "PCM_SBR", "BAD_WINDOW_SEQ", "XaacError", "XaacContext", "load_library", "library_path",
    "decode_mixed",
]

# decoder/ixheaacd_cnst.h:100-103
ONLY_LONG_SEQUENCE, LONG_START_SEQUENCE, EIGHT_SHORT_SEQUENCE, LONG_STOP_SEQUENCE = 0, 1, 2, 3
PCM_LC, PCM_SBR = 0, 1
BAD_WINDOW_SEQ = -0x7FFC   # XAAC_FATAL_BAD_WINDOW_SEQ (0xFFFF8004) as the int32 a status word holds

_HERE = os.path.dirname(os.path.abspath(__file__))


def library_path():
    # XAAC_AMD_LIBRARY: developer override to time an experimental build of the same library
    return os.environ.get("XAAC_AMD_LIBRARY") or os.path.join(_HERE, "libxaac_amd.so")


class XaacError(RuntimeError):
    """Non-zero IA_ERRORCODE-style return (bit 31 set = fatal)."""

    def __init__(self, code, where):
        self.code = code & 0xFFFFFFFF
        super().__init__("%s failed: 0x%08X" % (where, self.code))


ESBR_RATIO_2_1, ESBR_RATIO_8_3, ESBR_RATIO_4_1 = 0, 1, 2   # xaac_esbr.h: XAAC_ESBR_RATIO_*
OUT_MAP_NONE, OUT_MAP_DOWNMIX_STEREO, OUT_MAP_MONO_MIX, OUT_MAP_MONO_MIX_DUP, OUT_MAP_DUP_STEREO = 0, 1, 2, 3, 4   # XAAC_OUT_MAP_*
HANDOVER_PS_START, HANDOVER_STEREO_START = 1, 2
DRC_ONE = 1 << 25   # XAAC_DRC_ONE

# Sizes of the states and side-info rows that cross the boundary as byte / word tensors, read off their mirrors
# (tests/test_abi.py pins the values).
_size = ctypes.sizeof
SBR_HEADER_BYTES, SBR_FRAME_BYTES, SBR_STATE_BYTES = _size(abi.SbrHeader), _size(abi.SbrFrame), _size(abi.SbrState)
SBR_ELD_STATE_BYTES = _size(abi.SbrEldState)
PS_FRAME_BYTES, PS_STATE_BYTES = _size(abi.PsFrame), _size(abi.PsState)
LIMITER_STATE_BYTES = _size(LimiterState)
ESBR_SIDE_BYTES, ESBR_STATE_BYTES, ESBR_PS_STATE_BYTES = _size(abi.EsbrSide), _size(abi.EsbrState), _size(abi.EsbrPsState)
ESBR_PVC_SIDE_BYTES, ESBR_PVC_STATE_BYTES = _size(abi.EsbrPvcSide), _size(abi.EsbrPvcState)
PVC_FRAME_BYTES, PVC_STATE_BYTES = _size(abi.PvcFrame), _size(abi.PvcState)
HBE_STATE_BYTES, HBE_DFT_STATE_BYTES = _size(abi.HbeState), _size(abi.HbeDftAnalState)
HBE_DFT_FULL_STATE_BYTES, HBE_DFT_CFG_BYTES = _size(abi.HbeDftState), _size(abi.HbeDftCfg)
CORE_TOOLS_SIDE_BYTES, CORE_TOOLS_STATE_BYTES = _size(abi.CoreToolsSide), _size(abi.CoreToolsState)
QMF_ANA_STATE_WORDS, QMF_SYN_STATE_WORDS = _size(abi.QmfAnaState) // 2, _size(abi.QmfSynState) // 2                # int16 words
QMF_ANA_ELD_STATE_WORDS, QMF_SYN_ELD_STATE_WORDS = _size(abi.QmfAnaEldState) // 2, _size(abi.QmfSynEldState) // 2  # int16
ESBR_ANA_STATE_WORDS, ESBR_SYN_STATE_WORDS = _size(abi.EsbrAnaState) // 4, _size(abi.EsbrSynState) // 4            # int32
USAC_FAC_IN_WORDS, DRC_SIDE_WORDS = _size(abi.UsacFacIn) // 4, _size(DrcSide) // 4                                 # int32

# channel_config -> the frame's channel elements as (type: 0 SCE, 1 CPE, 3 LFE; slot in the output block), bitstream order
_OUT_MAP_ELEMENTS = {3: ((0, 2), (1, 0)), 4: ((0, 2), (1, 0), (0, 3)), 5: ((0, 2), (1, 0), (1, 3)),
                     6: ((0, 2), (1, 0), (1, 4), (3, 3))}
_OUT_MAP_NAMES = {"downmix": OUT_MAP_DOWNMIX_STEREO, "mono": OUT_MAP_MONO_MIX, "mono_dup": OUT_MAP_MONO_MIX_DUP,
                  "dup": OUT_MAP_DUP_STEREO}


def out_map(kind, channel_config=0):
    """the xaac_out_map of a kind ("downmix" | "mono" | "mono_dup" | "dup" or an OUT_MAP_* value); a downmix takes the element
    list of ADTS channel_config 3 .. 6 and the matrix the reference picks for it (5.1 for six channels, else 5.0)"""
    m = OutMap()
    m.kind = _OUT_MAP_NAMES[kind] if isinstance(kind, str) else int(kind)
    if m.kind == OUT_MAP_DOWNMIX_STEREO:
        els = _OUT_MAP_ELEMENTS[int(channel_config)]
        m.matrix, m.n_elements = int(channel_config == 6), len(els)
        for k, (ty, slot) in enumerate(els):
            m.element_type[k], m.element_slot[k] = ty, slot
    return m


def out_map_channels(m, num_channels):
    """channels the map leaves of num_channels (0: it does not take that many)"""
    return {OUT_MAP_NONE: num_channels, OUT_MAP_DOWNMIX_STEREO: 2 if 3 <= num_channels <= 6 else 0,
            OUT_MAP_MONO_MIX: int(num_channels == 2), OUT_MAP_MONO_MIX_DUP: 2 * int(num_channels == 2),
            OUT_MAP_DUP_STEREO: 2 * int(num_channels == 1)}.get(m.kind, 0)


_lib = None


def load_library():
    """dlopen the product library and bind every entry point's prototype (abi.bind); loud failure when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 and owns the
    # streams / device memory handed to the C ABI, so it must be the copy that
    # libxaac_amd.so binds to -- import torch first whenever it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or make -C libxaac_amd/csrc); there is no CPU fallback" % path)
    _lib = abi.bind(ctypes.CDLL(path))
    return _lib


def _ptr(t, dtype_name, numel=None, allow_none=False, device_ok=None):
    """data pointer of a torch tensor or numpy array after shape/dtype checks"""
    if t is None:
        if allow_none:
            return None
        raise ValueError("required buffer is None")
    if hasattr(t, "data_ptr"):  # torch
        if not t.is_contiguous():
            raise ValueError("buffer must be contiguous")
        if str(t.dtype).replace("torch.", "") != dtype_name:
            raise TypeError("expected %s, got %s" % (dtype_name, t.dtype))
        if device_ok is not None and t.is_cuda != device_ok:
            raise ValueError("buffer is on the wrong side of the PCIe bus")
        n, p = t.numel(), t.data_ptr()
    else:  # numpy
        if not t.flags["C_CONTIGUOUS"]:
            raise ValueError("buffer must be contiguous")
        if t.dtype.name != dtype_name:
            raise TypeError("expected %s, got %s" % (dtype_name, t.dtype))
        if device_ok:
            raise ValueError("host array passed where a device tensor is required")
        n, p = t.size, t.ctypes.data
    if numel is not None and n != numel:
        raise ValueError("buffer has %d elements, expected %d" % (n, numel))
    return p


def peak_limiter_init(num_channels, sample_rate):
    """ixheaacd_peak_limiter_init: -> (LimiterState, delay in samples)"""
    st = LimiterState()
    rc = load_library().xaac_peak_limiter_init(ctypes.byref(st), int(num_channels), int(sample_rate))
    if rc < 0:
        raise XaacError(rc, "xaac_peak_limiter_init")
    return st, rc


class XaacContext:
    """One context per GPU / stream (xaac_create ... xaac_destroy)."""

    def __init__(self, device=0, stream_handle=None):
        """stream_handle: a hipStream_t as an int (e.g. torch.cuda.Stream().cuda_stream; 0 = the
        legacy null stream); None lets the library create and own a stream."""
        self._lib = load_library()
        h = ctypes.c_void_p()
        rc = self._lib.xaac_create(ctypes.byref(h), int(device), None)
        if rc != 0:
            raise XaacError(rc, "xaac_create")
        self._h = h
        self.device = device
        if stream_handle is not None:
            self.set_stream(stream_handle)

    def _call(self, name, *args):
        """entry point `name` (bound by load_library) on this context; a non-zero return raises the XaacError that names it"""
        rc = getattr(self._lib, name)(self._h, *args)
        if rc != 0:
            raise XaacError(rc, name)

    def set_stream(self, stream_handle):
        self._call("xaac_set_stream", ctypes.c_void_p(int(stream_handle)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.xaac_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._call("xaac_sync")

    def warm_up(self):
        """every kernel's code object onto the device now (otherwise: at each module's first launch)"""
        self._call("xaac_warm_up")

    def last_launch(self):
        g, b, l = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._lib.xaac_last_launch(self._h, ctypes.byref(g), ctypes.byref(b), ctypes.byref(l))
        return {"grid": g.value, "block": b.value, "lds_bytes": l.value}

    def _batch(self, n_ch, spec, ics, overlap, state, out32, pcm16, qshift_adj, ch_fac, pcm_mode, on_device, status=None,
               frame=1024):
        b = ImdctBatch()
        b.n_ch, b.ch_fac, b.pcm_mode = int(n_ch), int(ch_fac), int(pcm_mode)
        b.spec = _ptr(spec, "int32", n_ch * frame, device_ok=on_device)
        b.ics = _ptr(ics, "uint8", n_ch * 2, device_ok=on_device)
        b.overlap = _ptr(overlap, "int32", n_ch * frame // 2, device_ok=on_device)
        b.state = _ptr(state, "uint8", n_ch * 2, device_ok=on_device)
        b.out32 = _ptr(out32, "int32", n_ch * frame, allow_none=True, device_ok=on_device)
        b.pcm16 = _ptr(pcm16, "int16", n_ch * frame, allow_none=True, device_ok=on_device)
        b.qshift_adj = _ptr(qshift_adj, "int8", n_ch, allow_none=True, device_ok=on_device)
        b.status = _ptr(status, "int32", n_ch, allow_none=True, device_ok=on_device)
        return b

    def imdct_process_batch(self, spec, ics, overlap, state, out32=None, pcm16=None, qshift_adj=None,
                            ch_fac=1, pcm_mode=PCM_LC, status=None):
        """Batched ixheaacd_imdct_process on device tensors (asynchronous).

        spec int32[N,1024]; ics uint8[N,2] = (window_sequence, window_shape);
        overlap int32[N,512] in/out; state uint8[N,2] in/out (previous
        window_sequence, window_shape); optional outputs out32 int32[N*1024],
        pcm16 int16[N*1024] (interleaved at stride ch_fac), qshift_adj int8[N], status int32[N] (0, or
        BAD_WINDOW_SEQ for a channel-frame whose window bytes no bitstream can carry: left untouched)."""
        n_ch = spec.shape[0] if spec.dim() == 2 else spec.numel() // 1024
        b = self._batch(n_ch, spec, ics, overlap, state, out32, pcm16, qshift_adj, ch_fac, pcm_mode, True, status)
        self._call("xaac_imdct_process_batch", ctypes.byref(b))

    def aac_tools_process_batch(self, spec, side, state, status=None, spec_stride=None, first_row=0):
        """The AAC spectral tools (M/S, intensity, PNS, TNS: the tool half of ixheaacd_channel_pair_process) on device tensors
        (asynchronous), in front of imdct_process_batch: spec int32[N, 2, 1024] (or [N, 1024] for mono elements) as the host
        parser's stage 1 delivers it, in / out; side uint8[N, CORE_TOOLS_SIDE_BYTES] (xaac_parse_core_tools_side); state
        uint8[N, CORE_TOOLS_STATE_BYTES] in / out (a new stream's: xaac_parse_core_tools_state); optional status int32[N]: 0, or -1 for side info
        the tools refuse (that element is left untouched).  first_row: the element's first channel is row first_row of the
        spec_stride / 1024 rows every stream has in spec (streams of several channel elements: one call per element index)."""
        n = side.shape[0]
        stride = int(spec_stride) if spec_stride is not None else spec.numel() // max(n, 1)
        first_row = int(first_row)
        if first_row < 0 or (first_row + 1) * 1024 > stride:
            raise ValueError("first_row outside the rows of a stream")
        b = AacToolsBatch()
        b.n, b.spec_stride = n, stride
        b.spec = _ptr(spec, "int32", n * stride, device_ok=True) + 4096 * first_row
        b.side = _ptr(side, "uint8", n * CORE_TOOLS_SIDE_BYTES, device_ok=True)
        b.state = _ptr(state, "uint8", n * CORE_TOOLS_STATE_BYTES, device_ok=True)
        b.status = _ptr(status, "int32", n, allow_none=True, device_ok=True)
        self._call("xaac_aac_tools_process_batch", ctypes.byref(b))

    def drc_apply_batch(self, spec, side, status=None, spec_stride=1024):
        """MPEG-4 dynamic range control in the spectral domain (ixheaacd_drc_apply without SBR) on device tensors (asynchronous),
        in front of imdct_process_batch: spec int32, row i's 1024 lines at word i * spec_stride, in / out; side
        int32[N, DRC_SIDE_WORDS] (xaac_drc_side rows: xaac_parse_drc_side); optional status int32[N]: 0, or -1 for a row whose
        side info is outside the struct's capacity (left untouched)."""
        n, stride = side.shape[0], int(spec_stride)
        if n and spec.numel() < (n - 1) * stride + 1024:
            raise ValueError("spec is shorter than %d rows at a stride of %d words" % (n, stride))
        b = DrcBatch()
        b.n, b.spec_stride = n, stride
        b.spec = _ptr(spec, "int32", device_ok=True)
        b.side = _ptr(side, "int32", n * DRC_SIDE_WORDS, device_ok=True)
        b.status = _ptr(status, "int32", n, allow_none=True, device_ok=True)
        self._call("xaac_drc_apply_batch", ctypes.byref(b))

    def imdct960_process_batch(self, spec, ics, overlap, state, out32=None, pcm16=None, qshift_adj=None, ch_fac=1,
                               pcm_mode=PCM_LC, status=None):
        """Batched ixheaacd_imdct_process for frame_length 960 on device tensors (asynchronous): spec int32[N,960],
        overlap int32[N,480] in/out, out32 / pcm16 [N*960]; everything else as imdct_process_batch."""
        n_ch = spec.shape[0]
        b = self._batch(n_ch, spec, ics, overlap, state, out32, pcm16, qshift_adj, ch_fac, pcm_mode, True, status, frame=960)
        self._call("xaac_imdct960_process_batch", ctypes.byref(b))

    def imdct_ld_process_batch(self, spec, window_shape, overlap, shape_prev, pcm16, frame_length, eld, ch_fac=1, status=None):
        """Batched ixheaacd_imdct_process for AAC-LD (eld = 0) / AAC-ELD (eld = 1) frames on device tensors: spec
        int32[N, frame_length] (512 or 480), window_shape uint8[N], overlap int32[N, frame_length / 2] (LD) or
        [N, 3 * frame_length] (ELD) in/out, shape_prev uint8[N] in/out, pcm16 int16[N * frame_length] at stride ch_fac."""
        n_ch = spec.shape[0]
        b = ImdctLdBatch()
        b.n_ch, b.ch_fac, b.frame_length, b.eld = n_ch, int(ch_fac), int(frame_length), int(eld)
        b.spec = _ptr(spec, "int32", n_ch * frame_length, device_ok=True)
        b.window_shape = _ptr(window_shape, "uint8", n_ch, device_ok=True)
        b.overlap = _ptr(overlap, "int32", n_ch * (3 * frame_length if eld else frame_length // 2), device_ok=True)
        b.shape_prev = _ptr(shape_prev, "uint8", n_ch, device_ok=True)
        b.pcm16 = _ptr(pcm16, "int16", n_ch * frame_length, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, allow_none=True, device_ok=True)
        self._call("xaac_imdct_ld_process_batch", ctypes.byref(b))

    def imdct_process_batch_host(self, spec, ics, overlap, state, out32=None, pcm16=None, qshift_adj=None,
                                 ch_fac=1, pcm_mode=PCM_LC, status=None):
        """Same on host numpy arrays (copies over PCIe, synchronous)."""
        n_ch = spec.shape[0]
        b = self._batch(n_ch, spec, ics, overlap, state, out32, pcm16, qshift_adj, ch_fac, pcm_mode, False, status)
        self._call("xaac_imdct_process_batch_host", ctypes.byref(b))

    def qmf_analysis_batch(self, pcm, state, qmf, low_pow, usb=32, slot_stride=None, ch_fac=1):
        """Batched ixheaacd_cplx_anal_qmffilt: one frame (1024 PCM16 -> 32 slots x 32 bands) per channel.
        pcm int16[n_ch*1024] interleaved at ch_fac; state int16[n_ch, 322] in/out; qmf int32[n_ch, 32, slot_stride]
        (real bands at +0, imaginary at +64 in HQ mode)."""
        n_ch = state.shape[0]
        if slot_stride is None:
            slot_stride = 64 if low_pow else 128
        b = QmfAnaBatch()
        b.n_ch, b.ch_fac, b.low_pow, b.usb, b.slot_stride = n_ch, int(ch_fac), int(bool(low_pow)), int(usb), slot_stride
        b.pcm = _ptr(pcm, "int16", n_ch * 1024, device_ok=True)
        b.state = _ptr(state, "int16", n_ch * QMF_ANA_STATE_WORDS, device_ok=True)
        b.qmf = _ptr(qmf, "int32", n_ch * 32 * slot_stride, device_ok=True)
        self._call("xaac_qmf_analysis_batch", ctypes.byref(b))

    def qmf_synthesis_batch(self, qmf, scale, state, pcm, low_pow, lsb, usb, split=6, slot_stride=None, ch_fac=1,
                            down_sample=False):
        """Batched ixheaacd_cplx_synt_qmffilt (no PS): 32 slots x 64 bands -> 2048 PCM16 per channel.
        qmf int32[n_ch, 32, slot_stride]; scale int16[n_ch, 4] = lb_scale, ov_lb_scale, hb_scale, st_syn_scale;
        state int16[n_ch, 1282] in/out; pcm int16[n_ch*2048] interleaved at ch_fac.  down_sample: the 32-channel
        bank (1024 samples per channel out)."""
        n_ch = state.shape[0]
        if slot_stride is None:
            slot_stride = 64 if low_pow else 128
        b = QmfSynBatch()
        b.n_ch, b.ch_fac, b.low_pow, b.lsb, b.usb, b.split = n_ch, int(ch_fac), int(bool(low_pow)), int(lsb), int(usb), int(split)
        b.slot_stride = slot_stride
        b.down_sample = int(bool(down_sample))
        b.qmf = _ptr(qmf, "int32", n_ch * 32 * slot_stride, device_ok=True)
        b.scale = _ptr(scale, "int16", n_ch * 4, device_ok=True)
        b.state = _ptr(state, "int16", n_ch * QMF_SYN_STATE_WORDS, device_ok=True)
        b.pcm = _ptr(pcm, "int16", n_ch * (1024 if down_sample else 2048), device_ok=True)
        self._call("xaac_qmf_synthesis_batch", ctypes.byref(b))

    def esbr_workspace_bytes(self, n_ch, sbr_ratio=0):
        return int(self._lib.xaac_esbr_workspace_bytes_ratio(int(n_ch), int(sbr_ratio)))

    def esbr_sbr_process_batch(self, core, header, frame, side, state, out, workspace, status=None, ps_frame=None,
                               ps_state=None, out_r=None, hbe_state=None, hbe_max_synth_size=0, pvc_side=None, pvc_state=None,
                               sbr_ratio=0, down_sample=False, hbe_dft=None):
        """One frame of every channel through the Path A (eSBR, -esbr:1) branch of ixheaacd_sbr_dec, mono / stereo
        channels without PS: core float32[n_ch, 1024]; header / frame / side / state uint8 views of the xaac_sbr_header,
        xaac_sbr_frame, xaac_esbr_side, xaac_esbr_state arrays; out float32[n_ch, 2048].  With ps_frame / ps_state (uint8
        views of xaac_ps_frame / xaac_esbr_ps_state arrays) / out_r: HE-AACv2 streams, float parametric stereo, out = left.
        hbe_state (uint8[n_ch, HBE_STATE_BYTES]): the harmonic transposer runs on every frame and frames with harmonic_sbr
        set take its output.  sbr_ratio ESBR_RATIO_8_3: 768 samples of a core row through the 24-channel bank;
        ESBR_RATIO_4_1: the 16-channel bank, 64 slots, out float32[n_ch, 4096], workspace of esbr_workspace_bytes(n_ch, ratio).
        hbe_dft = (state uint8[n_ch, HBE_DFT_FULL_STATE_BYTES], cfg_tab uint8[n_cfg, HBE_DFT_CFG_BYTES], coef_re, coef_im
        float32[n_cfg, 64, 128], cfg int32[n_ch] or None) instead of hbe_state: -esbr_hq:1, the DFT transposer."""
        n_ch = out.shape[0]
        b = EsbrSbrBatch()
        b.sbr_ratio = int(sbr_ratio)
        b.down_sample = int(bool(down_sample))    # the 32-channel synthesis bank(s): half the samples at the same row pitch
        b.n_ch = n_ch
        b.core = _ptr(core, "float32", n_ch * 1024, device_ok=True)
        b.header = _ptr(header, "uint8", n_ch * SBR_HEADER_BYTES, device_ok=True)
        b.frame = _ptr(frame, "uint8", n_ch * SBR_FRAME_BYTES, device_ok=True)
        b.side = _ptr(side, "uint8", n_ch * ESBR_SIDE_BYTES, device_ok=True)
        b.state = _ptr(state, "uint8", n_ch * ESBR_STATE_BYTES, device_ok=True)
        b.out = _ptr(out, "float32", n_ch * (4096 if b.sbr_ratio == ESBR_RATIO_4_1 else 2048), device_ok=True)
        b.ps_frame = _ptr(ps_frame, "uint8", n_ch * PS_FRAME_BYTES, allow_none=True, device_ok=True)
        b.ps_state = _ptr(ps_state, "uint8", n_ch * ESBR_PS_STATE_BYTES, allow_none=True, device_ok=True)
        b.out_r = _ptr(out_r, "float32", n_ch * 2048, allow_none=True, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, allow_none=True, device_ok=True)
        b.workspace = _ptr(workspace, "uint8", device_ok=True)
        b.workspace_bytes = workspace.numel()
        b.hbe_state = _ptr(hbe_state, "uint8", n_ch * HBE_STATE_BYTES, allow_none=True, device_ok=True)
        b.hbe_max_synth_size = int(hbe_max_synth_size)   # 4 / 8: no larger transposer bank in the batch (less LDS per channel); 0: any
        # USAC channels with PVC frames: uint8 views of the xaac_esbr_pvc_side / xaac_esbr_pvc_state arrays (both or neither)
        b.pvc_side = _ptr(pvc_side, "uint8", n_ch * ESBR_PVC_SIDE_BYTES, allow_none=True, device_ok=True)
        b.pvc_state = _ptr(pvc_state, "uint8", n_ch * ESBR_PVC_STATE_BYTES, allow_none=True, device_ok=True)
        if hbe_dft is not None:
            d_state, d_cfg_tab, d_cre, d_cim, d_cfg = hbe_dft
            b.hbe_dft_state = _ptr(d_state, "uint8", n_ch * HBE_DFT_FULL_STATE_BYTES, device_ok=True)
            b.hbe_dft_cfg_tab = _ptr(d_cfg_tab, "uint8", device_ok=True)
            b.hbe_dft_coef_re = _ptr(d_cre, "float32", device_ok=True)
            b.hbe_dft_coef_im = _ptr(d_cim, "float32", device_ok=True)
            b.hbe_dft_cfg = _ptr(d_cfg, "int32", n_ch, allow_none=True, device_ok=True)
        self._call("xaac_esbr_sbr_process_batch", ctypes.byref(b))

    def esbr_core_from_pcm16(self, pcm, core, ch_fac=1):
        """the core decoder's PCM16 (int16[n_ch * 1024], channels of an element interleaved at ch_fac) as float planes
        core float32[n_ch, 1024] (api.c:3385-3432)"""
        b = EsbrCoreInBatch()
        b.n_ch, b.ch_fac = int(core.shape[0]), int(ch_fac)
        b.pcm = _ptr(pcm, "int16", b.n_ch * 1024, device_ok=True)
        b.core = _ptr(core, "float32", b.n_ch * 1024, device_ok=True)
        self._call("xaac_esbr_core_from_pcm16_batch", ctypes.byref(b))

    def esbr_pcm16_from_float(self, left, right, pcm, stride=2048):
        """ixheaacd_samples_sat for two channels: stream i's float planes left / right (device tensors; element offset
        i * stride) -> pcm int16[n * 2048 * 2]; left is right for a duplicated mono channel"""
        n = pcm.numel() // 4096
        b = EsbrPcmOutBatch()
        b.n, b.stride = int(n), int(stride)
        b.left = _ptr(left, "float32", device_ok=True)
        b.right = _ptr(right, "float32", device_ok=True)
        b.pcm = _ptr(pcm, "int16", n * 4096, device_ok=True)
        self._call("xaac_esbr_pcm16_from_float_batch", ctypes.byref(b))

    def mc_core_from_out32(self, out32, qshift_adj, core, channel_config):
        """more than two channels: the IMDCT's WORD32 rows (int32[n * n_ch, 1024], ch_fac 1, channels in bitstream order) and
        their qshift_adj (int8[n * n_ch]) -> the float planes core float32[n * n_ch, 1024] the Path A branch reads, through the
        reference's in-place 16-bit conversion of every channel element in the frame's block (xaac_mc_core_in_batch)"""
        b = McCoreInBatch()
        rows = int(core.shape[0])
        b.n_streams, b.channel_config = rows // int(channel_config), int(channel_config)
        if b.n_streams * b.channel_config != rows:
            raise ValueError("rows are no multiple of the channel count")
        b.out32 = _ptr(out32, "int32", rows * 1024, device_ok=True)
        b.qshift_adj = _ptr(qshift_adj, "int8", rows, device_ok=True)
        b.core = _ptr(core, "float32", rows * 1024, device_ok=True)
        self._call("xaac_mc_core_from_out32_batch", ctypes.byref(b))

    def mc_pcm16_from_planes(self, planes, pcm, slot, stride=2048, out_map=None):
        """more than two channels: stream i's plane c (float32: clamped and truncated as ixheaacd_samples_sat_mc does; int16: as it
        is) at element (i * n_ch + c) * stride of `planes` -> pcm int16[n * 2048 * n_ch], plane c as output channel slot[c].
        out_map (an OutMap of kind OUT_MAP_DOWNMIX_STEREO): the downmix to stereo on the way out, pcm int16[n * 2048 * 2]"""
        n_ch = len(slot)
        mb = McPcmOutMapBatch()
        b = mb.out
        b.n_streams, b.n_ch, b.stride = pcm.numel() // (2048 * (2 if out_map is not None else n_ch)), n_ch, int(stride)
        for c, to in enumerate(slot):
            b.slot[c] = int(to)
        flt = str(planes.dtype).endswith("float32")
        b.planes = _ptr(planes, "float32" if flt else "int16", device_ok=True)
        if planes.numel() < (b.n_streams * n_ch - 1) * b.stride + 2048:
            raise ValueError("planes are shorter than the batch")
        b.pcm = _ptr(pcm, "int16", b.n_streams * 2048 * (2 if out_map is not None else n_ch), device_ok=True)
        fn = "xaac_mc_pcm16_from_float_batch" if flt else "xaac_mc_pcm16_from_planes_batch"
        if out_map is not None:
            mb.map = out_map
            fn = fn.replace("_batch", "_map_batch")
        self._call(fn, ctypes.byref(mb if out_map is not None else b))

    def sbr_state_handover(self, mode, src, dst, state, ps_state=None):
        """ixheaacd_sbrdecoder.c:762-806 for the listed streams: mode HANDOVER_PS_START (dst indexes ps_state) or
        HANDOVER_STEREO_START (dst indexes state); src / dst int32 device tensors; state / ps_state uint8 views of the
        xaac_sbr_state / xaac_ps_state arrays."""
        b = HandoverBatch()
        b.n, b.mode = int(src.numel()), int(mode)
        b.src = _ptr(src, "int32", device_ok=True)
        b.dst = _ptr(dst, "int32", b.n, device_ok=True)
        b.state = _ptr(state, "uint8", device_ok=True)
        b.ps_state = _ptr(ps_state, "uint8", allow_none=True, device_ok=True)
        self._call("xaac_sbr_state_handover", ctypes.byref(b))

    def sbr_state_apply_side_batch(self, header, flags, state, ch_fac, ps_state=None):
        """ixheaacd_sbr_dec_reset / ixheaacd_prepare_upsamp (sbrdecoder.c:103-276) on the resident states of the streams whose
        flag rows say so: header uint8[n * ch_fac, SBR_HEADER_BYTES] (this frame's), flags int32[n, abi.SBR_FLAG_WORDS] (the parser's rows;
        zero for streams without a frame), state / ps_state the uint8 views of the xaac_sbr_state / xaac_ps_state arrays."""
        b = ApplySideBatch()
        b.n_streams, b.ch_fac = int(flags.shape[0]), int(ch_fac)
        b.header = _ptr(header, "uint8", b.n_streams * b.ch_fac * SBR_HEADER_BYTES, device_ok=True)
        b.flags = _ptr(flags, "int32", b.n_streams * abi.SBR_FLAG_WORDS, device_ok=True)
        b.state = _ptr(state, "uint8", b.n_streams * b.ch_fac * SBR_STATE_BYTES, device_ok=True)
        b.ps_state = _ptr(ps_state, "uint8", allow_none=True, device_ok=True)
        self._call("xaac_sbr_state_apply_side_batch", ctypes.byref(b))

    def usac_imdct_process_batch(self, coef, ics, overlap, shape_prev, out32=None, time=None, status=None, ccfl=1024,
                                 lpd_flags=None, fac=None, fac_in=None, fac_work=None):
        """Batched ixheaacd_fd_frm_dec (USAC FD frame after an FD frame, ccfl 1024 or 768, no FAC): coef int32[n_ch, ccfl];
        ics uint8[n_ch, 2] (window_sequence 0..4, window_shape); overlap int32[n_ch, ccfl] in/out; shape_prev uint8[n_ch]
        in/out; out32 int32[n_ch, ccfl] (Q15) and / or time float32[n_ch, ccfl]; status int32[n_ch]."""
        n_ch = overlap.shape[0]
        b = UsacImdctBatch()
        b.n_ch, b.ccfl = n_ch, int(ccfl)
        b.coef = _ptr(coef, "int32", n_ch * ccfl, device_ok=True)
        b.ics = _ptr(ics, "uint8", n_ch * 2, device_ok=True)
        b.overlap = _ptr(overlap, "int32", n_ch * ccfl, device_ok=True)
        b.shape_prev = _ptr(shape_prev, "uint8", n_ch, device_ok=True)
        b.out32 = _ptr(out32, "int32", n_ch * ccfl, allow_none=True, device_ok=True)
        b.time = _ptr(time, "float32", n_ch * ccfl, allow_none=True, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, allow_none=True, device_ok=True)
        # LPD -> FD transitions: lpd_flags uint8[n_ch] (bit 0 td_frame_prev, bit 1 fac_data_present), fac int32[n_ch, 257]
        # (struct xaac_usac_fac: q, data[256])
        b.lpd_flags = _ptr(lpd_flags, "uint8", n_ch, allow_none=True, device_ok=True)
        b.fac = _ptr(fac, "int32", n_ch * 257, allow_none=True, device_ok=True)
        # ... or the signal made on the device (ixheaacd_cal_fac_data): fac_in int32 view of [n_ch] xaac_usac_fac_in, fac_work
        # int32[n_ch, 257] scratch
        b.fac_in = _ptr(fac_in, "int32", n_ch * USAC_FAC_IN_WORDS, allow_none=True, device_ok=True)
        b.fac_work = _ptr(fac_work, "int32", n_ch * 257, allow_none=True, device_ok=True)
        self._call("xaac_usac_imdct_process_batch", ctypes.byref(b))

    def hbe_real_synth_batch(self, qmf_re, qmf_im, state, status=None, num_columns=32):
        """Batched ixheaacd_real_synth_filt (the harmonic transposer's real synthesis bank): qmf_re / qmf_im
        float32[n_ch, num_columns, 64]; state uint8[n_ch, HBE_STATE_BYTES] in/out (struct xaac_hbe_state);
        status int32[n_ch] or None."""
        n_ch = state.shape[0]
        b = HbeSynthBatch()
        b.n_ch, b.num_columns = n_ch, num_columns
        b.qmf_re = _ptr(qmf_re, "float32", n_ch * num_columns * 64, device_ok=True)
        b.qmf_im = _ptr(qmf_im, "float32", n_ch * num_columns * 64, device_ok=True)
        b.state = _ptr(state, "uint8", n_ch * HBE_STATE_BYTES, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, device_ok=True) if status is not None else None
        self._call("xaac_hbe_real_synth_batch", ctypes.byref(b))

    def hbe_apply_batch(self, qmf_re, qmf_im, state, pv_re, pv_im, status=None, pitch_in_bins=None, max_synth_size=0):
        """Batched ixheaacd_qmf_hbe_apply (the QMF-domain harmonic transposer, frames without a pitch): qmf_re / qmf_im
        float32[n_ch, 32, 64]; state uint8[n_ch, HBE_STATE_BYTES] in/out; pv_re / pv_im float32[n_ch, 32, 64] (bands
        start_band..end_band-1 written); status int32[n_ch] or None; pitch_in_bins int32[n_ch] or None."""
        n_ch = state.shape[0]
        b = HbeApplyBatch()
        b.n_ch = n_ch
        b.qmf_re = _ptr(qmf_re, "float32", n_ch * 2048, device_ok=True)
        b.qmf_im = _ptr(qmf_im, "float32", n_ch * 2048, device_ok=True)
        b.pitch_in_bins = _ptr(pitch_in_bins, "int32", n_ch, device_ok=True) if pitch_in_bins is not None else None
        b.state = _ptr(state, "uint8", n_ch * HBE_STATE_BYTES, device_ok=True)
        b.pv_re = _ptr(pv_re, "float32", n_ch * 2048, device_ok=True)
        b.pv_im = _ptr(pv_im, "float32", n_ch * 2048, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, device_ok=True) if status is not None else None
        b.max_synth_size = int(max_synth_size)
        self._call("xaac_hbe_apply_batch", ctypes.byref(b))

    def hbe_dft_anal_batch(self, time_in, coef_re, coef_im, state, qmf_re, qmf_im, cfg=None, status=None, no_bins=32):
        """Batched ixheaacd_dft_hbe_cplx_anal_filt (the DFT transposer's analysis bank): time_in float32[n_ch, stride];
        coef_re / coef_im float32[n_cfg, 64, 128]; state uint8[n_ch, HBE_DFT_STATE_BYTES] in/out; qmf_re / qmf_im
        float32[n_ch, no_bins + 2, 64] in/out; cfg int32[n_ch] or None."""
        n_ch = state.shape[0]
        b = HbeDftAnalBatch()
        b.n_ch, b.no_bins, b.in_stride = n_ch, no_bins, int(time_in.shape[1])
        b.time_in = _ptr(time_in, "float32", n_ch * b.in_stride, device_ok=True)
        b.coef_re = _ptr(coef_re, "float32", device_ok=True)
        b.coef_im = _ptr(coef_im, "float32", device_ok=True)
        b.cfg = _ptr(cfg, "int32", n_ch, device_ok=True) if cfg is not None else None
        b.state = _ptr(state, "uint8", n_ch * HBE_DFT_STATE_BYTES, device_ok=True)
        b.qmf_re = _ptr(qmf_re, "float32", n_ch * (no_bins + 2) * 64, device_ok=True)
        b.qmf_im = _ptr(qmf_im, "float32", n_ch * (no_bins + 2) * 64, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, device_ok=True) if status is not None else None
        self._call("xaac_hbe_dft_anal_batch_run", ctypes.byref(b))

    def hbe_dft_apply_batch(self, qmf_re, qmf_im, cfg_tab, coef_re, coef_im, state, pv_re, pv_im, status, pitch_in_bins=None,
                            oversampling=None, cfg=None, rows32=False):
        """Batched ixheaacd_dft_hbe_apply (the DFT harmonic transposer, -esbr_hq:1): qmf_re / qmf_im float32[n_ch, 32, 64];
        cfg_tab uint8[n_cfg, HBE_DFT_CFG_BYTES]; coef_re / coef_im float32[n_cfg, 64, 128]; state
        uint8[n_ch, HBE_DFT_FULL_STATE_BYTES] in/out; pv_re / pv_im float32[n_ch, 34, 64] in/out; status int32[n_ch];
        pitch_in_bins / oversampling / cfg int32[n_ch] or None."""
        n_ch = state.shape[0]
        b = HbeDftApplyBatch()
        b.n_ch = n_ch
        b.qmf_re = _ptr(qmf_re, "float32", n_ch * 2048, device_ok=True)
        b.qmf_im = _ptr(qmf_im, "float32", n_ch * 2048, device_ok=True)
        b.pitch_in_bins = _ptr(pitch_in_bins, "int32", n_ch, device_ok=True) if pitch_in_bins is not None else None
        b.oversampling = _ptr(oversampling, "int32", n_ch, device_ok=True) if oversampling is not None else None
        b.cfg_tab = _ptr(cfg_tab, "uint8", device_ok=True)
        b.coef_re = _ptr(coef_re, "float32", device_ok=True)
        b.coef_im = _ptr(coef_im, "float32", device_ok=True)
        b.cfg = _ptr(cfg, "int32", n_ch, device_ok=True) if cfg is not None else None
        b.state = _ptr(state, "uint8", n_ch * HBE_DFT_FULL_STATE_BYTES, device_ok=True)
        b.rows32 = int(bool(rows32))      # pv blocks of 32 rows, written whole (see include/xaac_hbe.h)
        b.pv_re = _ptr(pv_re, "float32", n_ch * (32 if rows32 else 34) * 64, device_ok=True)
        b.pv_im = _ptr(pv_im, "float32", n_ch * (32 if rows32 else 34) * 64, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, device_ok=True)
        self._call("xaac_hbe_dft_apply_batch_run", ctypes.byref(b))

    def pvc_process_batch(self, frame, qmf_re, qmf_im, state, out, status=None):
        """Batched PVC envelope decoder (ixheaacd_qmf_enrg_calc + ixheaacd_pvc_process): frame uint8[n_ch, PVC_FRAME_BYTES];
        qmf_re / qmf_im float32[n_ch, rows, 64] (row 2 of the QMF buffers onwards; rows >= 32, and >= 64 for batches that hold
        pvc_rate 4 frames: on fewer rows such a frame is refused with status -1); state uint8[n_ch, PVC_STATE_BYTES]
        in/out; out float32[n_ch, 16, 64]; status int32[n_ch] or None."""
        n_ch = state.shape[0]
        b = PvcBatch()
        if qmf_re.dim() != 3 or qmf_re.shape[2] != 64 or qmf_re.shape[1] < 32 or tuple(qmf_im.shape) != tuple(qmf_re.shape):
            raise ValueError("qmf_re / qmf_im must be [n_ch, rows >= 32, 64] and alike")
        b.n_ch, b.qmf_stride = n_ch, int(qmf_re.shape[1]) * int(qmf_re.shape[2])
        b.frame = _ptr(frame, "uint8", n_ch * PVC_FRAME_BYTES, device_ok=True)
        b.qmf_re = _ptr(qmf_re, "float32", n_ch * b.qmf_stride, device_ok=True)
        b.qmf_im = _ptr(qmf_im, "float32", n_ch * b.qmf_stride, device_ok=True)
        b.state = _ptr(state, "uint8", n_ch * PVC_STATE_BYTES, device_ok=True)
        b.out = _ptr(out, "float32", n_ch * 16 * 64, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, device_ok=True) if status is not None else None
        self._call("xaac_pvc_process_batch", ctypes.byref(b))

    def hbe_cplx_anal_batch(self, state, status=None):
        """Batched ixheaacd_complex_anal_filt (the harmonic transposer's complex analysis bank): state
        uint8[n_ch, HBE_STATE_BYTES] in/out; status int32[n_ch] or None."""
        n_ch = state.shape[0]
        b = HbeAnalBatch()
        b.n_ch = n_ch
        b.state = _ptr(state, "uint8", n_ch * HBE_STATE_BYTES, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, device_ok=True) if status is not None else None
        self._call("xaac_hbe_cplx_anal_batch", ctypes.byref(b))

    def qmf_analysis_eld_batch(self, pcm, state, qmf, n_slots, usb, status=None):
        """Batched LD / ELD complex analysis bank: pcm int16[n_ch, 32 * n_slots]; state int16[n_ch, 324] in/out (ring, wr,
        f1, f2, fp; a new stream: zeros with f2 = 32); qmf int32[n_ch, n_slots, slot_stride >= 96]."""
        n_ch = state.shape[0]
        b = QmfAnaEldBatch()
        b.n_ch, b.n_slots, b.usb, b.slot_stride = n_ch, n_slots, usb, int(qmf.shape[2])
        b.pcm = _ptr(pcm, "int16", n_ch * 32 * n_slots, device_ok=True)
        b.state = _ptr(state, "int16", n_ch * QMF_ANA_ELD_STATE_WORDS, device_ok=True)
        b.qmf = _ptr(qmf, "int32", n_ch * n_slots * b.slot_stride, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, device_ok=True) if status is not None else None
        self._call("xaac_qmf_analysis_eld_batch", ctypes.byref(b))

    def qmf_synthesis_eld_batch(self, qmf, scale, state, pcm, n_slots, lsb, usb, split, status=None, qmf_scaled=None):
        """Batched LD / ELD complex synthesis bank: qmf int32[n_ch, n_slots, slot_stride >= 128]; scale int16[n_ch, 4] (lb,
        ov_lb, hb, st_syn); state int16[n_ch, 1284] in/out (ring, drc_offset, phase, fp, sixty4; a new stream: zeros with
        sixty4 = 64); pcm int16[n_ch, 64 * n_slots]."""
        n_ch = state.shape[0]
        b = QmfSynEldBatch()
        b.n_ch, b.n_slots, b.lsb, b.usb, b.split, b.slot_stride = n_ch, n_slots, lsb, usb, split, int(qmf.shape[2])
        b.qmf = _ptr(qmf, "int32", n_ch * n_slots * b.slot_stride, device_ok=True)
        b.scale = _ptr(scale, "int16", n_ch * 4, device_ok=True)
        b.state = _ptr(state, "int16", n_ch * QMF_SYN_ELD_STATE_WORDS, device_ok=True)
        b.pcm = _ptr(pcm, "int16", n_ch * 64 * n_slots, device_ok=True)
        b.status = _ptr(status, "int32", n_ch, device_ok=True) if status is not None else None
        b.qmf_scaled = _ptr(qmf_scaled, "int32", n_ch * n_slots * b.slot_stride, allow_none=True, device_ok=True)
        self._call("xaac_qmf_synthesis_eld_batch", ctypes.byref(b))

    def esbr_qmf_analysis_batch(self, core, state, qmf_re, qmf_im):
        """Batched ixheaacd_esbr_analysis_filt_block (eSBR / Path A, 32 channels): core float32[n_ch, 1024];
        state int32[n_ch, 322] in/out (ring, pos, win_off); qmf_re / qmf_im float32[n_ch, 32, 64], bands 0..31 written."""
        n_ch = state.shape[0]
        b = EsbrAnaBatch()
        b.n_ch = n_ch
        b.core = _ptr(core, "float32", n_ch * 1024, device_ok=True)
        b.state = _ptr(state, "int32", n_ch * ESBR_ANA_STATE_WORDS, device_ok=True)
        b.qmf_re = _ptr(qmf_re, "float32", n_ch * 2048, device_ok=True)
        b.qmf_im = _ptr(qmf_im, "float32", n_ch * 2048, device_ok=True)
        self._call("xaac_esbr_qmf_analysis_batch", ctypes.byref(b))

    def esbr_qmf_analysis_nb_batch(self, n_bands, n_slots, core, state, qmf_re, qmf_im):
        """The 24- / 16-channel analysis banks of 8:3 / 4:1 SBR (sbr_dec.c:213-236): core float32[n_ch, core_stride];
        state int32[n_ch, 322] in/out; qmf_re / qmf_im float32[n_ch, n_slots, 64]."""
        n_ch = state.shape[0]
        b = EsbrAnaNbBatch()
        b.n_ch, b.n_bands, b.n_slots = n_ch, n_bands, n_slots
        b.core_stride = int(core.shape[1])
        b.core = _ptr(core, "float32", n_ch * b.core_stride, device_ok=True)
        b.state = _ptr(state, "int32", n_ch * ESBR_ANA_STATE_WORDS, device_ok=True)
        b.qmf_re = _ptr(qmf_re, "float32", n_ch * n_slots * 64, device_ok=True)
        b.qmf_im = _ptr(qmf_im, "float32", n_ch * n_slots * 64, device_ok=True)
        self._call("xaac_esbr_qmf_analysis_nb_batch", ctypes.byref(b))

    def esbr_qmf_synthesis_batch(self, qmf_re, qmf_im, state, out):
        """Batched synthesis bank of ixheaacd_esbr_synthesis_filt_block (eSBR / Path A, 64 channels):
        qmf_re / qmf_im float32[n_ch, 32, 64]; state int32[n_ch, 1282] in/out (ring, drc_offset, filt_off);
        out float32[n_ch, 2048]."""
        n_ch = state.shape[0]
        b = EsbrSynBatch()
        b.n_ch = n_ch
        b.qmf_re = _ptr(qmf_re, "float32", n_ch * 2048, device_ok=True)
        b.qmf_im = _ptr(qmf_im, "float32", n_ch * 2048, device_ok=True)
        b.state = _ptr(state, "int32", n_ch * ESBR_SYN_STATE_WORDS, device_ok=True)
        b.out = _ptr(out, "float32", n_ch * 2048, device_ok=True)
        self._call("xaac_esbr_qmf_synthesis_batch", ctypes.byref(b))

    def esbr_qmf_synthesis_ds_batch(self, qmf_re, qmf_im, state, out):
        """The same bank down-sampled (32 synthesis channels, sbr_dec.c:605-628): out float32[n_ch, 1024]."""
        n_ch = state.shape[0]
        b = EsbrSynBatch()
        b.n_ch = n_ch
        b.qmf_re = _ptr(qmf_re, "float32", n_ch * 2048, device_ok=True)
        b.qmf_im = _ptr(qmf_im, "float32", n_ch * 2048, device_ok=True)
        b.state = _ptr(state, "int32", n_ch * ESBR_SYN_STATE_WORDS, device_ok=True)
        b.out = _ptr(out, "float32", n_ch * 1024, device_ok=True)
        self._call("xaac_esbr_qmf_synthesis_ds_batch", ctypes.byref(b))

    def sbr_eld_workspace_bytes(self, n_ch):
        return int(self._lib.xaac_sbr_eld_workspace_bytes(int(n_ch)))

    def sbr_eld_process_batch(self, pcm_in, header, frame, state, pcm_out, workspace, n_slots, status=None, in_ch_fac=1,
                              out_ch_fac=1, qmf_handed_on=None):
        """Batched ixheaacd_sbr_dec for AAC-ELD channels (low-delay SBR): pcm_in int16[n_ch * 32 n_slots], state
        uint8[n_ch, SBR_ELD_STATE_BYTES] (xaac_sbr_eld_state), pcm_out int16[n_ch * 64 n_slots]; n_slots 16 or 15"""
        n_ch = state.shape[0]
        b = SbrEldBatch()
        b.n_ch, b.n_slots, b.in_ch_fac, b.out_ch_fac = n_ch, int(n_slots), int(in_ch_fac), int(out_ch_fac)
        b.pcm_in = _ptr(pcm_in, "int16", n_ch * 32 * int(n_slots), device_ok=True)
        b.header = _ptr(header, "uint8", n_ch * SBR_HEADER_BYTES, device_ok=True)
        b.frame = _ptr(frame, "uint8", n_ch * SBR_FRAME_BYTES, device_ok=True)
        b.state = _ptr(state, "uint8", n_ch * SBR_ELD_STATE_BYTES, device_ok=True)
        b.pcm_out = _ptr(pcm_out, "int16", n_ch * 64 * int(n_slots), device_ok=True)
        b.status = _ptr(status, "int32", n_ch, allow_none=True, device_ok=True)
        b.workspace = _ptr(workspace, "uint8", device_ok=True)
        b.workspace_bytes = workspace.numel()
        b.qmf_handed_on = _ptr(qmf_handed_on, "int32", n_ch * int(n_slots) * 128, allow_none=True, device_ok=True)
        self._call("xaac_sbr_eld_process_batch", ctypes.byref(b))

    def sbr_hq_workspace_bytes(self, n_ch, with_ps=True):
        return int(self._lib.xaac_sbr_hq_workspace_bytes(int(n_ch), int(bool(with_ps))))

    def _sbr_hq_batch(self, pcm_in, header, frame, state, pcm_out, workspace, ps_frame, ps_state, status, in_ch_fac, out_ch_fac,
                      down_sample, max_band_hint, frame_in):
        n_ch = state.shape[0]
        with_ps = ps_frame is not None
        b = SbrHqBatch()
        b.n_ch, b.in_ch_fac, b.out_ch_fac = n_ch, int(in_ch_fac), int(out_ch_fac)
        b.down_sample = int(bool(down_sample))
        b.pcm_in = _ptr(pcm_in, "int16", n_ch * frame_in, device_ok=True)
        b.header = _ptr(header, "uint8", n_ch * SBR_HEADER_BYTES, device_ok=True)
        b.frame = _ptr(frame, "uint8", n_ch * SBR_FRAME_BYTES, device_ok=True)
        b.state = _ptr(state, "uint8", n_ch * SBR_STATE_BYTES, device_ok=True)
        b.ps_frame = _ptr(ps_frame, "uint8", n_ch * PS_FRAME_BYTES, allow_none=True, device_ok=True)
        b.ps_state = _ptr(ps_state, "uint8", n_ch * PS_STATE_BYTES, allow_none=True, device_ok=True)
        b.pcm_out = _ptr(pcm_out, "int16", n_ch * (frame_in if down_sample else 2 * frame_in) * (2 if with_ps else 1), device_ok=True)
        b.status = _ptr(status, "int32", n_ch, allow_none=True, device_ok=True)
        b.workspace = _ptr(workspace, "uint8", device_ok=True)
        b.workspace_bytes = workspace.numel()
        b.max_band_hint = int(max_band_hint)   # 48: no stream of the batch reaches above QMF band 48 (xaac_amd.h); 0: no assertion
        return b

    def sbr_hq_process_batch(self, pcm_in, header, frame, state, pcm_out, workspace, ps_frame=None, ps_state=None,
                             status=None, in_ch_fac=1, out_ch_fac=1, down_sample=False, max_band_hint=0):
        """Batched ixheaacd_sbr_dec, HQ mode: one frame per stream.  With ps_frame / ps_state (uint8[n, PS_*_BYTES])
        the parametric-stereo tool runs too (HE-AACv2) and pcm_out is int16[n*2048*2] of L,R pairs; without them
        pcm_out is int16[n*2048] (HE-AAC mono, HQ)."""
        b = self._sbr_hq_batch(pcm_in, header, frame, state, pcm_out, workspace, ps_frame, ps_state, status, in_ch_fac,
                               out_ch_fac, down_sample, max_band_hint, 1024)
        self._call("xaac_sbr_hq_process_batch", ctypes.byref(b))

    def sbr_hq960_process_batch(self, pcm_in, header, frame, state, pcm_out, workspace, ps_frame=None, ps_state=None,
                                status=None, in_ch_fac=1, out_ch_fac=1, down_sample=False, max_band_hint=0):
        """The same for 960-sample cores (DAB+ / DRM HE-AAC mono and HE-AACv2: 15 time slots, 30 QMF slots a frame):
        pcm_in int16[n*960], pcm_out int16[n*1920] (x 2 with PS); the workspace of sbr_hq_workspace_bytes.  down_sample is
        refused (XAAC_FATAL_BAD_ARG)."""
        b = self._sbr_hq_batch(pcm_in, header, frame, state, pcm_out, workspace, ps_frame, ps_state, status, in_ch_fac,
                               out_ch_fac, down_sample, max_band_hint, 960)
        self._call("xaac_sbr_hq960_process_batch", ctypes.byref(b))

    def peak_limiter_workspace_bytes(self, n_streams):
        return int(self._lib.xaac_peak_limiter_workspace_bytes(int(n_streams)))

    def peak_limiter_process_map_batch(self, samples, qshift_adj, state, num_channels, workspace, pcm16, out_map, frame_len=1024,
                                       stride=None, status=None, planar=False):
        """peak_limiter_process_batch with an output map (an OutMap: out_map()) on the PCM16 hand-off: pcm16
        int16[n_streams * frame_len * mapped channels]; samples and state come out as from the unmapped call."""
        n = state.shape[0]
        if stride is None:
            stride = frame_len * num_channels
        mb = LimiterMapBatch()
        b = mb.lim
        b.n_streams, b.frame_len, b.num_channels, b.stride = n, int(frame_len), int(num_channels), int(stride)
        b.planar = int(bool(planar))
        b.samples = _ptr(samples, "int32", n * stride, device_ok=True)
        b.qshift_adj = _ptr(qshift_adj, "int8", n * num_channels, device_ok=True)
        b.state = _ptr(state, "uint8", n * LIMITER_STATE_BYTES, device_ok=True)
        b.pcm16 = _ptr(pcm16, "int16", n * frame_len * max(1, out_map_channels(out_map, num_channels)), device_ok=True)
        b.status = _ptr(status, "int32", n, allow_none=True, device_ok=True)
        b.workspace = _ptr(workspace, "uint8", device_ok=True)
        b.workspace_bytes = workspace.numel()
        mb.map = out_map
        self._call("xaac_peak_limiter_process_map_batch", ctypes.byref(mb))

    def pcm16_scale_adjust_map_batch(self, samples, qshift_adj, num_channels, pcm16, out_map=None, frame_len=1024, stride=None,
                                     planar=False):
        """The limiter-off hand-off (ixheaacd_scale_adjust + round16) with an optional output map: samples
        int32[n_streams * stride] (planar or interleaved), qshift_adj int8[n_streams * num_channels] -> pcm16
        int16[n_streams * frame_len * mapped channels]."""
        n = qshift_adj.numel() // num_channels
        if stride is None:
            stride = frame_len * num_channels
        b = ScaleAdjustMapBatch()
        b.n_streams, b.frame_len, b.num_channels, b.stride = n, int(frame_len), int(num_channels), int(stride)
        b.planar = int(bool(planar))
        if out_map is not None:
            b.map = out_map
        b.samples = _ptr(samples, "int32", n * stride, device_ok=True)
        b.qshift_adj = _ptr(qshift_adj, "int8", n * num_channels, device_ok=True)
        b.pcm16 = _ptr(pcm16, "int16", n * frame_len * max(1, out_map_channels(b.map, num_channels)), device_ok=True)
        self._call("xaac_pcm16_scale_adjust_map_batch", ctypes.byref(b))

    def peak_limiter_process_batch(self, samples, qshift_adj, state, num_channels, workspace, frame_len=1024,
                                   pcm16=None, stride=None, status=None, planar=False):
        """Batched ixheaacd_peak_limiter_process (+ the round16 hand-off): one frame of every stream.
        samples int32[n_streams * stride] in/out, frame_len x num_channels interleaved per stream (what
        imdct_process_batch leaves in out32); qshift_adj int8[n_streams * num_channels]; state
        uint8[n_streams, LIMITER_STATE_BYTES] in/out (peak_limiter_init() makes one); pcm16 optional
        int16[n_streams * frame_len * num_channels]; workspace uint8[>= peak_limiter_workspace_bytes(n_streams)]."""
        n = state.shape[0]
        if stride is None:
            stride = frame_len * num_channels
        b = LimiterBatch()
        b.n_streams, b.frame_len, b.num_channels, b.stride = n, int(frame_len), int(num_channels), int(stride)
        b.planar = int(bool(planar))
        b.samples = _ptr(samples, "int32", n * stride, device_ok=True)
        b.qshift_adj = _ptr(qshift_adj, "int8", n * num_channels, device_ok=True)
        b.state = _ptr(state, "uint8", n * LIMITER_STATE_BYTES, device_ok=True)
        b.pcm16 = _ptr(pcm16, "int16", n * frame_len * num_channels, allow_none=True, device_ok=True)
        b.status = _ptr(status, "int32", n, allow_none=True, device_ok=True)
        b.workspace = _ptr(workspace, "uint8", device_ok=True)
        b.workspace_bytes = workspace.numel()
        self._call("xaac_peak_limiter_process_batch", ctypes.byref(b))

    def sbr_lp_workspace_bytes(self, n_ch):
        return int(self._lib.xaac_sbr_lp_workspace_bytes(int(n_ch)))

    def _sbr_lp_batch(self, pcm_in, header, frame, state, pcm_out, workspace, status, in_ch_fac, out_ch_fac, down_sample,
                      frame_in):
        n_ch = state.shape[0]
        b = SbrLpBatch()
        b.n_ch, b.in_ch_fac, b.out_ch_fac = n_ch, int(in_ch_fac), int(out_ch_fac)
        b.down_sample = int(bool(down_sample))
        b.pcm_in = _ptr(pcm_in, "int16", n_ch * frame_in, device_ok=True)
        b.header = _ptr(header, "uint8", n_ch * SBR_HEADER_BYTES, device_ok=True)
        b.frame = _ptr(frame, "uint8", n_ch * SBR_FRAME_BYTES, device_ok=True)
        b.state = _ptr(state, "uint8", n_ch * SBR_STATE_BYTES, device_ok=True)
        b.pcm_out = _ptr(pcm_out, "int16", n_ch * (frame_in if down_sample else 2 * frame_in), device_ok=True)
        b.status = _ptr(status, "int32", n_ch, allow_none=True, device_ok=True)
        b.workspace = _ptr(workspace, "uint8", device_ok=True)
        b.workspace_bytes = workspace.numel()
        return b

    def sbr_lp_process_batch(self, pcm_in, header, frame, state, pcm_out, workspace, status=None, in_ch_fac=1,
                             out_ch_fac=1, down_sample=False):
        """Batched ixheaacd_sbr_dec, low-power mode (HE-AACv1): one frame per channel.
        pcm_in int16[n_ch*1024]; header/frame/state uint8[n_ch, SBR_*_BYTES] (structs of include/xaac_sbr.h,
        state in/out); pcm_out int16[n_ch*2048]; workspace uint8[>= sbr_lp_workspace_bytes(n_ch)];
        status optional int32[n_ch]."""
        b = self._sbr_lp_batch(pcm_in, header, frame, state, pcm_out, workspace, status, in_ch_fac, out_ch_fac, down_sample,
                               1024)
        self._call("xaac_sbr_lp_process_batch", ctypes.byref(b))

    def sbr_lp960_process_batch(self, pcm_in, header, frame, state, pcm_out, workspace, status=None, in_ch_fac=1,
                                out_ch_fac=1, down_sample=False):
        """The same for 960-sample cores (DAB+ / DRM: 15 time slots, 30 QMF slots a frame): pcm_in int16[n_ch*960],
        pcm_out int16[n_ch*1920]; the workspace of sbr_lp_workspace_bytes(n_ch).  down_sample is refused (XAAC_FATAL_BAD_ARG)."""
        b = self._sbr_lp_batch(pcm_in, header, frame, state, pcm_out, workspace, status, in_ch_fac, out_ch_fac, down_sample,
                               960)
        self._call("xaac_sbr_lp960_process_batch", ctypes.byref(b))


def decode_mixed(streams, **kwargs):
    """libxaac_amd.decoder.decode_mixed: ADTS streams of several kinds in one call -> (PCM arrays, output rates), both in the
    order of `streams`.  (The decoder module builds on this one, so it is imported by the first call.)"""
    from . import decoder
    return decoder.decode_mixed(streams, **kwargs)
