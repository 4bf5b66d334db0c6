"""libxaac_amd.abi -- the Python statement of the C boundary (include/*.h): one ctypes mirror per struct, registered under
its C type name in STRUCTS, the prototypes of the device library's entry points (BATCH_ENTRY_POINTS,
OTHER_ENTRY_POINTS; bind() applies them) and of the host library's (HOST_ENTRY_POINTS; bind_host()), and the positions of the
parser's flag row (F_*).  Sizes are never restated beside it: callers take ctypes.sizeof of a mirror.
tests/test_abi.py holds every mirror's size and every field's offset and size against what a C compiler makes of the headers.
"""
import ctypes

I8, U8, I16, U16, I32, U32, I64, U64 = (ctypes.c_int8, ctypes.c_uint8, ctypes.c_int16, ctypes.c_uint16, ctypes.c_int32,
                                        ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64)
F32, F64, PTR = ctypes.c_float, ctypes.c_double, ctypes.c_void_p

STRUCTS = {}   # C type name -> mirror


def _mirror(c_name):
    def register(cls):
        cls.c_name = c_name
        STRUCTS[c_name] = cls
        return cls
    return register


# ---- include/xaac_sbr.h
# enum xaac_sbr_flag, the parser's flag row: XAAC_SBR_FLAG_<name> is the name's place here, XAAC_SBR_FLAG_WORDS their number
# (tests/test_abi.py holds both against the header)
SBR_FLAG_NAMES = ("APPLY", "RESET", "RESET_CHANNELS", "UPSAMPLING", "STEREO", "PS", "PS_START", "FRAME_OK")
SBR_FLAG_WORDS = len(SBR_FLAG_NAMES)
F_APPLY, F_RESET, F_RESET_CHANNELS, F_UPSAMPLING, F_STEREO, F_PS, F_PS_START, F_FRAME_OK = range(SBR_FLAG_WORDS)


@_mirror("xaac_sbr_patch")
class SbrPatch(ctypes.Structure):
    _fields_ = [(n, I16) for n in ("src_start_band", "src_end_band", "guard_start_band", "dst_start_band",
                                   "dst_end_band", "num_bands_in_patch")]


@_mirror("xaac_sbr_header")
class SbrHeader(ctypes.Structure):
    _fields_ = [("num_time_slots", I16), ("time_step", I16), ("channel_mode", I16), ("limiter_gains", I16),
                ("interpol_freq", I16), ("smoothing_mode", I16), ("num_sf_bands", I16 * 2), ("num_nf_bands", I16),
                ("sub_band_start", I16), ("sub_band_end", I16), ("num_lf_bands", I16), ("num_if_bands", I16),
                ("freq_band_tbl_lim", I16 * 13), ("freq_band_tbl_lo", I16 * 29), ("freq_band_tbl_hi", I16 * 57),
                ("freq_band_tbl_noise", I16 * 6), ("num_columns", I16), ("num_patches", I16), ("start_patch", I16),
                ("stop_patch", I16), ("bw_borders", I16 * 10), ("patch", SbrPatch * 6)]


@_mirror("xaac_sbr_frame")
class SbrFrame(ctypes.Structure):
    _fields_ = [("num_env", I16), ("transient_env", I16), ("num_noise_env", I16), ("frame_class", I16),
                ("border_vec", I16 * 9), ("freq_res", I16 * 8), ("noise_border_vec", I16 * 3), ("amp_res", I16),
                ("apply_processing", I16), ("coupling_mode", I32), ("max_qmf_subband_aac", I32),
                ("sbr_invf_mode", I32 * 10), ("add_harmonics", U8 * 56), ("int_env_sf_arr", I16 * 448),
                ("int_noise_floor", I16 * 10)]


@_mirror("xaac_sbr_state")
class SbrState(ctypes.Structure):
    _fields_ = [("ana_ring", I16 * 320), ("ana_wr", I16), ("ana_phase", I16), ("syn_ring", I16 * 1280),
                ("syn_drc_offset", I16), ("syn_phase", I16), ("codec_usb", I16), ("syn_lsb", I16), ("syn_usb", I16), ("pad2_", I16),
                ("overlap", I32 * 768), ("lpc_real", (I32 * 32) * 2),
                ("lpc_imag", (I32 * 32) * 2), ("bw_array_prev", I32 * 6), ("lb_scale", I16), ("st_lb_scale", I16),
                ("ov_lb_scale", I16), ("hb_scale", I16), ("ov_hb_scale", I16), ("st_syn_scale", I16),
                ("ps_scale", I16), ("pad0_", I16), ("prev_invf_mode", I32 * 10), ("prev_max_qmf_subband_aac", I32),
                ("prev_coupling_mode", I32), ("prev_end_position", I16), ("prev_amp_res", I16),
                ("filt_buf_me", I16 * 112), ("filt_buf_noise_m", I16 * 56), ("filt_buf_noise_e", I32),
                ("start_up", I32), ("ph_index", I16), ("tansient_env_prev", I16), ("harm_index", I16), ("pad1_", I16),
                ("harm_flags_prev", I8 * 56)]


@_mirror("xaac_ps_frame")
class PsFrame(ctypes.Structure):
    _fields_ = [("iid_quant", I16), ("freq_res_ipd", I16), ("border_position", I16 * 7), ("num_env", I16),
                ("iid_par_table", (I16 * 34) * 7), ("icc_par_table", (I16 * 34) * 7)]


@_mirror("xaac_ps_state")
class PsState(ctypes.Structure):
    _fields_ = [("ser", ((I16 * 64) * 3) * 5), ("ap", (I16 * 64) * 2), ("ld", (I16 * 24) * 14), ("sd", I16 * 64),
                ("sub", (I16 * 32) * 2), ("sub_ser", ((I16 * 32) * 3) * 5), ("idx_ser", I16 * 3), ("sample_ser", I16 * 3),
                ("idx", I16), ("idx_long", I16), ("peak_decay_diff", I32 * 20), ("energy_prev", I32 * 20),
                ("peak_decay_diff_prev", I32 * 20), ("hyb_buf", ((I32 * 12) * 2) * 3), ("h11_h12_vec", I16 * 48),
                ("h21_h22_vec", I16 * 48), ("H11_H12", I16 * 48), ("H21_H22", I16 * 48), ("delta_h11_h12", I16 * 48),
                ("delta_h21_h22", I16 * 48), ("delay_buffer_scale", I16), ("usb", I16), ("syn_ring_r", I16 * 1280),
                ("syn_drc_offset_r", I16), ("syn_phase_r", I16), ("syn_lsb_r", I16), ("syn_usb_r", I16),
                ("st_syn_scale_r", I16), ("lb_scale_r", I16), ("ov_lb_scale_r", I16), ("hb_scale_r", I16)]


# ---- include/xaac_amd.h
@_mirror("xaac_ics_info")
class IcsInfo(ctypes.Structure):
    _fields_ = [("window_sequence", U8), ("window_shape", U8)]


@_mirror("xaac_ovl_state")
class OvlState(ctypes.Structure):
    _fields_ = [("window_sequence", U8), ("window_shape", U8)]


@_mirror("xaac_imdct_batch")
class ImdctBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("ch_fac", I32), ("spec", PTR), ("ics", PTR), ("overlap", PTR), ("state", PTR), ("out32", PTR),
                ("pcm16", PTR), ("qshift_adj", PTR), ("pcm_mode", I32), ("status", PTR)]


@_mirror("xaac_imdct_ld_batch")
class ImdctLdBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("ch_fac", I32), ("frame_length", I32), ("eld", I32), ("spec", PTR), ("window_shape", PTR),
                ("overlap", PTR), ("shape_prev", PTR), ("pcm16", PTR), ("status", PTR)]


@_mirror("xaac_qmf_ana_state")
class QmfAnaState(ctypes.Structure):
    _fields_ = [("ring", I16 * 320), ("wr", I16), ("phase", I16)]


@_mirror("xaac_qmf_syn_state")
class QmfSynState(ctypes.Structure):
    _fields_ = [("ring", I16 * 1280), ("drc_offset", I16), ("phase", I16)]


@_mirror("xaac_qmf_ana_eld_state")
class QmfAnaEldState(ctypes.Structure):
    _fields_ = [("ring", I16 * 320), ("wr", I16), ("f1", I16), ("f2", I16), ("fp", I16)]


@_mirror("xaac_qmf_syn_eld_state")
class QmfSynEldState(ctypes.Structure):
    _fields_ = [("ring", I16 * 1280), ("drc_offset", I16), ("phase", I16), ("fp", I16), ("sixty4", I16)]


@_mirror("xaac_qmf_ana_eld_batch")
class QmfAnaEldBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("n_slots", I32), ("usb", I32), ("slot_stride", I32), ("pcm", PTR), ("state", PTR), ("qmf", PTR),
                ("status", PTR)]


@_mirror("xaac_qmf_syn_eld_batch")
class QmfSynEldBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("n_slots", I32), ("lsb", I32), ("usb", I32), ("split", I32), ("slot_stride", I32), ("qmf", PTR),
                ("scale", PTR), ("state", PTR), ("pcm", PTR), ("status", PTR), ("qmf_scaled", PTR)]


@_mirror("xaac_qmf_ana_batch")
class QmfAnaBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("ch_fac", I32), ("low_pow", I32), ("usb", I32), ("slot_stride", I32), ("pcm", PTR),
                ("state", PTR), ("qmf", PTR)]


@_mirror("xaac_qmf_syn_batch")
class QmfSynBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("ch_fac", I32), ("low_pow", I32), ("lsb", I32), ("usb", I32), ("split", I32),
                ("slot_stride", I32), ("down_sample", I32), ("qmf", PTR), ("scale", PTR), ("state", PTR), ("pcm", PTR)]


@_mirror("xaac_sbr_lp_batch")
class SbrLpBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("in_ch_fac", I32), ("out_ch_fac", I32), ("down_sample", I32), ("pcm_in", PTR), ("header", PTR),
                ("frame", PTR), ("state", PTR), ("pcm_out", PTR), ("status", PTR), ("workspace", PTR), ("workspace_bytes", U64)]


@_mirror("xaac_sbr_hq_batch")
class SbrHqBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("in_ch_fac", I32), ("out_ch_fac", I32), ("down_sample", I32), ("pcm_in", PTR), ("header", PTR),
                ("frame", PTR), ("state", PTR), ("ps_frame", PTR), ("ps_state", PTR), ("pcm_out", PTR), ("status", PTR),
                ("workspace", PTR), ("workspace_bytes", U64), ("max_band_hint", I32)]


@_mirror("xaac_sbr_eld_state")
class SbrEldState(ctypes.Structure):   # the low-delay banks in front of xaac_sbr_state's tail (XAAC_SBR_STATE_TAIL_FIELDS)
    _fields_ = [("ana", QmfAnaEldState), ("syn", QmfSynEldState), ("codec_usb", I16), ("syn_lsb", I16), ("syn_usb", I16),
                ("pad2_", I16)] + SbrState._fields_[SbrState._fields_.index(("lpc_real", (I32 * 32) * 2)):]


@_mirror("xaac_sbr_eld_batch")
class SbrEldBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("n_slots", I32), ("in_ch_fac", I32), ("out_ch_fac", I32), ("pcm_in", PTR), ("header", PTR),
                ("frame", PTR), ("state", PTR), ("pcm_out", PTR), ("status", PTR), ("workspace", PTR), ("workspace_bytes", U64),
                ("qmf_handed_on", PTR)]


@_mirror("xaac_sbr_handover_batch")
class HandoverBatch(ctypes.Structure):
    _fields_ = [("n", I32), ("mode", I32), ("src", PTR), ("dst", PTR), ("state", PTR), ("ps_state", PTR)]


@_mirror("xaac_sbr_apply_side_batch")
class ApplySideBatch(ctypes.Structure):
    _fields_ = [("n_streams", I32), ("ch_fac", I32), ("header", PTR), ("flags", PTR), ("state", PTR), ("ps_state", PTR)]


LIM_MAX_ATTACK, LIM_MAX_CH = 480, 8


@_mirror("xaac_limiter_state")
class LimiterState(ctypes.Structure):   # ia_peak_limiter_struct with its buffers inline
    _fields_ = [("attack_constant", F32), ("release_constant", F32), ("num_channels", U32), ("attack_time_samples", U32),
                ("limiter_on", U32), ("gain_modified", F32), ("min_gain", F32), ("delayed_input_index", U32),
                ("pre_smoothed_gain", F64), ("max_idx", I32), ("cir_buf_pnt", I32), ("max_buf", F32 * LIM_MAX_ATTACK),
                ("delayed_input", F32 * (LIM_MAX_ATTACK * LIM_MAX_CH))]


@_mirror("xaac_limiter_batch")
class LimiterBatch(ctypes.Structure):
    _fields_ = [("n_streams", I32), ("frame_len", I32), ("samples", PTR), ("stride", I64), ("qshift_adj", PTR), ("state", PTR),
                ("num_channels", I32), ("planar", I32), ("pcm16", PTR), ("status", PTR), ("workspace", PTR),
                ("workspace_bytes", U64)]


@_mirror("xaac_out_map")
class OutMap(ctypes.Structure):
    _fields_ = [("kind", I32), ("matrix", I32), ("n_elements", I32), ("element_type", I32 * 4), ("element_slot", I32 * 4)]


@_mirror("xaac_limiter_map_batch")
class LimiterMapBatch(ctypes.Structure):
    _fields_ = [("lim", LimiterBatch), ("map", OutMap)]


@_mirror("xaac_scale_adjust_map_batch")
class ScaleAdjustMapBatch(ctypes.Structure):
    _fields_ = [("n_streams", I32), ("frame_len", I32), ("num_channels", I32), ("planar", I32), ("samples", PTR), ("stride", I64),
                ("qshift_adj", PTR), ("pcm16", PTR), ("map", OutMap)]


@_mirror("xaac_esbr_ana_state")
class EsbrAnaState(ctypes.Structure):
    _fields_ = [("ring", I32 * 320), ("pos", I32), ("win_off", I32)]


@_mirror("xaac_esbr_syn_state")
class EsbrSynState(ctypes.Structure):
    _fields_ = [("ring", I32 * 1280), ("drc_offset", I32), ("filt_off", I32)]


@_mirror("xaac_esbr_ana_batch")
class EsbrAnaBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("core", PTR), ("state", PTR), ("qmf_re", PTR), ("qmf_im", PTR)]


@_mirror("xaac_esbr_ana_nb_batch")
class EsbrAnaNbBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("n_bands", I32), ("n_slots", I32), ("core_stride", I32), ("core", PTR), ("state", PTR),
                ("qmf_re", PTR), ("qmf_im", PTR)]


@_mirror("xaac_esbr_syn_batch")
class EsbrSynBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("qmf_re", PTR), ("qmf_im", PTR), ("state", PTR), ("out", PTR)]


@_mirror("xaac_usac_ics")
class UsacIcs(ctypes.Structure):
    _fields_ = [("window_sequence", U8), ("window_shape", U8)]


@_mirror("xaac_usac_fac")
class UsacFac(ctypes.Structure):
    _fields_ = [("q", I32), ("data", I32 * 256)]


@_mirror("xaac_usac_fac_in")
class UsacFacIn(ctypes.Structure):
    _fields_ = [("fac_data", I32 * 129), ("lpc_prev", F32 * 17), ("acelp_in", F32 * 256)]


@_mirror("xaac_usac_imdct_batch")
class UsacImdctBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("ccfl", I32), ("coef", PTR), ("ics", PTR), ("overlap", PTR), ("shape_prev", PTR), ("out32", PTR),
                ("time", PTR), ("status", PTR), ("lpd_flags", PTR), ("fac", PTR), ("fac_in", PTR), ("fac_work", PTR)]


@_mirror("xaac_aac_tools_batch")
class AacToolsBatch(ctypes.Structure):
    _fields_ = [("n", I32), ("spec_stride", I32), ("spec", PTR), ("side", PTR), ("state", PTR), ("status", PTR)]


# ---- include/xaac_drc.h
@_mirror("xaac_drc_config")
class DrcConfig(ctypes.Structure):
    _fields_ = [("cut", I32), ("boost", I32), ("target_level", I32)]


@_mirror("xaac_drc_side")
class DrcSide(ctypes.Structure):   # one channel-frame's bands and Q25 gain factors
    _fields_ = [("n_bands", I32), ("end", I32 * 16), ("fac", I32 * 16)]


@_mirror("xaac_drc_batch")
class DrcBatch(ctypes.Structure):
    _fields_ = [("n", I32), ("spec_stride", I32), ("spec", PTR), ("side", PTR), ("status", PTR)]


# ---- include/xaac_tools.h
@_mirror("xaac_tns_filter_side")
class TnsFilterSide(ctypes.Structure):
    _fields_ = [("start_band", U8), ("stop_band", U8), ("order", I8), ("direction", I8), ("resolution", U8), ("reserved", U8 * 3),
                ("coef", I8 * 12)]


@_mirror("xaac_core_tools_channel")
class CoreToolsChannel(ctypes.Structure):
    _fields_ = [("window_sequence", U8), ("max_sfb", U8), ("num_groups", U8), ("pns_active", U8), ("tns_present", U8), ("wide", U8),
                ("reserved", U8 * 2), ("group_len", U8 * 8), ("n_filt", U8 * 8), ("cb", U8 * 128), ("sf", I16 * 128),
                ("pns_used", U8 * 128), ("tns", TnsFilterSide * 8)]


@_mirror("xaac_core_tools_side")
class CoreToolsSide(ctypes.Structure):   # what the M/S, intensity, PNS and TNS tools read of one channel element
    _fields_ = [("element_id", U8), ("n_ch", U8), ("common_window", U8), ("sr_index", U8), ("ms_used", U8 * 128),
                ("pns_correlated", U8 * 128), ("ch", CoreToolsChannel * 2)]


@_mirror("xaac_core_tools_state")
class CoreToolsState(ctypes.Structure):   # the noise generator of one stream (a new one's: xaac_parse_core_tools_state)
    _fields_ = [("pns_seed", I32), ("pns_corr_seed", I32 * 128)]


# ---- include/xaac_pvc.h
@_mirror("xaac_pvc_frame")
class PvcFrame(ctypes.Structure):
    _fields_ = [("pvc_mode", U8), ("ns_mode", U8), ("pvc_rate", U8), ("low_power", U8), ("first_bnd_idx", I16),
                ("first_pvc_timeslot", I16), ("pvc_id", U16 * 16)]


@_mirror("xaac_pvc_state")
class PvcState(ctypes.Structure):
    _fields_ = [("esg", (F32 * 3) * 15), ("prev_first_bnd_idx", I16), ("prev_pvc_id", U16), ("prev_pvc_flg", U8),
                ("prev_pvc_rate", U8), ("reserved", U8 * 2)]


@_mirror("xaac_pvc_batch")
class PvcBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("frame", PTR), ("qmf_re", PTR), ("qmf_im", PTR), ("qmf_stride", I32), ("state", PTR), ("out", PTR),
                ("status", PTR)]


# ---- include/xaac_hbe.h
@_mirror("xaac_hbe_state")
class HbeState(ctypes.Structure):
    _fields_ = [("input_buf", F32 * (1024 + 64)), ("synth_buf", F32 * 1280), ("analy_buf", F32 * 640),
                ("qmf_in_buf", (F32 * 128) * 32), ("qmf_out_buf", (F32 * 128) * 64),
                ("synth_size", I32), ("k_start", I32), ("start_band", I32), ("end_band", I32),
                ("x_over_qmf", I32 * 6), ("max_stretch", I32), ("fft_ready", I32)]


@_mirror("xaac_hbe_synth_batch")
class HbeSynthBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("num_columns", I32), ("qmf_re", PTR), ("qmf_im", PTR), ("state", PTR), ("status", PTR)]


@_mirror("xaac_hbe_apply_batch_desc")
class HbeApplyBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("qmf_re", PTR), ("qmf_im", PTR), ("pitch_in_bins", PTR), ("state", PTR), ("pv_re", PTR),
                ("pv_im", PTR), ("status", PTR), ("max_synth_size", I32)]


@_mirror("xaac_hbe_dft_anal_state")
class HbeDftAnalState(ctypes.Structure):
    _fields_ = [("analy_buf", F32 * 640), ("analy_size", I32), ("a_start", I32)]


@_mirror("xaac_hbe_dft_anal_batch")
class HbeDftAnalBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("no_bins", I32), ("time_in", PTR), ("in_stride", I32), ("coef_re", PTR), ("coef_im", PTR),
                ("cfg", PTR), ("state", PTR), ("qmf_re", PTR), ("qmf_im", PTR), ("status", PTR)]


@_mirror("xaac_hbe_dft_state")
class HbeDftState(ctypes.Structure):
    _fields_ = [("input_buf", F32 * 1024), ("output_buf", F32 * 3072), ("synth_buf", F32 * 1280), ("anal", HbeDftAnalState),
                ("synth_size", I32), ("k_start", I32), ("start_band", I32), ("end_band", I32), ("max_stretch", I32),
                ("x_over_qmf", I32 * 6), ("last_status", I32)]


@_mirror("xaac_hbe_dft_cfg")
class HbeDftCfg(ctypes.Structure):
    _fields_ = [("anal_window", F32 * 512), ("synth_window", F32 * 768), ("fd_win", ((F32 * 772) * 2) * 3)]


@_mirror("xaac_hbe_dft_apply_batch")
class HbeDftApplyBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("qmf_re", PTR), ("qmf_im", PTR), ("pitch_in_bins", PTR), ("oversampling", PTR), ("cfg_tab", PTR),
                ("coef_re", PTR), ("coef_im", PTR), ("cfg", PTR), ("state", PTR), ("pv_re", PTR), ("pv_im", PTR), ("status", PTR),
                ("rows32", I32)]


@_mirror("xaac_hbe_anal_batch")
class HbeAnalBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("state", PTR), ("status", PTR)]


# ---- include/xaac_esbr.h
@_mirror("xaac_esbr_side")
class EsbrSide(ctypes.Structure):
    _fields_ = [("out_sampling_freq", I32), ("limiter_bands", I16), ("num_mf_bands", I16), ("f_master_tbl", I16 * 57),
                ("qmf_sb_prev", I16), ("reset_flag", I16), ("harmonic_sbr", I16), ("sbr_invf_mode_prev", I32 * 10),
                ("inter_temp_shape_mode", I32 * 8), ("flt_env_sf_arr", F32 * 448), ("flt_noise_floor", F32 * 10), ("pitch_in_bins", I32)]


@_mirror("xaac_esbr_state")
class EsbrState(ctypes.Structure):
    _fields_ = [("ana", EsbrAnaState), ("syn", EsbrSynState), ("qmf_re", (F32 * 64) * 40), ("qmf_im", (F32 * 64) * 40),
                ("out_re", (F32 * 64) * 8), ("out_im", (F32 * 64) * 8), ("bw_array_prev", F32 * 6),
                ("e_gain", (F32 * 64) * 5), ("noise_buf", (F32 * 64) * 5), ("lim_table", (I32 * 13) * 4),
                ("gate_mode", I32 * 4), ("harm_index", I32), ("phase_index", I32), ("esbr_start_up", I32),
                ("env_short_flag_prev", I32), ("patch_start_subband", I32 * 7), ("num_patches", I32),
                ("harm_flag_prev", I8 * 64), ("prev_sbr_patching_mode", I32), ("ph_re", (F32 * 64) * 8),
                ("ph_im", (F32 * 64) * 8)]


@_mirror("xaac_esbr_pvc_side")
class EsbrPvcSide(ctypes.Structure):
    _fields_ = [("sbr_mode", I16), ("sine_position", I16), ("sin_start_for_cur_top", I16), ("sin_len_for_cur_top", I16),
                ("border_vec", I16 * 9), ("freq_res", I16 * 8), ("pad_", I16), ("pvc", PvcFrame)]


@_mirror("xaac_esbr_pvc_state")
class EsbrPvcState(ctypes.Structure):
    _fields_ = [("pvc", PvcState), ("qmapped", (F32 * 48) * 64), ("prev_noise_level", F32 * 10), ("harm_flag_varlen_prev", I8 * 64),
                ("harm_flag_varlen", I8 * 64), ("prev_freq_res", I16 * 2), ("var_len_id_prev", I16), ("prev_sbr_mode", I16),
                ("esbr_start_up_pvc", I32)]


@_mirror("xaac_esbr_ps_state")
class EsbrPsState(ctypes.Structure):
    _fields_ = [("hyb_hist_re", (F32 * 12) * 3), ("hyb_hist_im", (F32 * 12) * 3), ("qmf_delay_re", (F32 * 64) * 14),
                ("qmf_delay_im", (F32 * 64) * 14), ("sub_delay_re", (F32 * 12) * 2), ("sub_delay_im", (F32 * 12) * 2),
                ("ser_qmf_re", ((F32 * 64) * 5) * 3), ("ser_qmf_im", ((F32 * 64) * 5) * 3),
                ("ser_sub_re", ((F32 * 12) * 5) * 3), ("ser_sub_im", ((F32 * 12) * 5) * 3), ("h_prev", (F32 * 20) * 8),
                ("peak_decay_fast", F32 * 20), ("prev_nrg", F32 * 20), ("prev_peak_diff", F32 * 20),
                ("delay_buf_idx", I32), ("delay_buf_idx_ser", I32 * 3), ("delay_qmf_idx", I32 * 64), ("syn_r", EsbrSynState)]


@_mirror("xaac_esbr_sbr_batch")
class EsbrSbrBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("core", PTR), ("header", PTR), ("frame", PTR), ("side", PTR), ("state", PTR), ("out", PTR),
                ("ps_frame", PTR), ("ps_state", PTR), ("out_r", PTR), ("status", PTR), ("workspace", PTR), ("workspace_bytes", U64),
                ("hbe_state", PTR), ("hbe_max_synth_size", I32), ("pvc_side", PTR), ("pvc_state", PTR), ("sbr_ratio", I32),
                ("down_sample", I32), ("hbe_dft_state", PTR), ("hbe_dft_cfg_tab", PTR), ("hbe_dft_coef_re", PTR),
                ("hbe_dft_coef_im", PTR), ("hbe_dft_cfg", PTR)]


@_mirror("xaac_esbr_core_in_batch")
class EsbrCoreInBatch(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("ch_fac", I32), ("pcm", PTR), ("core", PTR)]


@_mirror("xaac_esbr_pcm_out_batch")
class EsbrPcmOutBatch(ctypes.Structure):
    _fields_ = [("n", I32), ("stride", I32), ("left", PTR), ("right", PTR), ("pcm", PTR)]


@_mirror("xaac_mc_core_in_batch")
class McCoreInBatch(ctypes.Structure):
    _fields_ = [("n_streams", I32), ("channel_config", I32), ("out32", PTR), ("qshift_adj", PTR), ("core", PTR)]


@_mirror("xaac_mc_pcm_out_batch")
class McPcmOutBatch(ctypes.Structure):
    _fields_ = [("n_streams", I32), ("n_ch", I32), ("stride", I32), ("slot", I32 * 6), ("planes", PTR), ("pcm", PTR)]


@_mirror("xaac_mc_pcm_out_map_batch")
class McPcmOutMapBatch(ctypes.Structure):
    _fields_ = [("out", McPcmOutBatch), ("map", OutMap)]


# ---- include/xaac_parse.h (the CPU front end, libxaac_host.so)
@_mirror("xaac_adts_header")
class AdtsHeader(ctypes.Structure):
    _fields_ = [(n, I32) for n in ("id", "layer", "protection_absent", "profile", "sr_index", "sampling_rate",
                                   "channel_config", "frame_bytes", "raw_blocks", "header_bytes")]


@_mirror("xaac_core_frame")
class CoreFrame(ctypes.Structure):
    _fields_ = [("n_ch", I32), ("element_id", I32), ("common_window", I32), ("sbr_ext_type", I32), ("sbr_bytes", I32),
                ("tools", I32), ("ics", (I16 * 4) * 2), ("spec", (I32 * 1024) * 2), ("sbr", U8 * 272)]


@_mirror("xaac_sbr_side")
class SbrSide(ctypes.Structure):   # header / frame / ps_frame as the byte rows the GPU entry points take
    _fields_ = [(n.lower(), I32) for n in SBR_FLAG_NAMES] + \
               [("header", U8 * ctypes.sizeof(SbrHeader)), ("frame", (U8 * ctypes.sizeof(SbrFrame)) * 2),
                ("ps_frame", U8 * ctypes.sizeof(PsFrame))]


@_mirror("xaac_parse_batch")
class ParseBatch(ctypes.Structure):
    _fields_ = [(n, I32) for n in ("n_streams", "n_ch", "with_sbr", "ps_enable", "stage", "threads")] + \
               [(n, PTR) for n in ("parser", "data", "bytes", "spec", "ics", "header", "frame", "ps_frame", "flags",
                                   "tools", "consumed", "status", "esbr_side", "reset_pitch", "pos")] + \
               [("frames", I32), ("lines", PTR), ("tools_side", PTR), ("channel_config", I32), ("mc_sbr", I32), ("drc_side", PTR)]


# ---- the device library's entry points
# XAAC_API int32_t f(xaac_ctx *, const T *): name -> T's mirror
BATCH_ENTRY_POINTS = {
    "xaac_imdct_process_batch": ImdctBatch, "xaac_imdct_process_batch_host": ImdctBatch, "xaac_imdct960_process_batch": ImdctBatch,
    "xaac_imdct_ld_process_batch": ImdctLdBatch, "xaac_usac_imdct_process_batch": UsacImdctBatch,
    "xaac_aac_tools_process_batch": AacToolsBatch, "xaac_drc_apply_batch": DrcBatch,
    "xaac_qmf_analysis_batch": QmfAnaBatch, "xaac_qmf_synthesis_batch": QmfSynBatch,
    "xaac_qmf_analysis_eld_batch": QmfAnaEldBatch, "xaac_qmf_synthesis_eld_batch": QmfSynEldBatch,
    "xaac_esbr_qmf_analysis_batch": EsbrAnaBatch, "xaac_esbr_qmf_analysis_nb_batch": EsbrAnaNbBatch,
    "xaac_esbr_qmf_synthesis_batch": EsbrSynBatch, "xaac_esbr_qmf_synthesis_ds_batch": EsbrSynBatch,
    "xaac_sbr_lp_process_batch": SbrLpBatch, "xaac_sbr_lp960_process_batch": SbrLpBatch,
    "xaac_sbr_hq_process_batch": SbrHqBatch, "xaac_sbr_hq960_process_batch": SbrHqBatch,
    "xaac_sbr_eld_process_batch": SbrEldBatch, "xaac_sbr_state_handover": HandoverBatch,
    "xaac_sbr_state_apply_side_batch": ApplySideBatch, "xaac_peak_limiter_process_batch": LimiterBatch,
    "xaac_peak_limiter_process_map_batch": LimiterMapBatch, "xaac_pcm16_scale_adjust_map_batch": ScaleAdjustMapBatch,
    "xaac_esbr_sbr_process_batch": EsbrSbrBatch, "xaac_esbr_core_from_pcm16_batch": EsbrCoreInBatch,
    "xaac_esbr_pcm16_from_float_batch": EsbrPcmOutBatch, "xaac_mc_core_from_out32_batch": McCoreInBatch,
    "xaac_mc_pcm16_from_float_batch": McPcmOutBatch, "xaac_mc_pcm16_from_planes_batch": McPcmOutBatch,
    "xaac_mc_pcm16_from_float_map_batch": McPcmOutMapBatch, "xaac_mc_pcm16_from_planes_map_batch": McPcmOutMapBatch,
    "xaac_hbe_real_synth_batch": HbeSynthBatch, "xaac_hbe_cplx_anal_batch": HbeAnalBatch, "xaac_hbe_apply_batch": HbeApplyBatch,
    "xaac_hbe_dft_anal_batch_run": HbeDftAnalBatch, "xaac_hbe_dft_apply_batch_run": HbeDftApplyBatch,
    "xaac_pvc_process_batch": PvcBatch,
}
# every other signature: name -> (restype, argtypes)
OTHER_ENTRY_POINTS = {
    "xaac_version": (ctypes.c_char_p, []),
    "xaac_create": (I32, [ctypes.POINTER(PTR), I32, PTR]),
    "xaac_destroy": (I32, [PTR]), "xaac_sync": (I32, [PTR]), "xaac_warm_up": (I32, [PTR]),
    "xaac_set_stream": (I32, [PTR, PTR]),
    "xaac_last_launch": (I32, [PTR] + [ctypes.POINTER(I32)] * 3),
    "xaac_peak_limiter_init": (I32, [ctypes.POINTER(LimiterState), U32, U32]),
    "xaac_sbr_lp_workspace_bytes": (U64, [I32]), "xaac_sbr_hq_workspace_bytes": (U64, [I32, I32]),
    "xaac_sbr_eld_workspace_bytes": (U64, [I32]), "xaac_peak_limiter_workspace_bytes": (U64, [I32]),
    "xaac_esbr_workspace_bytes": (U64, [I32]), "xaac_esbr_workspace_bytes_ratio": (U64, [I32, I32]),
}


# ---- the host library's entry points (include/xaac_parse.h): name -> (restype, argtypes)
_P32, _PSZ = ctypes.POINTER(I32), ctypes.POINTER(ctypes.c_size_t)
HOST_ENTRY_POINTS = {
    "xaac_parser_create": (I32, [ctypes.POINTER(PTR)]), "xaac_parser_destroy": (None, [PTR]),
    "xaac_parser_set_esbr": (I32, [PTR, I32]),
    "xaac_adts_parse_header": (I32, [PTR, ctypes.c_size_t, ctypes.POINTER(AdtsHeader)]),
    "xaac_parse_adts_frame": (I32, [PTR, PTR, ctypes.c_size_t, I32, ctypes.POINTER(CoreFrame), _PSZ]),
    "xaac_parse_adts_frame_mc": (I32, [PTR, PTR, ctypes.c_size_t, I32, PTR, I32, _P32, _PSZ]),
    "xaac_parse_sbr_side": (I32, [PTR, I32, ctypes.POINTER(SbrSide)]),
    "xaac_parse_esbr_side": (I32, [PTR, I32, PTR]), "xaac_parse_reset_pitch": (I32, [PTR, _P32]),
    "xaac_parse_core_tools_side": (I32, [PTR, PTR]), "xaac_parse_core_tools_side_mc": (I32, [PTR, I32, PTR]),
    "xaac_parse_core_tools_state": (I32, [PTR, PTR]), "xaac_parse_core_tools_state_mc": (I32, [PTR, I32, PTR]),
    "xaac_core_tools_apply_host": (I32, [PTR, PTR, PTR]),
    "xaac_parse_drc_config": (I32, [PTR, ctypes.POINTER(DrcConfig)]), "xaac_parse_drc_side": (I32, [PTR, PTR]),
    "xaac_drc_apply_host": (I32, [PTR, PTR]),
    "xaac_sbr_state_init": (None, [PTR]), "xaac_ps_state_init": (None, [PTR]), "xaac_esbr_state_init": (None, [PTR]),
    "xaac_esbr_ps_state_init": (None, [PTR]), "xaac_hbe_state_init": (None, [PTR]),
    "xaac_hbe_state_reinit": (I32, [PTR, PTR]), "xaac_hbe_state_reinit_tails": (I32, [PTR, PTR, I32]),
    "xaac_sbr_state_apply_side": (None, [PTR, ctypes.POINTER(SbrSide), I32]),
    "xaac_ps_state_apply_side": (None, [PTR, ctypes.POINTER(SbrSide)]),
    "xaac_out_map_apply_host": (I32, [PTR, I32, PTR, I64, PTR]), "xaac_out_map_row_bound": (I32, [I32, ctypes.POINTER(I64)]),
    # (_run / _start: the original layout's symbols, no pos / frames / lines)
    "xaac_parse_batch_run": (I32, [PTR]), "xaac_parse_batch_start": (I32, [PTR]), "xaac_parse_batch_wait": (I32, [PTR]),
    "xaac_parse_batch_run_sized": (I32, [PTR, U64]), "xaac_parse_batch_start_sized": (I32, [PTR, U64]),
}


def _apply(lib, table):
    for name, (restype, argtypes) in table.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    return lib


def bind_host(lib):
    """the prototypes of HOST_ENTRY_POINTS onto a loaded libxaac_host.so"""
    return _apply(lib, HOST_ENTRY_POINTS)


def bind(lib):
    """the prototypes above onto a loaded libxaac_amd.so (this also resolves every function once, so that a call finds it cached)"""
    for name, desc in BATCH_ENTRY_POINTS.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = I32, [PTR, ctypes.POINTER(desc)]
    return _apply(lib, OTHER_ENTRY_POINTS)
