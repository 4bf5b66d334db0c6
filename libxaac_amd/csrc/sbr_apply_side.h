/* sbr_apply_side.h -- what a frame with the reset or the up-sampling flag does to the resident SBR state: sbrdecoder.c:103-252
   (ixheaacd_sbr_dec_reset) and :254-276 (ixheaacd_prepare_upsamp), the words they rewrite.  One statement for the host library
   (xaac_sbr_state_apply_side, xaac_ps_state_apply_side) and the device (xaac_sbr_apply_side_kernel). */
#ifndef XAAC_SBR_APPLY_SIDE_H
#define XAAC_SBR_APPLY_SIDE_H

#include "../../include/xaac_sbr.h"
#include "fx.h"

/* one channel's state; sub_band_start / sub_band_end: the frame's header, channel: 0 or 1 of its element */
FX_HD void xs_apply_side_channel(xaac_sbr_state *s, int sub_band_start, int sub_band_end, int reset, int reset_channels,
                                 int upsampling, int channel) {
  if (reset && channel < reset_channels) {
    s->ph_index = 0;
    s->filt_buf_noise_e = 0;
    s->start_up = 1;
    s->syn_lsb = s->codec_usb = (int16_t)sub_band_start;
    s->syn_usb = (int16_t)sub_band_end;
    for (int k = 0; k < XAAC_SBR_MAX_PATCHES; k++) s->bw_array_prev[k] = 0;
  }
  if (upsampling) {
    s->syn_lsb = s->codec_usb = 32;
    s->syn_usb = 64;
  }
}

/* the right channel's synthesis bank kept in the PS state (channel 1 of a mono + PS stream) */
FX_HD void xs_apply_side_ps(xaac_ps_state *s, int sub_band_start, int sub_band_end, int reset, int reset_channels, int upsampling) {
  if (reset && reset_channels > 1) {
    s->syn_lsb_r = (int16_t)sub_band_start;
    s->syn_usb_r = (int16_t)sub_band_end;
  }
  if (upsampling) {
    s->syn_lsb_r = 32;
    s->syn_usb_r = 64;
  }
}

#endif
