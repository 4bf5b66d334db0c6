/*
 * xaac_tools.h -- the boundary structs of the AAC spectral tools (M/S stereo, intensity stereo, perceptual noise
 * substitution, temporal noise shaping): what the tool half of ixheaacd_channel_pair_process
 * (decoder/ixheaacd_channel.c:602-725) reads beside the spectra, as plain C for the host parser (xaac_parse.h:
 * xaac_parse_core_tools_side, xaac_core_tools_apply_host) and the GPU entry point (xaac_amd.h: xaac_aac_tools_process_batch).
 * Types only: the functions are declared in those two headers.
 */
#ifndef XAAC_TOOLS_H
#define XAAC_TOOLS_H

#include <stdint.h>

#define XAAC_TOOLS_BANDS 128        /* band index: 16 * window group + sfb (EIGHT_SHORT), sfb (long windows, at most 51) */
#define XAAC_TOOLS_TNS_FILTERS 8    /* filter slots of a channel: long windows use slots 0 .. n_filt[0]-1 (at most 3),
                                       EIGHT_SHORT uses slot w for window w (at most one filter per window) */
#define XAAC_TOOLS_TNS_MAX_ORDER 12 /* MAX_ORDER_LONG, for short windows too (channel.c:1021) */

typedef struct xaac_tns_filter_side {
  uint8_t start_band, stop_band; /* as ixheaacd_read_tns_data leaves them (channel.c:1005-1012) */
  int8_t order;                  /* 0 .. XAAC_TOOLS_TNS_MAX_ORDER */
  int8_t direction;              /* +1 upwards, -1 downwards */
  uint8_t resolution;            /* coef_res: 0 = 3-bit, 1 = 4-bit coefficient table */
  uint8_t reserved[3];
  int8_t coef[XAAC_TOOLS_TNS_MAX_ORDER]; /* sign-extended indices: -4 .. 3 (resolution 0), -8 .. 7 (resolution 1) */
} xaac_tns_filter_side;

typedef struct xaac_core_tools_channel {
  uint8_t window_sequence; /* 0 .. 3 (XAAC_EIGHT_SHORT = 2) */
  uint8_t max_sfb;
  uint8_t num_groups;      /* 1 for long windows */
  uint8_t pns_active;
  uint8_t tns_present;
  uint8_t wide;            /* the stream has more than two channels: the reference then keeps three more bits in the spectra up
                              to the stereo tools (scale factors with q_factor 34, block.c:1263; shifted down behind them,
                              channel.c:642-652) and runs the 32-bit TNS variant (pns_js_thumb.c:328-475).  The same in every
                              channel of a stream */
  uint8_t reserved[2];
  uint8_t group_len[8];    /* windows per group; they add up to 8 in an EIGHT_SHORT frame */
  uint8_t n_filt[8];       /* TNS filters per window (long windows: n_filt[0] only) */
  uint8_t cb[XAAC_TOOLS_BANDS];       /* code book per band: 13 noise, 14 / 15 intensity */
  int16_t sf[XAAC_TOOLS_BANDS];       /* scale factor / intensity position / noise energy per band */
  uint8_t pns_used[XAAC_TOOLS_BANDS];
  xaac_tns_filter_side tns[XAAC_TOOLS_TNS_FILTERS];
} xaac_core_tools_channel;

/* one channel element of one frame */
typedef struct xaac_core_tools_side {
  uint8_t element_id;    /* 0 SCE, 1 CPE, 3 LFE */
  uint8_t n_ch;          /* 1 or 2 */
  uint8_t common_window;
  uint8_t sr_index;      /* sampling frequency index 0 .. 11: selects the scale factor band tables */
  uint8_t ms_used[XAAC_TOOLS_BANDS];        /* as the tools apply it: the bit stream's flag, cleared in the bands where both
                                               channels substitute correlated noise (channel.c:702-725) */
  uint8_t pns_correlated[XAAC_TOOLS_BANDS]; /* the bit stream's ms_used of a common_window pair with noise substitution */
  xaac_core_tools_channel ch[2];
} xaac_core_tools_side;

/* what outlives a frame, per stream.  A new stream: pns_seed 0, pns_corr_seed as one pass of the tools over the stream's first
   frame from an all-zero state leaves it -- the reference decodes that frame twice (ixheaacd_dec_init, api.c:2097, then as the
   first output frame) and random_vector, scratch memory (aacdecoder.c:153-186), outlives the first pass while current_seed is
   set up afresh.  xaac_parse.h: xaac_parse_core_tools_state fills one for a parser's stream */
typedef struct xaac_core_tools_state {
  int32_t pns_seed;                        /* pstr_pns_rand_vec_data->current_seed */
  int32_t pns_corr_seed[XAAC_TOOLS_BANDS]; /* pstr_pns_corr_info->random_vector */
} xaac_core_tools_state;

#endif /* XAAC_TOOLS_H */
