/*
 * aac_core.h -- host-side AAC-LC syntax decoder: one raw_data_block (ISO/IEC 14496-3 4.4.2.1 as the reference reads it,
 * decoder/ixheaacd_aacdecoder.c:362-647) -> the spectra of its SCE / CPE exactly as the reference hands them to
 * ixheaacd_imdct_process (Q-format, rounding and the reference's quirks included), plus the raw SBR extension payload.
 * CPU code: the bitstream syntax is serial; everything behind this seam runs on the GPU.
 * Scope: AAC-LC objects (AOT 2; 5 / 29 through the SBR payload), 1024-line frames, one SCE or CPE per raw_data_block, or the
 * SCE / CPE / LFE sequence of channel_config 3 .. 6 (with the reference's q_factor / TNS variants for more than two
 * channels: XhCoreState::wide); no CCE, no LTP, no gain control, no error concealment.  dynamic_range_info is read and mapped to
 * the channels where the caller keeps a DRC state (XhCoreState::drc: mono and stereo streams), and skipped otherwise.
 */
#ifndef XAAC_HOST_AAC_CORE_H
#define XAAC_HOST_AAC_CORE_H

#include <stdint.h>

#include "../../include/xaac_tools.h"
#include "bits.h"

enum { XH_ONLY_LONG = 0, XH_LONG_START = 1, XH_EIGHT_SHORT = 2, XH_LONG_STOP = 3 };
enum { XH_ID_SCE = 0, XH_ID_CPE = 1, XH_ID_CCE = 2, XH_ID_LFE = 3, XH_ID_DSE = 4, XH_ID_PCE = 5, XH_ID_FIL = 6, XH_ID_END = 7 };
enum { XH_ZERO_HCB = 0, XH_ESC_HCB = 11, XH_NOISE_HCB = 13, XH_INTENSITY_HCB2 = 14, XH_INTENSITY_HCB = 15 };

/* error codes (negative returns) */
enum {
  XH_ERR_BITS = -1,        /* ran out of bits */
  XH_ERR_SYNTAX = -2,      /* a value the syntax forbids (max_sfb, section length, code book 12, pulse / TNS range ...) */
  XH_ERR_UNSUPPORTED = -3, /* prediction, gain control, CCE, more elements than this decoder builds */
  XH_ERR_ESCAPE = -4       /* escape value beyond what the inverse quantiser takes (channel.c:1066) */
};

struct XhIcs {
  int window_sequence, window_shape, max_sfb, num_swb, num_groups;
  uint8_t group_len[8];
};

struct XhTnsFilter {
  int start_band, stop_band, order, direction, resolution;
  int8_t coef[32];
};

struct XhTns {
  int present;
  int n_filt[8];
  XhTnsFilter f[8][4];
};

struct XhPulse {
  int present, number, start_band;
  uint8_t offset[4], amp[4];
};

#define XH_SPEC_SLACK 16 /* the reference's TNS filter runs order (rounded up to 4) lines even over a shorter region */

struct XhChannel {
  XhIcs ics;
  int global_gain;
  uint8_t cb[8 * 16];  /* long blocks: bands 0 .. 50 contiguous; short: 16 per group (longblock.c:146) */
  int16_t sf[8 * 16];
  XhPulse pulse;
  XhTns tns;
  int pns_active;
  int16_t noise_energy;
  uint8_t pns_used[8 * 16];
  /* the frame's lines: XH_SPEC_WORDS words of the CALLER's (set before xh_parse_raw_data_block; a parser that keeps one
     such buffer per thread instead of one per stream has 8 KB less state to drag through the caches per frame) */
  int32_t *spec_mem;
  int32_t *spec() { return spec_mem + XH_SPEC_SLACK; }
};
#define XH_SPEC_WORDS (1024 + 2 * XH_SPEC_SLACK)

/* what is constant between ADTS headers of one stream.  (The state that outlives a frame is the caller's, one per channel element:
   the noise generator xaac_core_tools_state -- pns_seed = pstr_pns_rand_vec_data->current_seed, which starts at 0 and runs on from
   frame to frame; pns_corr_seed = pstr_pns_corr_info->random_vector: the left channel's seed of a band whose noise the M/S flag
   correlates; a right channel that substitutes noise in such a band where the left one does not finds the value an earlier frame
   left, the reference keeps it in scratch memory that AAC-LC decoding does not reuse in between -- nor between its initialisation
   pass over the first frame (ixheaacd_dec_init, api.c:2097) and the first output frame: a new stream's pns_corr_seed is what the
   tools leave behind one pass over its first frame from zero, while current_seed is set back to 0 (xh_tools_state_begin; the
   first block a parser reads sets its elements' generators up that way, whatever the stage).  Only stage-2 parsing advances it:
   behind a stage-1 parse the tools' caller keeps the state, xaac_core_tools_apply_host or the GPU's xaac_aac_tools_process_batch,
   and starts from the parser's, xaac_parse_core_tools_state.) */
struct XhCoreState {
  int sr_index;            /* 0 .. 11 */
  int16_t swb_long[52], swb_short[16];
  const int8_t *width_long, *width_short;
  int num_swb_long, num_swb_short;
  int wide;                /* the stream has more than two channels (set by the caller behind xh_core_init): scale factors with
                              q_factor 34 and the 32-bit TNS variant (block.c:1263, channel.c:642, pns_js_thumb.c:328) */
  struct XhDrc *drc;       /* the stream's dynamic range control state, or null: dynamic_range_info is then skipped unread (set by
                              the caller behind xh_core_init, like `wide`) */
  int tools_born;          /* a block of the stream has parsed: its elements' noise generators have been set up
                              (xh_tools_state_begin; the caller carries it over xh_core_init, like `wide`) */
};

/* ---- dynamic range control: what ia_drc_dec_struct keeps for the spectral-domain branch (decoder/ixheaacd_drc_data_struct.h) ---- */
#define XH_DRC_MAX_ELEMENTS 10 /* MAX_BS_ELEMENT: dynamic_range_info elements kept per frame; further ones are read and dropped */
#define XH_DRC_MAX_CHANNELS 8  /* MAX_AUDIO_CHANNELS: the channels an element's exclusion mask speaks of */
#define XH_DRC_MAX_BANDS 16    /* MAX_DRC_BANDS */

struct XhDrcElement { /* ixheaac_drc_bs_data_struct: one dynamic_range_info as read (drc_freq_dec.c:609-672) */
  uint8_t channel_on[XH_DRC_MAX_CHANNELS];
  uint8_t prog_ref_level_present, prog_ref_level, num_bands;
  uint8_t band_top[XH_DRC_MAX_BANDS];
  int8_t dyn_rng[XH_DRC_MAX_BANDS]; /* sign and 7 bits */
};

struct XhDrcChannel { /* ixheaac_drc_data_struct, by the channel's index inside the element; outlives the frame */
  int n_bands;
  int16_t n_mdct_bands[XH_DRC_MAX_BANDS], drc_fac[XH_DRC_MAX_BANDS];
};

struct XhDrc {
  int cut, boost, target_ref_level; /* 0 .. 100, 0 .. 100, 0 .. 127 (api.c:1918-1923) */
  int prog_ref_level;               /* starts as the target level (api.c:1924) */
  int num_elements;                 /* of the frame in work (api.c:3055 clears it per frame) */
  XhDrcElement el[XH_DRC_MAX_ELEMENTS];
  XhDrcChannel ch[2];
};

/* ixheaacd_drc_dec_create (drc_freq_dec.c:530-578) + api.c:1918-1925 */
void xh_drc_init(XhDrc *d, int cut, int boost, int target_level);

struct XhElement {
  int id;                   /* XH_ID_SCE / XH_ID_CPE */
  int n_ch, tag, common_window;
  uint8_t ms_used[8][64];
  uint8_t pns_correlated[8 * 16];
  int tools_derived;        /* pns_correlated / ms_used have been through channel.c:702-725 */
  XhChannel ch[2];
  /* SBR extension payload of the FIL element behind the channel element (aacpluscheck.c:59): extension type 13 / 14,
     then the payload bytes with the first byte holding the 4 bits that follow the extension type */
  int sbr_ext_type, sbr_bytes;
  uint8_t sbr[272];
};

/* |q|^(4/3) in Q13 of a quantised magnitude as the reference computes it (table, then its interpolation: channel.c:1055);
   *err is set beyond 8191 + 32 */
int32_t xh_inverse_quant(int32_t magnitude, int *err);

/* sr_index 0 .. 11; returns 0 or XH_ERR_UNSUPPORTED */
int xh_core_init(XhCoreState *st, int sr_index);

/* Parses one raw_data_block at the reader's position (up to and including ID_END and the byte alignment) of up to `cap` channel
   elements (SCE / CPE / LFE in bitstream order; one more is XH_ERR_UNSUPPORTED): element k into els[k] and the line buffers
   els[k]->ch[c].spec_mem point to, its noise generator tools[k] -- the reference keeps one core decoder instance, and so one
   generator, per element (api.c:2433-2458) --; *n_els = how many the block held.  The SBR payload of a FIL element goes to the
   channel element in front of it.  Dequantises, applies the scale factors and the tools (M/S, intensity, PNS, TNS):
   el->ch[c].spec() are the lines the IMDCT takes.
   `stage`: 2 = everything; 1 = stop before the tools (spectra as at the entry of ixheaacd_channel_pair_process).
   Returns 0 or a negative XH_ERR_*. */
int xh_parse_raw_data_block(XhCoreState *st, XhBits *br, XhElement *const *els, xaac_core_tools_state *const *tools, int cap,
                            int *n_els, int stage);

/* A new stream's noise generator, from the tools' side info of its first frame: the seeds of the correlated noise bands as one
   pass of the tools over that frame from a zero state leaves them, pns_seed 0.  The reference decodes the first frame twice -- while
   it initialises (ixheaacd_dec_init, api.c:2097) and again as the first output frame --; pstr_pns_corr_info->random_vector lies in
   scratch memory (aacdecoder.c:153-186) that outlives the first pass, current_seed belongs to the decoder instance that is set up
   afresh in between. */
void xh_tools_state_begin(const xaac_core_tools_side *first, xaac_core_tools_state *state);

/* What the tools read of the element parsed last, as the boundary struct of include/xaac_tools.h (ms_used and
   pns_correlated as the tools apply them).  Writes the bands below max_sfb, the filters n_filt counts and the scalar
   members; a caller that hands the struct out clears it first. */
void xh_export_tools_side(const XhCoreState *st, XhElement *el, xaac_core_tools_side *side);

#endif /* XAAC_HOST_AAC_CORE_H */
