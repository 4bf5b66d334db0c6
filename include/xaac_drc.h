/*
 * xaac_drc.h -- MPEG-4 dynamic range control and level normalisation in the spectral domain: the branch of ixheaacd_drc_apply
 * (decoder/ixheaacd_drc_freq_dec.c:879-1106) that an AAC-LC stream without SBR takes (:1012-1017), on the lines that
 * ixheaacd_imdct_process is about to read (decoder/ixheaacd_aacdecoder.c:981-992).  The gain factors are made on the host from
 * the dynamic_range_info of the frame's fill elements (xaac_parse.h: xaac_parse_drc_config, xaac_parse_drc_side); the GPU
 * multiplies.  The CPU twin with the same arithmetic is xaac_drc_apply_host (xaac_parse.h); the arithmetic itself is
 * libxaac_amd/csrc/drc.h.
 * Out of scope: the QMF-domain branch of streams with SBR, heavy compression (DVB ancillary data), more than two channels.
 */
#ifndef XAAC_DRC_H
#define XAAC_DRC_H

#include <stdint.h>

#include "xaac_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XAAC_DRC_MAX_BANDS 16          /* MAX_DRC_BANDS */
#define XAAC_DRC_ONE (1 << 25)         /* a factor of 1.0 (Q25): DRC_SBR_ONE_Q25 */
#define XAAC_DRC_REFUSED -1            /* the status word of a row whose side info is outside the struct's capacity */

/* what the decoder's user asks for (api.c:629-664, :1918-1946): the reference keeps (WORD32)(factor * 100) of its two float flags */
typedef struct xaac_drc_config {
  int32_t cut;          /* 0 .. 100: -drc_cut_fac * 100 */
  int32_t boost;        /* 0 .. 100: -drc_boost_fac * 100 */
  int32_t target_level; /* 0 .. 127: -drc_target_level, in units of -0.25 dB (108 where the flag is not given) */
} xaac_drc_config;

/* one channel of one frame: the bands in the order ixheaacd_drc_apply walks them.  Band k covers the lines
   [k ? end[k - 1] : 0, end[k]); ends need not rise -- a band whose end lies below its start is empty, and the band behind it starts
   from that lower end, so lines can be multiplied twice --; lines behind the last end are untouched.  A row whose factors are all
   XAAC_DRC_ONE is the identity. */
typedef struct xaac_drc_side {
  int32_t n_bands;                   /* 1 .. XAAC_DRC_MAX_BANDS */
  int32_t end[XAAC_DRC_MAX_BANDS];   /* 0 .. 1024, multiples of 4 */
  int32_t fac[XAAC_DRC_MAX_BANDS];   /* Q25, >= 0 */
} xaac_drc_side;

typedef struct xaac_drc_batch {
  int32_t n;                 /* channel-frames, >= 0 */
  int32_t spec_stride;       /* int32 words from one row's lines to the next one's: a multiple of 4, >= 1024 */
  int32_t *spec;             /* in / out, 16-byte aligned: row i's 1024 lines at spec + i * spec_stride */
  const xaac_drc_side *side; /* [n] */
  int32_t *status;           /* optional [n]: 0, or XAAC_DRC_REFUSED for side info outside the struct's capacity (n_bands outside
                                1 .. 16, an end above 1024, negative or no multiple of 4): that row's lines are left as they are,
                                its neighbours are processed */
} xaac_drc_batch;

/* every line of every band times the band's factor: sat32((int64) line * fac >> 25) (drc_freq_dec.c:103-118), in place, device
   pointers, asynchronous on the context's stream */
XAAC_API int32_t xaac_drc_apply_batch(xaac_ctx *ctx, const xaac_drc_batch *batch);

#ifdef __cplusplus
}
#endif
#endif /* XAAC_DRC_H */
