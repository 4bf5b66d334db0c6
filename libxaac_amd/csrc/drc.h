/*
 * drc.h -- the arithmetic of MPEG-4 dynamic range control in the spectral domain, for host (libxaac_host.so: the gain factors of
 * xaac_parse_drc_side, and xaac_drc_apply_host, the CPU twin) and gfx950 (drc_kernel.hip), one function per step of
 * ixheaacd_drc_apply (decoder/ixheaacd_drc_freq_dec.c:879-1106) with sbr_found == 0:
 *
 *   xd_norm       the level normalisation 2^((target_ref_level - prog_ref_level) / 24) in Q25 (:930-954)
 *   xd_band_fac   a band's gain 2^(drc_fac * cut|boost / 2400) in Q25, times the normalisation (:972-1006)
 *   xd_line       one line times a band's factor (:1013-1016)
 *   xd_side_ok    what a side row has to satisfy for xd_apply_row to stay inside the row
 *   xd_apply_row  the ordered walk over the bands (:956-957, :1010-1017, :1098)
 *
 * The window sequence does not enter this branch.  Heavy compression (:958-970, float pow) is not restated.
 */
#ifndef XAAC_DRC_ARITH_H
#define XAAC_DRC_ARITH_H

#include <stdint.h>

#include "../../include/xaac_drc.h"
#include "fx.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include "tables_drc.inc"

/* ixheaacd_get_div_value_24 (:805-814) and ixheaacd_get_div_value_2400 (:816-825): value / 24 and value / 2400 by a rounded Q30
   reciprocal */
FX_HD int32_t xd_div_24(int32_t value) { return (int32_t)(((int64_t)value * 44739243 + 22369621) >> 30); }
FX_HD int32_t xd_div_2400(int32_t value) { return (int32_t)(((int64_t)value * 447392 + 223696) >> 30); }
/* ixheaacd_mult32x16in32_shift29 (:91-101): the 64-bit product >> 29, truncated to 32 bits */
FX_HD int32_t xd_mult_shift29(int32_t a, int32_t b) { return (int32_t)(((int64_t)a * (int64_t)b) >> 29); }
#endif

/* ixheaacd_mult32x16in32_shift25 (:103-118): the 64-bit product >> 25 (arithmetic: a floor, also for negative lines), saturated.
   On the GPU: v_mul_lo_u32 and v_mul_hi_i32, a funnel shift of the two halves, and the clamp decided on the high half. */
FX_HD int32_t xd_line(int32_t line, int32_t fac) { return fx_sat64(((int64_t)line * (int64_t)fac) >> 25); }

#if !defined(__HIP_DEVICE_COMPILE__)
/* :930-954 with drc_dig_norm == 1 (a target level below 0, which switches it off, cannot be asked for: xaac_drc_config).
   2^(-d / 24) for d = target - prog >= 0, 2^(d / 24) for d < 0: the whole octaves as a shift, the rest from the table */
FX_HD int32_t xd_norm(int32_t target_ref_level, int32_t prog_ref_level) {
  int32_t diff = target_ref_level - prog_ref_level;
  const int32_t *table = xd_pow_tbl_1_2_q29;
  int32_t norm;
  if (diff < 0) {
    diff = -diff;
    table = xd_pow_tbl_2_q29;
    const int32_t div = xd_div_24(diff);
    norm = fx_shlw(1, 25 + div);
    diff = (diff - div * 24) * 1000;
  } else {
    const int32_t div = xd_div_24(diff);
    norm = fx_shlw(1, 25 - div);
    diff = (diff - div * 24) * 1000;
  }
  return xd_mult_shift29(norm, table[xd_div_24(diff)]);
}

/* :972-1006: drc_fac = the band's dyn_rng word (sign and 7 bits, -127 .. 127, in units of 0.25 dB); a negative word is scaled by
   the cut factor, any other by the boost factor (0 .. 100) */
FX_HD int32_t xd_band_fac(int32_t drc_fac, int32_t cut, int32_t boost, int32_t norm) {
  int32_t v = drc_fac * (drc_fac < 0 ? cut : boost);
  const int32_t *table = xd_pow_tbl_2_q29;
  int32_t fac;
  if (v < 0) {
    v = -v;
    table = xd_pow_tbl_1_2_q29;
    const int32_t div = xd_div_2400(v);
    fac = fx_shlw(1, 25 - div);
    v = (v - div * 2400) * 10;
  } else {
    const int32_t div = xd_div_2400(v);
    fac = fx_shlw(1, 25 + div);
    v = (v - div * 2400) * 10;
  }
  fac = xd_mult_shift29(fac, table[xd_div_24(v)]);
  return xd_line(fac, norm);
}
#endif

/* a side row xd_apply_row / the kernel take: the struct's capacity, ends inside the row and on the groups of four lines both walk */
FX_HD int xd_side_ok(const xaac_drc_side *s) {
  if (s->n_bands < 1 || s->n_bands > XAAC_DRC_MAX_BANDS) return 0;
  for (int k = 0; k < s->n_bands; k++)
    if (s->end[k] < 0 || s->end[k] > 1024 || (s->end[k] & 3)) return 0;
  return 1;
}

FX_HD int xd_side_identity(const xaac_drc_side *s) {
  for (int k = 0; k < s->n_bands; k++)
    if (s->fac[k] != XAAC_DRC_ONE) return 0;
  return 1;
}

/* the walk itself (a row that passed xd_side_ok): start_pos = the band before's end_pos, whatever that was */
static inline void xd_apply_row(const xaac_drc_side *s, int32_t *spec) {
  int start = 0;
  for (int k = 0; k < s->n_bands; k++) {
    const int end = s->end[k];
    for (int i = start; i < end; i++) spec[i] = xd_line(spec[i], s->fac[k]);
    start = end;
  }
}

#endif /* XAAC_DRC_ARITH_H */
