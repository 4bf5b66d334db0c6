/*
 * out_map.h -- the arithmetic of the reference's output stage behind the limiter / the SBR tools, on PCM16 words, for host
 * (libxaac_host.so: xaac_out_map_apply_host, the CPU twin) and gfx950 (limiter_kernel.hip, mc_sbr_kernel.hip,
 * out_map_kernel.hip), one function per map:
 *
 *   DOWNMIX_STEREO  ixheaacd_dec_downmix_to_stereo (decoder/ixheaacd_multichannel.c:364-422, call at ixheaacd_api.c:3726)
 *   MONO_MIX        the mono mix of a stereo block (api.c:3735-3757)
 *   MONO_MIX_DUP    ... written to both channels (flag_to_stereo, api.c:3751-3753)
 *   DUP_STEREO      a mono channel written twice (api.c:3645-3661; on WORD32 in front of the limiter there, which sees two equal
 *                   channels and leaves two equal channels: the same words as the limiter's mono output written twice)
 *
 * and the limiter-off hand-off in front of them (ixheaacd_scale_adjust, peak_limiter.c:324-334, + api.c:3676-3681).
 */
#ifndef XAAC_OUT_MAP_H
#define XAAC_OUT_MAP_H

#include <stdint.h>

#include <type_traits>

#include "../../include/xaac_amd.h"
#include "fx.h"

#include "tables_out_map.inc"

/* one term of the downmix: ixheaac_mult32x16in32 (the 48-bit product >> 16, arithmetic) and then >> 14 -- a floor per term, and the
   two shifts are one floor: floor(m x / 2^30).  With both factors doubled that is the high word of a 32 x 32 product (one
   v_mul_hi_i32 on the GPU instead of the two halves of a 64-bit product and a funnel shift): 0 <= m < 2^30 (xo_term_fits), so 2 m
   and 2 x are WORD32s. */
FX_HD int32_t xo_term(int32_t m, int16_t x) { return (int32_t)(((int64_t)(m << 1) * (int64_t)((int32_t)x << 1)) >> 32); }

/* The reference walks the channel elements: an SCE or LFE at slot s adds M[k][0][s] x[s] to the left and M[k][1][s] x[s] to the right
   sum, a CPE at slot s adds M[k][0][s] x[s] to the left and M[k][1][s + 1] x[s + 1] to the right.  That is one coefficient per
   (side, slot) -- those the walk never reads are not part of the mix: zero here.  k = 1 for six channels, 0 for fewer (the 5.0
   matrix serves 3.0 and 4.0 too; in 4.0 the rear centre reaches the left side only: M[0][1][3] = 0).
   coef[0][s] / coef[1][s]: left / right coefficient of slot s.  Returns 0, or -1 for a descriptor that is no downmix of nch channels. */
static inline int xo_resolve(const xaac_out_map *m, int nch, int32_t coef[2][8]) {
  for (int s = 0; s < 8; s++) coef[0][s] = coef[1][s] = 0;
  if (nch < 3 || nch > 6 || m->matrix < 0 || m->matrix > 1 || m->n_elements < 1 || m->n_elements > XAAC_OUT_MAP_MAX_ELEMENTS) return -1;
  uint32_t seen = 0;
  for (int e = 0; e < m->n_elements; e++) {
    const int ty = m->element_type[e], s = m->element_slot[e];
    if ((ty != 0 && ty != 1 && ty != 3) || s < 0 || s + (ty == 1) >= nch) return -1;
    const uint32_t bits = (ty == 1 ? 3u : 1u) << s;
    if (seen & bits) return -1;
    seen |= bits;
    coef[0][s] = xo_down_mix_matrix[m->matrix][0][s];
    coef[1][s + (ty == 1)] = xo_down_mix_matrix[m->matrix][1][s + (ty == 1)];
  }
  return seen == (1u << nch) - 1u ? 0 : -1;
}

/* the reference's temp_l / temp_r are WORD16 and take a WORD16 term at a time: every term fits (xo_term_fits), so the sum of the
   terms in 32 bits, cut to 16 at the end, is the same word whether or not a WORD16 partial sum wrapped on the way */
template <int NCH>
FX_HD void xo_downmix(const int32_t (&cl)[NCH], const int32_t (&cr)[NCH], const int16_t (&x)[NCH], int16_t &l, int16_t &r) {
  int32_t a = 0, b = 0;
  for (int s = 0; s < NCH; s++) a += xo_term(cl[s], x[s]), b += xo_term(cr[s], x[s]);
  l = (int16_t)a, r = (int16_t)b;
}

/* api.c:3749 */
FX_HD int16_t xo_mono_mix(int16_t l, int16_t r) { return (int16_t)((l >> 1) + (r >> 1)); }

/* ixheaacd_scale_adjust (a wrapping multiply by 2^qshift_adj) and ixheaac_round16 behind it */
FX_HD int16_t xo_scale_round16(int32_t x, int qshift_adj) { return fx_round16(fx_shlw(x, qshift_adj)); }

/* The (map kind, channels in, channels out) rows the GPU has a kernel for -- the one list of them: xo_out_channels answers the
   checks from it and xo_dispatch hands a row to the launchers as compile-time values, so a pair that passes a check has a kernel. */
#define XO_MAP_ROWS(X)                                                                                                              \
  X(XAAC_OUT_MAP_NONE, 1, 1) X(XAAC_OUT_MAP_NONE, 2, 2) X(XAAC_OUT_MAP_NONE, 3, 3)                                                  \
  X(XAAC_OUT_MAP_NONE, 4, 4) X(XAAC_OUT_MAP_NONE, 5, 5) X(XAAC_OUT_MAP_NONE, 6, 6)                                                  \
  X(XAAC_OUT_MAP_DOWNMIX_STEREO, 3, 2) X(XAAC_OUT_MAP_DOWNMIX_STEREO, 4, 2)                                                         \
  X(XAAC_OUT_MAP_DOWNMIX_STEREO, 5, 2) X(XAAC_OUT_MAP_DOWNMIX_STEREO, 6, 2)                                                         \
  X(XAAC_OUT_MAP_MONO_MIX, 2, 1) X(XAAC_OUT_MAP_MONO_MIX_DUP, 2, 2) X(XAAC_OUT_MAP_DUP_STEREO, 1, 2)

/* channels a map leaves of `nch`; 0: the map does not take that many.  (No map leaves any count as it is: the host twin copies
   the seven and eight channels there is no kernel for; the GPU entry points bound the count themselves.) */
static inline int xo_out_channels(int kind, int nch) {
#define XO_ROW(k, n, oc) \
  if (kind == k && nch == n) return oc;
  XO_MAP_ROWS(XO_ROW)
#undef XO_ROW
  return kind == XAAC_OUT_MAP_NONE ? nch : 0;
}

/* f(integral_constant<int, NCH>, integral_constant<int, MAP>) for the row of (kind, nch); false: there is no such row */
template <class F>
static inline bool xo_dispatch(int kind, int nch, F &&f) {
#define XO_ROW(k, n, oc)                                                         \
  if (kind == k && nch == n) {                                                   \
    f(std::integral_constant<int, n>(), std::integral_constant<int, (int)k>());  \
    return true;                                                                 \
  }
  XO_MAP_ROWS(XO_ROW)
#undef XO_ROW
  return false;
}

/* What the sums of a row can reach, over the table itself (the way xp_gsum_fits looks at its table): the largest |term| of a
   coefficient m is ceil(m / 2^15) -- at x = -32768, where the floor rounds away from zero -- so a row's sums stay within
   +- sum ceil(m / 2^15).  Returns the largest such bound over the rows of matrix k; *row_sum the largest plain sum of a row.
   (The table holds the 5.0 and the 5.1 matrix: a stream of more than six channels does not reach this code.)
   No row sums to 2^30, so no sum passes +32767; the 5.1 rows reach -32769 by the floors when the four channels of a side all sit
   at -32768, which wraps to +32767 in the reference's WORD16 sums and in xo_downmix's final cut alike. */
static inline int32_t xo_row_bound(int k, int64_t *row_sum) {
  int32_t worst = 0;
  int64_t sum_worst = 0;
  for (int side = 0; side < 2; side++) {
    int32_t bound = 0;
    int64_t sum = 0;
    for (int s = 0; s < 8; s++) {
      const int32_t m = xo_down_mix_matrix[k][side][s];
      bound += (int32_t)(((int64_t)m + 32767) >> 15);
      sum += m;
    }
    worst = bound > worst ? bound : worst;
    sum_worst = sum > sum_worst ? sum : sum_worst;
  }
  if (row_sum) *row_sum = sum_worst;
  return worst;
}
/* every coefficient is in [0, 2^30): a term is a WORD16 (|term| <= 2^15), which the reference's (WORD16) cast of it relies on */
static inline int xo_term_fits(void) {
  for (int k = 0; k < 2; k++)
    for (int side = 0; side < 2; side++)
      for (int s = 0; s < 8; s++)
        if (xo_down_mix_matrix[k][side][s] < 0 || xo_down_mix_matrix[k][side][s] >= (1 << 30)) return 0;
  return 1;
}

#endif /* XAAC_OUT_MAP_H */
