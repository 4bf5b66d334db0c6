/*
 * sbr_ps_frame.h -- one whole frame (32 QMF slots, or 30 for the 960-sample cores of DAB+ / DRM) of the fixed-point
 * parametric-stereo tool, arranged for a 64-lane wave instead of for a slot loop.
 *
 * The reference runs the tool slot by slot inside the left channel's synthesis loop (decoder/ixheaacd_qmf_dec.c:
 * 1015-1031 -> ixheaacd_apply_ps, thumb_ps_dec.c:69).  Of everything it does per slot only three things are
 * recursions over the slots:
 *   - the transient detector's three smoothed values per bin            (ps_dec.c:547-590),
 *   - the all-pass chains of the 10 hybrid sub-bands and QMF bands 3..22 (ps_dec.c:236 / :339: delay lines),
 *   - the envelope counter that decides where new mixing coefficients start (qmf_dec.c:1019).
 * The rest -- hybrid analysis (a FIR), band powers, the bin sums, the transient ratio's division, the plain 14- and
 * 1-slot delays, the interpolated 2x2 rotation (H advances by a constant per slot: H_l = H_0 + n * delta mod 2^16),
 * the hybrid synthesis sums, the scale shifts -- depends on its slot only.  So the frame runs in phases:
 *
 *   P1 hybrid analysis of all NS slots            lane = slot / (band, slot)
 *   P2 envelope walk: segments of constant delta  scalar; coefficients of each border: lane = parameter group
 *   P3 band powers, all-pass / delay inputs       lane = QMF band, loop over slots (coalesced row reads)
 *      group sums of the upper bins               a running sum over the band lanes per slot, then lane = (slot, group):
 *                                                 the addends are >= 0, so the saturating sum is min(MAX, exact sum)
 *                                                 whatever the order (xp_gsum_*)
 *   P4 transient detector                         lane = bin (peak decay) | 32 + bin (energy), loop over slots (the
 *                                                 recursion), then the 640 ratios (one division each) lane-parallel
 *   P5 all-pass chains                            lane = chain (30), loop over slots (the recursion)
 *   P6 rotation in the hybrid domain + its sums   lane = (slot, re | im), loop over the ten sub-bands
 *   P7 delays, rotation, output scaling           lane = QMF band, loop over slots (coalesced row reads / writes)
 * Every value is computed by the same operations in the same order as in the slot loop (sbr_ps.h, which stays the
 * oracle's restatement of the reference); what changes is only when.  The same source compiled for the host with
 * lane count 1 is checked against that slot loop on the reference's captured frames and on fuzzed side info
 * (tests/test_ps_frame_cpu.py) before the GPU sees it.
 *
 * The slot count NS is a template parameter: the reference's synthesis loop passes num_time_slots as no_col
 * (qmf_dec.c:1016-1030), so at 30 slots the tool runs over 30 sub-samples, the hybrid look-ahead's delay shift switches
 * at slot NS - 6 = 24 (thumb_ps_dec.c:77-85) and the parser ends the PS grid at border 30 (ps_bitdec.c:106, :243-249).
 * Borders no parser produces are handled as the slot loop would: the envelope counter only ever looks at its
 * current border (a border that lies behind the current slot is never reached), and if the first border is not
 * slot 0 the band limit `usb` (and the clearing of newly active all-pass delay lines, ps_dec.c:733-757) switches
 * at that slot.
 */
#ifndef XAAC_SBR_PS_FRAME_H
#define XAAC_SBR_PS_FRAME_H

#include <stddef.h>

#include "sbr_ps.h"

#ifndef XP_T
#define XP_T(i) /* optional phase timer hook (tools/prof_sbr_core.py ps) */
#endif

#define XP_NO_PS_SCALE 0x7fffffff
#define XP_MAX_SEG (XAAC_PS_MAX_ENV + 2) /* the segment carried in from the last frame + one per border (env 0..5) */

#if defined(__HIPCC__)
#define XP_UNROLL _Pragma("unroll")
#define XP_NOUNROLL _Pragma("nounroll")
#define XP_LAMBDA_INLINE __attribute__((always_inline))
#else
#define XP_UNROLL
#define XP_NOUNROLL
#define XP_LAMBDA_INLINE
#endif

struct XpFrameWork {
  union {                    /* scratch areas that are never live together */
    int32_t hyb_u[3][2][44]; /* P1: hybrid filter input of QMF bands 0..2: 12 slots of history + this frame's NS */
    uint32_t gscan[32][8];   /* P3: per slot the running sum of the group addends at the last band of groups 0..5; column 6:
                                the other lanes' stores */
    int32_t peak[32][20];    /* P4: transient peak difference */
    uint32_t dl[14 + 32][13]; /* P5/P7: the 14-slot delay lines of QMF bands 23..34, unrolled over the frame: row l holds what
                                slot l reads (rows 0..13: the state's ring in slot order), slot l writes row l + 14 -- the
                                band's rounded sample, or what it read if the band is not active.  Column 12 takes the other
                                lanes' stores, so that the store needs no predicate */
  };
  int32_t hyb_l[32][20];     /* left hybrid sub-band samples of every slot: re 0..9 | im 10..19 */
  union {
    int32_t binpw[32][20];   /* P3: bin powers; P4: smoothed energy ... */
    int16_t ratio[32][20];   /* ... compacted in place into the transient ratios (entry i lands inside entry i / 2) */
  };
  uint32_t ap_h[32][11];     /* outputs of the hybrid sub-bands' all-pass chains (re, im pairs); column 10: the other lanes' */
  uint32_t seg_hd[XP_MAX_SEG][4][24]; /* per segment and group: H11, H12, H21, H22 before the segment's first slot (high
                                          half) and their per-slot increments (low half): a border reloads four words */
};
static_assert(sizeof(XpFrameWork::dl) <= sizeof(XpFrameWork::peak), "the unrolled 14-slot lines fit the scratch union as it was");
template <bool B>
struct XpBool {
  static constexpr bool value = B;
};

FX_HD int xp_popc(uint32_t v) { return __builtin_popcount(v); }
FX_HD int xp_clz(uint32_t v) { return __builtin_clz(v); } /* v != 0 */
FX_HD uint32_t xp_pack16(int16_t lo, int16_t hi) { return (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16); }
FX_HD int16_t xp_lo16(uint32_t v) { return (int16_t)(v & 0xffffu); }
FX_HD int16_t xp_hi16(uint32_t v) { return (int16_t)(v >> 16); }

/* a.lo * b.lo + a.hi * b.hi of two packed pairs of int16, wrapping: one v_dot2_i32_i16 on the GPU.  Written out: the
   builtin (__builtin_amdgcn_sdot2 with a zero addend) is selected as the accumulating two-operand v_dot2c_i32_i16 with a
   v_mov_b32 of zero in front of it -- eight extra instructions in every slot of the walk. */
FX_HD int32_t xp_dot2(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  int32_t r;
  asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
  return r;
#else
  return (int32_t)((uint32_t)((int32_t)xp_lo16(a) * xp_lo16(b)) + (uint32_t)((int32_t)xp_hi16(a) * xp_hi16(b)));
#endif
}
/* a segment's word of XpFrameWork::seg_hd n slots into the segment: H + n * delta, wrapping as the reference's int16 adds do */
FX_HD int16_t xp_seg_coeff(uint32_t hd, int n) { return (int16_t)(xp_hi16(hd) + n * xp_lo16(hd)); }
/* two neighbouring int16 of an array, the first at an even index of a word-aligned row, as one packed pair: one LDS word
   read on the GPU */
FX_HD uint32_t xp_load_pair(const int16_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t __attribute__((may_alias)) xp_u32_alias;
  return *reinterpret_cast<const xp_u32_alias *>(p);
#else
  return xp_pack16(p[0], p[1]);
#endif
}
FX_HD void xp_store_pair(int16_t *p, uint32_t v) { /* ... and the store that goes with it */
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t __attribute__((may_alias)) xp_u32_alias;
  *reinterpret_cast<xp_u32_alias *>(p) = v;
#else
  p[0] = xp_lo16(v);
  p[1] = xp_hi16(v);
#endif
}
/* a complex 16-bit rotation factor (re, im) as the two pairs the products of xp_allpass take: (re, -im) gives the real
   part, (im, re) the imaginary one.  The PS tables hold no -32768 (tests/test_tables.py), so -im is a short and the sum of
   two products of a sample and a factor stays below 2^31: the reference's saturating add / subtract never saturates
   there, and the wrapping dot product is the same number. */
struct XpPhase {
  uint32_t re_pair, im_pair;
};
FX_HD XpPhase xp_phase_pairs(int16_t re, int16_t im) {
  XpPhase p;
  p.re_pair = xp_pack16(re, (int16_t)-im);
  p.im_pair = xp_pack16(im, re);
  return p;
}
/* The chain's 16-bit arithmetic on (re, im) pairs, both halves at once.  (int16_t)(v >> 15) is bits 15..30 of v; of a
   product with twice the factor those are the word's high half, which a byte permute moves -- so a sample pair times a
   decay factor is two 24-bit multiplies and one v_perm_b32, and the wrapping adds and subtracts are packed ones.  (As
   single int16 values every product was a multiply, a shift and its own add, 17 instructions per link; now 13.) */
FX_HD uint32_t xp_q15_pair(int32_t a, int32_t b) { /* ((int16_t)(a >> 15), (int16_t)(b >> 15)) */
  return (((uint32_t)a >> 15) & 0xffffu) | (((uint32_t)b << 1) & 0xffff0000u);
}
FX_HD uint32_t xp_hi_pair(int32_t a, int32_t b) { /* the high halves of a and b */
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x07060302u);
#else
  return ((uint32_t)a >> 16) | ((uint32_t)b & 0xffff0000u);
#endif
}
/* xs_mult16_shl of both halves of p with the factor f, handed in as 2 * f (17 bits) */
FX_HD uint32_t xp_mult16_shl_pair(uint32_t p, int32_t f2) {
#if defined(__HIP_DEVICE_COMPILE__)
  return xp_hi_pair(__mul24(xp_lo16(p), f2), __mul24(xp_hi16(p), f2));
#else
  return xp_hi_pair((int32_t)((uint32_t)(int32_t)xp_lo16(p) * (uint32_t)f2), (int32_t)((uint32_t)(int32_t)xp_hi16(p) * (uint32_t)f2));
#endif
}
/* xp_m16x16_shl (sbr_ps.h) with the doubling moved into the second factor: one 24-bit multiply per product */
FX_HD int32_t xp_m16x16_shl_pre(int16_t a, int32_t b2) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul24(a, b2);
#else
  return (int32_t)((uint32_t)(int32_t)a * (uint32_t)b2);
#endif
}
FX_HD uint32_t xp_add16_pair(uint32_t a, uint32_t b) { /* wrapping, per half */
#if defined(__HIP_DEVICE_COMPILE__)
  typedef short xp_short2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, (xp_short2)(__builtin_bit_cast(xp_short2, a) + __builtin_bit_cast(xp_short2, b)));
#else
  return ((a + b) & 0xffffu) | ((a & 0xffff0000u) + (b & 0xffff0000u));
#endif
}
FX_HD uint32_t xp_sub16_pair(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef short xp_short2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, (xp_short2)(__builtin_bit_cast(xp_short2, a) - __builtin_bit_cast(xp_short2, b)));
#else
  return ((a - b) & 0xffffu) | ((a & 0xffff0000u) - (b & 0xffff0000u));
#endif
}
/* xp_allpass (sbr_ps.h, ps_dec.c:236 / :339) on packed (re, im) pairs: d0 = the 2-slot line's oldest entry (replaced by the
   new sample), e0 / e1 / e2 = the three links' entries at their read positions (replaced); returns the chain's output pair */
FX_HD uint32_t xp_allpass_packed(uint32_t &d0, uint32_t new_pair, const XpPhase &ph, uint32_t &e0, uint32_t &e1, uint32_t &e2,
                                 const XpPhase &p0, const XpPhase &p1, const XpPhase &p2, int16_t decay0, int16_t decay1,
                                 int16_t decay2) {
  uint32_t in = xp_q15_pair(xp_dot2(d0, ph.re_pair), xp_dot2(d0, ph.im_pair));
  d0 = new_pair;
  uint32_t *e[3] = {&e0, &e1, &e2};
  const XpPhase *pp[3] = {&p0, &p1, &p2};
  const int32_t decay2x[3] = {2 * decay0, 2 * decay1, 2 * decay2};
  XP_UNROLL
  for (int m = 0; m < 3; m++) {
    const uint32_t s = *e[m];
    const uint32_t t = xp_sub16_pair(xp_q15_pair(xp_dot2(s, pp[m]->re_pair), xp_dot2(s, pp[m]->im_pair)),
                                     xp_mult16_shl_pair(in, decay2x[m]));
    *e[m] = xp_add16_pair(in, xp_mult16_shl_pair(t, decay2x[m]));
    in = t;
  }
  return in;
}

/* env_calc.c:1099 on one word, without a branch: a left count and a right count of which at most one is not zero (a shift
   by zero is the identity either way).  Inside the slot walks the counts are lane constants; as three-way branches per word
   the same thing cost a dozen scalar instructions around two vector ones. */
FX_HD int32_t xp_adj_word(int32_t v, int shift) {
  if (shift > 31) shift = 31;
  if (shift < -31) shift = -31;
  const int shl = shift > 0 ? shift : 0, shr = shift < 0 ? -shift : 0;
  return (int32_t)((uint32_t)v << shl) >> shr;
}

/* floor(u * 2^15 / v) for u < 2^16 and 2^14 <= v < 2^16 without an integer division.  u * 2^15 (sixteen significant bits)
   and v are exact as floats; with a reciprocal r good to one unit in the last place (the host's division is, and so is
   v_rcp_f32) and the product rounded once, the product is off by less than 2^17 * 2^-22 = 2^-5 and its integer part is the
   quotient or a neighbour of it; the remainder says which.  (The compiler's 32-bit division: two dozen instructions behind
   a predicate; this: a dozen, no branch.)  r is a parameter so that a test can hand in the neighbours of 1 / v too. */
FX_HD uint32_t xp_quot15_rcp(uint32_t u, uint32_t v, float r) {
  const uint32_t n = u << 15;
  uint32_t q = (uint32_t)((float)n * r);
#if defined(__HIP_DEVICE_COMPILE__)
  const int32_t rem = (int32_t)(n - __umul24(q, v)); /* q < 2^18, v < 2^16 */
#else
  const int32_t rem = (int32_t)(n - q * v);
#endif
  q += rem >= (int32_t)v ? 1u : 0u;
  q -= rem < 0 ? 1u : 0u;
  return q;
}
FX_HD uint32_t xp_quot15(uint32_t u, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return xp_quot15_rcp(u, v, __builtin_amdgcn_rcpf((float)v));
#else
  return xp_quot15_rcp(u, v, 1.0f / (float)v);
#endif
}
/* xp_divide16_pos (sbr_ps.h, ps_dec.c:212) where the frame calls it: 0 <= op1 < op2, so that the normalised heads are
   u <= v with v in [2^14, 2^15) -- the same word for every such pair (tests/test_ps_prep_cpu.py; u = 0 gives 0 by itself) */
FX_HD int32_t xp_divide16_norm(int32_t op1, int32_t op2) {
  const int nrm = fx_norm32(op2);
  const uint32_t u = (uint32_t)xs_shl(op1, nrm) >> 16, v = (uint32_t)xs_shl(op2, nrm) >> 16;
  return (int32_t)(xp_quot15(u, v) & 0xffffu);
}

/* ps_dec.c:470-519: the eight transient-detector bins that live in the hybrid domain */
FX_HD int32_t xp_bin_power_hyb(const XpTables *T, int bin, const int32_t *re, const int32_t *im) {
  if (bin < 2) {
    const int a = bin == 0 ? 0 : 4, b = bin == 0 ? 5 : 1;
    int32_t pw = xp_power(re[a], im[a]);
    pw = fx_add_sat(pw, fx_mul32x16(re[b], (int16_t)(re[b] >> 16)));
    return fx_add_sat(pw, fx_mul32x16(im[b], (int16_t)(im[b] >> 16)));
  }
  const int sb = T->borders_group[bin + 2];
  return xp_power(re[sb], im[sb]);
}

/* ---- the group sums of transient-detector bins 14..19 (ps_dec.c:520-545; sbr_ps.h: xp_bin_power, bin >= 14) as
   differences of a running sum.  The reference adds a group's shifted band powers with saturating adds; the addends are
   >= 0, so that is min(0x7fffffff, exact sum) whatever the order -- and with the table's shifts the exact sum of every
   group fits an unsigned word (xp_gsum_fits: bands x (0x7fffffff >> shift) < 2^32).  So the sums may wrap: with
   S[k] = addend[0] + .. + addend[k] modulo 2^32 over all 64 bands (bands below 9, bands at or above the slot's band limit
   and whatever else a group does not read add zero or cancel), group [b0, b1) is
       min(0x7fffffff, (S[b1 - 1] - S[b0 - 1]) mod 2^32),
   bit for bit the reference's value.  On the GPU the lane is the band and S is six data-parallel-primitive adds (the scan of
   sbr_core.h: xs_prefix_max with + for max); on the host it is the running sum of the band loop. */
/* the band's addend: its power in its group's scale if a group reads it, else nothing */
FX_HD uint32_t xp_gsum_addend(int32_t pw, int group_shift, bool counts) { return counts ? (uint32_t)(pw >> group_shift) : 0u; }
/* the same with "does not count" folded into the shift: a power is >= 0 (xp_power: two products of a word and its own high
   half), so a count of 31 leaves nothing of it -- the slot's predicate and select become a choice between two lane constants */
FX_HD int xp_gsum_shift(int group_shift, bool counts) { return counts ? group_shift : 31; }
FX_HD uint32_t xp_gsum_addend_sh(int32_t pw, int shift) { return (uint32_t)(pw >> shift); }
/* S of this band: `run` carries the sum over the bands before it where bands are walked one after the other (the host) */
FX_HD uint32_t xp_gsum_scan(const XsCx &cx, uint32_t a, uint32_t &run) {
#if defined(__HIP_DEVICE_COMPILE__)
  int32_t r = (int32_t)a;
#define XP_DPP_ADD(ctrl, rows) r += __builtin_amdgcn_update_dpp(0, r, ctrl, rows, 0xf, false); /* no source lane: adds 0 */
  XP_DPP_ADD(0x111, 0xf) /* row_shr:1 */
  XP_DPP_ADD(0x112, 0xf) /* row_shr:2 */
  XP_DPP_ADD(0x114, 0xf) /* row_shr:4 */
  XP_DPP_ADD(0x118, 0xf) /* row_shr:8 */
  XP_DPP_ADD(0x142, 0xa) /* row_bcast:15 into rows 1 and 3 */
  XP_DPP_ADD(0x143, 0xc) /* row_bcast:31 into rows 2 and 3 */
#undef XP_DPP_ADD
  (void)cx;
  (void)run;
  return (uint32_t)r;
#else
  (void)cx;
  run += a;
  return run;
#endif
}
/* the group's sum from S at its last band and S at the band in front of its first */
FX_HD int32_t xp_gsum_sum(uint32_t s_last, uint32_t s_before) {
  const uint32_t d = s_last - s_before;
  return (int32_t)(d < 0x7fffffffu ? d : 0x7fffffffu);
}
/* The bound the wrapping sums rest on, worked out from the tables themselves (borders_group[16..22] = 9 11 14 18 23 35 64,
   group_shift = 0 1 1 2 3 4: 2, 3, 4, 5, 12, 29 bands of at most 0x7fffffff >> shift, the largest sum 29 * (2^27 - 1)).  The
   tables are generated data and no constant expressions, so this is a function and not a static_assert:
   tests/test_ps_phases_cpu.py calls it on the tables the library is built with, a changed table fails there. */
FX_HD bool xp_gsum_fits(const XpTables *T) {
  if (T->borders_group[16] != 9) return false; /* the first group starts where the addends start (xp_ps_frame, P3) */
  for (int g = 0; g < 6; g++) {
    const int b0 = T->borders_group[16 + g], b1 = T->borders_group[17 + g], shift = T->group_shift[g];
    if (b1 <= b0 || b1 > 64 || shift < 0 || shift > 31) return false;
    if ((uint64_t)(b1 - b0) * (uint64_t)(0x7fffffff >> shift) >= ((uint64_t)1 << 32)) return false;
  }
  return true;
}

/* P4, the transient detector of a whole frame (ps_dec.c:547-590; sbr_ps.h: xp_decorrelation has it per slot): peak decay
   against smoothed energy, per bin.  In: w->binpw[l][bin], the bin powers of the NS slots; out: w->ratio[l][bin] and the
   three carried values of every bin.  Two lanes per bin: lane `bin` carries the peak decay and its smoothed difference,
   lane 32 + bin the smoothed energy.  Both smoothings are acc = acc * 0.75 + (t >> 2) with their own t, so the step is
   issued once for the two (as one lane per bin it was three recursions one after the other in every step). */
template <int NS, class PS>
FX_HD void xp_transient_frame(const XsCx &cx, PS *ps, XpFrameWork *w) {
  XS_PAR(i, 0, 32 + 20) {
    const int bin = i & 31;
    const bool en = i >= 32;
    if (bin >= 20) continue;
    int32_t pd = ps->peak_decay_diff[bin], acc = en ? ps->energy_prev[bin] : ps->peak_decay_diff_prev[bin];
    int32_t *out = en ? &w->binpw[0][bin] : &w->peak[0][bin]; /* (rows of 20 words both) */
    int32_t pin[NS]; /* the bin's NS powers first: the recursion below then waits for no LDS load */
    XP_UNROLL
    for (int l = 0; l < NS; l++) pin[l] = w->binpw[l][bin];
    cx.sync(); /* both lanes of a bin have read its powers before the energy overwrites them */
    XP_UNROLL
    for (int l = 0; l < NS; l++) {
      int32_t pw = fx_shl(pin[l], 1);
      if (pw < 0) pw = 0;
      pd = fx_mul32x16_shl(pd, 0x620a);
      if (pw > pd) pd = pw;
      const int32_t t = en ? pw : fx_sub_sat(pd, pw);
      acc = fx_add_sat(fx_mul32x16_shl(acc, 0x6000), t >> 2);
      out[20 * l] = en ? acc : fx_add_sat(acc, acc >> 1);
    }
    if (en) {
      ps->energy_prev[bin] = acc;
    } else {
      ps->peak_decay_diff[bin] = pd;
      ps->peak_decay_diff_prev[bin] = acc;
    }
  }
  cx.sync();
#if defined(__HIP_DEVICE_COMPILE__)
  { /* the 640 (energy, peak) pairs of all ten trips are read before any lane stores a ratio: entry i lands inside word
       i / 2 of the energies, and ten trips of their own were ten LDS round trips with a pair of fences each.  (Rows 30 and
       31 of a 30-slot frame hold older words; their ratios are not read.) */
    int32_t pk[10], nrg[10];
    XP_UNROLL
    for (int t = 0; t < 10; t++) {
      pk[t] = (&w->peak[0][0])[64 * t + cx.lane];
      nrg[t] = (&w->binpw[0][0])[64 * t + cx.lane];
    }
    cx.sync();
    XP_UNROLL
    for (int t = 0; t < 10; t++)
      (&w->ratio[0][0])[64 * t + cx.lane] = pk[t] <= nrg[t] ? (int16_t)0x7fff : (int16_t)xp_divide16_norm(nrg[t], pk[t]);
  }
#else
  for (int i = 0; i < 20 * NS; i++) { /* in order: entry i / 2 has been consumed */
    const int32_t pk = (&w->peak[0][0])[i], nrg = (&w->binpw[0][0])[i];
    (&w->ratio[0][0])[i] = pk <= nrg ? (int16_t)0x7fff : (int16_t)xp_divide16_norm(nrg, pk);
  }
#endif
}

/* One frame of NS slots (32, or 30).  xl: the stream's QMF matrix, slot 0 at xl (rows of 64 re | 64 im; rows 0..NS + 5
   are read, rows 0..NS - 1 are rewritten with the left channel in the scale the synthesis bank expects); xr: NS rows out,
   the right channel.  lb/ov_lb/hb_scale, st_syn, lsb, usb: what the SBR core left for the synthesis bank.  Returns
   ps_scale. */
template <int NS = 32, class PS>
FX_HD int xp_ps_frame(const XsCx &cx, const XpTables *T, PS *ps, const xaac_ps_frame *pf, XpFrameWork *w, int32_t *xl,
                      int32_t *xr, int lb_scale, int ov_lb_scale, int hb_scale, int st_syn, int lsb, int usb,
                      int ps_scale_done = XP_NO_PS_SCALE) {
  static_assert(NS == 32 || NS == 30, "frames of 32 or 30 QMF slots");
#if defined(__HIP_DEVICE_COMPILE__)
  /* The matrix rows this frame reads before anything rewrites them, fetched now: P1's look-ahead words of QMF bands
     0..2 (lane = slot) and P3's NS slots of the lane's band (slots NS..31 of a shorter frame: zero powers, not used).  Issued ahead of the state rescale and the hybrid
     filters, their memory latency is covered instead of being paid once per phase and per group of eight slots. */
  int32_t p1v[3][2], p3re[32], p3im[32];
  {
    const int l1 = cx.lane & 31;
    XP_UNROLL
    for (int b = 0; b < 3; b++) {
      p1v[b][0] = xl[(l1 + 6) * 128 + b];
      p1v[b][1] = xl[(l1 + 6) * 128 + 64 + b];
    }
    XP_UNROLL
    for (int l = 0; l < 32; l++) {
      p3re[l] = NS == 32 || l < NS ? xl[l * 128 + cx.lane] : 0;
      p3im[l] = NS == 32 || l < NS ? xl[l * 128 + 64 + cx.lane] : 0;
    }
  }
#endif
  /* sbr_dec.c:1252.  The GPU kernel has been through it already, on the state words in registers on their way into LDS
     (sbr_ps_kernel.hip: xp_init_ps_scale_regs), and hands the result in */
  const int ps_scale = ps_scale_done != XP_NO_PS_SCALE ? ps_scale_done : xp_init_ps_scale(cx, ps, lb_scale, ov_lb_scale, hb_scale);
  const int ov_lb_shift = ps_scale - ov_lb_scale, lb_shift = ps_scale - lb_scale, hb_shift = ps_scale - hb_scale;
  const int common_shift = (st_syn - ps_scale) - 8;
  XP_T(1);

  /* ---- P1: hybrid analysis (hybrid.c:214: a 13-tap FIR on QMF bands 0..2 looking six slots ahead).  Input of step
     l: row l + 6 as adjust_scale leaves it (qmf_dec.c:937: slots of the next frame are not rescaled), then the
     delay-buffer shift of thumb_ps_dec.c:77 (from slot NS - MAX_OV_COLS on). */
  XS_PAR(l, 0, NS) {
    const int shiftdelay = l < NS - 6 ? 0 : (int16_t)(lb_scale - ps_scale);
    for (int b = 0; b < 3; b++) {
      const int sha = l + 6 < NS ? (b < lsb ? lb_shift : (b < usb ? hb_shift : 0)) : 0;
      for (int c = 0; c < 2; c++) {
#if defined(__HIP_DEVICE_COMPILE__)
        int32_t v = xp_adj_word(p1v[b][c], sha); /* lane = slot l */
#else
        int32_t v = xp_adj_word(xl[(l + 6) * 128 + 64 * c + b], sha);
#endif
        v = shiftdelay < 0 ? fx_shl(v, -shiftdelay) : fx_shr(v, shiftdelay);
        w->hyb_u[b][c][12 + l] = v;
      }
    }
  }
  XS_PAR(i, 0, 12)
    for (int b = 0; b < 3; b++) {
      w->hyb_u[b][0][i] = ps->hyb_buf[b][0][i];
      w->hyb_u[b][1][i] = ps->hyb_buf[b][1][i];
    }
  cx.sync();
  XS_PAR(l, 0, NS) { /* QMF band 0: eight-channel filter, six sub-bands */
    int32_t re[8], im[8];
    xp_filt_8ch(T, &w->hyb_u[0][0][l], &w->hyb_u[0][1][l], re, im);
    for (int k = 0; k < 6; k++) {
      w->hyb_l[l][k] = re[k];
      w->hyb_l[l][10 + k] = im[k];
    }
  }
  XS_PAR(i, 0, 64) { /* QMF bands 1 and 2: two sub-bands each */
    const int b = 1 + (i >> 5), l = i & 31;
    if (NS != 32 && l >= NS) continue;
    int32_t re[2], im[2];
    xp_filt_2ch(T, &w->hyb_u[b][0][l], &w->hyb_u[b][1][l], re, im);
    w->hyb_l[l][4 + 2 * b] = re[0];
    w->hyb_l[l][5 + 2 * b] = re[1];
    w->hyb_l[l][14 + 2 * b] = im[0];
    w->hyb_l[l][15 + 2 * b] = im[1];
  }
  XS_PAR(i, 0, 12)
    for (int b = 0; b < 3; b++) {
      ps->hyb_buf[b][0][i] = w->hyb_u[b][0][NS + i];
      ps->hyb_buf[b][1][i] = w->hyb_u[b][1][NS + i];
    }
  cx.sync();
  XP_T(2);

  /* ---- P2: the envelope walk of qmf_dec.c:1019 ("if slot == border[env]: init_rot_env; env++").  Segment 0
     continues the last frame's interpolation from the state; every border reached starts a new one. */
  XS_PAR(g, 0, XAAC_PS_GROUPS) {
    w->seg_hd[0][0][g] = xp_pack16(ps->delta_h11_h12[2 * g], ps->H11_H12[2 * g]);
    w->seg_hd[0][1][g] = xp_pack16(ps->delta_h11_h12[2 * g + 1], ps->H11_H12[2 * g + 1]);
    w->seg_hd[0][2][g] = xp_pack16(ps->delta_h21_h22[2 * g], ps->H21_H22[2 * g]);
    w->seg_hd[0][3][g] = xp_pack16(ps->delta_h21_h22[2 * g + 1], ps->H21_H22[2 * g + 1]);
  }
  const int usb_prev = cx.uni(ps->usb);
  uint32_t seg_mask = 0; /* bit l: a border was reached at slot l -- segment popcount(bits 0..l) starts there (a scalar) */
  int clear_slot = NS; /* first slot that runs with the new usb: the slot of border 0, if it is reached at all */
  {
    int env = 0, nseg = 1;
    int next = cx.uni(pf->border_position[0]); /* the border the counter is waiting for; 64 = none left */
    for (int l = 0; l < NS; l++) {
      if (l == next) {
        if (env == 0) clear_slot = l;
        cx.sync();
        xp_rot_env_coeffs(cx, T, ps, pf, env); /* ps->H.. = the old targets, ps->delta.., ps->h.._vec = the new ones */
        XS_PAR(g, 0, XAAC_PS_GROUPS) {
          w->seg_hd[nseg][0][g] = xp_pack16(ps->delta_h11_h12[2 * g], ps->H11_H12[2 * g]);
          w->seg_hd[nseg][1][g] = xp_pack16(ps->delta_h11_h12[2 * g + 1], ps->H11_H12[2 * g + 1]);
          w->seg_hd[nseg][2][g] = xp_pack16(ps->delta_h21_h22[2 * g], ps->H21_H22[2 * g]);
          w->seg_hd[nseg][3][g] = xp_pack16(ps->delta_h21_h22[2 * g + 1], ps->H21_H22[2 * g + 1]);
        }
        seg_mask |= 1u << l;
        nseg++;
        env++;
        next = env <= XAAC_PS_MAX_ENV ? cx.uni(pf->border_position[env]) : 64;
      }
    }
  }
  cx.sync();
  XP_T(3);

  /* ---- P3: band powers (ps_dec.c:520-545).  A lane walks its band through eight slots at a time: the sixteen row
     words of the next eight are in flight while these are worked on.  Bands 9..63 feed the group sums of bins 14..19
     (xp_gsum_*): per slot one running sum over the bands, of which the six lanes that end a group keep their value. */
  {
    XP_UNROLL
    for (int c = 0; c < 4; c++) {
      uint32_t run[8] = {0, 0, 0, 0, 0, 0, 0, 0}; /* (host: the running sums of the eight slots over the band loop) */
      XS_PAR(sb, 0, 64) {
        int32_t rre[8], rim[8];
        XP_UNROLL
        for (int ls = 0; ls < 8; ls++) {
#if defined(__HIP_DEVICE_COMPILE__)
          rre[ls] = p3re[8 * c + ls]; /* lane = band sb */
          rim[ls] = p3im[8 * c + ls];
#else
          rre[ls] = xl[(8 * c + ls) * 128 + sb];
          rim[ls] = xl[(8 * c + ls) * 128 + 64 + sb];
#endif
        }
        const int gsh = sb < 11 ? 0 : (sb < 18 ? 1 : (sb < 23 ? 2 : (sb < 35 ? 3 : 4))); /* group_shift of the band's group */
        /* where the lane's word of a slot goes: bands 3..8 are bins of their own (their power), the last band of group g
           keeps the running sum in column g of gscan, every other lane writes the spare column 6 -- one store per slot
           through a lane pointer and a lane stride instead of a tree of predicated regions */
        const bool own_bin = sb >= 3 && sb < 9;
        int gcol = 6;
        XP_UNROLL
        for (int g = 0; g < 6; g++) gcol = sb == T->borders_group[17 + g] - 1 ? g : gcol;
        int32_t *dst = own_bin ? &w->binpw[8 * c][sb + 5] : reinterpret_cast<int32_t *>(&w->gscan[8 * c][gcol]);
        const int dstride = own_bin ? 20 : 8;
        /* lane constants of the slot body: the band's scale shift in the overlap slots and behind them, and the group
           shift under the old band limit and under the new one (which slot takes which is a fact of the unrolled loop
           for the first, one uniform compare for the second) */
        const int sh_ov = sb < lsb ? ov_lb_shift : (sb < usb ? hb_shift : 0), sh_lb = sb < lsb ? lb_shift : (sb < usb ? hb_shift : 0);
        const int gsh_old = xp_gsum_shift(gsh, sb >= 9 && sb < usb_prev), gsh_new = xp_gsum_shift(gsh, sb >= 9 && sb < usb);
        XP_UNROLL
        for (int ls = 0; ls < 8; ls++) {
          const int l = 8 * c + ls;
          const int sh = l < 6 ? sh_ov : sh_lb;
          const int32_t re = xp_adj_word(rre[ls], sh), im = xp_adj_word(rim[ls], sh);
          const int32_t pw = xp_power(re, im);
          const uint32_t s = xp_gsum_scan(cx, xp_gsum_addend_sh(pw, l >= clear_slot ? gsh_new : gsh_old), run[ls]);
          dst[ls * dstride] = own_bin ? pw : (int32_t)s;
        }
      }
    }
  }
  cx.sync();
  XS_PAR(i, 0, 6 * NS) { /* bins 14..19 = sums over the groups [9,11) [11,14) [14,18) [18,23) [23,35) [35,64) */
    const int l = i / 6, g = i % 6;
    /* the running sum in front of the group: the group before ends there; in front of the first group (band 9) nothing
       has been added.  (Read by every lane and selected: no predicated region.) */
    const uint32_t prev = w->gscan[l][g > 0 ? g - 1 : 0];
    const uint32_t before = g > 0 ? prev : 0u;
    w->binpw[l][14 + g] = xp_gsum_sum(w->gscan[l][g], before);
  }
  XS_PAR(i, 0, 8 * NS) {
    const int l = i >> 3, bin = i & 7;
    w->binpw[l][bin] = xp_bin_power_hyb(T, bin, &w->hyb_l[l][0], &w->hyb_l[l][10]);
  }
  cx.sync();
  XP_T(4);

  /* ---- P4: transient detector */
  xp_transient_frame<NS>(cx, ps, w);
  cx.sync();
  XP_T(5);

  /* ---- P5 + P7, one walk over the slots per lane.
     All-pass chains (ps_dec.c:236 hybrid sub-bands, :339 QMF bands 3..22 whatever usb is): the chain of QMF band sb
     runs on lane sb -- its input is the lane's own row word, its output feeds the lane's own rotation --, the chains
     of the ten hybrid sub-bands on lanes 32..41 (their outputs go to LDS for P6).  A chain's delay lines (a 2-slot
     line and three links of 3, 4 and 5 slots) are loaded oldest-first into registers, shifted by renaming in the
     unrolled loop, and stored back at the end: no LDS traffic inside the recursion.
     Delays, rotation, output (ps_dec.c:602-648, :893-945, generic:1610): the 14-slot delay reads the lane's own
     column of dl 14 rows back, the 1-slot delay and the interpolated coefficients of the band's group stay in
     registers too.  Bands 0..2 are written by P6. */
  {
    const int idx0 = cx.uni(ps->idx), idx_long0 = cx.uni(ps->idx_long);
    const int is0 = cx.uni(ps->idx_ser[0]), is1 = cx.uni(ps->idx_ser[1]), is2 = cx.uni(ps->idx_ser[2]);
    const int clear_lo = (usb > usb_prev && usb_prev) ? usb_prev : 64; /* ps_dec.c:733-757: bands that just became active */
    const int clear_hi = usb < 23 ? usb : 23;
    const int p14_0 = idx_long0 % 14;
    const int cs_right = common_shift < 0 ? (-common_shift > 31 ? 31 : -common_shift) : 0;
    uint32_t events = seg_mask | (1u << 6); /* bit l: slot l sets lane state of the walk again (see there) */
    if (clear_slot < NS) events |= 1u << clear_slot;
    /* The 14-slot ring of the state, laid out in the order the slots read it: rows 0..13 of dl (four lanes per row, three
       bands each).  From there on the line is a plain look-back of 14 rows -- a slot whose band is not active hands what
       it read on to row l + 14, as the ring keeps an entry nobody overwrites -- and no slot reads the state. */
    static_assert(sizeof(ps->ld[0]) == 24 * sizeof(int16_t), "rows of the 14-slot ring: 24 int16, whole words");
    static_assert(offsetof(PS, ld) % 4 == 0 && alignof(PS) % 4 == 0, "the 14-slot ring starts on a word of a word-aligned state");
    XS_PAR(i, 0, 4 * 14) {
      const int r = i >> 2, j0 = 3 * (i & 3);
      const int pos = p14_0 + r >= 14 ? p14_0 + r - 14 : p14_0 + r;
      XP_UNROLL
      for (int k = 0; k < 3; k++) w->dl[r][j0 + k] = xp_load_pair(&ps->ld[pos][2 * (j0 + k)]);
    }
    cx.sync();
    XS_PAR(sb, 0, 64) {
      /* -- the lane's chain, if it has one */
      const int qmf_chain = sb >= 3 && sb < 23, hyb_chain = sb >= 32 && sb < 42, chain = qmf_chain || hyb_chain;
      const int csb = qmf_chain ? sb : (hyb_chain ? sb - 32 : 3);
      const int di = 9 + 3 * (csb - 3);
      const int16_t *ph = hyb_chain ? &T->frac_delay_phase_fac_qmf_sub_re_im[2 * csb] : &T->frac_delay_phase_fac_qmf_re_im[2 * csb];
      const int16_t *pser = hyb_chain ? &T->frac_delay_phase_fac_qmf_sub_ser_re_im[2 * csb] : &T->frac_delay_phase_fac_qmf_ser_re_im[2 * csb];
      const int pstep = hyb_chain ? 32 : 64;
      const XpPhase phase = xp_phase_pairs(ph[0], ph[1]);
      const XpPhase ps0 = xp_phase_pairs(pser[0], pser[1]), ps1 = xp_phase_pairs(pser[pstep], pser[pstep + 1]),
                    ps2 = xp_phase_pairs(pser[2 * pstep], pser[2 * pstep + 1]);
      const int16_t dec0 = hyb_chain ? T->rev_link_decay_ser[0] : T->decay_scale_factor[qmf_chain ? di : 9];
      const int16_t dec1 = hyb_chain ? T->rev_link_decay_ser[1] : T->decay_scale_factor[qmf_chain ? di + 1 : 10];
      const int16_t dec2 = hyb_chain ? T->rev_link_decay_ser[2] : T->decay_scale_factor[qmf_chain ? di + 2 : 11];
      uint32_t d0[2] = {0, 0}, r0[3] = {0, 0, 0}, r1[4] = {0, 0, 0, 0}, r2[5] = {0, 0, 0, 0, 0}; /* oldest first */
      if (chain) {
        XP_UNROLL
        for (int j = 0; j < 2; j++) {
          const int16_t *q = hyb_chain ? &ps->sub[(idx0 + j) % 2][2 * csb] : &ps->ap[(idx0 + j) % 2][2 * csb];
          d0[j] = xp_pack16(q[0], q[1]);
        }
        XP_UNROLL
        for (int j = 0; j < 3; j++) {
          const int16_t *q = hyb_chain ? &ps->sub_ser[(is0 + j) % 3][0][2 * csb] : &ps->ser[(is0 + j) % 3][0][2 * csb];
          r0[j] = xp_pack16(q[0], q[1]);
        }
        XP_UNROLL
        for (int j = 0; j < 4; j++) {
          const int16_t *q = hyb_chain ? &ps->sub_ser[(is1 + j) % 4][1][2 * csb] : &ps->ser[(is1 + j) % 4][1][2 * csb];
          r1[j] = xp_pack16(q[0], q[1]);
        }
        XP_UNROLL
        for (int j = 0; j < 5; j++) {
          const int16_t *q = hyb_chain ? &ps->sub_ser[(is2 + j) % 5][2][2 * csb] : &ps->ser[(is2 + j) % 5][2][2 * csb];
          r2[j] = xp_pack16(q[0], q[1]);
        }
      }
      /* -- the lane's band */
      const int g = T->band_to_group[sb];
      const int bin_sb = sb < 23 ? T->delay_to_bin[sb] : (sb < 35 ? 18 : 19); /* the band's transient-detector bin */
      /* The interpolated coefficients of the band's group, as fx_mul32x16's multiplier words: the int16 in the high half, the
         low half zero.  Adding the increment's word wraps exactly as the reference's int16 add does, and the rotation takes
         the words as they are (as int16 values they cost an add and a shift each in every slot). */
      uint32_t h11, h12, h21, h22, d11, d12, d21, d22;
      const auto seg_load = [&](int s) {
        const uint32_t a = w->seg_hd[s][0][g], b = w->seg_hd[s][1][g], c = w->seg_hd[s][2][g], d = w->seg_hd[s][3][g];
        h11 = a & 0xffff0000u, h12 = b & 0xffff0000u, h21 = c & 0xffff0000u, h22 = d & 0xffff0000u;
        d11 = a << 16, d12 = b << 16, d21 = c << 16, d22 = d << 16;
      };
      seg_load(0); /* segment 0 continues the last frame's interpolation */
      uint32_t prev = sb >= 35 ? xp_pack16(ps->sd[2 * (sb - 35)], ps->sd[2 * (sb - 35) + 1]) : 0u;
      /* The walk: four slots per pass of the loop (the delay lines of 2 and 4 slots are back in place after four
         steps, the 3- and 5-slot ones cost a few moves), the next pass's eight row words and the next slot's LDS
         operands in flight meanwhile.  The body has no lane-dependent branches: every lane runs the chain arithmetic
         (on don't-care values where it has no chain), band classes are selects, only the stores are predicated. */
      const int is_ap = sb < 23, is_d14 = sb >= 23 && sb < 35;
      /* the band's scale shift as the two counts of xp_adj_word, for the overlap slots (l < 6) and for the others */
      int shl_ov, shr_ov, shl_lb, shr_lb;
      {
        const int s_ov = sb < lsb ? ov_lb_shift : (sb < usb ? hb_shift : 0), s_lb = sb < lsb ? lb_shift : (sb < usb ? hb_shift : 0);
        const int c_ov = s_ov > 31 ? 31 : (s_ov < -31 ? -31 : s_ov), c_lb = s_lb > 31 ? 31 : (s_lb < -31 ? -31 : s_lb);
        shl_ov = c_ov > 0 ? c_ov : 0, shr_ov = c_ov < 0 ? -c_ov : 0;
        shl_lb = c_lb > 0 ? c_lb : 0, shr_lb = c_lb < 0 ? -c_lb : 0;
      }
      /* What depends on the slot but changes a few times per frame at most is lane state, set again at the slots named by
         `events` (one uniform bit test per slot; worked out in every slot these were three dozen instructions of it):
           shl / shr     the shift counts in force                           (slot 6)
           active        the band lies below the slot's band limit           (clear_slot)
           h.. / d..     the coefficient words                               (the borders)
         and the three links' lines of newly active bands are cleared at clear_slot. */
      int shl = shl_ov, shr = shr_ov;
      bool active = sb < usb_prev;
      const int dlj = is_d14 ? sb - 23 : 12, apj = hyb_chain ? csb : 10;
      int16_t tr_nx = w->ratio[0][bin_sb];
      int32_t hre_nx = w->hyb_l[0][csb], him_nx = w->hyb_l[0][10 + csb];
      uint32_t o14_nx = w->dl[0][dlj]; /* (a lane without a 14-slot line reads the spare column and does not use it) */
      int32_t nre[4], nim[4];
      XP_UNROLL
      for (int j = 0; j < 4; j++) {
        nre[j] = xl[j * 128 + sb];
        nim[j] = xl[j * 128 + 64 + sb];
      }
      /* common_shift is the frame's: its sign is decided once, in front of the walk, and the walk exists twice -- with the
         plain arithmetic shift of every chain met so far (common_shift <= 0) and with the saturating left shift */
      const auto walk = [&](auto cs_positive) XP_LAMBDA_INLINE {
        XP_NOUNROLL
        for (int l0 = 0; l0 < NS; l0 += 4) {
          int32_t cre[4], cim[4];
          XP_UNROLL
          for (int j = 0; j < 4; j++) {
            cre[j] = nre[j];
            cim[j] = nim[j];
          }
          if (l0 + 4 < NS) {
            XP_UNROLL
            for (int j = 0; j < 4; j++) {
              nre[j] = xl[(l0 + 4 + j) * 128 + sb];
              nim[j] = xl[(l0 + 4 + j) * 128 + 64 + sb];
            }
          }
          const uint32_t events4 = events >> l0;
          XP_UNROLL
          for (int j = 0; j < 4; j++) {
            const int l = l0 + j;
            if (NS % 4 != 0 && l >= NS) break; /* (30 slots: the last pass has two) */
            const int16_t tr = tr_nx;
            const int32_t hre = hre_nx, him = him_nx;
            const uint32_t o14 = o14_nx; /* what the 14-slot line holds at this slot */
            {
              const int ln = l + 1 < NS ? l + 1 : NS - 1;
              tr_nx = w->ratio[ln][bin_sb];
              hre_nx = w->hyb_l[ln][csb];
              him_nx = w->hyb_l[ln][10 + csb];
              o14_nx = w->dl[l + 1][dlj]; /* written 13 slots ago (after the last slot: row NS, not used) */
            }
            if ((events4 >> j) & 1u) { /* (uniform) */
#if defined(__HIP_DEVICE_COMPILE__)
              asm volatile(""); /* keeps this a scalar branch taken a few times per frame: as selects it ran in every slot */
#endif
              shl = l < 6 ? shl_ov : shl_lb;
              shr = l < 6 ? shr_ov : shr_lb;
              active = sb < (l >= clear_slot ? usb : usb_prev);
              if (l == clear_slot) { /* the three links' lines of the bands that just became active */
                const int c = qmf_chain && sb >= clear_lo && sb < clear_hi;
                XP_UNROLL
                for (int m = 0; m < 3; m++) r0[m] = c ? 0u : r0[m];
                XP_UNROLL
                for (int m = 0; m < 4; m++) r1[m] = c ? 0u : r1[m];
                XP_UNROLL
                for (int m = 0; m < 5; m++) r2[m] = c ? 0u : r2[m];
              }
              if ((seg_mask >> l) & 1u) /* a border: the coefficients restart from the old targets */
                seg_load(xp_popc(seg_mask & (0xffffffffu >> (31 - l))));
            }
            const int32_t re0 = (int32_t)((uint32_t)cre[j] << shl) >> shr, im0 = (int32_t)((uint32_t)cim[j] << shl) >> shr;
            const int16_t q_re = fx_round16(re0), q_im = fx_round16(im0);
            const uint32_t q = xp_pack16(q_re, q_im);
            /* the chain */
            const uint32_t in_pair = hyb_chain ? xp_pack16(fx_round16(hre), fx_round16(him)) : q;
            uint32_t dv = d0[0], e0 = r0[0], e1 = r1[0], e2 = r2[0];
            const uint32_t o_chain = xp_allpass_packed(dv, in_pair, phase, e0, e1, e2, ps0, ps1, ps2, dec0, dec1, dec2);
            d0[0] = d0[1];
            d0[1] = dv;
            r0[0] = r0[1]; r0[1] = r0[2];
            r0[2] = e0;
            r1[0] = r1[1]; r1[1] = r1[2]; r1[2] = r1[3];
            r1[3] = e1;
            r2[0] = r2[1]; r2[1] = r2[2]; r2[2] = r2[3]; r2[3] = r2[4];
            r2[4] = e2;
            w->ap_h[l][apj] = o_chain; /* lanes without a hybrid chain write the spare column */
            h11 += d11; /* the interpolation advances whether or not the band is rotated */
            h12 += d12;
            h21 += d21;
            h22 += d22;
            /* the decorrelated sample of the band: all-pass output, or the input of 14 slots / 1 slot ago (the line's
               word came in a slot ahead, read by every lane: no predicated region and no wait inside the walk).  Either
               line takes the band's sample if the band is active and keeps what it held if not: one select for both. */
            const uint32_t held = is_d14 ? o14 : prev;
            const uint32_t o = is_ap ? o_chain : held;
            prev = active ? q : held;
            w->dl[l + 14][dlj] = prev; /* lanes without a 14-slot line write the spare column */
            int32_t re = re0, im = im0;
            int32_t r_re = xp_m16x16_shl_pre(xp_lo16(o), 2 * tr), r_im = xp_m16x16_shl_pre(xp_hi16(o), 2 * tr);
            xp_rotate_w(&re, &r_re, h11, h12, h21, h22);
            xp_rotate_w(&im, &r_im, h11, h12, h21, h22);
            re = active ? re : re0; /* above usb: the left sample passes, the right one is zero */
            im = active ? im : im0;
            r_re = active ? r_re : 0;
            r_im = active ? r_im : 0;
            if (decltype(cs_positive)::value) {
              re = fx_shl_sat(re, common_shift);
              im = fx_shl_sat(im, common_shift);
            } else {
              re = re >> cs_right;
              im = im >> cs_right;
            }
            if (sb >= 3) {
              xl[l * 128 + sb] = re;
              xl[l * 128 + 64 + sb] = im;
              xr[l * 128 + sb] = r_re;
              xr[l * 128 + 64 + sb] = r_im;
            }
          }
        }
      };
      if (common_shift > 0)
        walk(XpBool<true>());
      else
        walk(XpBool<false>());
      /* -- the delay lines as the slot loop leaves them */
      if (chain) {
        XP_UNROLL
        for (int j = 0; j < 2; j++) {
          int16_t *q = hyb_chain ? &ps->sub[(idx0 + j) % 2][2 * csb] : &ps->ap[(idx0 + j) % 2][2 * csb]; /* an even NS: same phase */
          q[0] = xp_lo16(d0[j]);
          q[1] = xp_hi16(d0[j]);
        }
        XP_UNROLL
        for (int j = 0; j < 3; j++) {
          int16_t *q = hyb_chain ? &ps->sub_ser[(is0 + NS + j) % 3][0][2 * csb] : &ps->ser[(is0 + NS + j) % 3][0][2 * csb];
          q[0] = xp_lo16(r0[j]);
          q[1] = xp_hi16(r0[j]);
        }
        XP_UNROLL
        for (int j = 0; j < 4; j++) {
          int16_t *q = hyb_chain ? &ps->sub_ser[(is1 + NS + j) % 4][1][2 * csb] : &ps->ser[(is1 + NS + j) % 4][1][2 * csb];
          q[0] = xp_lo16(r1[j]);
          q[1] = xp_hi16(r1[j]);
        }
        XP_UNROLL
        for (int j = 0; j < 5; j++) {
          int16_t *q = hyb_chain ? &ps->sub_ser[(is2 + NS + j) % 5][2][2 * csb] : &ps->ser[(is2 + NS + j) % 5][2][2 * csb];
          q[0] = xp_lo16(r2[j]);
          q[1] = xp_hi16(r2[j]);
        }
      }
      if (sb >= 35) { /* the 1-slot delay line as the last slot leaves it */
        ps->sd[2 * (sb - 35)] = xp_lo16(prev);
        ps->sd[2 * (sb - 35) + 1] = xp_hi16(prev);
      }
    }
    cx.sync();
    /* the 14-slot ring as the slot loop leaves it: what the frame's last 14 slots wrote or handed on (rows NS..NS + 13),
       back at their ring positions */
    XS_PAR(i, 0, 4 * 14) {
      const int r = i >> 2, j0 = 3 * (i & 3), p0 = (idx_long0 + NS) % 14;
      const int pos = p0 + r >= 14 ? p0 + r - 14 : p0 + r;
      XP_UNROLL
      for (int k = 0; k < 3; k++) xp_store_pair(&ps->ld[pos][2 * (j0 + k)], w->dl[NS + r][j0 + k]);
    }
    XS_ONE {
      ps->idx = (int16_t)idx0; /* NS (even) slots later the 2-slot line is in the same phase */
      ps->idx_ser[0] = (int16_t)((is0 + NS) % 3);
      ps->idx_ser[1] = (int16_t)((is1 + NS) % 4);
      ps->idx_ser[2] = (int16_t)((is2 + NS) % 5);
      ps->idx_long = (int16_t)((idx_long0 + NS) % 14);
      if (clear_slot < NS) ps->usb = (int16_t)usb;
    }
  }
  cx.sync();
  XP_T(6);

  /* ---- P6: rotation of the hybrid sub-bands (ps_dec.c:856, groups 0..9) and hybrid synthesis of QMF bands 0..2
     (the saturating sums of ps_dec.c:899-925, in sub-band order), one (slot, re | im) per lane: 2 * NS lanes, one trip.
     The lane walks the ten sub-bands in order with one pair of sums per QMF band (sub-bands 0..5, 6..7, 8..9): the
     sub-band is a constant of the unrolled body and no lane waits for a band with more sub-bands than its own. */
  XS_PAR(i, 0, 2 * NS) {
    const int l = i >> 1, c = i & 1;
    const uint32_t below = seg_mask & (0xffffffffu >> (31 - l));     /* borders at or before slot l */
    const int s = xp_popc(below), nn = l - (below ? 31 - xp_clz(below) : 0) + 1; /* slots since the segment began */
    int32_t acc_l[3] = {0, 0, 0}, acc_r[3] = {0, 0, 0};
    XP_UNROLL
    for (int sb = 0; sb < 10; sb++) {
      const int b = sb < 6 ? 0 : (sb < 8 ? 1 : 2);
      const bool first = sb == 0 || sb == 6 || sb == 8;
      const int16_t h11 = xp_seg_coeff(w->seg_hd[s][0][sb], nn), h12 = xp_seg_coeff(w->seg_hd[s][1][sb], nn);
      const int16_t h21 = xp_seg_coeff(w->seg_hd[s][2][sb], nn), h22 = xp_seg_coeff(w->seg_hd[s][3][sb], nn);
      const int16_t tr = w->ratio[l][T->hybrid_to_bin[sb]];
      const uint32_t o = w->ap_h[l][sb];
      int32_t lv = w->hyb_l[l][10 * c + sb];
      int32_t rv = xp_m16x16_shl(c ? xp_hi16(o) : xp_lo16(o), tr);
      xp_rotate(&lv, &rv, h11, h12, h21, h22);
      acc_l[b] = first ? lv : fx_add_sat(acc_l[b], lv);
      acc_r[b] = first ? rv : fx_add_sat(acc_r[b], rv);
    }
    XP_UNROLL
    for (int b = 0; b < 3; b++) {
      int32_t v = acc_l[b];
      if (common_shift < 0)
        v = fx_shr(v, -common_shift > 31 ? 31 : -common_shift);
      else if (common_shift > 0)
        v = fx_shl_sat(v, common_shift);
      xl[l * 128 + 64 * c + b] = v;
      xr[l * 128 + 64 * c + b] = acc_r[b];
    }
  }
  {
    const int s = xp_popc(seg_mask), n = NS - (seg_mask ? 31 - xp_clz(seg_mask) : 0);
    XS_PAR(g, 0, XAAC_PS_GROUPS) {
      ps->H11_H12[2 * g] = xp_seg_coeff(w->seg_hd[s][0][g], n);
      ps->H11_H12[2 * g + 1] = xp_seg_coeff(w->seg_hd[s][1][g], n);
      ps->H21_H22[2 * g] = xp_seg_coeff(w->seg_hd[s][2][g], n);
      ps->H21_H22[2 * g + 1] = xp_seg_coeff(w->seg_hd[s][3][g], n);
    }
  }
  cx.sync();
  XP_T(7);
  return ps_scale;
}

#endif /* XAAC_SBR_PS_FRAME_H */
