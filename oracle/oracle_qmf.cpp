/*
 * oracle/oracle_qmf.cpp -- TEST INFRASTRUCTURE ONLY (checker + CPU baseline).
 *
 * CPU restatement of the fixed-point SBR QMF banks ("Path B"): the 32-band analysis
 * bank ixheaacd_cplx_anal_qmffilt (decoder/generic/ixheaacd_qmf_dec_generic.c:590)
 * and the 64-band synthesis bank ixheaacd_cplx_synt_qmffilt
 * (decoder/ixheaacd_qmf_dec.c:811), low-power (real, DCT) and HQ (complex) modes.
 * The per-slot arithmetic is libxaac_amd/csrc/sbr_qmf.h (shared with the GPU
 * kernels); this file adds the reference's ring-buffer state machines exactly as
 * they evolve (filter-state rings, window phase, drc offset), so state can be
 * compared word for word with the reference.
 *
 * Parity status: PINNED -- tests/test_qmf_oracle_vs_reference.py compares every
 * exported piece (radix4bfly, postradixcompute2/4, dct3_32, cos_sin_mod,
 * fwd_modulation, dct2_64 path, shiftrountine_with_rnd path) and the two complete
 * banks, state included, with the compiled reference on seeded inputs.
 */
#include <stdint.h>
#include <string.h>

#include "../libxaac_amd/csrc/sbr_qmf.h"
#include "oracle_qmf.h"

extern "C" {

/* ---- unit entry points (each mirrors one reference symbol) -------------------- */
void xo_radix4(const int16_t *w, int32_t *x, int index1, int index) { xq_radix4(w, x, index1, index); }
void xo_postradix4(int32_t *y, const int32_t *x) { xq_postradix4(y, x); }
void xo_postradix2(int32_t *y, const int32_t *x) { xq_postradix2(y, x); }
void xo_dct3_32(int32_t *in, int32_t *out) { xq_dct3_32(in, out); }
void xo_cos_sin_mod(int32_t *s, int m) {
  int32_t t[128];
  if (m == 32)
    xq_cos_sin_mod<32>(s, t);
  else
    xq_cos_sin_mod<16>(s, t);
}
void xo_fwd_modulation(const int32_t *in, int32_t *s, int nrot) {
  int32_t t[128];
  xq_fwd_modulation(in, s, t, nrot);
}
void xo_dct2_64_lp(int32_t *x, int16_t *b) {
  int32_t X[64];
  xq_dct2_64_lp(x, X, b);
}
void xo_synth_hq_slot(int32_t *s, int16_t *b, int shift) {
  int32_t t[128];
  xq_synth_hq_slot(s, t, b, shift);
}

/* ---- analysis bank -------------------------------------------------------------- */
void xo_qmf_ana_init(xo_qmf_ana_state *st) { memset(st, 0, sizeof(*st)); }

/* generic:528: 5-tap polyphase sums; never saturates (max sum|c| = 32757 < 65536) */
static void ana_winadd(const int16_t *i1, const int16_t *i2, const int16_t *q1, const int16_t *q2, int32_t *o) {
  for (int n = 0; n < 32; n++) {
    int32_t a = 0, b = 0;
    for (int j = 0; j < 5; j++) {
      a = fx_add_sat(a, (int32_t)i1[n + 64 * j] * q1[2 * (n + 64 * j)]);
      b = fx_add_sat(b, (int32_t)i2[n + 64 * j] * q2[2 * (n + 64 * j)]);
    }
    o[n] = a;
    o[32 + n] = b;
  }
}

/* One frame: n_slots (32, or 30 for a 960-line core) slots of 32 new samples.  qmf: slot s at qmf + s*slot_stride; LP
   writes 32 reals, HQ writes 32 reals at +0 and 32 imaginaries at +64.  usb = analysis bank's usb (HQ rotation count).
   The ring walk is literal, so wr and phase come out where the reference leaves them after n_slots steps. */
void xo_qmf_analysis_ns(const int16_t *pcm, int stride, xo_qmf_ana_state *st, int low_pow, int usb, int32_t *qmf,
                        int slot_stride, int n_slots) {
  const int16_t *c = xaac_qmf_qmf_c;
  int f1 = st->phase, f2 = st->phase + 64; /* offsets into qmf_c (int16 units) */
  int wr = st->wr;
  int fp1 = 0, fp2 = 32;
  for (int s = 0; s < n_slots; s++) {
    int32_t z[64], t[128], sb[128];
    for (int k = 0; k < 32; k++) st->ring[wr + 31 - k] = pcm[stride * (32 * s + k)];
    ana_winadd(st->ring + fp1, st->ring + fp2, c + f1, c + f2, z);
    wr -= 32;
    if (wr < 0) wr = 288;
    { int tmp = fp1; fp1 = fp2; fp2 = tmp; }
    f1 += 64;
    f2 += 64;
    { int tmp = f1; f1 = f2; f2 = tmp; }
    if (f2 > 640) {
      f1 = 0;
      f2 = 64;
    }
    int32_t *o = qmf + (size_t)s * slot_stride;
    if (low_pow) {
      xq_dct3_32(z, o);
    } else {
      xq_fwd_modulation(z, sb, t, usb);
      memcpy(o, sb, 32 * sizeof(int32_t));
      memcpy(o + 64, sb + 64, 32 * sizeof(int32_t));
    }
  }
  st->phase = (int16_t)f1;
  st->wr = (int16_t)wr;
}
void xo_qmf_analysis(const int16_t *pcm, int stride, xo_qmf_ana_state *st, int low_pow, int usb, int32_t *qmf,
                     int slot_stride) {
  xo_qmf_analysis_ns(pcm, stride, st, low_pow, usb, qmf, slot_stride, 32);
}

/* ---- synthesis bank --------------------------------------------------------------- */
/* The LD / ELD flavour of the complex analysis bank (ixheaacd_cplx_anal_qmffilt with AOT_ER_AAC_ELD, generic:590-741, and
   ixheaacd_sbr_qmfanal32_winadd_eld, qmf_dec.c:484-535), literally: the reference's rotating pointers as offsets.
   st: ring[320], wr, f1 (filter_pos), f2 (filter_2), fp (fp1_anal: 0 or 32; fp2_anal is the other half).  n_slots = 16
   (512-sample frames) or 15 (480).  qmf: [n_slots][slot_stride], real bands at +0, imaginary at +64. */
void xo_qmf_analysis_eld(const int16_t *pcm, int stride, int16_t *ring, int16_t *state4, int n_slots, int usb, int32_t *qmf,
                         int slot_stride) {
  const int16_t *c = xaac_qmf_eld_c3; /* one period of qmf_c_eld3: the ROM's second copy continues it */
  int wr = state4[0], f1 = state4[1], f2 = state4[2], fp1 = state4[3], fp2 = 32 - state4[3];
  for (int s = 0; s < n_slots; s++) {
    int32_t z[64], t[128], sb[128];
    for (int k = 0; k < 32; k++) ring[wr + 31 - k] = pcm[stride * (32 * s + k)];
    for (int n = 0; n < 32; n++) { /* winadd_eld: five taps 64 apart, coefficient index = sample index + the filter offset */
      int32_t a1 = 0, a2 = 0;
      for (int j = 0; j < 5; j++) {
        a1 = fx_add_sat(a1, (int32_t)ring[fp1 + n + 64 * j] * c[(f1 + n + 64 * j) % 320]);
        a2 = fx_add_sat(a2, (int32_t)ring[fp2 + n + 64 * j] * c[(f2 + n + 64 * j) % 320]);
      }
      z[n] = a1;
      z[n + 32] = a2;
    }
    wr -= 32;
    if (wr < 0) wr = 288;
    { int tmp = fp1; fp1 = fp2; fp2 = tmp; }
    f1 += 32;
    f2 += 32;
    { int tmp = f1; f1 = f2; f2 = tmp; }
    if (f2 > 320) {
      f1 = 0;
      f2 = 32;
    }
    xq_fwd_modulation(z, sb, t, usb, true);
    int32_t *o = qmf + (size_t)s * slot_stride;
    memcpy(o, sb, 32 * sizeof(int32_t));
    memcpy(o + 64, sb + 64, 32 * sizeof(int32_t));
  }
  state4[0] = (int16_t)wr;
  state4[1] = (int16_t)f1;
  state4[2] = (int16_t)f2;
  state4[3] = (int16_t)fp1;
}

void xo_qmf_syn_init(xo_qmf_syn_state *st) { memset(st, 0, sizeof(*st)); }

static inline int32_t adj(int32_t v, int shift) {
  if (shift == 0) return v;
  if (shift > 31) shift = 31;
  if (shift < -31) shift = -31;
  return shift > 0 ? fx_shlw(v, shift) : (v >> -shift);
}

/* The LD / ELD flavour of the complex synthesis bank (ixheaacd_cplx_synt_qmffilt with AOT_ER_AAC_ELD, qmf_dec.c:811-1135,
   no PS, no DRC), literally.  ring: filter_states[1280]; state4 = {ixheaacd_drc_offset, filter_pos_syn - qmf_c_eld,
   fp1_syn - filter_states (0 or 64), sixty4 (64 or -64)}; a new stream: {0, 0, 0, 64}.  qmf rows are not modified.
   sf = {lb_scale, ov_lb_scale, hb_scale, st_syn_scale}.  pcm: 64 * n_slots samples at `stride`. */
/* the region rescale alone (qmf_dec.c:925-953 with the LD / ELD shifts): what the reference leaves in place of its input */
void xo_qmf_eld_region_scale(const int32_t *qmf, int slot_stride, const int16_t *sf, int lsb, int usb, int split, int n_slots,
                             int32_t *out) {
  const int st_syn = sf[3], ov_lb_shift = (st_syn - sf[1]) - 7, lb_shift = (st_syn - sf[0]) - 7, hb_shift = (st_syn - sf[2]) - 7;
  for (int s = 0; s < n_slots; s++)
    for (int p = 0; p < 2; p++)
      for (int k = 0; k < 64; k++) {
        int32_t v = qmf[(size_t)s * slot_stride + 64 * p + k];
        if (k < lsb)
          v = adj(v, s < split ? ov_lb_shift : lb_shift);
        else if (k < usb)
          v = adj(v, hb_shift);
        out[(size_t)s * slot_stride + 64 * p + k] = v;
      }
}

void xo_qmf_synthesis_eld(const int32_t *qmf, int slot_stride, const int16_t *sf, int lsb, int usb, int split, int16_t *ring,
                          int16_t *state4, int n_slots, int16_t *pcm, int stride) {
  const int lb_scale = sf[0], ov_lb_scale = sf[1], hb_scale = sf[2], st_syn = sf[3];
  const int ov_lb_shift = (st_syn - ov_lb_scale) - 7, lb_shift = (st_syn - lb_scale) - 7, hb_shift = (st_syn - hb_scale) - 7; /* :925-928 */
  const int out_scale = -(st_syn - 3);
  int d = state4[0], ph = state4[1], fp1 = state4[2], sixty4 = state4[3], fp2 = fp1 + sixty4;
  const int16_t *c = xaac_qmf_eld_c;
  for (int s = 0; s < n_slots; s++) {
    int32_t x[128], t[128];
    const int32_t *row = qmf + (size_t)s * slot_stride;
    for (int p = 0; p < 2; p++)
      for (int k = 0; k < 64; k++) {
        int32_t v = row[64 * p + k];
        if (k < lsb)
          v = adj(v, s < split ? ov_lb_shift : lb_shift);
        else if (k < usb)
          v = adj(v, hb_shift);
        x[64 * p + k] = v;
      }
    xq_synth_eld_slot(x, t, ring + d, out_scale); /* temp_out_scale_fac = out_scale_factor + 1 - 1 (:1054-1058) */
    const int16_t *t1 = ring + fp1, *t2 = ring + fp2, *cf = c + ph;
    for (int k = 0; k < 64; k++) { /* ixheaacd_sbr_qmfsyn64_winadd with shift 2 (:1091-1097) */
      int32_t acc = 0x8000 >> 2;
      for (int m = 0; m < 5; m++) acc = fx_add_sat(acc, (int32_t)t1[256 * m + k] * cf[k + 128 * m]);
      for (int m = 0; m < 5; m++) acc = fx_add_sat(acc, (int32_t)t2[128 + 256 * m + k] * cf[k + 64 + 128 * m]);
      pcm[(size_t)stride * (64 * s + k)] = (int16_t)(fx_shl_sat(acc, 2) >> 16);
    }
    fp1 += sixty4;
    fp2 -= sixty4;
    sixty4 = -sixty4;
    d -= 128;
    if (d < 0) d += 1280;
    ph += 64;
    if (ph == 640) ph = 0;
  }
  state4[0] = (int16_t)d;
  state4[1] = (int16_t)ph;
  state4[2] = (int16_t)fp1;
  state4[3] = (int16_t)sixty4;
}

/* env_calc.c:1099 on one sample */

/* One slot of the synthesis bank: x = 64 reals (+ 64 imaginaries in HQ), already in the output scale of
   the frame; transform into the ring, 10-tap polyphase sum, 64 PCM16 at `stride`; advances the ring
   state.  `slot` is the slot's index in the frame (the two ring halves alternate with its parity).
   ds: the down-sampled bank (32 channels, qmf_dec.c:749 ixheaacd_sbr_qmfsyn32_winadd): only bands 0..31 of
   x are used, the ring is 640 samples, every second prototype coefficient, 32 PCM16 per slot. */
void xo_qmf_synthesis_slot_n(const int32_t *x, xo_qmf_syn_state *st, int slot, int low_pow, int out_scale, int16_t *pcm,
                             int stride, int ds) {
  const int16_t *c = xaac_qmf_qmf_c;
  const int L = ds ? 32 : 64, ring = 20 * L;
  int d = st->drc_offset, ph = st->phase;
  const int fp1 = (slot & 1) ? L : 0, fp2 = (slot & 1) ? 0 : L;
  int32_t xin[128], t[128];
  int16_t *b = st->ring + d;
  for (int k = 0; k < L; k++) {
    xin[k] = x[k];
    if (!low_pow) xin[64 + k] = x[64 + k];
  }
  if (low_pow) {
    if (ds)
      xq_dct2_32_lp(xin, t, b);
    else
      xq_dct2_64_lp(xin, t, b);
  } else {
    if (ds)
      xq_synth_hq_slot_ds(xin, t, b, out_scale + 1);
    else
      xq_synth_hq_slot(xin, t, b, out_scale + 1);
  }
  /* generic:1508 / qmf_dec.c:749: 10-tap polyphase sum (cannot saturate: sum|c| = 57308), then the output shift */
  const int shift = low_pow ? 2 : 1, cs = ds ? 2 : 1;
  const int16_t *t1 = st->ring + fp1, *t2 = st->ring + fp2, *cf = c + ph;
  for (int k = 0; k < L; k++) {
    int32_t acc = 0x8000 >> shift;
    for (int m = 0; m < 5; m++) acc = fx_add_sat(acc, (int32_t)t1[4 * L * m + k] * cf[cs * (k + 2 * L * m)]);
    for (int m = 0; m < 5; m++) acc = fx_add_sat(acc, (int32_t)t2[2 * L + 4 * L * m + k] * cf[cs * (k + L + 2 * L * m)]);
    pcm[stride * k] = (int16_t)(fx_shl_sat(acc, shift) >> 16);
  }
  d -= 2 * L;
  if (d < 0) d += ring;
  ph += 64;
  if (ph == 640) ph = 0;
  st->drc_offset = (int16_t)d;
  st->phase = (int16_t)ph;
}
void xo_qmf_synthesis_slot(const int32_t *x, xo_qmf_syn_state *st, int slot, int low_pow, int out_scale, int16_t *pcm,
                           int stride) {
  xo_qmf_synthesis_slot_n(x, st, slot, low_pow, out_scale, pcm, stride, 0);
}

/* One frame: n_slots (32 or 30) slots -> 64 n_slots (ds: 32 n_slots) PCM16 at `stride`.  qmf rows as for analysis (64
   reals, +64 imaginaries in HQ); they are NOT modified here (the reference scales and transforms them in place).
   sf = {lb_scale, ov_lb_scale, hb_scale, st_syn_scale}; no PS (active = 0). */
void xo_qmf_synthesis_ns(const int32_t *qmf, int slot_stride, const int16_t *sf, int lsb, int usb, int split,
                         xo_qmf_syn_state *st, int low_pow, int16_t *pcm, int stride, int ds, int n_slots) {
  const int lb_scale = sf[0], ov_lb_scale = sf[1], hb_scale = sf[2], st_syn = sf[3];
  const int bias = low_pow ? 4 : 8; /* qmf_dec.c:906-933 */
  const int ov_lb_shift = (st_syn - ov_lb_scale) - bias, lb_shift = (st_syn - lb_scale) - bias,
            hb_shift = (st_syn - hb_scale) - bias;
  const int out_scale = low_pow ? -(st_syn - 1) : -(st_syn - 3);
  const int L = ds ? 32 : 64;
  for (int s = 0; s < n_slots; s++) {
    int32_t x[128];
    const int32_t *row = qmf + (size_t)s * slot_stride;
    const int nparts = low_pow ? 1 : 2;
    for (int p = 0; p < nparts; p++)
      for (int k = 0; k < 64; k++) {
        int32_t v = row[64 * p + k];
        if (k < lsb)
          v = adj(v, s < split ? ov_lb_shift : lb_shift);
        else if (k < usb)
          v = adj(v, hb_shift);
        x[64 * p + k] = v;
      }
    xo_qmf_synthesis_slot_n(x, st, s, low_pow, out_scale, pcm + (size_t)stride * L * s, stride, ds);
  }
}
void xo_qmf_synthesis_n(const int32_t *qmf, int slot_stride, const int16_t *sf, int lsb, int usb, int split,
                        xo_qmf_syn_state *st, int low_pow, int16_t *pcm, int stride, int ds) {
  xo_qmf_synthesis_ns(qmf, slot_stride, sf, lsb, usb, split, st, low_pow, pcm, stride, ds, 32);
}
void xo_qmf_synthesis(const int32_t *qmf, int slot_stride, const int16_t *sf, int lsb, int usb, int split,
                      xo_qmf_syn_state *st, int low_pow, int16_t *pcm, int stride) {
  xo_qmf_synthesis_n(qmf, slot_stride, sf, lsb, usb, split, st, low_pow, pcm, stride, 0);
}

}  // extern "C"

/* ======================================================================================================================
 * eSBR ("Path A", -esbr:1) QMF banks, ring-faithful like the banks above: the reference's pointer state machines
 * restated with explicit offsets; the slot transforms are sbr_qmf.h's (the same templates on 32-bit constants).
 *   xo_esbr_analysis   ixheaacd_esbr_analysis_filt_block  decoder/ixheaacd_sbr_dec.c:185  (32 analysis channels)
 *                      + ixheaacd_esbr_qmfanal32_winadd   decoder/ixheaacd_qmf_dec.c:537
 *   xo_esbr_synthesis  the bank loop of ixheaacd_esbr_synthesis_filt_block  sbr_dec.c:572-656  (64 synthesis channels)
 *                      + ixheaacd_esbr_qmfsyn64_winadd    generic/ixheaacd_qmf_dec_generic.c:1544
 * The float <-> WORD32 conversions at the banks' edges are exact (multiplications / divisions by powers of two, one
 * truncating cast), so the float outputs are bit-identical to the reference's, not merely close.
 * ====================================================================================================================== */
extern "C" {

/* core: 1024 floats; ring: WORD32[320]; pos: where the next 32 samples go (state_new_samples_pos_low_32 - ring);
   win_off: filter_pos_32 - esbr_qmf_c; re / im: [32][64] floats, bands 0..31 written */
void xo_esbr_analysis(const float *core, int32_t *ring, int32_t *pos, int32_t *win_off, float *re, float *im) {
  const int32_t *c = xaac_qmf_esbr_qmf_c;
  int p = *pos, w1 = *win_off, w2 = *win_off + 64;
  int f1 = 0, f2 = 32; /* the two ring halves the window-add starts from: reset per call, swapped per slot */
  for (int s = 0; s < 32; s++) {
    for (int z = 0; z < 32; z++) ring[p + 31 - z] = fx_f2i_trunc(core[32 * s + z] * 32768.0f);
    int32_t anal[64], sb[128], t[128];
    for (int n = 0; n < 32; n++) {
      int64_t a1 = 0, a2 = 0;
      for (int j = 0; j < 5; j++) a1 = xq_add64(a1, (int64_t)ring[f1 + n + 64 * j] * c[w1 + 2 * (n + 64 * j)]);
      for (int j = 0; j < 5; j++) a2 = xq_add64(a2, (int64_t)ring[f2 + n + 64 * j] * c[w2 + 2 * (n + 64 * j)]);
      anal[n] = (int32_t)(a1 >> 31);
      anal[32 + n] = (int32_t)(a2 >> 31);
    }
    p -= 32;
    if (p < 0) p = 10 * 32 - 32;
    { const int tmp = f1; f1 = f2; f2 = tmp; }
    w1 += 64;
    w2 += 64;
    { const int tmp = w1; w1 = w2; w2 = tmp; }
    if (w2 > 64 * 10) { w1 = 0; w2 = 64; }
    xq_esbr_fwd_modulation(anal, sb, t);
    for (int z = 0; z < 32; z++) {
      re[64 * s + z] = (float)sb[z] * (1.0f / 256.0f);
      im[64 * s + z] = (float)sb[64 + z] * (1.0f / 256.0f);
    }
  }
  *pos = p;
  *win_off = w1;
}

/* The same block for the banks of 8:3 and 4:1 SBR (sbr_dec.c:213-236): nb = 24 | 16 (| 32) analysis channels, n_slots time
   slots of nb core samples each; ring: WORD32[10 nb]; win_off: filter_pos_32 - analy_win_coeff_32 (esbr_qmf_c_24 for 24
   channels); re / im: [n_slots][64] floats, bands 0..nb-1 written */
}  // extern "C"
namespace {
struct XoRing {
  const int32_t *r;
  int32_t operator()(int i) const { return r[i]; }
};
template <int NB>
void esbr_analysis_nb(const float *core, int n_slots, int32_t *ring, int32_t *pos, int32_t *win_off, float *re, float *im) {
  int p = *pos, w1 = *win_off, w2 = *win_off + XqEsbrAna<NB>::fo;
  int f1 = 0, f2 = NB;
  const float gain = XqEsbrAna<NB>::gain();
  for (int s = 0; s < n_slots; s++) {
    for (int z = 0; z < NB; z++) ring[p + NB - 1 - z] = fx_f2i_trunc(core[NB * s + z] * 32768.0f);
    int32_t anal[64], sb[128], t[128];
    const XoRing rg = {ring};
    xq_esbr_winadd_nb<NB>(rg, f1, f2, w1, w2, anal);
    p -= NB;
    if (p < 0) p = 10 * NB - NB;
    { const int tmp = f1; f1 = f2; f2 = tmp; }
    xq_esbr_win_step<NB>(w1, w2);
    xq_esbr_fwd_modulation_nb<NB>(anal, sb, t);
    for (int z = 0; z < NB; z++) {
      re[64 * s + z] = (float)sb[z] * gain;
      im[64 * s + z] = (float)sb[64 + z] * gain;
    }
  }
  *pos = p;
  *win_off = w1;
}
}  // namespace
extern "C" {
void xo_esbr_analysis_nb(const float *core, int nb, int n_slots, int32_t *ring, int32_t *pos, int32_t *win_off, float *re, float *im) {
  if (nb == 24) esbr_analysis_nb<24>(core, n_slots, ring, pos, win_off, re, im);
  else if (nb == 16) esbr_analysis_nb<16>(core, n_slots, ring, pos, win_off, re, im);
  else esbr_analysis_nb<32>(core, n_slots, ring, pos, win_off, re, im);
}

/* re / im: [32][64] floats; ring: WORD32[1280]; drc_off: ixheaacd_drc_offset; filt_off: filter_pos_syn_32 - esbr_qmf_c;
   out: 2048 floats */
void xo_esbr_synthesis(const float *re, const float *im, int32_t *ring, int32_t *drc_off, int32_t *filt_off, float *out) {
  const int32_t *c = xaac_qmf_esbr_qmf_c;
  int d = *drc_off, fl = *filt_off;
  int f1 = 0, f2 = 64, step = 64;
  for (int s = 0; s < 32; s++) {
    int32_t x[128], t[128];
    for (int k = 0; k < 64; k++) {
      x[k] = fx_f2i_trunc(re[64 * s + k] * 64);
      x[64 + k] = fx_f2i_trunc(im[64 * s + k] * 64);
    }
    xq_esbr_synth_slot(x, t, ring + d, 5 + 1);
    for (int k = 0; k < 64; k++) {
      int64_t acc = 0;
      for (int j = 0; j < 5; j++) acc = xq_add64(acc, (int64_t)ring[f1 + 256 * j + k] * c[fl + k + 128 * j]);
      for (int j = 0; j < 5; j++) acc = xq_add64(acc, (int64_t)ring[f2 + 128 + 256 * j + k] * c[fl + k + 64 + 128 * j]);
      out[64 * s + k] = (float)(int32_t)(acc >> 31) / 65536.0f;
    }
    f1 += step;
    f2 -= step;
    step = -step;
    d -= 128;
    if (d < 0) d += 1280;
    fl += 64;
    if (fl == 640) fl = 0;
  }
  *drc_off = d;
  *filt_off = fl;
}

/* ... with the down-sampled bank (no_synthesis_channels 32: sbr_dec.c:605-628, ixheaacd_esbr_qmfsyn32_winadd generic:1577): the ring's
   first 640 words, 1024 floats out */
void xo_esbr_synthesis_ds(const float *re, const float *im, int32_t *ring, int32_t *drc_off, int32_t *filt_off, float *out) {
  const int32_t *c = xaac_qmf_esbr_qmf_c;
  int d = *drc_off, fl = *filt_off;
  int f1 = 0, f2 = 32, step = 32;
  for (int s = 0; s < 32; s++) {
    int32_t x[128], t[128];
    for (int k = 0; k < 64; k++) {
      x[k] = fx_f2i_trunc(re[64 * s + k] * 64);
      x[64 + k] = fx_f2i_trunc(im[64 * s + k] * 64);
    }
    xq_esbr_synth_slot_ds(x, t, ring + d, 5 + 1);
    for (int k = 0; k < 32; k++) {
      int64_t acc = 0;
      for (int j = 0; j < 5; j++) acc = xq_add64(acc, (int64_t)ring[f1 + 128 * j + k] * c[fl + 2 * (k + 64 * j)]);
      for (int j = 0; j < 5; j++) acc = xq_add64(acc, (int64_t)ring[f2 + 64 + 128 * j + k] * c[fl + 2 * (k + 32 + 64 * j)]);
      out[32 * s + k] = (float)(int32_t)(acc >> 31) / 65536.0f;
    }
    f1 += step;
    f2 -= step;
    step = -step;
    d -= 64;
    if (d < 0) d += 640;
    fl += 64;
    if (fl == 640) fl = 0;
  }
  *drc_off = d;
  *filt_off = fl;
}

}  // extern "C"
