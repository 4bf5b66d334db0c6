/* tests/ps_phases_shim.cpp -- host build of the parametric-stereo tool's two arrangements for tests/test_ps_phases_cpu.py:
   the group-sum helper of sbr_ps_frame.h next to the sequential saturating loop of sbr_ps.h: xp_bin_power, and whole frames of
   NS = 32 or 30 slots through xp_ps_frame<NS> (lane count 1) next to the slot loop, on a QMF matrix handed in.  Compiled by the
   test with g++; never part of the product. */
#include <stdint.h>
#include <string.h>

#include "../include/xaac_amd.h"
#include "../libxaac_amd/csrc/sbr_core.h"
#include "../libxaac_amd/csrc/sbr_ps.h"
#include "../libxaac_amd/csrc/sbr_ps_frame.h"

extern "C" int xpt_gsum_fits(void) { return xp_gsum_fits(&xaac_ps_tables) ? 1 : 0; }

/* band_pw: the 64 band powers of one slot (>= 0, as xp_power leaves them); usb: the slot's band limit.  out_new[g]: bins
   14 + g by the helper (running sum over the bands, difference at the group's borders, clamp); out_ref[g]: by xp_bin_power. */
extern "C" void xpt_group_sums(const int32_t *band_pw, int usb, int32_t *out_new, int32_t *out_ref) {
  const XpTables *T = &xaac_ps_tables;
  const XsCx cx = {0, 1};
  uint32_t run = 0, S[64];
  for (int sb = 0; sb < 64; sb++) {
    int g = 0;
    while (g < 5 && sb >= T->borders_group[17 + g]) g++;
    S[sb] = xp_gsum_scan(cx, xp_gsum_addend(band_pw[sb], T->group_shift[g], sb >= 9 && sb < usb), run);
  }
  XpHyb hy;
  memset(&hy, 0, sizeof(hy));
  for (int g = 0; g < 6; g++) {
    const int b0 = T->borders_group[16 + g], b1 = T->borders_group[17 + g];
    out_new[g] = xp_gsum_sum(S[b1 - 1], g > 0 ? S[b0 - 1] : 0u);
    out_ref[g] = xp_bin_power(T, 14 + g, &hy, band_pw, usb);
  }
}

static int32_t adj_word(int32_t v, int shift) {
  if (shift > 31) shift = 31;
  if (shift < -31) shift = -31;
  return shift > 0 ? (int32_t)((uint32_t)v << shift) : (v >> -shift);
}

/* The tool alone on one frame of ns slots.  x: the QMF matrix, 38 rows of 64 re | 64 im, slot 0 first (rows 0..ns + 5 are
   read); phased = 1: xp_ps_frame<ns>, 0: the slot loop of the reference (qmf_dec.c:1015-1031 as oracle_sbr.cpp restates it
   for 32 slots, with ns for no_col).  xl_out / xr_out: ns rows each, left in the synthesis bank's scale, right.  Returns
   ps_scale. */
template <int NS>
static int run_frame(int phased, xaac_ps_state *ps, const xaac_ps_frame *pf_in, const int32_t *x_in, int lb_scale, int ov_lb_scale,
                     int hb_scale, int st_syn, int lsb, int usb, int32_t *xl_out, int32_t *xr_out) {
  const XsCx cx = {0, 1};
  static int32_t x[38 * 128], xr[32 * 128];
  memcpy(x, x_in, sizeof(x));
  memset(xr, 0, sizeof(xr));
  xaac_ps_frame pf = *pf_in;
  int ps_scale;
  if (phased) {
    static XpFrameWork wk;
    ps_scale = xp_ps_frame<NS>(cx, &xaac_ps_tables, ps, &pf, &wk, x, xr, lb_scale, ov_lb_scale, hb_scale, st_syn, lsb, usb);
  } else {
    ps_scale = xp_init_ps_scale(cx, ps, lb_scale, ov_lb_scale, hb_scale);
    const int ov_lb_shift = ps_scale - ov_lb_scale, lb_shift = ps_scale - lb_scale, hb_shift = ps_scale - hb_scale;
    const int common_shift = (st_syn - ps_scale) - 8;
    for (int l = 0; l < NS; l++) /* adjust_scale (qmf_dec.c:937): this frame's slots only */
      for (int k = 0; k < 64; k++) {
        const int sh = k < lsb ? (l < 6 ? ov_lb_shift : lb_shift) : (k < usb ? hb_shift : 0);
        x[l * 128 + k] = adj_word(x[l * 128 + k], sh);
        x[l * 128 + 64 + k] = adj_word(x[l * 128 + 64 + k], sh);
      }
    int env = 0;
    for (int l = 0; l < NS; l++) {
      int32_t right[128];
      XpHyb hy;
      memset(&hy, 0, sizeof(hy));
      memset(right, 0, sizeof(right));
      int16_t ratio[21];
      int32_t band_pw[64];
      if (env <= XAAC_PS_MAX_ENV && l == pf.border_position[env]) {
        xp_init_rot_env(cx, &xaac_ps_tables, ps, &pf, env, usb);
        env++;
      }
      const int shiftdelay = l < NS - 6 ? 0 : (int16_t)(lb_scale - ps_scale); /* thumb_ps_dec.c:77 */
      xp_hybrid_analysis(cx, &xaac_ps_tables, &x[(l + 6) * 128], &x[(l + 6) * 128 + 64], ps, &hy, shiftdelay);
      xp_decorrelation(cx, &xaac_ps_tables, ps, &hy, &x[l * 128], right, ratio, band_pw);
      xp_apply_rot(cx, &xaac_ps_tables, ps, &hy, &x[l * 128], right);
      if (common_shift) /* generic:1610 */
        for (int k = 0; k < 128; k++) {
          int32_t *p = &x[l * 128 + k];
          *p = common_shift < 0 ? fx_shr(*p, -common_shift > 31 ? 31 : -common_shift) : fx_shl_sat(*p, common_shift);
        }
      memcpy(&xr[l * 128], right, sizeof(right));
    }
  }
  memcpy(xl_out, x, sizeof(int32_t) * NS * 128);
  memcpy(xr_out, xr, sizeof(int32_t) * NS * 128);
  return ps_scale;
}

extern "C" int xpt_ps_frame(int ns, int phased, xaac_ps_state *ps, const xaac_ps_frame *pf, const int32_t *x, int lb_scale,
                            int ov_lb_scale, int hb_scale, int st_syn, int lsb, int usb, int32_t *xl_out, int32_t *xr_out) {
  return ns == 30 ? run_frame<30>(phased, ps, pf, x, lb_scale, ov_lb_scale, hb_scale, st_syn, lsb, usb, xl_out, xr_out)
                  : run_frame<32>(phased, ps, pf, x, lb_scale, ov_lb_scale, hb_scale, st_syn, lsb, usb, xl_out, xr_out);
}

/* ---- how large the group sums get inside a real HE-AACv2 frame: the oracle's path up to the tool (oracle_sbr.cpp:
   xo_sbr_dec_hq -- overlap, analysis bank, SBR core, the PS scale), then the band powers as the tool forms them and each
   group's sum in 64 bits, unclamped.  For tests that must know whether their inputs reach the clamp of the group sums;
   works on copies, advances nothing.  exact: [32][6].  Returns 0, 1 if the frame does not run the tool, -1 if refused. */
#include "../oracle/oracle_qmf.h"

extern "C" int xpt_hq_group_sums(const xaac_sbr_header *h, const xaac_sbr_frame *f, const xaac_sbr_state *st_in,
                                 const xaac_ps_frame *pf, const xaac_ps_state *ps_in, const int16_t *pcm_in, int64_t *exact) {
  static int32_t buf[41 * 128];
  static XsWork w;
  static int16_t rand_hi[568];
  for (int i = 0; i < 568; i++) rand_hi[i] = (int16_t)(xaac_sbr_rand_ph[i] >> 16);
  XsQmfHq x = {buf};
  const XsCx cx = {0, 1};
  xaac_sbr_state st = *st_in;
  xaac_ps_state ps = *ps_in;
  memset(buf, 0, sizeof(buf));
  memcpy(&x(0, 0), st.overlap, sizeof(int32_t) * 12 * 64);
  if (xs_side_info_bad(cx, h, f, &st)) return -1;
  st.lb_scale = 0;
  if (f->apply_processing) xs_rescale_x_overlap(cx, h, f, &st, x);
  {
    xo_qmf_ana_state a;
    memcpy(a.ring, st.ana_ring, sizeof(a.ring));
    a.wr = st.ana_wr;
    a.phase = st.ana_phase;
    xo_qmf_analysis(pcm_in, 1, &a, 0, st.codec_usb, &x(6, 0), 128);
    st.st_lb_scale = 0;
    st.lb_scale = -8;
  }
  int save_lb_scale = 0;
  if (xs_sbr_core(cx, h, f, f->int_env_sf_arr, f->int_noise_floor, &st, x, &w, rand_hi, &save_lb_scale)) return -1;
  if (!(f->apply_processing && h->channel_mode == 3)) return 1;
  const XpTables *T = &xaac_ps_tables;
  const int usb_prev = ps.usb;
  const int ps_scale = xp_init_ps_scale(cx, &ps, st.lb_scale, st.ov_lb_scale, st.hb_scale);
  const int lsb = st.syn_lsb, usb = st.syn_usb;
  const int ov_lb_shift = ps_scale - st.ov_lb_scale, lb_shift = ps_scale - st.lb_scale, hb_shift = ps_scale - st.hb_scale;
  int b0 = pf->border_position[0];
  b0 = b0 < 0 ? 0 : b0; /* (xp_frame_sanitize) */
  for (int l = 0; l < 32; l++) {
    const int usb_l = l >= b0 ? usb : usb_prev;
    for (int g = 0; g < 6; g++) {
      int64_t sum = 0;
      for (int k = T->borders_group[16 + g]; k < T->borders_group[17 + g] && k < usb_l; k++) {
        const int sh = k < lsb ? (l < 6 ? ov_lb_shift : lb_shift) : (k < usb ? hb_shift : 0);
        sum += xp_power(adj_word(x(l, k), sh), adj_word(x.im(l, k), sh)) >> T->group_shift[g];
      }
      exact[l * 6 + g] = sum;
    }
  }
  return 0;
}
