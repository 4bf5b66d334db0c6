/* tests/ps_prep_shim.cpp -- host entry points for tests/test_ps_prep_cpu.py: the short division of sbr_ps_frame.h next to
   xp_divide16_pos of sbr_ps.h, and the frame-at-once transient detector (xp_transient_frame) next to the per-slot statement
   in sbr_ps.h: xp_decorrelation.  Compiled by the test with g++; never part of the product. */
#include <stdint.h>
#include <string.h>

#include "../include/xaac_amd.h"
#include "../libxaac_amd/csrc/sbr_core.h"
#include "../libxaac_amd/csrc/sbr_ps.h"
#include "../libxaac_amd/csrc/sbr_ps_frame.h"

/* n pairs of normalised heads: got[i] = xp_quot15(u, v) & 0xffff, want[i] = what xp_divide16_pos does with them */
extern "C" void xpp_quot15(const uint32_t *u, const uint32_t *v, int n, uint32_t *got, uint32_t *want) {
  for (int i = 0; i < n; i++) {
    got[i] = xp_quot15(u[i], v[i]) & 0xffffu;
    want[i] = u[i] == 0 ? 0u : ((u[i] << 15) / v[i]) & 0xffffu;
  }
}

/* returns the number of pairs (u <= v, v in [v0, v1), every `stride`-th u from a start that moves with v, plus u = 0, 1,
   v - 1, v) on which xp_quot15 differs from the integer division; *checked: pairs looked at.  ulps: the reciprocal handed in
   is the float that many steps above (below) the host's 1 / v -- a reciprocal instruction good to one unit in the last
   place may return either neighbour. */
extern "C" int64_t xpp_quot15_sweep(uint32_t v0, uint32_t v1, uint32_t stride, int ulps, int64_t *checked) {
  int64_t bad = 0, n = 0;
  for (uint32_t v = v0; v < v1; v++) {
    float r = 1.0f / (float)v;
    uint32_t bits;
    memcpy(&bits, &r, 4);
    bits += ulps; /* (positive floats: the next float up is the next bit pattern) */
    memcpy(&r, &bits, 4);
    const uint32_t edge[4] = {0, 1, v - 1, v};
    for (int e = 0; e < 4; e++, n++) bad += xp_quot15_rcp(edge[e], v, r) != (edge[e] << 15) / v;
    for (uint32_t u = (v * 2654435761u) % stride; u <= v; u += stride, n++) bad += xp_quot15_rcp(u, v, r) != (u << 15) / v;
  }
  *checked = n;
  return bad;
}

/* whole operands, as the detector hands them over (0 <= op1 < op2) */
extern "C" void xpp_divide16(const int32_t *op1, const int32_t *op2, int n, int32_t *got, int32_t *want) {
  for (int i = 0; i < n; i++) {
    got[i] = xp_divide16_norm(op1[i], op2[i]);
    want[i] = xp_divide16_pos(op1[i], op2[i]);
  }
}

/* The detector alone.  binpw: ns rows of 20 bin powers; state: peak_decay_diff | peak_decay_diff_prev | energy_prev, 20 words
   each, in and out.  phased = 1: xp_transient_frame<ns>; 0: the statements of sbr_ps.h: xp_decorrelation, slot by slot.
   ratio: ns rows of 20. */
template <int NS>
static void detector(int phased, const int32_t *binpw, int32_t *state, int16_t *ratio) {
  static xaac_ps_state ps;
  memset(&ps, 0, sizeof(ps));
  memcpy(ps.peak_decay_diff, state, 80);
  memcpy(ps.peak_decay_diff_prev, state + 20, 80);
  memcpy(ps.energy_prev, state + 40, 80);
  if (phased) {
    static XpFrameWork w;
    const XsCx cx = {0, 1};
    memset(&w, 0, sizeof(w));
    for (int l = 0; l < NS; l++)
      for (int b = 0; b < 20; b++) w.binpw[l][b] = binpw[20 * l + b];
    xp_transient_frame<NS>(cx, &ps, &w);
    for (int l = 0; l < NS; l++)
      for (int b = 0; b < 20; b++) ratio[20 * l + b] = w.ratio[l][b];
  } else {
    for (int l = 0; l < NS; l++)
      for (int bin = 0; bin < 20; bin++) { /* sbr_ps.h: xp_decorrelation, the transient detector's lines */
        int32_t pw = fx_shl(binpw[20 * l + bin], 1);
        if (pw < 0) pw = 0;
        int32_t pd = fx_mul32x16_shl(ps.peak_decay_diff[bin], 0x620a);
        if (pw > pd) pd = pw;
        ps.peak_decay_diff[bin] = pd;
        int32_t peak_diff = fx_add_sat(fx_mul32x16_shl(ps.peak_decay_diff_prev[bin], 0x6000), fx_sub_sat(pd, pw) >> 2);
        ps.peak_decay_diff_prev[bin] = peak_diff;
        const int32_t nrg = fx_add_sat(fx_mul32x16_shl(ps.energy_prev[bin], 0x6000), pw >> 2);
        ps.energy_prev[bin] = nrg;
        peak_diff = fx_add_sat(peak_diff, peak_diff >> 1);
        ratio[20 * l + bin] = peak_diff <= nrg ? (int16_t)0x7fff : (int16_t)xp_divide16_pos(nrg, peak_diff);
      }
  }
  memcpy(state, ps.peak_decay_diff, 80);
  memcpy(state + 20, ps.peak_decay_diff_prev, 80);
  memcpy(state + 40, ps.energy_prev, 80);
}

extern "C" void xpp_detector(int ns, int phased, const int32_t *binpw, int32_t *state, int16_t *ratio) {
  if (ns == 30)
    detector<30>(phased, binpw, state, ratio);
  else
    detector<32>(phased, binpw, state, ratio);
}
