/*
 * aac_tools_kernel.hip -- the AAC spectral tools (M/S, intensity, PNS, TNS: the tool half of ixheaacd_channel_pair_process,
 * decoder/ixheaacd_channel.c:602-725) for a batch of channel elements, one wave per element, with the arithmetic of
 * aac_tools.h (which the host parser compiles too).
 *
 * Layout of a wave: the element's 2 x 1024 lines and its side info sit in LDS.
 *   M/S + intensity   one pass over the lines, line i on lane i & 63 (16 per lane), the band of a line from a per-line
 *                     band index built once per element (both tools touch a line pair on its own, so they fuse).
 *   PNS               one lane per noise band of a window (4 slots per lane in the reference's order: channel, window, band).
 *                     A prefix sum over the band widths gives every slot its position in the 32-bit linear congruential
 *                     sequence and xt_lcg_jump (a^k, c (a^k - 1) / (a - 1) mod 2^32) its seed; the lane then runs the
 *                     reference's band routine (energy, fx_sqrt, division, scaling).  The correlated bands of the right
 *                     channel start from the seed the left channel's last window of the group found.
 *   TNS               the recursion is serial along the lines, so the taps are spread instead: DPP row r (16 lanes) takes
 *                     channel r, lane t of the row holds LPC coefficient t + 1 and state t + 1 lines back.  Per line: one
 *                     multiply per lane, a DPP all-reduce of the row, the clamps, and a row_shr:1 that moves the history on.
 *                     The reference adds the products with saturation from the highest tap down; where the magnitudes add
 *                     up to less than 2^31 (checked per line beside the sum) no partial sum can clamp and the plain sum is
 *                     that chain, otherwise the row walks the chain in order.  A channel's windows and filters run one after
 *                     the other: the reference's filters overrun short regions into the next window and shift window 0's
 *                     lines for a window without headroom (pns_js_thumb.c:455), so the order is observable.
 */
#include <hip/hip_runtime.h>

#include "aac_tools.h"
#include "aac_tools_kernel.h"

namespace {

template <int CTRL>
__device__ __forceinline__ int32_t xk_dpp(int32_t v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
/* over the 16 lanes of a DPP row, every lane gets the result: quad_perm [1,0,3,2], [2,3,0,1], row_ror:4, row_ror:8 */
__device__ __forceinline__ int32_t xk_row_sum(int32_t v) {
  v = fx_add(v, xk_dpp<0xB1>(v));
  v = fx_add(v, xk_dpp<0x4E>(v));
  v = fx_add(v, xk_dpp<0x124>(v));
  return fx_add(v, xk_dpp<0x128>(v));
}
__device__ __forceinline__ int32_t xk_row_or(int32_t v) {
  v |= xk_dpp<0xB1>(v);
  v |= xk_dpp<0x4E>(v);
  v |= xk_dpp<0x124>(v);
  return v | xk_dpp<0x128>(v);
}

/* `lines` lines of the channel at x from line `first` on in steps of inc (lines outside 0 .. 1023 read as zero and are not
   written: the reference's overrun of at most three lines lands in memory nothing reads), aac_tns.c:371-420 */
__device__ void xk_tns_run(int32_t *x, int first, int inc, int lines, int32_t lpc_hi, int t, int row_base, int shift_value,
                           int scale_spec) {
  int32_t h = 0; /* the state t + 1 lines back */
  int pos = first;
  int32_t xv = (unsigned)pos < 1024u ? x[pos] : 0;
  for (int i = 0; i < lines; i++) {
    const int next = pos + inc;
    const int32_t xn = (i + 1 < lines && (unsigned)next < 1024u) ? x[next] : 0; /* (this line's store does not touch it) */
    const int32_t y0 = fx_shl_sat(xv, scale_spec);
    const int32_t p = fx_mulhi(h, lpc_hi); /* = fx_mul32x16(state, lpc) */
    const uint32_t mag = (uint32_t)(p < 0 ? ~p : p) >> 4;
    int32_t acc = xk_row_sum(p);
    /* 16 * (sum of the lanes' mag + 16) bounds the sum of |p|: below 2^31 the saturating chain is the plain sum */
    if ((uint32_t)xk_row_sum((int32_t)mag) >= (1u << 27) - 16u) {
      acc = 0;
      for (int j = XAAC_TOOLS_TNS_MAX_ORDER; j > 0; j--) acc = fx_add_sat(acc, __shfl(p, row_base + j - 1));
    }
    const int32_t y = fx_sub_sat(y0, fx_shl_sat(acc, 1));
    const int32_t s = fx_shl_sat(y, shift_value);
    if (t == 0 && (unsigned)pos < 1024u) x[pos] = y >> scale_spec;
    const int32_t moved = xk_dpp<0x111>(h); /* row_shr:1 */
    h = t == 0 ? s : moved;
    pos = next, xv = xn;
  }
}

struct XkRowWork { /* per DPP row: the filter being set up (the 32-bit members: streams of more than two channels) */
  int16_t parcor[16], lpc[20], t1[16], t2[16];
  int32_t parcor32[16], lpc32[20], z[16], w[16];
  int32_t scale;
};

}  // namespace

__global__ __launch_bounds__(64) void xaac_aac_tools_kernel(XaacAacToolsParams p) {
  __shared__ __attribute__((aligned(16))) int32_t s_spec[2][1024];
  __shared__ __attribute__((aligned(16))) uint32_t s_side_words[(sizeof(xaac_core_tools_side) + 3) / 4];
  __shared__ uint8_t s_band_of_line[1024];
  __shared__ int32_t s_corr[XAAC_TOOLS_BANDS];
  __shared__ uint8_t s_group_of_win[2][8], s_win_in_group[2][8];
  __shared__ XkRowWork s_row[2];
  const int lane = threadIdx.x, e = blockIdx.x;
  if (e >= p.n) return;

  { /* the side info, and whether the tools can run on it */
    const uint32_t *src = reinterpret_cast<const uint32_t *>(p.side + e);
    for (int i = lane; i < (int)(sizeof(xaac_core_tools_side) / 4); i += 64) s_side_words[i] = src[i];
  }
  __syncthreads();
  const xaac_core_tools_side *sd = reinterpret_cast<const xaac_core_tools_side *>(s_side_words);
  /* (a pair needs two rows of lines: behind a stride of fewer than 2048 words its second row would be the next element's) */
  if (__any(xt_side_check(sd, lane, 64) || (sd->n_ch == 2 && p.spec_stride < 2048))) {
    if (lane == 0 && p.status) p.status[e] = -1; /* spectra and state stay as they are */
    return;
  }
  const int n_ch = sd->n_ch, sr = sd->sr_index;
  int32_t *g_spec = p.spec + (size_t)e * (size_t)p.spec_stride;
  xaac_core_tools_state *g_state = p.state + e;
  for (int c = 0; c < n_ch; c++)
    for (int i = lane; i < 256; i += 64)
      reinterpret_cast<int4 *>(s_spec[c])[i] = reinterpret_cast<const int4 *>(g_spec + 1024 * c)[i];
  for (int b = lane; b < XAAC_TOOLS_BANDS; b += 64) s_corr[b] = g_state->pns_corr_seed[b];
  const int32_t seed0 = g_state->pns_seed;
  if (lane < 2 * 8) { /* the group of every window, and the window's place in it */
    const int c = lane >> 3, w = lane & 7;
    const xaac_core_tools_channel &ch = sd->ch[c < n_ch ? c : 0];
    int g = 0, at = 0;
    if (xt_is_short(ch))
      while (g < ch.num_groups - 1 && at + ch.group_len[g] <= w) at += ch.group_len[g], g++;
    s_group_of_win[c][w] = (uint8_t)g;
    s_win_in_group[c][w] = (uint8_t)(w - at);
  }
  const xaac_core_tools_channel &rc = sd->ch[n_ch - 1]; /* stereo tools: the right channel's windows (stereo.c:129) */
  {
    const bool is_short = xt_is_short(rc);
    const int16_t *swb = is_short ? xt_swb_short[sr] : xt_swb_long[sr];
    if (lane < rc.max_sfb)
      for (int k = swb[lane]; k < swb[lane + 1]; k++) s_band_of_line[k] = (uint8_t)lane;
    const int top = swb[rc.max_sfb], end = is_short ? 128 : 1024;
    for (int k = top + lane; k < end; k += 64) s_band_of_line[k] = 0xff;
  }
  __syncthreads();

  /* ---- M/S and intensity ------------------------------------------------------------------------------------------- */
  if (n_ch == 2) {
    const bool is_short = xt_is_short(rc);
    for (int i = lane; i < 1024; i += 64) {
      const int sfb = s_band_of_line[is_short ? (i & 127) : i];
      if (sfb == 0xff) continue;
      const int band = is_short ? 16 * s_group_of_win[1][i >> 7] + sfb : sfb;
      int32_t l = s_spec[0][i], r = s_spec[1][i];
      const int ms = sd->ms_used[band], cb = rc.cb[band];
      if (ms && sd->common_window) {
        const int32_t a = l, b = r;
        l = fx_add_sat(a, b), r = fx_sub_sat(a, b);
        s_spec[0][i] = l;
      }
      if (cb >= XT_INTENSITY_HCB2) r = xt_intensity_line(l, xt_intensity_scale(rc.sf[band], cb, ms), rc.sf[band]);
      s_spec[1][i] = r;
    }
  }
  __syncthreads();
  /* a stream of more than two channels: the three bits its scale factors left on top come off behind the stereo tools */
  for (int c = 0; c < n_ch; c++)
    if (sd->ch[c].wide) {
      const int n = xt_wide_shift_lines(sd, c);
      for (int i = lane; i < n; i += 64) s_spec[c][i] >>= 3;
    }
  __syncthreads();

  /* ---- PNS ------------------------------------------------------------------------------------------------------------ */
  if (sd->ch[0].pns_active || (n_ch == 2 && sd->ch[1].pns_active)) {
    /* slots 4 lane .. 4 lane + 3 of 2 x 128: channel, then window * 16 + sfb (EIGHT_SHORT) or sfb (long), the order in which
       the reference draws from the generator */
    int width[4], band_of[4], line_of[4], mine = 0;
    bool main_seq[4];
    for (int k = 0; k < 4; k++) {
      const int slot = 4 * lane + k, c = slot >> 7, q = slot & 127;
      width[k] = 0;
      if (c >= n_ch) continue;
      const xaac_core_tools_channel &ch = sd->ch[c];
      const bool is_short = xt_is_short(ch);
      const int win = is_short ? q >> 4 : 0, sfb = is_short ? q & 15 : q;
      if (!ch.pns_active || sfb >= ch.max_sfb) continue;
      const int band = is_short ? 16 * s_group_of_win[c][win] + sfb : sfb;
      if (!ch.pns_used[band]) continue;
      const int16_t *swb = is_short ? xt_swb_short[sr] : xt_swb_long[sr];
      width[k] = swb[sfb + 1] - swb[sfb];
      band_of[k] = band;
      line_of[k] = 128 * win + swb[sfb];
      main_seq[k] = !(sd->pns_correlated[band] && c == 1);
      if (main_seq[k]) mine += width[k];
    }
    int before = mine; /* inclusive prefix sum over the lanes, then the lanes in front */
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(before, d);
      if (lane >= d) before += v;
    }
    const int total = __shfl(before, 63);
    before -= mine;
    int32_t seed[4];
    for (int k = 0; k < 4; k++) {
      if (!width[k] || !main_seq[k]) continue;
      seed[k] = xt_lcg_jump(seed0, (uint32_t)before);
      before += width[k];
      /* the left channel's seed of a correlated band: what its last window of the group starts from stays */
      const int slot = 4 * lane + k, c = slot >> 7, q = slot & 127;
      if (c == 0 && sd->pns_correlated[band_of[k]]) {
        const xaac_core_tools_channel &ch = sd->ch[0];
        const int win = xt_is_short(ch) ? q >> 4 : 0;
        if (s_win_in_group[0][win] == ch.group_len[s_group_of_win[0][win]] - 1) s_corr[band_of[k]] = seed[k];
      }
    }
    __syncthreads();
    for (int k = 0; k < 4; k++) {
      if (!width[k] || main_seq[k]) continue;
      const int win = xt_is_short(sd->ch[1]) ? ((4 * lane + k) & 127) >> 4 : 0;
      seed[k] = xt_lcg_jump(s_corr[band_of[k]], (uint32_t)(s_win_in_group[1][win] * width[k]));
    }
    __syncthreads();
    for (int k = 0; k < 4; k++) {
      if (!width[k]) continue;
      const int slot = 4 * lane + k, c = slot >> 7;
      const xaac_core_tools_channel &ch = sd->ch[c];
      const int sf = ch.sf[band_of[k]];
      int32_t s = seed[k];
      xt_gen_rand_vec(xt_pns_mant(sf), xt_pns_exp(sf), &s_spec[c][line_of[k]], width[k] - 1, &s);
      if (!main_seq[k]) { /* the right channel's draws move the band's seed on: the group's last window leaves it */
        const int win = xt_is_short(ch) ? (slot & 127) >> 4 : 0;
        if (s_win_in_group[1][win] == ch.group_len[s_group_of_win[1][win]] - 1) s_corr[band_of[k]] = s;
      }
    }
    __syncthreads();
    if (lane == 0) g_state->pns_seed = xt_lcg_jump(seed0, (uint32_t)total);
    for (int b = lane; b < XAAC_TOOLS_BANDS; b += 64) g_state->pns_corr_seed[b] = s_corr[b];
  }

  /* ---- TNS ------------------------------------------------------------------------------------------------------------ */
  {
    const int row = lane >> 4, t = lane & 15, row_base = lane & ~15;
    if (row < n_ch && sd->ch[row].tns_present) {
      const xaac_core_tools_channel &ch = sd->ch[row];
      const bool is_short = xt_is_short(ch);
      int32_t *x = s_spec[row];
      XkRowWork &wk = s_row[row];
      for (int win = 0; win < (is_short ? 8 : 1); win++)
        for (int f = 0; f < ch.n_filt[win]; f++) {
          const xaac_tns_filter_side &flt = ch.tns[is_short ? win : f];
          XtTnsPlan pl;
          if (!xt_tns_plan(sd, ch, win, flt, &pl)) continue;
          const bool wide = ch.wide != 0;
          if (t == 0) {
            int scale;
            if (wide) { /* the 32-bit variant: the taps are whole words, the recursion below is the same */
              for (int i = 0; i < flt.order; i++) wk.parcor32[i] = xt_tns_parcor32(flt, i);
              xt_parcor_to_lpc32(wk.parcor32, wk.lpc32, &scale, flt.order, wk.z, wk.w);
            } else {
              for (int i = 0; i < flt.order; i++) wk.parcor[i] = xt_tns_parcor(flt, i);
              xt_parcor_to_lpc(wk.parcor, wk.lpc, &scale, flt.order, wk.t1, wk.t2);
            }
            wk.scale = scale;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          const int scale_lpc = wk.scale;
          const int32_t lpc_hi = t >= flt.order ? 0 : wide ? wk.lpc32[t + 1] : (int32_t)((uint32_t)(uint16_t)wk.lpc[t + 1] << 16);
          int32_t *region = x + (win << 7) + pl.start;
          int32_t m = 0;
          for (int i = t; i < pl.size; i += 16) m |= xt_tns_mag_bits(region[i]);
          int scale_spec = xt_tns_scale_spec(fx_norm32(xk_row_or(m)), scale_lpc, wide);
          if (scale_spec > 0) {
            if (scale_spec > 31) scale_spec = 31;
            xk_tns_run(x, pl.first, pl.inc, pl.lines, lpc_hi, t, row_base, scale_lpc, scale_spec);
          } else {
            /* not enough headroom: window 0's lines of the region down (pns_js_thumb.c:455), filter, this window's up */
            int32_t *down = x + pl.start;
            scale_spec = -scale_spec;
            if (scale_spec > 31) scale_spec = 31;
            for (int i = t; i < pl.size; i += 16) down[i] >>= scale_spec;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            xk_tns_run(x, pl.first, pl.inc, pl.lines, lpc_hi, t, row_base, scale_lpc, 0);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int i = t; i < pl.size; i += 16) region[i] = fx_shlw(region[i], scale_spec);
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
    }
  }
  __syncthreads();

  for (int c = 0; c < n_ch; c++)
    for (int i = lane; i < 256; i += 64)
      reinterpret_cast<int4 *>(g_spec + 1024 * c)[i] = reinterpret_cast<const int4 *>(s_spec[c])[i];
  if (lane == 0 && p.status) p.status[e] = 0;
}

extern "C" hipError_t xaac_launch_aac_tools(const XaacAacToolsParams *p, hipStream_t stream) {
  hipLaunchKernelGGL(xaac_aac_tools_kernel, dim3(p->n), dim3(XAAC_AAC_TOOLS_BLOCK), 0, stream, *p);
  return hipGetLastError();
}

extern "C" int xaac_aac_tools_lds_bytes(void) {
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&xaac_aac_tools_kernel)) != hipSuccess) return 0;
  return (int)a.sharedSizeBytes;
}

/* xaac_warm_up (xaac_abi.cpp): asking for a kernel's attributes puts this translation unit's code object on the device */
extern "C" hipError_t xaac_warm_aac_tools(void) {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&xaac_aac_tools_kernel));
}
