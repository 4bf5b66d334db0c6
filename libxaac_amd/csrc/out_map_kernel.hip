/*
 * out_map_kernel.hip -- the AAC-LC hand-off with the limiter off (-peak_limiter_off:1) on gfx950: ixheaacd_scale_adjust
 * (decoder/ixheaacd_peak_limiter.c:324-334, a wrapping multiply by 2^qshift_adj) and the round16 loop of
 * decoder/ixheaacd_api.c:3676-3681, from the planar or interleaved WORD32 block xaac_imdct_process_batch leaves to interleaved
 * PCM16, with an output map of out_map.h (downmix to stereo, mono mix, mono twice) where one is asked for.
 *
 * One lane per (stream, sample): the sample's NCH words are loaded together, converted, mapped in registers and leave as one run.
 * Vector stores only, no LDS, no scratch.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "out_map.h"
#include "out_map_kernel.h"

static_assert(XAAC_SCALE_ADJUST_BLOCK == 256, "the kernel's (stream, sample) index is written for blocks of 256 lanes");
template <int NCH, int MAP>
__global__ __launch_bounds__(XAAC_SCALE_ADJUST_BLOCK) void xaac_scale_adjust_map_kernel(XaacScaleAdjustParams p) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; /* (stream, sample) */
  const int L = p.frame_len;
  if (e >= (int64_t)p.n_streams * L) return;
  const int64_t s = e / L;
  const int i = (int)(e - s * L);
  const int32_t *x = p.samples + s * p.stride;
  const int8_t *qs = p.qshift_adj + s * NCH;
  int32_t v[NCH];
  if (p.planar) {
#pragma unroll
    for (int c = 0; c < NCH; c++) v[c] = x[(int64_t)c * L + i];
  } else {
#pragma unroll
    for (int c = 0; c < NCH; c++) v[c] = x[(int64_t)i * NCH + c];
  }
  int16_t w[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) w[c] = xo_scale_round16(v[c], qs[c]);
  if constexpr (MAP == XAAC_OUT_MAP_NONE) {
    int16_t *dst = p.pcm16 + e * NCH;
    if constexpr ((NCH & 1) == 0) { /* an even number of words per sample: 4-byte aligned at every sample (xaac_abi.cpp checks pcm16) */
#pragma unroll
      for (int c = 0; c < NCH; c += 2)
        reinterpret_cast<uint32_t *>(dst)[c >> 1] = (uint32_t)(uint16_t)w[c] | ((uint32_t)(uint16_t)w[c + 1] << 16);
    } else {
#pragma unroll
      for (int c = 0; c < NCH; c++) dst[c] = w[c];
    }
  } else if constexpr (MAP == XAAC_OUT_MAP_MONO_MIX) {
    p.pcm16[e] = xo_mono_mix(w[0], w[NCH - 1]);
  } else {
    int16_t l, r;
    if constexpr (MAP == XAAC_OUT_MAP_DOWNMIX_STEREO) {
      int32_t cl[NCH], cr[NCH];
#pragma unroll
      for (int c = 0; c < NCH; c++) cl[c] = p.map_coef[0][c], cr[c] = p.map_coef[1][c];
      xo_downmix<NCH>(cl, cr, w, l, r);
    } else {
      l = r = MAP == XAAC_OUT_MAP_MONO_MIX_DUP ? xo_mono_mix(w[0], w[NCH - 1]) : w[0];
    }
    reinterpret_cast<uint32_t *>(p.pcm16)[e] = (uint32_t)(uint16_t)l | ((uint32_t)(uint16_t)r << 16);
  }
}

/* the map's channel count is the batch's (xaac_abi.cpp checks against the same rows of out_map.h); a pair without a row is an error */
extern "C" hipError_t xaac_launch_scale_adjust_map(const XaacScaleAdjustParams *p, hipStream_t stream) {
  const bool found = xo_dispatch(p->map_kind, p->num_channels, [&](auto nch, auto map) {
    hipLaunchKernelGGL((xaac_scale_adjust_map_kernel<decltype(nch)::value, decltype(map)::value>),
                       dim3((unsigned)xaac_scale_adjust_grid(p->n_streams, p->frame_len)), dim3(XAAC_SCALE_ADJUST_BLOCK), 0, stream, *p);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

/* xaac_warm_up (xaac_abi.cpp): asking for a kernel's attributes puts this translation unit's code object on the device */
extern "C" hipError_t xaac_warm_out_map(void) {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&xaac_scale_adjust_map_kernel<2, XAAC_OUT_MAP_NONE>));
}
