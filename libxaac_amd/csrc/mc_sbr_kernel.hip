/*
 * mc_sbr_kernel.hip -- the element-strided hand-offs on either side of the per-element SBR calls of a stream with more than two
 * channels (ADTS channel_config 3 .. 6; decoder/ixheaacd_api.c:3176-3178, :3373-3500: one SBR decoder per channel element, each
 * reading and writing its channels of the frame's interleaved block at stride total_channels from its slot).
 *
 *   xaac_mc_core_from_out32_kernel   the core decoder's WORD32 time samples -> the float planes the Path A branch reads,
 *                                    through the 16-bit conversion ixheaacd_allocate_sbr_scr makes IN PLACE in that block
 *   xaac_mc_pcm_out_kernel           the planes the SBR calls leave (float: ixheaacd_samples_sat_mc; PCM16: the low-power
 *                                    synthesis bank's) -> the [stream][2048][channel] PCM16 block in output channel order
 *   xaac_mc_pcm_out_map_kernel       ... -> the [stream][2048][2] block of the downmix to stereo (out_map.h)
 *
 * Vector stores only.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fx.h"
#include "mc_sbr_kernel.h"
#include "out_map.h"

namespace {

/* decode_main.c:145-150: clamp to [-32768, 32767], truncate towards zero */
__device__ __forceinline__ int16_t mc_sat(float v) {
  if (v > 32767.0f) v = 32767.0f;
  else if (v < -32768.0f) v = -32768.0f;
  return (int16_t)v;
}
__device__ __forceinline__ int16_t mc_sat(int16_t v) { return v; }

template <class T>
struct Pair;
template <>
struct Pair<float> {
  typedef float2 type;
};
template <>
struct Pair<int16_t> {
  typedef short2 type;
};

}  // namespace

/* A lane holds all NCH channels of two neighbouring samples: the NCH plane loads (8 / 4 bytes each) are issued together, the
   2 * NCH PCM16 words leave as NCH 32-bit words -- the arrangement of the limiter's CT = 3 .. 6 instantiations.  src[o]: the plane
   of output channel o. */
template <int NCH, class T>
__global__ __launch_bounds__(256) void xaac_mc_pcm_out_kernel(XaacMcPcmOutParams p, int32_t src0, int32_t src1, int32_t src2, int32_t src3,
                                                              int32_t src4, int32_t src5) {
  typedef typename Pair<T>::type T2;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; /* (stream, sample pair) */
  if (e >= (size_t)p.n_streams * 1024) return;
  const size_t i = e >> 10;
  const int k = (int)(e & 1023) * 2;
  const int32_t src[6] = {src0, src1, src2, src3, src4, src5};
  const T *planes = static_cast<const T *>(p.planes);
  T2 v[NCH];
#pragma unroll
  for (int o = 0; o < NCH; o++) v[o] = *reinterpret_cast<const T2 *>(planes + (i * NCH + (size_t)src[o]) * (size_t)p.stride + k);
  int16_t w[2 * NCH];
#pragma unroll
  for (int o = 0; o < NCH; o++) w[o] = mc_sat(v[o].x), w[NCH + o] = mc_sat(v[o].y);
  uint32_t *dst = reinterpret_cast<uint32_t *>(p.pcm) + ((i * 2048 + (size_t)k) * NCH) / 2;
#pragma unroll
  for (int d = 0; d < NCH; d++) dst[d] = (uint32_t)(uint16_t)w[2 * d] | ((uint32_t)(uint16_t)w[2 * d + 1] << 16);
}

/* The same with the downmix to stereo (out_map.h) on the way out: the lane's 2 * NCH words become two stereo pairs, and only
   [stream][2048][2] is stored.  cl / cr: the left / right Q30 coefficient of every output channel. */
template <int NCH, class T>
__global__ __launch_bounds__(256) void xaac_mc_pcm_out_map_kernel(XaacMcPcmOutParams p, XaacMcMapCoef m) {
  typedef typename Pair<T>::type T2;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; /* (stream, sample pair) */
  if (e >= (size_t)p.n_streams * 1024) return;
  const size_t i = e >> 10;
  const int k = (int)(e & 1023) * 2;
  const T *planes = static_cast<const T *>(p.planes);
  T2 v[NCH];
#pragma unroll
  for (int o = 0; o < NCH; o++) v[o] = *reinterpret_cast<const T2 *>(planes + (i * NCH + (size_t)m.src[o]) * (size_t)p.stride + k);
  int16_t a[NCH], b[NCH];
  int32_t cl[NCH], cr[NCH];
#pragma unroll
  for (int o = 0; o < NCH; o++) a[o] = mc_sat(v[o].x), b[o] = mc_sat(v[o].y), cl[o] = m.coef[0][o], cr[o] = m.coef[1][o];
  int16_t l0, r0, l1, r1;
  xo_downmix<NCH>(cl, cr, a, l0, r0);
  xo_downmix<NCH>(cl, cr, b, l1, r1);
  uint32_t *dst = reinterpret_cast<uint32_t *>(p.pcm) + (i * 2048 + (size_t)k);
  dst[0] = (uint32_t)(uint16_t)l0 | ((uint32_t)(uint16_t)r0 << 16);
  dst[1] = (uint32_t)(uint16_t)l1 | ((uint32_t)(uint16_t)r1 << 16);
}

/* ixheaacd_allocate_sbr_scr (api.c:351-359) for an element of a block of more than two channels, then api.c:3414-3434.  The
   element's channel j is converted with qshift_adj[j] of the FRAME (the j-th channel the frame decoded, whichever element it
   belongs to), and the conversion runs in place, channel after channel: the WORD16 results of a pair's first channel land in
   halves of WORD32 words of which some are its second channel's samples 0 .. 511, not yet converted -- where the pair's slot and
   the channel count put them there (mix: 1 the low half, 2 the high half; sample n takes channel c - 1's PCM sample 2 n + 1).
   A block of 256 threads works on a quarter of one channel-frame. */
__global__ __launch_bounds__(256) void xaac_mc_core_from_out32_kernel(XaacMcCoreInParams p) {
  const int row = (int)(blockIdx.x >> 2); /* < n_streams * n_ch: the grid is exactly four blocks per row */
  const int n = (int)(blockIdx.x & 3) * 256 + (int)threadIdx.x;
  const int c = row % p.n_ch, first = row - c;
  int32_t v = p.out32[(size_t)row * 1024 + n];
  const int mix = p.mix[c];
  if (mix && n < 512) {
    const int32_t peer = p.out32[(size_t)(row - 1) * 1024 + 2 * n + 1];
    const uint16_t h = (uint16_t)fx_round16(fx_shl_sat(peer, p.qshift_adj[first + p.q_src[c - 1]]));
    v = mix == 1 ? (int32_t)(((uint32_t)v & 0xffff0000u) | h) : (int32_t)(((uint32_t)h << 16) | ((uint32_t)v & 0xffffu));
  }
  p.core[(size_t)row * 1024 + n] = (float)fx_round16(fx_shl_sat(v, p.qshift_adj[first + p.q_src[c]]));
}

namespace {
template <class T>
hipError_t launch_out(const XaacMcPcmOutParams *p, hipStream_t stream) {
  int32_t src[6] = {0, 0, 0, 0, 0, 0};
  for (int c = 0; c < p->n_ch; c++) src[p->slot[c]] = c;
  const dim3 grid((unsigned)(((size_t)p->n_streams * 1024 + 255) / 256)), block(256);
  switch (p->n_ch) {
    case 3: hipLaunchKernelGGL((xaac_mc_pcm_out_kernel<3, T>), grid, block, 0, stream, *p, src[0], src[1], src[2], src[3], src[4], src[5]); break;
    case 4: hipLaunchKernelGGL((xaac_mc_pcm_out_kernel<4, T>), grid, block, 0, stream, *p, src[0], src[1], src[2], src[3], src[4], src[5]); break;
    case 5: hipLaunchKernelGGL((xaac_mc_pcm_out_kernel<5, T>), grid, block, 0, stream, *p, src[0], src[1], src[2], src[3], src[4], src[5]); break;
    case 6: hipLaunchKernelGGL((xaac_mc_pcm_out_kernel<6, T>), grid, block, 0, stream, *p, src[0], src[1], src[2], src[3], src[4], src[5]); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
}  // namespace

extern "C" hipError_t xaac_launch_mc_pcm16_from_float(const XaacMcPcmOutParams *p, hipStream_t stream) { return launch_out<float>(p, stream); }
extern "C" hipError_t xaac_launch_mc_pcm16_from_planes(const XaacMcPcmOutParams *p, hipStream_t stream) { return launch_out<int16_t>(p, stream); }

namespace {
template <class T>
hipError_t launch_out_map(const XaacMcPcmOutParams *p, const int32_t (*coef)[6], hipStream_t stream) {
  XaacMcMapCoef m;
  for (int c = 0; c < 6; c++) m.src[c] = 0, m.coef[0][c] = coef[0][c], m.coef[1][c] = coef[1][c];
  for (int c = 0; c < p->n_ch; c++) m.src[p->slot[c]] = c;
  const dim3 grid((unsigned)(((size_t)p->n_streams * 1024 + 255) / 256)), block(256);
  hipError_t e = hipErrorInvalidValue; /* no downmix row of out_map.h for this many channels: no kernel */
  xo_dispatch(XAAC_OUT_MAP_DOWNMIX_STEREO, p->n_ch, [&](auto nch, auto map) {
    if constexpr (decltype(map)::value == XAAC_OUT_MAP_DOWNMIX_STEREO) {
      hipLaunchKernelGGL((xaac_mc_pcm_out_map_kernel<decltype(nch)::value, T>), grid, block, 0, stream, *p, m);
      e = hipGetLastError();
    }
  });
  return e;
}
}  // namespace

extern "C" hipError_t xaac_launch_mc_pcm16_from_float_map(const XaacMcPcmOutParams *p, const int32_t (*coef)[6], hipStream_t stream) {
  return launch_out_map<float>(p, coef, stream);
}
extern "C" hipError_t xaac_launch_mc_pcm16_from_planes_map(const XaacMcPcmOutParams *p, const int32_t (*coef)[6], hipStream_t stream) {
  return launch_out_map<int16_t>(p, coef, stream);
}

extern "C" hipError_t xaac_launch_mc_core_from_out32(const XaacMcCoreInParams *p, hipStream_t stream) {
  hipLaunchKernelGGL(xaac_mc_core_from_out32_kernel, dim3((unsigned)((size_t)p->n_streams * p->n_ch * 4)), dim3(256), 0, stream, *p);
  return hipGetLastError();
}

/* xaac_warm_up (xaac_abi.cpp): asking for a kernel's attributes puts this translation unit's code object on the device */
extern "C" hipError_t xaac_warm_mc_sbr(void) {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(xaac_mc_core_from_out32_kernel));
}
