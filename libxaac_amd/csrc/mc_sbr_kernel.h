/* mc_sbr_kernel.h -- launch helpers of mc_sbr_kernel.hip: the element-strided hand-offs around the per-element SBR calls of a
   stream with more than two channels (include/xaac_esbr.h: xaac_mc_*_batch). */
#ifndef XAAC_MC_SBR_KERNEL_H
#define XAAC_MC_SBR_KERNEL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define XAAC_MC_MAX_CH 6

typedef struct XaacMcPcmOutParams {
  int32_t n_streams, n_ch, stride;  /* stride: floats / int16 words between consecutive planes (even, >= 2048) */
  int32_t slot[XAAC_MC_MAX_CH];     /* output channel of plane c */
  const void *planes;               /* float or int16 [n_streams * n_ch] planes of 2048 samples */
  int16_t *pcm;                     /* [n_streams][2048][n_ch] */
} XaacMcPcmOutParams;

typedef struct XaacMcMapCoef {
  int32_t src[XAAC_MC_MAX_CH];      /* plane of output channel o */
  int32_t coef[2][XAAC_MC_MAX_CH];  /* left / right Q30 downmix coefficient of output channel o */
} XaacMcMapCoef;

typedef struct XaacMcCoreInParams {
  int32_t n_streams, n_ch;
  int32_t q_src[XAAC_MC_MAX_CH];    /* channel of the stream whose qshift_adj channel c is converted with */
  int32_t mix[XAAC_MC_MAX_CH];      /* 0; 1 / 2: the low / high half of samples 0..511 comes from channel c - 1's PCM */
  const int32_t *out32;             /* [n_streams * n_ch][1024] */
  const int8_t *qshift_adj;         /* [n_streams * n_ch] */
  float *core;                      /* [n_streams * n_ch][1024] */
} XaacMcCoreInParams;

#ifdef __cplusplus
extern "C" {
#endif
hipError_t xaac_launch_mc_pcm16_from_float(const XaacMcPcmOutParams *p, hipStream_t stream);
hipError_t xaac_launch_mc_pcm16_from_planes(const XaacMcPcmOutParams *p, hipStream_t stream);
/* the downmix to stereo on the way out: pcm is [n_streams][2048][2]; coef[side][output channel] from xo_resolve (out_map.h) */
hipError_t xaac_launch_mc_pcm16_from_float_map(const XaacMcPcmOutParams *p, const int32_t (*coef)[6], hipStream_t stream);
hipError_t xaac_launch_mc_pcm16_from_planes_map(const XaacMcPcmOutParams *p, const int32_t (*coef)[6], hipStream_t stream);
hipError_t xaac_launch_mc_core_from_out32(const XaacMcCoreInParams *p, hipStream_t stream);
hipError_t xaac_warm_mc_sbr(void);
#ifdef __cplusplus
}
#endif
#endif
