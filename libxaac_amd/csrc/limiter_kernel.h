/* limiter_kernel.h -- launch interface of the peak limiter kernel (internal). */
#ifndef XAAC_LIMITER_KERNEL_H
#define XAAC_LIMITER_KERNEL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/xaac_amd.h"

#define XAAC_LIM_BLOCK 64 /* one wave per stream (front, apply) or per 64 streams (gain) */
#define XAAC_LIM_FRONT_LDS ((2 * (XAAC_LIM_MAX_ATTACK + 1024) + 64) * 4) /* the front kernel's static arrays: s_w, s_g, s_run */

typedef struct XaacLimiterParams {
  int32_t n_streams, frame_len, num_channels;
  int32_t planar; /* samples: [channel][frame_len] per stream instead of [frame_len][channel] */
  int32_t *samples;
  int64_t stride;
  const int8_t *qshift_adj;
  xaac_limiter_state *state;
  int16_t *pcm16;
  int32_t *status;
  float *ws_gain;   /* [n_streams][1024]: target gains -> gains of the streams the recursion runs on */
  int32_t *ws_flag; /* [n_streams][2]: finished by the front kernel?, first sample of the recursion */
  long long *dbg; /* phase timers (profiling builds) */
  int32_t map_kind;        /* xaac_launch_limiter_map: XAAC_OUT_MAP_* on the PCM16 hand-off, pcm16 dense at the mapped channel count */
  int32_t map_coef[2][6];  /* ... DOWNMIX_STEREO: left / right Q30 coefficient of every slot (out_map.h: xo_resolve) */
} XaacLimiterParams;

#ifdef __cplusplus
extern "C" {
#endif
hipError_t xaac_launch_limiter(const XaacLimiterParams *p, hipStream_t stream);
hipError_t xaac_launch_limiter_map(const XaacLimiterParams *p, hipStream_t stream);
hipError_t xaac_warm_limiter(void);
#ifdef __cplusplus
}
#endif
#endif
