/* out_map_kernel.h -- launch interface of out_map_kernel.hip: the limiter-off PCM16 hand-off with an output map (internal). */
#ifndef XAAC_OUT_MAP_KERNEL_H
#define XAAC_OUT_MAP_KERNEL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define XAAC_SCALE_ADJUST_BLOCK 256 /* one lane per (stream, sample); no LDS */
static inline int64_t xaac_scale_adjust_grid(int32_t n_streams, int32_t frame_len) {
  return ((int64_t)n_streams * frame_len + XAAC_SCALE_ADJUST_BLOCK - 1) / XAAC_SCALE_ADJUST_BLOCK;
}

typedef struct XaacScaleAdjustParams {
  int32_t n_streams, frame_len, num_channels;
  int32_t planar;          /* samples: [channel][frame_len] per stream instead of [frame_len][channel] */
  const int32_t *samples;
  int64_t stride;
  const int8_t *qshift_adj;
  int16_t *pcm16;
  int32_t map_kind;        /* XAAC_OUT_MAP_* */
  int32_t map_coef[2][6];  /* DOWNMIX_STEREO: left / right Q30 coefficient of every slot (out_map.h: xo_resolve) */
} XaacScaleAdjustParams;

#ifdef __cplusplus
extern "C" {
#endif
hipError_t xaac_launch_scale_adjust_map(const XaacScaleAdjustParams *p, hipStream_t stream);
hipError_t xaac_warm_out_map(void);
#ifdef __cplusplus
}
#endif
#endif
