/* drc_kernel.h -- launch interface of drc_kernel.hip: dynamic range control on the spectra in front of the IMDCT (internal). */
#ifndef XAAC_DRC_KERNEL_H
#define XAAC_DRC_KERNEL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/xaac_drc.h"

#define XAAC_DRC_WAVES 4                     /* one wave per channel-frame row; no LDS */
#define XAAC_DRC_BLOCK (64 * XAAC_DRC_WAVES)
#define XAAC_DRC_LDS_BYTES 0
static inline int32_t xaac_drc_grid(int32_t n) { return (n + XAAC_DRC_WAVES - 1) / XAAC_DRC_WAVES; }

typedef struct XaacDrcParams {
  int32_t n;
  int32_t spec_stride;
  int32_t *spec;
  const xaac_drc_side *side;
  int32_t *status; /* or null */
} XaacDrcParams;

#ifdef __cplusplus
extern "C" {
#endif
hipError_t xaac_launch_drc(const XaacDrcParams *p, hipStream_t stream);
hipError_t xaac_warm_drc(void);
#ifdef __cplusplus
}
#endif
#endif
