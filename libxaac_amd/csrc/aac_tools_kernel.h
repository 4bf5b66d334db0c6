/* aac_tools_kernel.h -- launch interface of the AAC spectral tools kernel (internal). */
#ifndef XAAC_AAC_TOOLS_KERNEL_H
#define XAAC_AAC_TOOLS_KERNEL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/xaac_tools.h"

#define XAAC_AAC_TOOLS_BLOCK 64 /* one wave per channel element */
#ifdef __cplusplus
extern "C" {
#endif
int xaac_aac_tools_lds_bytes(void); /* the kernel's static LDS, from its attributes (0 if they cannot be read) */
#ifdef __cplusplus
}
#endif

typedef struct XaacAacToolsParams {
  int32_t n;
  int32_t spec_stride;               /* words between two elements' spectra */
  int32_t *spec;                     /* in / out */
  const xaac_core_tools_side *side;  /* [n] */
  xaac_core_tools_state *state;      /* [n] in / out */
  int32_t *status;                   /* [n] or NULL */
} XaacAacToolsParams;

#ifdef __cplusplus
extern "C" {
#endif
hipError_t xaac_launch_aac_tools(const XaacAacToolsParams *p, hipStream_t stream);
hipError_t xaac_warm_aac_tools(void);
#ifdef __cplusplus
}
#endif
#endif
