/* sbr_ld_core_kernel.h -- launch interface of the low-delay SBR core kernel (internal). */
#ifndef XAAC_SBR_LD_CORE_KERNEL_H
#define XAAC_SBR_LD_CORE_KERNEL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/xaac_amd.h"
#include "sbr_chain.h"

#define XAAC_SBR_LD_CORE_BLOCK 64 /* one wave per channel, no dynamic LDS: what xaac_sbr_eld_process_batch reports of its chain */

typedef struct XaacSbrLdCoreParams {
  int32_t n_ch, n_slots;
  const xaac_sbr_header *header;
  const xaac_sbr_frame *frame;
  xaac_sbr_eld_state *state;
  int32_t *x;        /* [n_ch][n_slots][XAAC_SBR_ROW_WORDS_HQ]: the analysed slots in, the synthesis bank's rows out */
  XaacSynPar *syn_par; /* [n_ch]: out, for the synthesis bank (sbr_chain.h); skip = 1 where the frame is not synthesised */
  int32_t *status;   /* optional [n_ch] */
} XaacSbrLdCoreParams;

#ifdef __cplusplus
extern "C" {
#endif
hipError_t xaac_launch_sbr_ld_core(const XaacSbrLdCoreParams *p, hipStream_t stream);
hipError_t xaac_warm_sbr_ld_core(void);
#ifdef __cplusplus
}
#endif
#endif
