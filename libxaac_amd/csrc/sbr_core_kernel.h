/* sbr_core_kernel.h -- launch interface of the SBR core kernel (internal). */
#ifndef XAAC_SBR_CORE_KERNEL_H
#define XAAC_SBR_CORE_KERNEL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/xaac_amd.h"
#include "sbr_chain.h"

#define XAAC_SBR_NARROW_BANDS 48                 /* bands per LDS row of the HQ core's narrow-row kernel */
#ifndef XAAC_SBR_CORE_HQ_WAVES
#define XAAC_SBR_CORE_HQ_WAVES 4                 /* its waves per workgroup (they share the lookup tables in LDS) */
#endif

typedef struct XaacSbrCoreParams {
  int32_t n_ch;
  const xaac_sbr_header *header;
  const xaac_sbr_frame *frame;
  xaac_sbr_state *state;
  int32_t *x;        /* [n_ch][XAAC_SBR_X_WORDS] */
  XaacSynPar *syn_par; /* [n_ch]: out, for the synthesis bank (sbr_chain.h) */
  int32_t *status;   /* optional [n_ch] */
  /* HQ only, optional (both or neither): [n_ch] stream numbers + one counter.  With them the launch runs the narrow-row
     kernel first and the streams it cannot take through the 64-band rows afterwards (sbr_core_kernel.hip) */
  int32_t *defer_list, *defer_count;
  int32_t *work_counter; /* = defer_count + 1: the persistent waves' next channel-frame */
  int32_t num_cu;        /* compute units of the device (grid of the persistent launch) */
  int32_t counters_zeroed; /* 1: an earlier launch on the stream has cleared defer_count / work_counter */
  int32_t qmf_slots;       /* QMF slots of the frames: 0 / 32, or 30 (960-sample cores: xaac_sbr_lp960_process_batch,
                              xaac_sbr_hq960_process_batch) */
  int32_t narrow_only;     /* the caller's assertion (xaac_sbr_hq_batch.max_band_hint): no list launch; a stream that needs the 64-band
                              rows is refused */
} XaacSbrCoreParams;

#ifdef __cplusplus
extern "C" {
#endif
hipError_t xaac_launch_sbr_core_lp(const XaacSbrCoreParams *p, hipStream_t stream);
/* qmf_slots 30 only: xs_side_info_bad of every channel up front, the verdict in syn_par[ch].refused */
hipError_t xaac_launch_sbr_screen(const XaacSbrCoreParams *p, hipStream_t stream);
/* HQ: x rows are 128 words (64 real | 64 imaginary): [n_ch][2 * XAAC_SBR_X_WORDS] */
hipError_t xaac_launch_sbr_core_hq(const XaacSbrCoreParams *p, hipStream_t stream);
hipError_t xaac_warm_sbr_core(void);
#ifdef __cplusplus
}
#endif
#endif
