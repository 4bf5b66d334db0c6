/* sbr_ps_kernel.h -- launch interface of the parametric-stereo kernel (internal). */
#ifndef XAAC_SBR_PS_KERNEL_H
#define XAAC_SBR_PS_KERNEL_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/xaac_amd.h"
#include "../../include/xaac_sbr.h"
#include "sbr_chain.h"

typedef struct XaacPsParams {
  int32_t n;                  /* streams */
  int32_t *x;                 /* [n][2 * XAAC_SBR_X_WORDS]: the HQ QMF matrix the core kernel left (sbr_chain.h); the n_slots rows
                                 from XAAC_SBR_X_SLOT0_ROW on become the LEFT channel, in the scale the synthesis bank wants */
  int32_t *xr;                /* [n][XAAC_SBR_XR_WORDS]: out, the RIGHT channel's n_slots slots */
  const xaac_sbr_header *header;   /* [n]: channel_mode */
  const xaac_sbr_frame *sbr_frame; /* [n]: apply_processing */
  const xaac_ps_frame *frame; /* [n] */
  xaac_ps_state *state;       /* [n] */
  xaac_sbr_state *sbr_state;  /* [n]: ps_scale is recorded here */
  XaacSynPar *par_l;          /* [n] in: the scales and band limits the core kernel left (sbr_chain.h);
                                 out: the same members rewritten for the left synthesis launch */
  XaacSynPar *par_r;          /* [n] out: scale / band parameters of the right synthesis launch;
                                 skip = 1 where the stream has no PS this frame (bank and output left alone) */
  int32_t *status;            /* optional [n]: -1 where PS side info had to be clamped into its tables */
  int32_t *dbg;               /* profiling builds (-DXS_PROFILE) only: 32 cycle counters, else unused */
  int32_t n_slots;            /* 0 / 32, or 30 (960-sample cores: par_l[i].refused != 0 marks a stream refused up front) */
} XaacPsParams;

#ifdef __cplusplus
extern "C" {
#endif
hipError_t xaac_launch_sbr_handover(const xaac_sbr_handover_batch *b, hipStream_t stream);
hipError_t xaac_launch_sbr_apply_side(const xaac_sbr_apply_side_batch *b, hipStream_t stream);
hipError_t xaac_launch_ps(const XaacPsParams *p, hipStream_t stream);
hipError_t xaac_warm_sbr_ps(void);
#ifdef __cplusplus
}
#endif
#endif
