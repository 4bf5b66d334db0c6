/*
 * drc_kernel.hip -- MPEG-4 dynamic range control in the spectral domain on gfx950: the sbr_found == 0 branch of ixheaacd_drc_apply
 * (decoder/ixheaacd_drc_freq_dec.c:956-1017, :1098) on the lines xaac_imdct_process_batch is about to read, with the gain factors
 * the host made (drc.h: xd_band_fac).
 *
 * One wave per channel-frame row.  A lane owns four groups of four consecutive lines, group g at line 4 * (64 g + lane): a load or
 * store instruction of the wave covers 1 KB of the row, 16 bytes a lane.  Band ends are multiples of four (xd_side_ok), so a group
 * lies in a band or outside it as a whole.  The side row is the wave's alone: its words come in through the scalar cache.  The
 * bands are walked in order, each from the end of the one before, so lines that two bands cover are multiplied twice, each time
 * with its own truncation and saturation, as the reference does.  A row whose factors are all 1.0 returns before it reads a
 * line; only groups that a band covered are written back.  Vector stores only, no LDS, no scratch.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "drc.h"
#include "drc_kernel.h"

static_assert(XAAC_DRC_BLOCK == 256 && XAAC_DRC_WAVES == 4, "the kernel's row index is written for four waves of 64 lanes");
__global__ __launch_bounds__(XAAC_DRC_BLOCK) void xaac_drc_kernel(XaacDrcParams p) {
  const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * XAAC_DRC_WAVES + (threadIdx.x >> 6)));
  if (row >= p.n) return;
  const int lane = threadIdx.x & 63;
  const xaac_drc_side *s = p.side + row;
  const int ok = xd_side_ok(s);
  if (p.status && lane == 0) p.status[row] = ok ? 0 : XAAC_DRC_REFUSED;
  if (!ok || xd_side_identity(s)) return;
  int4 *x = reinterpret_cast<int4 *>(p.spec + (int64_t)row * p.spec_stride) + lane;
  int4 v[4];
#pragma unroll
  for (int g = 0; g < 4; g++) v[g] = x[64 * g];
  const int n_bands = s->n_bands;
  int start = 0;
  unsigned touched = 0;
  for (int k = 0; k < n_bands; k++) {
    const int end = s->end[k];
    const int32_t fac = s->fac[k];
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int at = 4 * (64 * g + lane);
      if (at >= start && at < end) {
        v[g].x = xd_line(v[g].x, fac), v[g].y = xd_line(v[g].y, fac), v[g].z = xd_line(v[g].z, fac), v[g].w = xd_line(v[g].w, fac);
        touched |= 1u << g;
      }
    }
    start = end;
  }
#pragma unroll
  for (int g = 0; g < 4; g++)
    if (touched & (1u << g)) x[64 * g] = v[g];
}

extern "C" hipError_t xaac_launch_drc(const XaacDrcParams *p, hipStream_t stream) {
  hipLaunchKernelGGL(xaac_drc_kernel, dim3((unsigned)xaac_drc_grid(p->n)), dim3(XAAC_DRC_BLOCK), XAAC_DRC_LDS_BYTES, stream, *p);
  return hipGetLastError();
}

/* xaac_warm_up (xaac_abi.cpp): asking for a kernel's attributes puts this translation unit's code object on the device */
extern "C" hipError_t xaac_warm_drc(void) {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&xaac_drc_kernel));
}
