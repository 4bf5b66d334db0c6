/*
 * xaac_abi.cpp -- the C-ABI layer of libxaac_amd.so (include/xaac_amd.h):
 * argument validation, error codes in the reference's IA_ERRORCODE convention,
 * launch geometry, and the host-buffer convenience path.  No arithmetic lives
 * here; the work is in imdct_kernel.hip.  There is deliberately NO CPU fallback:
 * without a HIP device xaac_create fails with XAAC_FATAL_NO_DEVICE.
 * Stated once, elsewhere: a kernel's block and LDS (what xaac_last_launch reports) in its *_kernel.h, a workspace's layout in
 * its struct below, the (output map, channel count) pairs in out_map.h.
 */
#include <hip/hip_runtime_api.h>
#include "build_id.h" /* build/build_id.h: XAAC_BUILD_ID (Makefile) */

#include <cstdint>
#include <cstdlib>
#include <new>

#include "../../include/xaac_amd.h"
#include "imdct_kernel.h"
#include "sbr_qmf_kernel.h"
#include "sbr_core_kernel.h"
#include "sbr_ld_core_kernel.h"
#include "sbr_ps_kernel.h"
#include "limiter_kernel.h"
#include "esbr_qmf_kernel.h"
#include "usac_imdct_kernel.h"
#include "imdct960_kernel.h"
#include "imdct_ld_kernel.h"
#include "esbr_core_kernel.h"
#include "hbe_kernel.h"
#include "pvc_kernel.h"
#include "aac_tools_kernel.h"
#include "mc_sbr_kernel.h"
#include "out_map.h"
#include "out_map_kernel.h"
#include "drc_kernel.h"
#include <cmath>
#include <cstddef>
#include <cstring>

struct xaac_ctx {
  int device;
  hipStream_t stream;
  bool owns_stream;
  int num_cu;
  int blocks_per_cu;
  int qmf_blocks_per_cu[4];
  int last_grid, last_block, last_lds;
};

/* Profiling builds (-DXS_PROFILE / -DXL_PROFILE, tools/prof_sbr_core.py, tools/time_limiter.py) collect 64-bit phase
   counters in the caller's status buffer; it then has to hold 128 of them, which the tools' batches (>= 256
   channels) do.  Regular builds never hand the kernels a counter buffer. */
#if defined(XS_PROFILE) || defined(XL_PROFILE)
#define XAAC_DBG_BUF(status, n) ((n) >= 256 ? (status) : nullptr)
#else
#define XAAC_DBG_BUF(status, n) static_cast<int32_t *>(nullptr)
#endif

/* inside an entry point: a launch (or any HIP call) that fails ends it */
#define XAAC_TRY(e) do { if (!hip_ok(e)) return XAAC_FATAL_HIP; } while (0)

namespace {

inline bool hip_ok(hipError_t e) { return e == hipSuccess; }

inline bool bad_ch_fac(int ch_fac) { return ch_fac != 1 && ch_fac != 2; }

/* persistent grid: enough workgroups to fill every CU at the kernel's occupancy, never more than the batch needs */
int fill_grid(int need, int resident) {
  const int g = need < resident ? need : resident;
  return g < 1 ? 1 : g;
}
int pick_grid(const xaac_ctx *c, int n_ch) { return fill_grid((n_ch + XAAC_IMDCT_WAVES - 1) / XAAC_IMDCT_WAVES, c->num_cu * c->blocks_per_cu); }
int qmf_grid(const xaac_ctx *c, int n_ch, int which) { /* a wave owns two channel-frames */
  return fill_grid(((n_ch + 1) / 2 + XAAC_QMF_WAVES - 1) / XAAC_QMF_WAVES, c->num_cu * c->qmf_blocks_per_cu[which]);
}

int32_t check_batch(const xaac_imdct_batch *b) {
  if (!b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  if (bad_ch_fac(b->ch_fac)) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch % b->ch_fac) return XAAC_FATAL_BAD_ARG;
  if (b->pcm_mode != XAAC_PCM_LC && b->pcm_mode != XAAC_PCM_SBR) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch > 0 && (!b->spec || !b->ics || !b->overlap || !b->state)) return XAAC_FATAL_NULL_ARG;
  return XAAC_OK;
}

/* what xaac_last_launch reports of the call that just went out */
int32_t report(xaac_ctx *c, int grid, int block, int lds) {
  c->last_grid = grid; c->last_block = block; c->last_lds = lds;
  return XAAC_OK;
}

/* the tail of an entry point whose arguments have passed: the context's device, then the launch */
template <class Launch>
int32_t run(xaac_ctx *c, Launch &&launch) {
  XAAC_TRY(hipSetDevice(c->device));
  XAAC_TRY(launch());
  return XAAC_OK;
}
/* ... and the figures of the launch */
template <class Launch>
int32_t run(xaac_ctx *c, int grid, int block, int lds, Launch &&launch) {
  const int32_t rc = run(c, launch);
  return rc == XAAC_OK ? report(c, grid, block, lds) : rc;
}

/* ---- workspace layouts ----
   One struct per workspace: its constructor walks a cursor from the caller's base over the sub-buffers, in the order they lie.
   The entry point uses the pointers; the *_workspace_bytes function makes the same walk from a null base, where every alignment
   step costs its worst case, and returns where that walk ends.  What the published sizes hold beyond that is a named constant:
   the sizes are part of the ABI (callers cache them), so they stay what they have been. */
struct Cursor {
  uintptr_t at;
  bool sizing;
  Cursor(void *base, uintptr_t a) : at(reinterpret_cast<uintptr_t>(base)), sizing(base == nullptr) { align(a); }
  Cursor &align(uintptr_t a) {
    at = sizing ? at + (a - 1) : (at + (a - 1)) & ~(a - 1);
    return *this;
  }
  template <class T>
  T *take(size_t count) {
    T *p = reinterpret_cast<T *>(at);
    at += count * sizeof(T);
    return p;
  }
};

struct SbrLpWs {
  int32_t *x;        /* [n][XAAC_SBR_X_WORDS]: the channels' QMF matrices */
  XaacSynPar *par;   /* [n]: the synthesis parameters */
  int32_t *counters; /* the core's work counter and its neighbour */
  uint64_t end;
  SbrLpWs(void *base, size_t n) {
    Cursor k(base, 256);
    x = k.take<int32_t>(n * XAAC_SBR_X_WORDS), par = k.take<XaacSynPar>(n);
    counters = k.align(64).take<int32_t>(2);
    end = k.at;
  }
};
constexpr uint64_t kSbrLpWsSurplus = 58; /* the size was written as the parts + 256 + 128: the two pads and the counters take 326 */

struct SbrHqWs {
  int32_t *x, *xr;           /* [n][2 * XAAC_SBR_X_WORDS]: rows of 64 real | 64 imaginary; PS: [n][XAAC_SBR_XR_WORDS], the right channel */
  XaacSynPar *par_l, *par_r; /* [n]: the synthesis parameters (par_r: PS) */
  int32_t *counters;      /* streams deferred to the 64-band rows, next stream of the persistent waves */
  int32_t *defer_list;    /* [n]: the deferred streams */
  uint64_t end;
  SbrHqWs(void *base, size_t n, bool with_ps) {
    Cursor k(base, 256);
    x = k.take<int32_t>(n * 2 * XAAC_SBR_X_WORDS), xr = k.take<int32_t>(with_ps ? n * XAAC_SBR_XR_WORDS : 0);
    par_l = k.take<XaacSynPar>(n), par_r = k.take<XaacSynPar>(with_ps ? n : 0);
    counters = k.align(64).take<int32_t>(2), defer_list = k.take<int32_t>(n);
    end = k.at;
  }
};
constexpr uint64_t kSbrHqWsSurplus = 314; /* ... as the parts + 512 + 128: the two pads and the counters take 326 */

struct SbrEldWs {
  int32_t *x;      /* [n][XAAC_SBR_LD_X_SLOTS][XAAC_SBR_ROW_WORDS_HQ]: the matrices */
  XaacSynPar *par; /* [n]: the synthesis parameters */
  uint64_t end;
  SbrEldWs(void *base, size_t n) {
    Cursor k(base, 256);
    x = k.take<int32_t>(n * XAAC_SBR_LD_X_SLOTS * XAAC_SBR_ROW_WORDS_HQ), par = k.take<XaacSynPar>(n);
    end = k.at;
  }
};
constexpr uint64_t kSbrEldWsSurplus = 257; /* ... as the parts + 512: the pad takes 255 */

struct LimiterWs {
  float *gain;   /* [n][1024]: target gains -> gains of the streams whose smoothing recursion has to run */
  int32_t *flag; /* [n][2]: the hand-over between the limiter's launches */
  uint64_t end;
  LimiterWs(void *base, size_t n) {
    Cursor k(base, 256);
    gain = k.take<float>(n * 1024), flag = k.take<int32_t>(n * 2);
    end = k.at;
  }
};
constexpr uint64_t kLimiterWsSurplus = 1; /* ... as the parts + 256: the pad takes 255 */

/* the two eSBR workspaces: the parts lists of esbr_core_kernel.h (XAAC_ESBR_WS_FLOATS[_4_1] add up the same lists), unaligned */
#define XAAC_WS_MEMBER(name, floats) float *name;
#define XAAC_WS_TAKE(name, floats) name = k.take<float>(n * (floats));
#define XAAC_WS_STRUCT(Name, PARTS) \
  struct Name {                     \
    PARTS(XAAC_WS_MEMBER)           \
    uint64_t end;                   \
    Name(void *base, size_t n) {    \
      Cursor k(base, 1);            \
      PARTS(XAAC_WS_TAKE)           \
      end = k.at;                   \
    }                               \
  }
XAAC_WS_STRUCT(EsbrWs, XAAC_ESBR_WS_PARTS);
XAAC_WS_STRUCT(EsbrWs41, XAAC_ESBR_WS_PARTS_4_1);

XaacEsbrSynParams esbr_syn_params(int n_ch, const float *re, const float *im, int32_t in_stride, xaac_esbr_syn_state *state,
                                  size_t state_stride, float *out, int32_t out_stride, const xaac_sbr_header *only_ps = nullptr) {
  XaacEsbrSynParams p = {};
  p.n_ch = n_ch; p.qmf_re = re; p.qmf_im = im; p.in_stride = in_stride;
  p.state = state; p.state_stride = (int32_t)state_stride;
  p.out = out; p.out_stride = out_stride; p.only_ps = only_ps;
  return p;
}

/* the analysis bank behind the DFT transposer's core launch: it reads the output signal that launch left in the channel's state,
   and a channel that launch refused or skipped (status_in, which the caller sets) is left alone.  rows32: a channel owns 32 rows,
   qmf_stride floats apart, and gets zeros below a_start */
XaacHbeDftParams hbe_dft_chain_ana(int n_ch, xaac_hbe_dft_state *state, const float *coef_re, const float *coef_im, const int32_t *cfg,
                                   float *qmf_re, float *qmf_im, bool rows32, int32_t qmf_stride) {
  XaacHbeDftParams p = {};
  p.n_ch = n_ch; p.no_bins = XAAC_HBE_NO_BINS;
  p.time_in = reinterpret_cast<const float *>(reinterpret_cast<const char *>(state) + offsetof(xaac_hbe_dft_state, output_buf));
  p.in_stride = (int32_t)(sizeof(xaac_hbe_dft_state) / sizeof(float));
  p.coef_re = coef_re; p.coef_im = coef_im; p.cfg = cfg;
  p.state = reinterpret_cast<xaac_hbe_dft_anal_state *>(reinterpret_cast<char *>(state) + offsetof(xaac_hbe_dft_state, anal));
  p.state_stride = (int32_t)sizeof(xaac_hbe_dft_state);
  p.qmf_re = qmf_re; p.qmf_im = qmf_im; p.chain = 1;
  if (rows32) p.qmf_stride = qmf_stride, p.max_rows = 32, p.zero_below = 1;
  return p;
}

/* the map of a mapped call: its (kind, num_channels) is a row of out_map.h's table, a downmix's element list covers the channels
   (-> coef, per slot), and a two-channel pcm16 is stored as 32-bit words */
int32_t out_map_check(const xaac_out_map *m, int num_channels, const int16_t *pcm16, int32_t coef[2][6]) {
  const int oc = xo_out_channels(m->kind, num_channels);
  if (!oc || num_channels > 6) return XAAC_FATAL_BAD_ARG;
  int32_t full[2][8];
  for (int s = 0; s < 8; s++) full[0][s] = full[1][s] = 0;
  if (m->kind == XAAC_OUT_MAP_DOWNMIX_STEREO && xo_resolve(m, num_channels, full)) return XAAC_FATAL_BAD_ARG;
  for (int s = 0; s < 6; s++) coef[0][s] = full[0][s], coef[1][s] = full[1][s];
  if (oc == 2 && ((uintptr_t)pcm16 & 3u)) return XAAC_FATAL_BAD_ARG;
  return XAAC_OK;
}

int32_t mc_pcm_out(xaac_ctx *c, const xaac_mc_pcm_out_batch *b, bool flt, const xaac_out_map *map = nullptr) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_streams < 0 || b->n_ch < 3 || b->n_ch > XAAC_MC_MAX_CH || b->stride < 2048 || (b->stride & 1)) return XAAC_FATAL_BAD_ARG;
  uint32_t seen = 0;
  for (int k = 0; k < b->n_ch; k++) {
    if (b->slot[k] < 0 || b->slot[k] >= b->n_ch) return XAAC_FATAL_BAD_ARG;
    seen |= 1u << b->slot[k];
  }
  if (seen != (1u << b->n_ch) - 1) return XAAC_FATAL_BAD_ARG;
  if (b->n_streams == 0) return XAAC_OK;
  if (!b->planes || !b->pcm) return XAAC_FATAL_NULL_ARG;
  if (((uintptr_t)b->planes & (flt ? 7u : 3u)) || ((uintptr_t)b->pcm & 3u)) return XAAC_FATAL_BAD_ARG;
  XaacMcPcmOutParams p = {};
  p.n_streams = b->n_streams, p.n_ch = b->n_ch, p.stride = b->stride, p.planes = b->planes, p.pcm = b->pcm;
  for (int k = 0; k < b->n_ch; k++) p.slot[k] = b->slot[k];
  int32_t coef[2][6];
  if (map) { /* the downmix to stereo on the way out: the one map this hand-off has kernels for; its channel counts are the table's */
    if (map->kind != XAAC_OUT_MAP_DOWNMIX_STEREO) return XAAC_FATAL_BAD_ARG;
    const int32_t rc = out_map_check(map, b->n_ch, b->pcm, coef);
    if (rc != XAAC_OK) return rc;
  }
  return run(c, [&] {
    if (map) return flt ? xaac_launch_mc_pcm16_from_float_map(&p, coef, c->stream) : xaac_launch_mc_pcm16_from_planes_map(&p, coef, c->stream);
    return flt ? xaac_launch_mc_pcm16_from_float(&p, c->stream) : xaac_launch_mc_pcm16_from_planes(&p, c->stream);
  });
}

/* ds: the 32-channel bank, 1024 samples out per channel */
int32_t esbr_qmf_synthesis(xaac_ctx *c, const xaac_esbr_syn_batch *b, bool ds) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->qmf_re || !b->qmf_im || !b->state || !b->out) return XAAC_FATAL_NULL_ARG;
  const XaacEsbrSynParams p = esbr_syn_params(b->n_ch, b->qmf_re, b->qmf_im, 2048, b->state, sizeof(xaac_esbr_syn_state), b->out, ds ? 1024 : 0);
  return run(c, (b->n_ch + 1) / 2, ds ? XAAC_ESBR_SYN_DS_BLOCK : XAAC_ESBR_SYN_REPORTED_BLOCK, ds ? 0 : XAAC_ESBR_SYN_LDS,
             [&] { return (ds ? xaac_launch_esbr_synthesis_ds : xaac_launch_esbr_synthesis)(&p, c->stream); });
}

/* The two SBR chains (B: xaac_sbr_lp_batch | xaac_sbr_hq_batch; ns: QMF slots of the frames -- 32, or 30: 960 samples in, 1920
   out) around their cores.  w: words of a slot, 64 real (| 64 imaginary).  The matrix' rows and the parameter row: sbr_chain.h. */

/* 0. 30 slots: the side-info check up front -- a refused channel's SBR state, PS state and output are left as they are
      (xaac_sbr_lp960_process_batch, xaac_sbr_hq960_process_batch)
   1. the analysis bank: ns new slots into the rows from XAAC_SBR_X_NEW_ROW on of each channel's matrix; it clears the core's counters on its way */
template <class B>
hipError_t sbr_front(xaac_ctx *c, const B *b, bool hq, int ns, int32_t *x, XaacSynPar *par, int32_t *counters) {
  const int w = hq ? XAAC_SBR_ROW_WORDS_HQ : XAAC_SBR_ROW_WORDS_LP;
  XaacQmfAnaParams pa = {};
  pa.n_ch = b->n_ch; pa.ch_fac = b->in_ch_fac; pa.low_pow = hq ? 0 : 1; pa.usb = 32; pa.slot_stride = w; pa.n_slots = ns;
  pa.state_stride = (int32_t)sizeof(xaac_sbr_state); pa.qmf_ch_stride = XAAC_SBR_X_ROWS * w; pa.pcm = b->pcm_in;
  pa.state = reinterpret_cast<xaac_qmf_ana_state *>(reinterpret_cast<char *>(b->state) + offsetof(xaac_sbr_state, ana_ring));
  pa.qmf = x + XAAC_SBR_X_NEW_ROW * w; pa.zero_words = counters;
  if (hq) pa.frame = b->frame;
  if (ns == 30) {
    XaacSbrCoreParams sc = {};
    sc.n_ch = b->n_ch; sc.header = b->header; sc.frame = b->frame; sc.state = b->state; sc.syn_par = par; sc.qmf_slots = ns;
    const hipError_t e = xaac_launch_sbr_screen(&sc, c->stream);
    if (e != hipSuccess) return e;
    pa.refused = par;
  }
  return xaac_launch_qmf_analysis(&pa, qmf_grid(c, b->n_ch, hq ? 1 : 0), c->stream);
}

/* 2. what both cores take: everything between the banks */
template <class B>
XaacSbrCoreParams sbr_core_params(const xaac_ctx *c, const B *b, int ns, int32_t *x, XaacSynPar *par, int32_t *counters) {
  XaacSbrCoreParams pc = {};
  pc.n_ch = b->n_ch; pc.header = b->header; pc.frame = b->frame; pc.state = b->state; pc.x = x; pc.syn_par = par;
  pc.status = b->status; pc.qmf_slots = ns;
  pc.defer_count = counters; pc.work_counter = counters + 1; pc.num_cu = c->num_cu; pc.counters_zeroed = 1;
  return pc;
}

/* 3. the synthesis bank over the ns rows from XAAC_SBR_X_SLOT0_ROW on (the delayed slots + the first ns - XAAC_SBR_X_OV_SLOTS new
      ones), and the chain's report */
template <class B>
int32_t sbr_back(xaac_ctx *c, const B *b, bool hq, int ns, const int32_t *x, const XaacSynPar *par) {
  const int w = hq ? XAAC_SBR_ROW_WORDS_HQ : XAAC_SBR_ROW_WORDS_LP;
  XaacQmfSynParams ps = {};
  ps.n_ch = b->n_ch; ps.ch_fac = b->out_ch_fac; ps.low_pow = hq ? 0 : 1; ps.split = XAAC_SBR_X_OV_SLOTS; ps.n_slots = ns; ps.down_sample = b->down_sample ? 1 : 0;
  ps.slot_stride = w; ps.state_stride = (int32_t)sizeof(xaac_sbr_state); ps.qmf_ch_stride = XAAC_SBR_X_ROWS * w;
  ps.scale_stride = XAAC_SYN_PAR_WORDS; ps.per_ch_bands = 1;
  ps.qmf = x + XAAC_SBR_X_SLOT0_ROW * w; ps.scale = &par->lb_scale; ps.pcm = b->pcm_out; ps.dbg = XAAC_DBG_BUF(b->status, b->n_ch);
  ps.state = reinterpret_cast<xaac_qmf_syn_state *>(reinterpret_cast<char *>(b->state) + offsetof(xaac_sbr_state, syn_ring));
  const int grid = qmf_grid(c, b->n_ch, hq ? 3 : 2);
  XAAC_TRY(xaac_launch_qmf_synthesis(&ps, grid, c->stream));
  return report(c, grid, XAAC_QMF_BLOCK, hq ? XAAC_QMF_SYN_LDS_HQ : XAAC_QMF_SYN_LDS_LP);
}

int32_t sbr_lp_run(xaac_ctx *c, const xaac_sbr_lp_batch *b, int ns) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  if (ns == 30 && b->down_sample) return XAAC_FATAL_BAD_ARG; /* see xaac_sbr_lp960_process_batch */
  if (bad_ch_fac(b->in_ch_fac) || bad_ch_fac(b->out_ch_fac)) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch % b->in_ch_fac || b->n_ch % b->out_ch_fac) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->pcm_in || !b->header || !b->frame || !b->state || !b->pcm_out || !b->workspace) return XAAC_FATAL_NULL_ARG;
  if (b->workspace_bytes < xaac_sbr_lp_workspace_bytes(b->n_ch)) return XAAC_FATAL_BAD_ARG;
  XAAC_TRY(hipSetDevice(c->device));
  const SbrLpWs w(b->workspace, (size_t)b->n_ch);
  XAAC_TRY(sbr_front(c, b, false, ns, w.x, w.par, w.counters));
  const XaacSbrCoreParams pc = sbr_core_params(c, b, ns, w.x, w.par, w.counters);
  XAAC_TRY(xaac_launch_sbr_core_lp(&pc, c->stream));
  return sbr_back(c, b, false, ns, w.x, w.par);
}

int32_t sbr_hq_run(xaac_ctx *c, const xaac_sbr_hq_batch *b, int ns) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  const bool with_ps = b->ps_frame != nullptr;
  if ((b->ps_frame == nullptr) != (b->ps_state == nullptr)) return XAAC_FATAL_BAD_ARG;
  if (ns == 30 && b->down_sample) return XAAC_FATAL_BAD_ARG; /* see xaac_sbr_hq960_process_batch */
  if (bad_ch_fac(b->in_ch_fac)) return XAAC_FATAL_BAD_ARG;
  if (!with_ps && bad_ch_fac(b->out_ch_fac)) return XAAC_FATAL_BAD_ARG;
  if (with_ps && b->down_sample) return XAAC_FATAL_BAD_ARG; /* see xaac_sbr_hq_batch.down_sample */
  if (b->n_ch % b->in_ch_fac || (!with_ps && b->n_ch % b->out_ch_fac)) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->pcm_in || !b->header || !b->frame || !b->state || !b->pcm_out || !b->workspace) return XAAC_FATAL_NULL_ARG;
  if (b->workspace_bytes < xaac_sbr_hq_workspace_bytes(b->n_ch, with_ps)) return XAAC_FATAL_BAD_ARG;
  XAAC_TRY(hipSetDevice(c->device));
  const SbrHqWs w(b->workspace, (size_t)b->n_ch, with_ps);
  XAAC_TRY(sbr_front(c, b, true, ns, w.x, w.par_l, w.counters));
  XaacSbrCoreParams pc = sbr_core_params(c, b, ns, w.x, w.par_l, w.counters);
  pc.defer_list = w.defer_list;
  pc.narrow_only = b->max_band_hint == XAAC_SBR_NARROW_BANDS ? 1 : 0;
  XAAC_TRY(xaac_launch_sbr_core_hq(&pc, c->stream));
  if (!with_ps) return sbr_back(c, b, true, ns, w.x, w.par_l);
  /* parametric stereo: the ns rows from XAAC_SBR_X_SLOT0_ROW on become the left channel, xr the right one */
  XaacPsParams pp = {};
  pp.n_slots = ns; pp.n = b->n_ch; pp.x = w.x; pp.xr = w.xr; pp.header = b->header; pp.sbr_frame = b->frame; pp.frame = b->ps_frame;
  pp.state = b->ps_state; pp.sbr_state = b->state; pp.par_l = w.par_l; pp.par_r = w.par_r; pp.status = b->status; pp.dbg = XAAC_DBG_BUF(b->status, b->n_ch);
  XAAC_TRY(xaac_launch_ps(&pp, c->stream));
  /* both synthesis banks of a stream in one workgroup, interleaved L,R out */
  XaacQmfSynPairParams pq = {};
  pq.n = b->n_ch; pq.split = XAAC_SBR_X_OV_SLOTS; pq.n_slots = ns;
  pq.qmf[0] = w.x + XAAC_SBR_X_SLOT0_ROW * XAAC_SBR_ROW_WORDS_HQ; pq.qmf_stride[0] = 2 * XAAC_SBR_X_WORDS; pq.scale[0] = w.par_l;
  pq.state[0] = reinterpret_cast<xaac_qmf_syn_state *>(reinterpret_cast<char *>(b->state) + offsetof(xaac_sbr_state, syn_ring));
  pq.state_stride[0] = (int32_t)sizeof(xaac_sbr_state);
  pq.qmf[1] = w.xr; pq.qmf_stride[1] = XAAC_SBR_XR_WORDS; pq.scale[1] = w.par_r;
  pq.state[1] = reinterpret_cast<xaac_qmf_syn_state *>(reinterpret_cast<char *>(b->ps_state) + offsetof(xaac_ps_state, syn_ring_r));
  pq.state_stride[1] = (int32_t)sizeof(xaac_ps_state);
  pq.pcm = b->pcm_out; pq.status = b->status;
  XAAC_TRY(xaac_launch_qmf_synthesis_pair(&pq, c->stream));
  return report(c, b->n_ch, XAAC_QMF_SYN_PAIR_BLOCK, XAAC_QMF_SYN_PAIR_LDS);
}

int32_t limiter_run(xaac_ctx *c, const xaac_limiter_batch *b, const xaac_out_map *map) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_streams < 0 || b->frame_len < 1 || b->frame_len > 1024) return XAAC_FATAL_BAD_ARG;
  if (b->num_channels < 1 || b->num_channels > XAAC_LIM_MAX_CH) return XAAC_FATAL_BAD_ARG;
  if (b->stride < (int64_t)b->frame_len * b->num_channels) return XAAC_FATAL_BAD_ARG;
  if (b->n_streams == 0) return XAAC_OK;
  if (!b->samples || !b->qshift_adj || !b->state || !b->workspace) return XAAC_FATAL_NULL_ARG;
  if (b->workspace_bytes < xaac_peak_limiter_workspace_bytes(b->n_streams)) return XAAC_FATAL_BAD_ARG;
  XAAC_TRY(hipSetDevice(c->device));
  const LimiterWs w(b->workspace, (size_t)b->n_streams);
  XaacLimiterParams p = {};
  p.ws_gain = w.gain; p.ws_flag = w.flag;
  p.n_streams = b->n_streams; p.frame_len = b->frame_len; p.num_channels = b->num_channels; p.planar = b->planar ? 1 : 0;
  p.samples = b->samples; p.stride = b->stride; p.qshift_adj = b->qshift_adj; p.state = b->state; p.pcm16 = b->pcm16; p.status = b->status;
  p.dbg = reinterpret_cast<long long *>(XAAC_DBG_BUF(b->status, b->n_streams)); /* phase timers of -DXL_PROFILE builds */
  if (map) {
    if (!b->pcm16) return XAAC_FATAL_NULL_ARG;
    p.map_kind = map->kind;
    if (map->kind == XAAC_OUT_MAP_NONE) return XAAC_FATAL_BAD_ARG;
    const int32_t rc = out_map_check(map, b->num_channels, b->pcm16, p.map_coef);
    if (rc != XAAC_OK) return rc;
  }
  XAAC_TRY(map ? xaac_launch_limiter_map(&p, c->stream) : xaac_launch_limiter(&p, c->stream));
  return report(c, b->n_streams, XAAC_LIM_BLOCK, XAAC_LIM_FRONT_LDS);
}

}  // namespace

extern "C" {

/* "... build <id>": the sha256 of the library's sources (Makefile: BUILD_ID), so that a counter profile names its library */
const char *xaac_version(void) { return "libxaac_amd 0.4 gfx950 build " XAAC_BUILD_ID; }

int32_t xaac_create(xaac_ctx **out, int32_t device, void *hip_stream) {
  if (!out) return XAAC_FATAL_NULL_ARG;
  *out = nullptr;
  int n = 0;
  if (!hip_ok(hipGetDeviceCount(&n)) || n <= 0) return XAAC_FATAL_NO_DEVICE;
  if (device < 0 || device >= n) return XAAC_FATAL_BAD_ARG;
  if (!hip_ok(hipSetDevice(device))) return XAAC_FATAL_HIP;
  xaac_ctx *c = new (std::nothrow) xaac_ctx();
  if (!c) return XAAC_FATAL_HIP;
  c->device = device;
  c->owns_stream = false;
  c->stream = static_cast<hipStream_t>(hip_stream);
  if (!hip_stream) {
    if (!hip_ok(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking))) {
      delete c;
      return XAAC_FATAL_HIP;
    }
    c->owns_stream = true;
  }
  hipDeviceProp_t prop;
  if (!hip_ok(hipGetDeviceProperties(&prop, device))) {
    if (c->owns_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return XAAC_FATAL_HIP;
  }
  c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->blocks_per_cu = xaac_imdct_blocks_per_cu();
  for (int i = 0; i < 4; i++) c->qmf_blocks_per_cu[i] = xaac_qmf_blocks_per_cu(i);
  c->last_grid = c->last_block = c->last_lds = 0;
  *out = c;
  return XAAC_OK;
}

int32_t xaac_destroy(xaac_ctx *c) {
  if (!c) return XAAC_FATAL_NULL_ARG;
  if (c->owns_stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return XAAC_OK;
}

int32_t xaac_set_stream(xaac_ctx *c, void *hip_stream) {
  if (!c) return XAAC_FATAL_NULL_ARG;
  if (c->owns_stream) (void)hipStreamDestroy(c->stream);
  c->owns_stream = false;
  c->stream = static_cast<hipStream_t>(hip_stream);
  return XAAC_OK;
}

int32_t xaac_warm_up(xaac_ctx *c) {
  if (!c) return XAAC_FATAL_NULL_ARG;
  XAAC_TRY(hipSetDevice(c->device));
  /* one hook per translation unit with kernels, each declared in that unit's *_kernel.h */
  hipError_t (*const hooks[])(void) = {xaac_warm_imdct,     xaac_warm_sbr_qmf,   xaac_warm_sbr_core, xaac_warm_sbr_ps,     xaac_warm_limiter,
                                       xaac_warm_esbr_qmf,  xaac_warm_esbr_core, xaac_warm_esbr_ps,  xaac_warm_hbe,        xaac_warm_usac_imdct,
                                       xaac_warm_imdct960,  xaac_warm_imdct_ld,  xaac_warm_pvc,      xaac_warm_sbr_ld_core,
                                       xaac_warm_aac_tools, xaac_warm_mc_sbr,    xaac_warm_out_map,  xaac_warm_drc};
  for (auto h : hooks) XAAC_TRY(h());
  return XAAC_OK;
}

int32_t xaac_sync(xaac_ctx *c) {
  if (!c) return XAAC_FATAL_NULL_ARG;
  return hip_ok(hipStreamSynchronize(c->stream)) ? XAAC_OK : XAAC_FATAL_HIP;
}

int32_t xaac_imdct_process_batch(xaac_ctx *c, const xaac_imdct_batch *b) {
  if (!c) return XAAC_FATAL_NULL_ARG;
  int32_t rc = check_batch(b);
  if (rc != XAAC_OK) return rc;
  if (b->n_ch == 0) return XAAC_OK;
  XaacImdctParams p = {};
  p.n_ch = b->n_ch; p.ch_fac = b->ch_fac; p.spec = b->spec; p.ics = b->ics; p.overlap = b->overlap; p.state = b->state;
  p.out32 = b->out32; p.pcm16 = b->pcm16; p.qshift_adj = b->qshift_adj; p.pcm_mode = b->pcm_mode; p.status = b->status;
  const int grid = pick_grid(c, b->n_ch);
  return run(c, grid, XAAC_IMDCT_BLOCK, XAAC_IMDCT_LDS_BYTES, [&] { return xaac_launch_imdct(&p, grid, c->stream); });
}

int32_t xaac_aac_tools_process_batch(xaac_ctx *c, const xaac_aac_tools_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n < 0) return XAAC_FATAL_BAD_ARG;
  if (b->n == 0) return XAAC_OK;
  if (!b->spec || !b->side || !b->state) return XAAC_FATAL_NULL_ARG;
  /* the rows are moved 16 bytes at a time */
  if (b->spec_stride < 1024 || (b->spec_stride & 3) || (reinterpret_cast<uintptr_t>(b->spec) & 15)) return XAAC_FATAL_BAD_ARG;
  XaacAacToolsParams p = {};
  p.n = b->n; p.spec_stride = b->spec_stride; p.spec = b->spec; p.side = b->side; p.state = b->state; p.status = b->status;
  const int32_t rc = run(c, [&] { return xaac_launch_aac_tools(&p, c->stream); });
  return rc == XAAC_OK ? report(c, b->n, XAAC_AAC_TOOLS_BLOCK, xaac_aac_tools_lds_bytes()) : rc;
}

int32_t xaac_imdct960_process_batch(xaac_ctx *c, const xaac_imdct_batch *b) {
  if (!c) return XAAC_FATAL_NULL_ARG;
  int32_t rc = check_batch(b);
  if (rc != XAAC_OK) return rc;
  /* the core -> SBR hand-off of a stereo element converts in place, channel after channel (api.c:353-366): channel 1's
     first samples take their low halves from channel 0's PCM.  The 1024-line kernel reproduces that; this one converts
     sample by sample, so the combination is refused rather than answered with different low bits */
  if (b->pcm16 && b->pcm_mode == XAAC_PCM_SBR && b->ch_fac == 2) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  return run(c, (b->n_ch + XAAC_I960_WAVES_PER_WG - 1) / XAAC_I960_WAVES_PER_WG, XAAC_I960_BLOCK, XAAC_I960_LDS,
             [&] { return xaac_launch_imdct960(b, c->stream); });
}

int32_t xaac_imdct_ld_process_batch(xaac_ctx *c, const xaac_imdct_ld_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || bad_ch_fac(b->ch_fac) || b->n_ch % b->ch_fac) return XAAC_FATAL_BAD_ARG;
  if ((b->frame_length != 512 && b->frame_length != 480) || (b->eld != 0 && b->eld != 1)) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->spec || !b->window_shape || !b->overlap || !b->shape_prev || !b->pcm16) return XAAC_FATAL_NULL_ARG;
  return run(c, (b->n_ch + XAAC_LD_WAVES_PER_WG - 1) / XAAC_LD_WAVES_PER_WG, XAAC_LD_BLOCK, XAAC_LD_LDS(b->frame_length, b->eld),
             [&] { return xaac_launch_imdct_ld(b, c->stream); });
}

int32_t xaac_imdct_process_batch_host(xaac_ctx *c, const xaac_imdct_batch *hb) {
  if (!c) return XAAC_FATAL_NULL_ARG;
  int32_t rc = check_batch(hb);
  if (rc != XAAC_OK) return rc;
  const size_t n = (size_t)hb->n_ch;
  if (n == 0) return XAAC_OK;
  XAAC_TRY(hipSetDevice(c->device));
  const size_t sz_spec = n * 1024 * 4, sz_ics = n * sizeof(xaac_ics_info), sz_ovl = n * 512 * 4,
               sz_st = n * sizeof(xaac_ovl_state), sz_o32 = hb->out32 ? n * 1024 * 4 : 0,
               sz_pcm = hb->pcm16 ? n * 1024 * 2 : 0, sz_q = hb->qshift_adj ? n : 0, sz_stat = hb->status ? n * 4 : 0;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t total = up(sz_spec) + up(sz_ics) + up(sz_ovl) + up(sz_st) + up(sz_o32) + up(sz_pcm) + up(sz_q) + up(sz_stat);
  char *d = nullptr;
  XAAC_TRY(hipMalloc(reinterpret_cast<void **>(&d), total));
  char *cur = d;
  auto carve = [&](size_t v) {
    char *r = cur;
    cur += up(v);
    return r;
  };
  xaac_imdct_batch db = *hb;
  char *d_spec = carve(sz_spec), *d_ics = carve(sz_ics), *d_ovl = carve(sz_ovl), *d_st = carve(sz_st);
  char *d_o32 = carve(sz_o32), *d_pcm = carve(sz_pcm), *d_q = carve(sz_q), *d_stat = carve(sz_stat);
  db.spec = reinterpret_cast<const int32_t *>(d_spec);
  db.ics = reinterpret_cast<const xaac_ics_info *>(d_ics);
  db.overlap = reinterpret_cast<int32_t *>(d_ovl);
  db.state = reinterpret_cast<xaac_ovl_state *>(d_st);
  db.out32 = hb->out32 ? reinterpret_cast<int32_t *>(d_o32) : nullptr;
  db.pcm16 = hb->pcm16 ? reinterpret_cast<int16_t *>(d_pcm) : nullptr;
  db.qshift_adj = hb->qshift_adj ? reinterpret_cast<int8_t *>(d_q) : nullptr;
  db.status = hb->status ? reinterpret_cast<int32_t *>(d_stat) : nullptr;
  bool ok = hip_ok(hipMemcpyAsync(d_spec, hb->spec, sz_spec, hipMemcpyHostToDevice, c->stream)) &&
            hip_ok(hipMemcpyAsync(d_ics, hb->ics, sz_ics, hipMemcpyHostToDevice, c->stream)) &&
            hip_ok(hipMemcpyAsync(d_ovl, hb->overlap, sz_ovl, hipMemcpyHostToDevice, c->stream)) &&
            hip_ok(hipMemcpyAsync(d_st, hb->state, sz_st, hipMemcpyHostToDevice, c->stream));
  if (ok) {
    rc = xaac_imdct_process_batch(c, &db);
    ok = (rc == XAAC_OK);
  }
  if (ok) {
    ok = hip_ok(hipMemcpyAsync(hb->overlap, d_ovl, sz_ovl, hipMemcpyDeviceToHost, c->stream)) &&
         hip_ok(hipMemcpyAsync(hb->state, d_st, sz_st, hipMemcpyDeviceToHost, c->stream));
    if (ok && sz_o32) ok = hip_ok(hipMemcpyAsync(hb->out32, d_o32, sz_o32, hipMemcpyDeviceToHost, c->stream));
    if (ok && sz_pcm) ok = hip_ok(hipMemcpyAsync(hb->pcm16, d_pcm, sz_pcm, hipMemcpyDeviceToHost, c->stream));
    if (ok && sz_q) ok = hip_ok(hipMemcpyAsync(hb->qshift_adj, d_q, sz_q, hipMemcpyDeviceToHost, c->stream));
    if (ok && sz_stat) ok = hip_ok(hipMemcpyAsync(hb->status, d_stat, sz_stat, hipMemcpyDeviceToHost, c->stream));
  }
  bool synced = hip_ok(hipStreamSynchronize(c->stream));
  (void)hipFree(d);
  if (rc != XAAC_OK) return rc;
  return (ok && synced) ? XAAC_OK : XAAC_FATAL_HIP;
}

int32_t xaac_qmf_analysis_batch(xaac_ctx *c, const xaac_qmf_ana_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || bad_ch_fac(b->ch_fac) || b->n_ch % b->ch_fac) return XAAC_FATAL_BAD_ARG;
  if (b->slot_stride < (b->low_pow ? 32 : 96) || b->usb < 0 || b->usb > 32) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->pcm || !b->state || !b->qmf) return XAAC_FATAL_NULL_ARG;
  XaacQmfAnaParams p = {};
  p.n_ch = b->n_ch; p.ch_fac = b->ch_fac; p.low_pow = b->low_pow ? 1 : 0; p.usb = b->usb;
  p.slot_stride = b->slot_stride; p.pcm = b->pcm; p.state = b->state; p.qmf = b->qmf;
  p.state_stride = (int32_t)sizeof(xaac_qmf_ana_state); p.qmf_ch_stride = 32 * b->slot_stride;
  const int grid = qmf_grid(c, b->n_ch, p.low_pow ? 0 : 1);
  return run(c, grid, XAAC_QMF_BLOCK, XAAC_QMF_ANA_LDS, [&] { return xaac_launch_qmf_analysis(&p, grid, c->stream); });
}

int32_t xaac_qmf_analysis_eld_batch(xaac_ctx *c, const xaac_qmf_ana_eld_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || (b->n_slots != 16 && b->n_slots != 15) || b->slot_stride < 96 || b->usb < 0 || b->usb > 32) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->pcm || !b->state || !b->qmf) return XAAC_FATAL_NULL_ARG;
  return run(c, (b->n_ch + 3) / 4, XAAC_QMF_ELD_BLOCK, XAAC_QMF_ELD_LDS, [&] { return xaac_launch_qmf_analysis_eld(b, c->stream); });
}

int32_t xaac_qmf_synthesis_eld_batch(xaac_ctx *c, const xaac_qmf_syn_eld_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || (b->n_slots != 16 && b->n_slots != 15) || b->slot_stride < 128) return XAAC_FATAL_BAD_ARG;
  if (b->lsb < 0 || b->usb < b->lsb || b->usb > 64 || b->split < 0 || b->split > b->n_slots) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->qmf || !b->scale || !b->state || !b->pcm) return XAAC_FATAL_NULL_ARG;
  return run(c, (b->n_ch + 3) / 4, XAAC_QMF_ELD_BLOCK, XAAC_QMF_ELD_SYN_LDS, [&] { return xaac_launch_qmf_synthesis_eld(b, c->stream); });
}

int32_t xaac_qmf_synthesis_batch(xaac_ctx *c, const xaac_qmf_syn_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || bad_ch_fac(b->ch_fac) || b->n_ch % b->ch_fac) return XAAC_FATAL_BAD_ARG;
  if (b->slot_stride < (b->low_pow ? 64 : 128)) return XAAC_FATAL_BAD_ARG;
  if (b->lsb < 0 || b->usb < b->lsb || b->usb > 64 || b->split < 0 || b->split > 32) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->qmf || !b->scale || !b->state || !b->pcm) return XAAC_FATAL_NULL_ARG;
  XaacQmfSynParams p = {};
  p.n_ch = b->n_ch; p.ch_fac = b->ch_fac; p.low_pow = b->low_pow ? 1 : 0; p.lsb = b->lsb; p.usb = b->usb;
  p.down_sample = b->down_sample ? 1 : 0;
  p.split = b->split; p.slot_stride = b->slot_stride; p.qmf = b->qmf; p.scale = b->scale; p.state = b->state;
  p.pcm = b->pcm;
  p.state_stride = (int32_t)sizeof(xaac_qmf_syn_state); p.qmf_ch_stride = 32 * b->slot_stride;
  p.scale_stride = XAAC_SYN_PAR_PUBLIC_WORDS; p.per_ch_bands = 0; /* the caller's rows: the first four members of XaacSynPar */
  const int grid = qmf_grid(c, b->n_ch, p.low_pow ? 2 : 3);
  return run(c, grid, XAAC_QMF_BLOCK, p.low_pow ? XAAC_QMF_SYN_LDS_LP : XAAC_QMF_SYN_LDS_HQ,
             [&] { return xaac_launch_qmf_synthesis(&p, grid, c->stream); });
}

uint64_t xaac_esbr_workspace_bytes(int32_t n_ch) { return n_ch > 0 ? EsbrWs(nullptr, (size_t)n_ch).end : 0; }
uint64_t xaac_esbr_workspace_bytes_ratio(int32_t n_ch, int32_t sbr_ratio) {
  if (sbr_ratio != XAAC_ESBR_RATIO_4_1) return xaac_esbr_workspace_bytes(n_ch);
  return n_ch > 0 ? EsbrWs41(nullptr, (size_t)n_ch).end : 0;
}

int32_t xaac_esbr_sbr_process_batch(xaac_ctx *c, const xaac_esbr_sbr_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->core || !b->header || !b->frame || !b->side || !b->state || !b->out || !b->workspace) return XAAC_FATAL_NULL_ARG;
  const bool with_ps = b->ps_frame != nullptr;
  if (with_ps != (b->ps_state != nullptr) || with_ps != (b->out_r != nullptr)) return XAAC_FATAL_BAD_ARG;
  if ((b->pvc_side != nullptr) != (b->pvc_state != nullptr)) return XAAC_FATAL_BAD_ARG;
  if (b->sbr_ratio < XAAC_ESBR_RATIO_2_1 || b->sbr_ratio > XAAC_ESBR_RATIO_4_1) return XAAC_FATAL_BAD_ARG;
  if (b->hbe_dft_state) { /* the DFT transposer: in the QMF one's place, 2:1 only */
    if (b->hbe_state || b->sbr_ratio != XAAC_ESBR_RATIO_2_1) return XAAC_FATAL_BAD_ARG;
    if (!b->hbe_dft_cfg_tab || !b->hbe_dft_coef_re || !b->hbe_dft_coef_im) return XAAC_FATAL_NULL_ARG;
  }
  if (b->workspace_bytes < xaac_esbr_workspace_bytes_ratio(b->n_ch, b->sbr_ratio)) return XAAC_FATAL_BAD_ARG;
  XAAC_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)b->n_ch;
  /* what the two ratios' core launches share; the banks' states are members of xaac_esbr_state / xaac_esbr_ps_state: the bank
     kernels take them at that stride */
  XaacEsbrCoreParams pc = {};
  pc.n_ch = b->n_ch; pc.header = b->header; pc.frame = b->frame; pc.side = b->side; pc.state = b->state; pc.status = b->status;
  pc.pvc_side = b->pvc_side; pc.pvc_state = b->pvc_state;
  XaacEsbrAnaNbParams pn = {};
  pn.n_ch = b->n_ch; pn.core = b->core; pn.core_stride = 1024; pn.state = &b->state->ana; pn.state_stride = (int32_t)sizeof(xaac_esbr_state);
  if (b->sbr_ratio == XAAC_ESBR_RATIO_4_1) { /* 16-channel bank -> 64-slot core -> the synthesis bank in two runs of 32 slots */
    if (with_ps || b->hbe_state) return XAAC_FATAL_BAD_ARG;
    const EsbrWs41 w(b->workspace, n);
    pn.nb = 16; pn.n_slots = 64; pn.out_stride = XAAC_ESBR_Q_ROWS_4_1 * 64;
    pn.qmf_re = w.q_re + XAAC_ESBR_OUT_HIST_ROWS_4_1 * 64; pn.qmf_im = w.q_im + XAAC_ESBR_OUT_HIST_ROWS_4_1 * 64;
    XAAC_TRY(xaac_launch_esbr_analysis_nb(&pn, c->stream));
    pc.out_re = w.out_re; pc.out_im = w.out_im; pc.syn_re = w.syn_re; pc.syn_im = w.syn_im; pc.pvc_out = w.pvc_out;
    pc.usf4 = 1; pc.q_re = w.q_re; pc.q_im = w.q_im;
    XAAC_TRY(xaac_launch_esbr_core(&pc, c->stream));
    for (int half = 0; half < 2; half++) { /* (down-sampled: half the samples of each run, at the same row pitch) */
      const XaacEsbrSynParams ps = esbr_syn_params(b->n_ch, w.syn_re + half * 2048, w.syn_im + half * 2048, 64 * 64, &b->state->syn,
                                                   sizeof(xaac_esbr_state), b->out + half * (b->down_sample ? 1024 : 2048), 4096);
      XAAC_TRY((b->down_sample ? xaac_launch_esbr_synthesis_ds : xaac_launch_esbr_synthesis)(&ps, c->stream));
    }
    return report(c, b->n_ch, XAAC_ESBR_CORE_BLOCK, 0);
  }
  const EsbrWs w(b->workspace, n);
  if (b->sbr_ratio == XAAC_ESBR_RATIO_8_3) { /* 768 samples a frame through the 24-channel bank; bands 24..31 of the rows zeroed */
    pn.nb = 24; pn.n_slots = 32; pn.out_stride = 2048; pn.qmf_re = w.ana_re; pn.qmf_im = w.ana_im;
    XAAC_TRY(xaac_launch_esbr_analysis_nb(&pn, c->stream));
  } else {
    XaacEsbrAnaParams pa = {};
    pa.n_ch = b->n_ch; pa.core = b->core; pa.state = &b->state->ana; pa.qmf_re = w.ana_re; pa.qmf_im = w.ana_im;
    pa.state_stride = (int32_t)sizeof(xaac_esbr_state);
    XAAC_TRY(xaac_launch_esbr_analysis(&pa, c->stream));
  }
  if (b->hbe_dft_state) {
    /* sbr_dec.c:880-892 (-esbr_hq:1): the DFT transposer in the QMF one's place -- its output signal, then its analysis bank into
       rows 8..39 of the ph scratch matrix (the reference's clears beyond row 39 left out, sub-bands below a_start zeroed) */
    XaacHbeDftCoreParams dc = {};
    dc.n_ch = b->n_ch; dc.qmf_re = w.ana_re; dc.qmf_im = w.ana_im; dc.cfg = b->hbe_dft_cfg; dc.cfg_tab = b->hbe_dft_cfg_tab;
    dc.state = b->hbe_dft_state; dc.frame = b->frame; dc.side = b->side;
    XAAC_TRY(xaac_launch_hbe_dft_core(&dc, c->stream));
    XaacHbeDftParams da = hbe_dft_chain_ana(b->n_ch, b->hbe_dft_state, b->hbe_dft_coef_re, b->hbe_dft_coef_im, b->hbe_dft_cfg,
                                            w.ph_re + 8 * 64, w.ph_im + 8 * 64, true, XAAC_ESBR_PH_ROWS * 64);
    da.frame = b->frame;
    da.status_in = reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(b->hbe_dft_state) + offsetof(xaac_hbe_dft_state, last_status));
    da.status_stride = (int32_t)sizeof(xaac_hbe_dft_state);
    XAAC_TRY(xaac_launch_hbe_dft_anal(&da, c->stream));
  } else if (b->hbe_state) {
    /* sbr_dec.c:882-909: the frame's new analysis rows through the channel's harmonic transposer (two launches),
       its 32 output rows into rows 8..39 of the ph scratch matrix; channels without SBR processing are skipped */
    XaacHbeBanksParams hs = {};
    hs.n_ch = b->n_ch; hs.num_columns = XAAC_HBE_NO_BINS; hs.qmf_re = w.ana_re; hs.qmf_im = w.ana_im; hs.state = b->hbe_state;
    hs.apply = 1; hs.frame = b->frame; hs.side = b->side; hs.in_stride = 2048;
    hs.phases = XAAC_HBE_PHASE_SYNTH | XAAC_HBE_PHASE_ANAL; hs.lds_synth_size = b->hbe_max_synth_size;
    XAAC_TRY(xaac_launch_hbe_banks(&hs, c->stream));
    XaacHbePostParams hp = {};
    hp.n_ch = b->n_ch; hp.state = b->hbe_state; hp.pv_re = w.ph_re + 8 * 64; hp.pv_im = w.ph_im + 8 * 64;
    hp.frame = b->frame; hp.side = b->side; hp.pv_stride = XAAC_ESBR_PH_ROWS * 64; hp.zero_outside = 1;
    hp.lds_synth_size = b->hbe_max_synth_size;
    XAAC_TRY(xaac_launch_hbe_post(&hp, c->stream));
  }
  pc.ana_re = w.ana_re; pc.ana_im = w.ana_im; pc.out_re = w.out_re; pc.out_im = w.out_im; pc.syn_re = w.syn_re; pc.syn_im = w.syn_im;
  pc.with_ps = with_ps ? 1 : 0; pc.hbe = b->hbe_state; pc.ph_re = w.ph_re; pc.ph_im = w.ph_im;
  pc.hbe_lds_synth_size = b->hbe_max_synth_size; pc.pvc_out = w.pvc_out; pc.dft = b->hbe_dft_state;
  XAAC_TRY(xaac_launch_esbr_core(&pc, c->stream));
  if (with_ps) {
    XaacEsbrPsParams pp = {};
    pp.n = b->n_ch; pp.header = b->header; pp.frame = b->frame; pp.ps_frame = b->ps_frame; pp.ps_state = b->ps_state;
    pp.l_re = w.syn_re; pp.l_im = w.syn_im; pp.r_re = w.r_re; pp.r_im = w.r_im; pp.status = b->status;
    XAAC_TRY(xaac_launch_esbr_ps(&pp, c->stream));
  }
  const auto syn = b->down_sample ? xaac_launch_esbr_synthesis_ds : xaac_launch_esbr_synthesis;
  const XaacEsbrSynParams ps = esbr_syn_params(b->n_ch, w.syn_re, w.syn_im, XAAC_ESBR_L_ROWS * 64, &b->state->syn, sizeof(xaac_esbr_state),
                                               b->out, 2048);
  XAAC_TRY(syn(&ps, c->stream));
  if (with_ps) {
    const XaacEsbrSynParams pr = esbr_syn_params(b->n_ch, w.r_re, w.r_im, 2048, &b->ps_state->syn_r, sizeof(xaac_esbr_ps_state),
                                                 b->out_r, 2048, b->header);
    XAAC_TRY(syn(&pr, c->stream));
  }
  return report(c, b->n_ch, XAAC_ESBR_CORE_BLOCK, 0);
}

int32_t xaac_esbr_core_from_pcm16_batch(xaac_ctx *c, const xaac_esbr_core_in_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || bad_ch_fac(b->ch_fac) || b->n_ch % b->ch_fac) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->pcm || !b->core) return XAAC_FATAL_NULL_ARG;
  XaacEsbrCoreInParams p = {b->n_ch, b->ch_fac, b->pcm, b->core};
  return run(c, [&] { return xaac_launch_esbr_core_from_pcm16(&p, c->stream); });
}

int32_t xaac_esbr_pcm16_from_float_batch(xaac_ctx *c, const xaac_esbr_pcm_out_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n < 0 || b->stride < 2048) return XAAC_FATAL_BAD_ARG;
  if (b->n == 0) return XAAC_OK;
  if (!b->left || !b->right || !b->pcm) return XAAC_FATAL_NULL_ARG;
  XaacEsbrPcmOutParams p = {};
  p.n = b->n; p.stride = b->stride; p.left = b->left; p.right = b->right; p.pcm = b->pcm;
  return run(c, [&] { return xaac_launch_esbr_pcm16_from_float(&p, c->stream); });
}

/* channel_config 3 .. 6: the element of every bitstream channel (SCE CPE | SCE CPE SCE | SCE CPE CPE | SCE CPE CPE LFE) and the
   slot the reference gives it in the frame's block (api.c:3176-3177: the first pair, the first SCE, the LFE, the second pair, the
   second SCE) */
int32_t xaac_mc_core_from_out32_batch(xaac_ctx *c, const xaac_mc_core_in_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_streams < 0 || b->channel_config < 3 || b->channel_config > 6) return XAAC_FATAL_BAD_ARG;
  if (b->n_streams == 0) return XAAC_OK;
  if (!b->out32 || !b->qshift_adj || !b->core) return XAAC_FATAL_NULL_ARG;
  static const int8_t k_pair_at[4][2] = {{1, -1}, {1, -1}, {1, 3}, {1, 3}};  /* first channel of the pairs, bitstream order */
  static const int8_t k_pair_slot[4][2] = {{0, -1}, {0, -1}, {0, 3}, {0, 4}}; /* ... and their slots */
  const int n_ch = b->channel_config;
  XaacMcCoreInParams p = {};
  p.n_streams = b->n_streams, p.n_ch = n_ch, p.out32 = b->out32, p.qshift_adj = b->qshift_adj, p.core = b->core;
  for (int k = 0; k < 2; k++) {
    const int at = k_pair_at[n_ch - 3][k], slot = k_pair_slot[n_ch - 3][k];
    if (at < 0) continue;
    p.q_src[at + 1] = 1; /* (every other channel is its element's first: q_src 0) */
    p.mix[at + 1] = n_ch == slot + 2 ? 1 : (n_ch == slot + 3 ? 2 : 0);
  }
  return run(c, [&] { return xaac_launch_mc_core_from_out32(&p, c->stream); });
}

int32_t xaac_mc_pcm16_from_float_map_batch(xaac_ctx *c, const xaac_mc_pcm_out_map_batch *b) {
  return b ? mc_pcm_out(c, &b->out, true, &b->map) : XAAC_FATAL_NULL_ARG;
}
int32_t xaac_mc_pcm16_from_planes_map_batch(xaac_ctx *c, const xaac_mc_pcm_out_map_batch *b) {
  return b ? mc_pcm_out(c, &b->out, false, &b->map) : XAAC_FATAL_NULL_ARG;
}
int32_t xaac_mc_pcm16_from_float_batch(xaac_ctx *c, const xaac_mc_pcm_out_batch *b) { return mc_pcm_out(c, b, true); }
int32_t xaac_mc_pcm16_from_planes_batch(xaac_ctx *c, const xaac_mc_pcm_out_batch *b) { return mc_pcm_out(c, b, false); }

int32_t xaac_sbr_state_handover(xaac_ctx *c, const xaac_sbr_handover_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n < 0 || (b->mode != XAAC_HANDOVER_PS_START && b->mode != XAAC_HANDOVER_STEREO_START)) return XAAC_FATAL_BAD_ARG;
  if (b->n == 0) return XAAC_OK;
  if (!b->src || !b->dst || !b->state || (b->mode == XAAC_HANDOVER_PS_START && !b->ps_state)) return XAAC_FATAL_NULL_ARG;
  return run(c, [&] { return xaac_launch_sbr_handover(b, c->stream); });
}

int32_t xaac_sbr_state_apply_side_batch(xaac_ctx *c, const xaac_sbr_apply_side_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_streams < 0 || bad_ch_fac(b->ch_fac)) return XAAC_FATAL_BAD_ARG;
  if (b->n_streams == 0) return XAAC_OK;
  if (!b->header || !b->flags || !b->state) return XAAC_FATAL_NULL_ARG;
  return run(c, [&] { return xaac_launch_sbr_apply_side(b, c->stream); });
}

int32_t xaac_usac_imdct_process_batch(xaac_ctx *c, const xaac_usac_imdct_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (b->ccfl != 0 && b->ccfl != 1024 && b->ccfl != 768) return XAAC_FATAL_BAD_ARG;
  if (!b->coef || !b->ics || !b->overlap || !b->shape_prev) return XAAC_FATAL_NULL_ARG;
  XAAC_TRY(hipSetDevice(c->device));
  XaacUsacImdctParams p = {};
  p.n_ch = b->n_ch; p.ccfl = b->ccfl ? b->ccfl : 1024; p.coef = b->coef; p.ics = b->ics; p.overlap = b->overlap;
  p.shape_prev = b->shape_prev; p.out32 = b->out32; p.time = b->time; p.status = b->status; p.lpd_flags = b->lpd_flags; p.fac = b->fac;
  if (b->fac_in) { /* the FAC signals of this batch's LPD -> FD transitions, made on the device first */
    if (!b->fac_work || !b->lpd_flags) return XAAC_FATAL_NULL_ARG;
    XaacUsacFacParams pf = {};
    pf.n_ch = b->n_ch; pf.ccfl = p.ccfl; pf.ics = b->ics; pf.lpd_flags = b->lpd_flags; pf.in = b->fac_in; pf.out = b->fac_work;
    XAAC_TRY(xaac_launch_usac_fac(&pf, c->stream));
    p.fac = b->fac_work;
  }
  XAAC_TRY(xaac_launch_usac_imdct(&p, c->stream));
  return report(c, (b->n_ch + XAAC_USAC_WAVES_PER_WG - 1) / XAAC_USAC_WAVES_PER_WG, XAAC_USAC_BLOCK, XAAC_USAC_LDS);
}

int32_t xaac_esbr_qmf_analysis_batch(xaac_ctx *c, const xaac_esbr_ana_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->core || !b->state || !b->qmf_re || !b->qmf_im) return XAAC_FATAL_NULL_ARG;
  XaacEsbrAnaParams p = {};
  p.n_ch = b->n_ch; p.core = b->core; p.state = b->state; p.qmf_re = b->qmf_re; p.qmf_im = b->qmf_im;
  p.state_stride = (int32_t)sizeof(xaac_esbr_ana_state);
  return run(c, (b->n_ch + 1) / 2, XAAC_ESBR_ANA_BLOCK, XAAC_ESBR_ANA_LDS, [&] { return xaac_launch_esbr_analysis(&p, c->stream); });
}

int32_t xaac_esbr_qmf_analysis_nb_batch(xaac_ctx *c, const xaac_esbr_ana_nb_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || (b->n_bands != 24 && b->n_bands != 16) || b->n_slots < 0 || b->n_slots > (b->n_bands == 24 ? 32 : 64) ||
      b->n_bands * b->n_slots > 1024 ||
      b->core_stride < b->n_bands * b->n_slots)
    return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->core || !b->state || !b->qmf_re || !b->qmf_im) return XAAC_FATAL_NULL_ARG;
  XaacEsbrAnaNbParams p = {};
  p.n_ch = b->n_ch; p.nb = b->n_bands; p.n_slots = b->n_slots; p.core = b->core; p.core_stride = b->core_stride;
  p.state = b->state; p.state_stride = (int32_t)sizeof(xaac_esbr_ana_state);
  p.qmf_re = b->qmf_re; p.qmf_im = b->qmf_im; p.out_stride = b->n_slots * 64;
  return run(c, b->n_ch, XAAC_ESBR_ANA_BLOCK, 0, [&] { return xaac_launch_esbr_analysis_nb(&p, c->stream); });
}

int32_t xaac_esbr_qmf_synthesis_batch(xaac_ctx *c, const xaac_esbr_syn_batch *b) { return esbr_qmf_synthesis(c, b, false); }
int32_t xaac_esbr_qmf_synthesis_ds_batch(xaac_ctx *c, const xaac_esbr_syn_batch *b) { return esbr_qmf_synthesis(c, b, true); }

int32_t xaac_hbe_real_synth_batch(xaac_ctx *c, const xaac_hbe_synth_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || b->num_columns < 0 || b->num_columns > XAAC_HBE_NO_BINS) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0 || b->num_columns == 0) return XAAC_OK;
  if (!b->qmf_re || !b->qmf_im || !b->state) return XAAC_FATAL_NULL_ARG;
  XaacHbeBanksParams p = {};
  p.n_ch = b->n_ch; p.num_columns = b->num_columns; p.qmf_re = b->qmf_re; p.qmf_im = b->qmf_im; p.state = b->state; p.status = b->status;
  p.in_stride = b->num_columns * 64; p.phases = XAAC_HBE_PHASE_SYNTH;
  return run(c, b->n_ch, XAAC_HBE_BANKS_THREADS, XAAC_HBE_BANKS_LDS, [&] { return xaac_launch_hbe_banks(&p, c->stream); });
}

int32_t xaac_hbe_cplx_anal_batch(xaac_ctx *c, const xaac_hbe_anal_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->state) return XAAC_FATAL_NULL_ARG;
  XaacHbeBanksParams p = {};
  p.n_ch = b->n_ch; p.state = b->state; p.status = b->status; p.phases = XAAC_HBE_PHASE_ANAL;
  return run(c, b->n_ch, XAAC_HBE_BANKS_THREADS, XAAC_HBE_BANKS_LDS, [&] { return xaac_launch_hbe_banks(&p, c->stream); });
}

int32_t xaac_hbe_dft_anal_batch_run(xaac_ctx *c, const xaac_hbe_dft_anal_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || b->no_bins < 1 || b->no_bins > XAAC_HBE_NO_BINS || b->in_stride < 1) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->time_in || !b->coef_re || !b->coef_im || !b->state || !b->qmf_re || !b->qmf_im) return XAAC_FATAL_NULL_ARG;
  XaacHbeDftParams p = {};
  p.n_ch = b->n_ch; p.no_bins = b->no_bins; p.time_in = b->time_in; p.in_stride = b->in_stride;
  p.coef_re = b->coef_re; p.coef_im = b->coef_im; p.cfg = b->cfg; p.state = b->state;
  p.qmf_re = b->qmf_re; p.qmf_im = b->qmf_im; p.status = b->status;
  return run(c, b->n_ch, XAAC_HBE_DFT_THREADS, XAAC_HBE_DFT_LDS, [&] { return xaac_launch_hbe_dft_anal(&p, c->stream); });
}

int32_t xaac_hbe_dft_apply_batch_run(xaac_ctx *c, const xaac_hbe_dft_apply_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->qmf_re || !b->qmf_im || !b->cfg_tab || !b->coef_re || !b->coef_im || !b->state || !b->pv_re || !b->pv_im || !b->status)
    return XAAC_FATAL_NULL_ARG; /* (status is how the second launch learns which channels the first one refused) */
  XaacHbeDftCoreParams pc = {};
  pc.n_ch = b->n_ch; pc.qmf_re = b->qmf_re; pc.qmf_im = b->qmf_im; pc.pitch = b->pitch_in_bins; pc.oversampling = b->oversampling;
  pc.cfg = b->cfg; pc.cfg_tab = b->cfg_tab; pc.state = b->state; pc.status = b->status;
  XaacHbeDftParams pa = hbe_dft_chain_ana(b->n_ch, b->state, b->coef_re, b->coef_im, b->cfg, b->pv_re, b->pv_im, b->rows32 != 0, 32 * 64);
  pa.status = b->status; pa.status_in = b->status; pa.status_stride = 4;
  return run(c, b->n_ch, XAAC_HBE_DFT_CORE_THREADS, XAAC_HBE_DFT_CORE_LDS, [&] {
    const hipError_t e = xaac_launch_hbe_dft_core(&pc, c->stream);
    return e == hipSuccess ? xaac_launch_hbe_dft_anal(&pa, c->stream) : e;
  });
}

int32_t xaac_pvc_process_batch(xaac_ctx *c, const xaac_pvc_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || b->qmf_stride < 32 * 64) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->frame || !b->qmf_re || !b->qmf_im || !b->state || !b->out) return XAAC_FATAL_NULL_ARG;
  XaacPvcParams p = {};
  p.n_ch = b->n_ch; p.frame = b->frame; p.qmf_re = b->qmf_re; p.qmf_im = b->qmf_im; p.qmf_stride = b->qmf_stride;
  p.state = b->state; p.out = b->out; p.status = b->status;
  return run(c, b->n_ch, XAAC_PVC_BLOCK, XAAC_PVC_LDS, [&] { return xaac_launch_pvc(&p, c->stream); });
}

int32_t xaac_hbe_apply_batch(xaac_ctx *c, const xaac_hbe_apply_batch_desc *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->qmf_re || !b->qmf_im || !b->state || !b->pv_re || !b->pv_im) return XAAC_FATAL_NULL_ARG;
  /* two launches on the context's stream: the two polyphase banks (with the frame's shift / re-initialisation and the
     parameter check that sets status), then products + output rows */
  XaacHbeBanksParams ps = {};
  ps.n_ch = b->n_ch; ps.num_columns = XAAC_HBE_NO_BINS; ps.qmf_re = b->qmf_re; ps.qmf_im = b->qmf_im; ps.state = b->state;
  ps.status = b->status; ps.pitch = b->pitch_in_bins; ps.apply = 1; ps.in_stride = 2048;
  ps.phases = XAAC_HBE_PHASE_SYNTH | XAAC_HBE_PHASE_ANAL; ps.lds_synth_size = b->max_synth_size;
  XaacHbePostParams pp = {};
  pp.n_ch = b->n_ch; pp.state = b->state; pp.pitch = b->pitch_in_bins; pp.pv_re = b->pv_re; pp.pv_im = b->pv_im; pp.pv_stride = 2048;
  pp.lds_synth_size = b->max_synth_size;
  return run(c, b->n_ch, XAAC_HBE_POST_THREADS, XAAC_HBE_POST_LDS, [&] {
    const hipError_t e = xaac_launch_hbe_banks(&ps, c->stream);
    return e == hipSuccess ? xaac_launch_hbe_post(&pp, c->stream) : e;
  });
}

uint64_t xaac_sbr_lp_workspace_bytes(int32_t n_ch) { return n_ch < 0 ? 0 : SbrLpWs(nullptr, (size_t)n_ch).end + kSbrLpWsSurplus; }
uint64_t xaac_sbr_hq_workspace_bytes(int32_t n_ch, int32_t with_ps) {
  return n_ch < 0 ? 0 : SbrHqWs(nullptr, (size_t)n_ch, with_ps != 0).end + kSbrHqWsSurplus;
}

int32_t xaac_sbr_lp_process_batch(xaac_ctx *c, const xaac_sbr_lp_batch *b) { return sbr_lp_run(c, b, 32); }
int32_t xaac_sbr_lp960_process_batch(xaac_ctx *c, const xaac_sbr_lp_batch *b) { return sbr_lp_run(c, b, 30); }
int32_t xaac_sbr_hq_process_batch(xaac_ctx *c, const xaac_sbr_hq_batch *b) { return sbr_hq_run(c, b, 32); }
int32_t xaac_sbr_hq960_process_batch(xaac_ctx *c, const xaac_sbr_hq_batch *b) { return sbr_hq_run(c, b, 30); }

/* the low-delay SBR chain of AAC-ELD channels: LD analysis bank -> core (sbr_ld_core_kernel.hip) -> LD synthesis bank */
uint64_t xaac_sbr_eld_workspace_bytes(int32_t n_ch) { return n_ch > 0 ? SbrEldWs(nullptr, (size_t)n_ch).end + kSbrEldWsSurplus : 0; }
int32_t xaac_sbr_eld_process_batch(xaac_ctx *c, const xaac_sbr_eld_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_ch < 0 || (b->n_slots != 16 && b->n_slots != 15)) return XAAC_FATAL_BAD_ARG;
  if (bad_ch_fac(b->in_ch_fac) || bad_ch_fac(b->out_ch_fac)) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch % b->in_ch_fac || b->n_ch % b->out_ch_fac) return XAAC_FATAL_BAD_ARG;
  if (b->n_ch == 0) return XAAC_OK;
  if (!b->pcm_in || !b->header || !b->frame || !b->state || !b->pcm_out || !b->workspace) return XAAC_FATAL_NULL_ARG;
  if (b->workspace_bytes < xaac_sbr_eld_workspace_bytes(b->n_ch)) return XAAC_FATAL_BAD_ARG;
  XAAC_TRY(hipSetDevice(c->device));
  const SbrEldWs w(b->workspace, (size_t)b->n_ch);
  char *st = reinterpret_cast<char *>(b->state);
  XaacQmfEldChain cn = {};
  cn.state_stride = (int32_t)sizeof(xaac_sbr_eld_state);
  /* 1. analysis: n_slots slots of 32 real | 32 imaginary bands into each channel's matrix */
  xaac_qmf_ana_eld_batch a = {};
  a.n_ch = b->n_ch; a.n_slots = b->n_slots; a.usb = 32; a.slot_stride = XAAC_SBR_ROW_WORDS_HQ; a.pcm = b->pcm_in;
  a.state = reinterpret_cast<xaac_qmf_ana_eld_state *>(st + offsetof(xaac_sbr_eld_state, ana));
  a.qmf = w.x; a.status = nullptr;
  cn.pcm_ch_fac = b->in_ch_fac; cn.frame = b->frame;
  cn.codec_usb = reinterpret_cast<const int16_t *>(st + offsetof(xaac_sbr_eld_state, codec_usb));
  XAAC_TRY(xaac_launch_qmf_analysis_eld_chain(&a, &cn, c->stream));
  /* 2. between the banks */
  XaacSbrLdCoreParams pc = {};
  pc.n_ch = b->n_ch; pc.n_slots = b->n_slots; pc.header = b->header; pc.frame = b->frame; pc.state = b->state;
  pc.x = w.x; pc.syn_par = w.par; pc.status = b->status;
  XAAC_TRY(xaac_launch_sbr_ld_core(&pc, c->stream));
  /* 3. synthesis */
  xaac_qmf_syn_eld_batch sy = {};
  sy.n_ch = b->n_ch; sy.n_slots = b->n_slots; sy.split = 0; sy.slot_stride = XAAC_SBR_ROW_WORDS_HQ; sy.qmf = w.x; sy.scale = &w.par->lb_scale;
  sy.state = reinterpret_cast<xaac_qmf_syn_eld_state *>(st + offsetof(xaac_sbr_eld_state, syn));
  sy.pcm = b->pcm_out; sy.status = nullptr; sy.qmf_scaled = b->qmf_handed_on;
  cn.pcm_ch_fac = b->out_ch_fac; cn.syn_par = w.par;
  XAAC_TRY(xaac_launch_qmf_synthesis_eld_chain(&sy, &cn, c->stream));
  return report(c, b->n_ch, XAAC_SBR_LD_CORE_BLOCK, 0);
}

/* ixheaacd_peak_limiter_init, decoder/ixheaacd_peak_limiter.c:46-77 (host side: a stream's state is made once) */
int32_t xaac_peak_limiter_init(xaac_limiter_state *s, uint32_t num_channels, uint32_t sample_rate) {
  if (!s) return XAAC_FATAL_NULL_ARG;
  const uint32_t attack = (uint32_t)(5.0f * sample_rate / 1000);
  if (attack < 1 || attack > XAAC_LIM_MAX_ATTACK || num_channels < 1 || num_channels > XAAC_LIM_MAX_CH)
    return XAAC_FATAL_BAD_ARG;
  std::memset(s, 0, sizeof(*s));
  s->attack_time_samples = attack;
  s->attack_constant = (float)std::pow(0.1, 1.0 / (attack + 1));
  s->release_constant = (float)std::pow(0.1, 1.0 / (50.0f * sample_rate / 1000 + 1));
  s->num_channels = num_channels;
  s->min_gain = 1.0f;
  s->limiter_on = 1;
  s->pre_smoothed_gain = 1.0f;
  s->gain_modified = 1.0f;
  return (int32_t)attack;
}

uint64_t xaac_peak_limiter_workspace_bytes(int32_t n_streams) {
  return n_streams < 0 ? 0 : LimiterWs(nullptr, (size_t)n_streams).end + kLimiterWsSurplus;
}

int32_t xaac_peak_limiter_process_batch(xaac_ctx *c, const xaac_limiter_batch *b) { return limiter_run(c, b, nullptr); }

int32_t xaac_peak_limiter_process_map_batch(xaac_ctx *c, const xaac_limiter_map_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  return limiter_run(c, &b->lim, &b->map);
}

/* ixheaacd_scale_adjust + round16 (+ the map): the limiter-off hand-off */
int32_t xaac_pcm16_scale_adjust_map_batch(xaac_ctx *c, const xaac_scale_adjust_map_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n_streams < 0 || b->frame_len < 1 || b->frame_len > 1024) return XAAC_FATAL_BAD_ARG;
  if (b->num_channels < 1 || b->num_channels > 6) return XAAC_FATAL_BAD_ARG;
  if (b->stride < (int64_t)b->frame_len * b->num_channels) return XAAC_FATAL_BAD_ARG;
  XaacScaleAdjustParams p = {};
  const int oc = xo_out_channels(b->map.kind, b->num_channels);
  if (!oc) return XAAC_FATAL_BAD_ARG;
  if (b->n_streams == 0) return XAAC_OK;
  if (!b->samples || !b->qshift_adj || !b->pcm16) return XAAC_FATAL_NULL_ARG;
  if (b->map.kind == XAAC_OUT_MAP_NONE) {
    if ((b->num_channels & 1) == 0 && ((uintptr_t)b->pcm16 & 3u)) return XAAC_FATAL_BAD_ARG;
  } else {
    const int32_t rc = out_map_check(&b->map, b->num_channels, b->pcm16, p.map_coef);
    if (rc != XAAC_OK) return rc;
  }
  p.n_streams = b->n_streams; p.frame_len = b->frame_len; p.num_channels = b->num_channels; p.planar = b->planar ? 1 : 0;
  p.samples = b->samples; p.stride = b->stride; p.qshift_adj = b->qshift_adj; p.pcm16 = b->pcm16; p.map_kind = b->map.kind;
  return run(c, (int32_t)xaac_scale_adjust_grid(b->n_streams, b->frame_len), XAAC_SCALE_ADJUST_BLOCK, 0,
             [&] { return xaac_launch_scale_adjust_map(&p, c->stream); });
}

/* ixheaacd_drc_apply's spectral branch on n channel-frame rows; what a row's side info has to satisfy is the kernel's (drc.h) */
int32_t xaac_drc_apply_batch(xaac_ctx *c, const xaac_drc_batch *b) {
  if (!c || !b) return XAAC_FATAL_NULL_ARG;
  if (b->n < 0 || b->spec_stride < 1024 || (b->spec_stride & 3)) return XAAC_FATAL_BAD_ARG;
  if (b->n == 0) return XAAC_OK;
  if (!b->spec || !b->side) return XAAC_FATAL_NULL_ARG;
  if ((uintptr_t)b->spec & 15u) return XAAC_FATAL_BAD_ARG;
  XaacDrcParams p = {};
  p.n = b->n; p.spec_stride = b->spec_stride; p.spec = b->spec; p.side = b->side; p.status = b->status;
  return run(c, xaac_drc_grid(b->n), XAAC_DRC_BLOCK, XAAC_DRC_LDS_BYTES, [&] { return xaac_launch_drc(&p, c->stream); });
}

int32_t xaac_last_launch(xaac_ctx *c, int32_t *grid, int32_t *block, int32_t *lds_bytes) {
  if (!c) return XAAC_FATAL_NULL_ARG;
  if (grid) *grid = c->last_grid;
  if (block) *block = c->last_block;
  if (lds_bytes) *lds_bytes = c->last_lds;
  return XAAC_OK;
}

}  // extern "C"
