/* sbr_chain.h -- what the launches of an SBR chain hand to each other (internal): the synthesis parameter row, the QMF
   matrix between the banks and the core, and the core kernels' LDS mirror of a channel's state.  Each is stated here once;
   the kernels and xaac_abi.cpp index by these names. */
#ifndef XAAC_SBR_CHAIN_H
#define XAAC_SBR_CHAIN_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/xaac_sbr.h"

#define XAAC_CHAIN_HD __host__ __device__ __forceinline__

/* ---- the synthesis parameter row: one per channel, in the chains' workspaces ---------------------------------------------
   The core kernel fills it for the synthesis bank behind it; the screen in front of the 30-slot chains, the parametric-stereo
   kernel and the banks read and rewrite single members.  The first four members are the row the generic banks' public entry
   points take (xaac_qmf_syn_batch.scale: scale_stride = XAAC_SYN_PAR_PUBLIC_WORDS). */
typedef struct XaacSynPar {
  int16_t lb_scale, ov_lb_scale, hb_scale, st_syn_scale; /* the scales of the matrix' regions and of the bank's ring */
  int16_t lsb, usb;                                      /* the synthesis bank's band limits */
  int16_t skip;    /* != 0: the bank leaves this channel alone (state and output samples as they are) */
  int16_t refused; /* != 0: refused by the screen in front of the banks (xaac_launch_sbr_screen; 30-slot chains only) */
} XaacSynPar;
/* a member's place in the row, in int16 words: the lane that holds it after a lane-indexed load, its half of a packed word */
#define XAAC_SYN_PAR_AT(member) ((int)(offsetof(XaacSynPar, member) / sizeof(int16_t)))
#define XAAC_SYN_PAR_WORDS ((int)(sizeof(XaacSynPar) / sizeof(int16_t)))
#define XAAC_SYN_PAR_PUBLIC_WORDS XAAC_SYN_PAR_AT(lsb)
static_assert(sizeof(XaacSynPar) == 16, "one 16-byte load takes a row");
static_assert(XAAC_SYN_PAR_AT(lb_scale) == 0 && XAAC_SYN_PAR_AT(ov_lb_scale) == 1 && XAAC_SYN_PAR_AT(hb_scale) == 2 &&
                  XAAC_SYN_PAR_AT(st_syn_scale) == 3,
              "the public four-word row");
static_assert(XAAC_SYN_PAR_AT(lsb) == 4 && XAAC_SYN_PAR_AT(usb) == 5 && XAAC_SYN_PAR_AT(skip) == 6 && XAAC_SYN_PAR_AT(refused) == 7,
              "the chains' own half");

/* Row i of `rows` (a pointer of the rows' own type), reached as int16 words from the array's start.  The analysis bank and the
   parametric-stereo kernel address their rows this way: it is the arithmetic their register allocation was tuned with (as
   `rows[i].member` the compiler shares the scaled index between the arrays, and both kernels come out with other register
   counts). */
#define XAAC_SYN_PAR_ROW(rows, i) ((decltype(rows))((const int16_t *)(rows) + XAAC_SYN_PAR_WORDS * (size_t)(i)))

/* what a core leaves for the synthesis bank; State: anything with XAAC_SBR_STATE_TAIL_FIELDS and the bank limits */
template <class State>
XAAC_CHAIN_HD void xaac_syn_par_fill(XaacSynPar *par, const State &st) {
  par->lb_scale = st.lb_scale;
  par->ov_lb_scale = st.ov_lb_scale;
  par->hb_scale = st.hb_scale;
  par->st_syn_scale = st.st_syn_scale;
  par->lsb = st.syn_lsb;
  par->usb = st.syn_usb;
}

/* member `OFF` bytes into a row that lies in four 32-bit words (the pair kernel's one 16-byte load) */
template <int OFF>
XAAC_CHAIN_HD int xaac_syn_par_of_words(const int (&w)[4]) {
  static_assert(OFF % 2 == 0 && OFF / 4 < 4, "a half of one of the four words");
  return OFF % 4 ? w[OFF / 4] >> 16 : (int)(int16_t)w[OFF / 4];
}
#define XAAC_SYN_PAR_OF_WORDS(w, member) xaac_syn_par_of_words<offsetof(XaacSynPar, member)>(w)

/* ---- the QMF matrix between the launches: one per channel, rows of 64 real (low power) or 64 real | 64 imaginary words ----- */
#define XAAC_SBR_X_LPC_ROWS 2                                               /* the LPC history in front of slot 0 */
#define XAAC_SBR_X_OV_SLOTS 6                                               /* slots carried from the frame before (op_delay) */
#define XAAC_SBR_X_SLOT0_ROW XAAC_SBR_X_LPC_ROWS                            /* row of slot 0: the synthesis bank starts here */
#define XAAC_SBR_X_NEW_ROW (XAAC_SBR_X_SLOT0_ROW + XAAC_SBR_X_OV_SLOTS)     /* row of the first slot the analysis bank writes */
#define XAAC_SBR_X_ROWS 40                                                  /* ... + 32 new slots (a 30-slot frame uses 38) */
#define XAAC_SBR_X_WORDS (XAAC_SBR_X_ROWS * 64)                             /* int32 words of a low-power matrix; HQ: twice */
#define XAAC_SBR_ROW_WORDS_LP 64
#define XAAC_SBR_ROW_WORDS_HQ 128
#define XAAC_SBR_XR_WORDS (32 * XAAC_SBR_ROW_WORDS_HQ) /* parametric stereo: the right channel's slots 0..31, nothing in front */
static_assert(XAAC_SBR_X_ROWS == XAAC_SBR_X_NEW_ROW + 32, "history, overlap, one frame");
/* low-delay SBR: no overlap slots.  The banks see the frame's slots alone ([n_slots][128], at most 16); the core's copy in
   LDS has the LPC history in front */
#define XAAC_SBR_LD_X_SLOTS 16
#define XAAC_SBR_LD_X_ROWS (XAAC_SBR_X_LPC_ROWS + XAAC_SBR_LD_X_SLOTS)

/* ---- the core kernels' LDS mirror of a channel's state: the four bank-limit shorts + the struct tail ----------------------- */
struct XsLdsState {
  int16_t codec_usb, syn_lsb, syn_usb, pad2_;
  XAAC_SBR_STATE_TAIL_FIELDS
};
/* where the two parts lie in State (xaac_sbr_state, xaac_sbr_eld_state), for copies by 32-bit words */
template <class State>
struct XsStateMirror {
  static constexpr int kHeadOff = offsetof(State, codec_usb);
  static constexpr int kTailOff = offsetof(State, lpc_real);
  static constexpr int kTailWords = (sizeof(State) - kTailOff) / 4;
  static_assert(kHeadOff % 4 == 0 && kTailOff % 4 == 0 && sizeof(State) % 4 == 0, "word copies");
  static_assert(offsetof(XsLdsState, lpc_real) == 8 && sizeof(XsLdsState) == 8 + kTailWords * 4, "mirror layout");
};
/* of the frame side info only the head lives in LDS: the envelope scale factors (896 B) are read once per envelope
   and stay in global memory, the noise floor gets its own twenty bytes (sbr_core.h hands both in beside `f`) */
constexpr int kFrameHeadBytes = offsetof(xaac_sbr_frame, int_env_sf_arr);
static_assert(sizeof(xaac_sbr_header) % 4 == 0 && sizeof(xaac_sbr_frame) % 4 == 0, "word copies");
static_assert(kFrameHeadBytes % 4 == 0 && offsetof(xaac_sbr_frame, int_noise_floor) % 4 == 0, "word copies");
static_assert(offsetof(xaac_sbr_frame, int_noise_floor) == kFrameHeadBytes + sizeof(((xaac_sbr_frame *)0)->int_env_sf_arr),
              "nothing but the two arrays behind the head");

#endif
