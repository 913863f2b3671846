// Routing of the ConvLSTM sequence kernels (k_lstm.hip): one table of channel counts (LSTM_SEQ_TABLE), one router (lstm_seq_route).
// leod_convlstm_seq_fwd / _bwd, the mode / gates16 / pack queries and leod_convlstm_seq_route all go through it; the launch switches of
// k_lstm.hip instantiate a kernel per table row and nothing else.
#pragma once
#include "common.hpp"

enum : int { LE_FWD = 0, LE_BWD = 1 };
// the flags of leod_convlstm_seq_route: what the entry points are given
enum : int { LF_PROJECTION = 1, LF_GATES16 = 2, LF_PACK = 4 };        // xin is the hoisted projection | gates16 | a wpack
// Route codes, family + C (include/leod_hip.h lists them for callers)
enum : int { LR_FUSED = 1000, LR_HOISTED = 2000, LR_STREAMED = 3000, LR_RESIDENT_BWD = 4000 };

// X(C, family in precision mode f32, family in the 16-bit modes): the forward family of a channel count -- 1 fused [x | h] contraction,
// 2 hoisted x projection (xin = gx), both with the wave's weight slice resident in registers; 3 hoisted, weights streamed from the packed
// 16-bit copy (leod_convlstm_seq_pack); 0 no sequence kernel.  The backward is streamed where the forward is, register-resident elsewhere.
// Resident B fragments per lane: 4 gates x K / 16 chunks x (2 | 4) dwords = K / 2 (16-bit) | K (fp32) registers, K = 2C fused, C hoisted
// and backward.  Beyond ~100 resident registers the kernels spill: fused up to 96, hoisted and backward up to 128 below C = 192.
#define LSTM_SEQ_TABLE(X)                                                                                                             \
    X(32, 1, 1)                     /* fused: 64 | 32 registers */                                                                    \
    X(48, 1, 1)                     /* fused: 96 | 48 */                                                                              \
    X(64, 2, 1)                     /* fp32: fused would be 128, hoisted 64; 16-bit: fused 64 */                                      \
    X(96, 2, 1)                     /* fp32: hoisted 96; 16-bit: fused 96, the last that fits */                                      \
    X(128, 2, 2)                    /* fp32: hoisted 128, the budget; 16-bit: fused would be 128, hoisted 64 */                       \
    /* C = 192: the register-resident kernels spill (96 weight registers of the 168 a wave gets at 12 waves per workgroup: 79 / 83    \
       spilled VGPRs, tools/kernel_regs.py) -- streamed fragments (295 KB per timestep and workgroup from L2) are the faster of the    \
       two.  fp32: 192 registers forward and backward, no sequence kernel (callers loop the per-timestep kernels). */                 \
    X(192, 0, 3)                                                                                                                      \
    X(256, 0, 3) X(384, 0, 3) X(512, 0, 3)      /* the weight slice of a wave does not fit its registers in any format */

static inline int lstm_seq_family(int C) {
    const bool bf = leod_precision() == 1;
#define LSTM_ROW(CV, F32, B16) if (C == CV) return bf ? B16 : F32;
    LSTM_SEQ_TABLE(LSTM_ROW)
#undef LSTM_ROW
    return 0;
}

// The one routing function of the sequence kernels: launches nothing, reads no device memory; of the precision state it reads
// leod_precision() only (the bf16 / fp16 operand format of a forward launch is picked by the launcher and is not part of the code).
//   forward   1000 + C fused | 2000 + C hoisted | 3000 + C streamed;    backward   3000 + C streamed | 4000 + C register-resident
//   < 0       LEOD_ERR_*: what the entry returns (NULL pointers and empty sizes apart)
static int lstm_seq_route(int entry, int C, int flags) {
    if (entry != LE_FWD && entry != LE_BWD) return LEOD_ERR_ARG;
    const int fam = lstm_seq_family(C);
    // fp16 gates / bf16 gate gradients: the 16-bit modes, wherever a sequence kernel exists (forward and backward exist together)
    if ((flags & LF_GATES16) && !(leod_precision() == 1 && fam != 0)) return LEOD_ERR_ARG;
    if (entry == LE_FWD && (fam == 0 || (fam == 1) != !(flags & LF_PROJECTION))) return LEOD_ERR_UNSUPPORTED;
    if (fam == 3) return (flags & LF_PACK) ? LR_STREAMED + C : LEOD_ERR_ARG;
    if (entry == LE_FWD) return (fam == 1 ? LR_FUSED : LR_HOISTED) + C;
    return fam != 0 ? LR_RESIDENT_BWD + C : LEOD_ERR_UNSUPPORTED;
}
// what leod_convlstm_seq_mode answers: the forward family, asked of the route with either kind of input
static inline int lstm_seq_mode(int C) {
    const int fused = lstm_seq_route(LE_FWD, C, LF_PACK), hoisted = lstm_seq_route(LE_FWD, C, LF_PACK | LF_PROJECTION);
    return fused > 0 ? fused / 1000 : hoisted > 0 ? hoisted / 1000 : 0;
}
