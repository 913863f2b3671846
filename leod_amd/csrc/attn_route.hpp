// Routing of the partition attention core (k_attn.hip): one router (attn_route).  leod_partition_attn_fwd / _bwd, the two 16-bit
// predicates and leod_partition_attn_route all go through it; launch_attn (k_attn.hip) holds the only switch that launches.  Same shape as
// ConvProb -> conv_route -> launch_conv in conv_route.hpp.
#pragma once
#include "common.hpp"

enum : int { AE_FWD = 0, AE_BWD = 1 };
// the flags of leod_partition_attn_route: what the entry points are told about their tensors
enum : int { AF_QKV16 = 1, AF_O16 = 2, AF_DQKV16 = 4 };      // qkv rows 16-bit | O (forward) / dO (backward) rows 16-bit | dqkv written as bf16 (backward)

// Route codes, 10000 F + 100 PT + D (include/leod_hip.h lists them for callers); PT = 16-token tiles of a partition.
//   F = 1   register-direct fp32 kernels attn_fwd_kernel<PT, DCH> / attn_bwd_q_kernel + attn_bwd_kv_kernel<PT, DCH>;  D = 16 DCH
//   F = 2   attn_fwd_lds_kernel / attn_bwd_lds_kernel<PT, D>: LDS tiles of fp32;                                      D = d (24 | 32)
//   F = 3   attn_fwd_lds16_kernel / attn_bwd_lds16_kernel<PT, D>: LDS tiles of 16-bit operands;                       D = d (24 | 32)
//   0       no partitions, nothing to launch;    < 0    LEOD_ERR_*: what the entry returns
enum : int { AR_REG = 10000, AR_LDS32 = 20000, AR_LDS16 = 30000 };

// The one routing function of the attention core: launches nothing, reads no device memory.  Of the precision state it reads
// leod_precision() and leod_precision_mode() (the same in and out of a LeodFwdScope); the bf16 / fp16 operand format inside a family is
// picked by the launchers and is not part of the code.
// (any_batch: the answer for a batch that has partitions -- the two 16-bit predicates ask about the geometry, not about the call)
static int attn_route(int entry, int B, int H, int W, int C, int heads, int ph, int pw, int flags, bool any_batch = false) {
    if ((entry != AE_FWD && entry != AE_BWD) || heads <= 0 || ph <= 0 || pw <= 0) return LEOD_ERR_ARG;
    const int d = C / heads;
    if (C != heads * d || (d & 3) || d > 32 || H % ph || W % pw) return LEOD_ERR_ARG;
    const int PT = (ph * pw + 15) / 16, DCH = (d + 15) / 16;
    const bool empty = !any_batch && B * (H / ph) * (W / pw) == 0;
    const bool q16 = flags & AF_QKV16, o16 = flags & AF_O16, dq16 = entry == AE_BWD && (flags & AF_DQKV16);
    const bool pt8 = PT <= 5 || PT == 8 || PT == 10 || PT == 15;           // the tile counts the 32-wide kernels of all three families exist for
    // One head per workgroup (5 waves for an 80-token partition) rather than two (10 waves, the CU's wave limit at three workgroups): six
    // workgroups per CU overlap their load / MFMA / store phases better -- backward 984 -> 889 us per step over the four stages, forward of
    // stage 1 126 -> 116 us, the rest equal (tools/kbench.py attn, profiles/r04_z_attn_hg_kbench.txt).  The two-head kernels are gone.
    if ((d == 24 || d == 32) && pt8) {
        if (empty) return 0;
        // 16-bit modes with 16-bit qkv rows (backward: and bf16 dqkv): the 16-bit-tile kernels
        if (leod_precision() == 1 && q16 && (entry == AE_FWD || dq16)) return AR_LDS16 + 100 * PT + d;
        // 16-bit O / dO rows, fp16 rows: the 16-bit-tile kernels only
        if (o16 || ((q16 || dq16) && leod_precision_mode() == 2)) return LEOD_ERR_UNSUPPORTED;
        return AR_LDS32 + 100 * PT + d;
    }
    if (q16 || o16 || dq16) return LEOD_ERR_UNSUPPORTED;                    // the register-direct kernels read / write fp32 only
    if (!(DCH == 2 ? pt8 : DCH == 1 && (PT == 1 || PT == 2 || PT == 4 || PT == 5))) return LEOD_ERR_UNSUPPORTED;
    return empty ? 0 : AR_REG + 100 * PT + 16 * DCH;
}

// ---- the one-launch attention sub-block (k_attn_block.hip): y = x + gamma * proj(attn(qkv(LN(x)))) -------------------------------------
// the flags of leod_attn_block_fwd_route: what the block knows about its parameters
enum : int { ABF_LN_AFFINE = 1, ABF_NO_NORM = 2 };            // norm1 is a LayerNorm with weight and bias | norm1 is the identity (first block of a stage)
//   F = 4   attn_block_fwd_kernel<C, heads>: 80-token partitions, d = 24; code 40000 + 100 PT + D like the families above
enum : int { AR_BLOCK = 40000 };
extern "C" int leod_attn_block_o16_ok(int B, int H, int W, int C, int heads, int ph, int pw);

// What the kernel itself covers: a 16-bit precision mode and full 80-token partitions of an instantiated (C, heads).  leod_attn_block_fwd
// launches on this value.
static int attn_block_kernel_route(int B, int H, int W, int C, int heads, int ph, int pw) {
    if (heads <= 0 || ph <= 0 || pw <= 0 || B < 0 || H <= 0 || W <= 0 || C != heads * (C / heads) || H % ph || W % pw) return LEOD_ERR_ARG;
    if (leod_precision() != 1 || ph * pw != 80 || (long)B * H * W > 0x7fffffffL) return LEOD_ERR_UNSUPPORTED;
    if (!((C == 48 && heads == 2) || (C == 96 && heads == 4))) return LEOD_ERR_UNSUPPORTED;      // RVT-S stages 1 and 2
    return B == 0 ? 0 : AR_BLOCK + 100 * 5 + 24;
}
// The routing function of the block's forward: launches nothing, reads no device memory.  Positive only where the kernel covers the
// geometry AND the block keeps O / dO as 16-bit rows (leod_attn_block_o16_ok: the saved tensors are those of the three-launch path, so
// the backward pass is the same either way) AND norm1 is a LayerNorm with weight and bias, or the identity; everything else is LEOD_ERR_UNSUPPORTED: the block runs its three launches.
static int attn_block_fwd_route(int B, int H, int W, int C, int heads, int ph, int pw, int flags) {
    const int k = attn_block_kernel_route(B, H, W, C, heads, ph, pw);
    if (k < 0) return k;
    if (!(flags & (ABF_LN_AFFINE | ABF_NO_NORM)) || !leod_attn_block_o16_ok(B ? B : 1, H, W, C, heads, ph, pw)) return LEOD_ERR_UNSUPPORTED;
    return k;
}
