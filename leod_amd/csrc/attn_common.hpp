// Device helpers shared by the attention core (k_attn.hip) and the one-launch attention sub-block (k_attn_block.hip): the geometry of a
// call, the row of a partition's token, and the fragments of the 16-bit LDS tiles.
#pragma once
#include "common.hpp"

struct AttnGeom {
    int B, H, W, C, heads, d, ph, pw, window;   // window: 1 = window partition, 0 = grid partition
    int fmt;                                    // precision mode bf16, LDS kernels only: bit 0 = qkv holds bf16, bit 1 = dqkv is written as
                                                // bf16 (q, k, v only ever enter bf16 MFMAs; dqkv's consumers feed bf16 MFMAs)
};

// row (token of the NHWC map) of token t of partition p, -1 beyond the partition
__device__ __forceinline__ long token_row(const AttnGeom& g, int p, int t) {
    const int nH = g.H / g.ph, nW = g.W / g.pw, per = nH * nW;
    if (t >= g.ph * g.pw) return -1;
    const int b = p / per, rem = p - b * per;
    const int py = rem / nW, px = rem - py * nW;
    const int ty = t / g.pw, tx = t - ty * g.pw;
    return g.window ? ((long)b * g.H + (long)py * g.ph + ty) * g.W + (long)px * g.pw + tx
                    : ((long)b * g.H + py + (long)ty * nH) * g.W + px + (long)tx * nW;
}

// 16-bit tiles: rows of SD dwords with SD % 16 == 8 (see the bf16-tile kernels of k_attn.hip for why both read patterns are conflict-free)
template <int D, int HG>
struct A16L {
    static constexpr int RW = HG * 3 * D, RWD = HG * D;                     // bf16 elements of a staged qkv / dO row
    static constexpr int SD = (RW / 2 + 7) / 16 * 16 + 8;                   // row strides in dwords, == 8 (mod 16)
    static constexpr int SDD = (RWD / 2 + 7) / 16 * 16 + 8;
    static_assert(RW % 8 == 0 && RWD % 8 == 0 && SD >= RW / 2 && SDD >= RWD / 2, "rows are staged in units of 8 elements");
};
typedef unsigned u4v_ __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4 lds_s4_;
// head-dimension fragment: 8 bf16 of row `row` starting at dword `dw` (+ 4 rg)
__device__ __forceinline__ s8v a16_frag(const unsigned* base, int row, int sd, int dw, int rg) {
    return __builtin_bit_cast(s8v, *reinterpret_cast<const u4v_*>(base + row * sd + dw + 4 * rg));
}
template <int D> __device__ __forceinline__ s8v a16_mask(s8v v, int rg) {   // d = 24: k = 24 .. 31 belongs to the next part of the row
    if (D == 24 && rg == 3) v = s8v{0, 0, 0, 0, 0, 0, 0, 0};
    return v;
}
// token-dimension fragment: element [4 rg + j][16-column tile at dword dw] of the 16-row tile starting at row0, for j = 0 .. 3
__device__ __forceinline__ s4 a16_tfrag(const unsigned* base, int row0, int sd, int dw, int i, int rg) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_*)(base + (row0 + 4 * rg + (i >> 2)) * sd + dw + 2 * (i & 3)));
}
