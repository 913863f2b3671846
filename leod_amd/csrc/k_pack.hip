// Packed event frames (.evp blobs; format: leod_amd/data/utils/packed.py): the decoder that expands what came over
// PCIe into the dense uint8 frames the stem reads, and the encoder that ingestion and the tree converter write with.
//
// A frame of E = C*H*W bytes is cut into blocks of 64 elements and groups of 64 blocks.  Blob: 16-byte header {u32 n_masks, u32 n_values},
// G = ceil(E / 4096) group entries {u64 l1, u32 mask_base, u32 value_base}, one u64 mask per non-zero block, the non-zero bytes.
//
// Mapping, both directions: one wave per group, lane = block for the bookkeeping (mask index = mask_base + popcount(l1 & lanes below),
// value offset = value_base + wave prefix sum of the mask popcounts); the 4 KB of the group cross global memory as 4 steps of
// 64 lanes x 16 bytes, i.e. lane l of step k holds quarter (l & 3) of block 16 k + (l >> 2) and fetches that block's mask and value
// offset from lane 16 k + (l >> 2) by shuffle.  Every output byte of the decoder is stored exactly once, zeros included.
//
// Bounds: every position derived from blob CONTENTS is compared with the extent of the blob buffer before it is read (a miss reads
// as zero), and every store goes to an element index below E of its own slot: a malformed blob gives wrong frames, never an access
// outside [blob, blob + nbytes) or outside out.  The encoder's positions derive from its own counts and stay below the worst-case
// stride by construction.
#include "common.hpp"

namespace {
typedef unsigned long long u64;
typedef unsigned char u8;

__device__ __forceinline__ u64 lanes_below(int lane) { return lane ? (~0ULL >> (64 - lane)) : 0ULL; }

// exclusive prefix sum over the wave; total = sum over all 64 lanes
__device__ __forceinline__ unsigned wave_excl_scan(unsigned v, int lane, unsigned& total) {
    unsigned s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(s, o, 64);
        if (lane >= o) s += t;
    }
    total = __shfl(s, 63, 64);
    return s - v;
}

__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) {
    return ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) | ((w & 0xff000000u) ? 8u : 0u);
}

// ---- decoder ----------------------------------------------------------------------------------------------------------------------
// grid (ceil(G / 4), slots), 256 threads = 4 waves = 4 groups.  vec: E % 16 == 0 and out 16-byte aligned (each slot then is);
// vec_flip: additionally H*W % 16 == 0, so a 16-byte run stays inside one channel plane.
__global__ __launch_bounds__(256) void unpack_kernel(const u8* __restrict__ blob, long nbytes, const long* __restrict__ slot_off,
                                                     const int* __restrict__ slot_flags, u8* __restrict__ out, long E, long HW, int C, int G,
                                                     int vec, int vec_flip) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;                                          // the whole wave leaves: no block-level barrier in this kernel
    const long slot = blockIdx.y;
    const long off = slot_off[slot];
    const int flip = slot_flags ? (slot_flags[slot] & 1) : 0;
    const bool live = off >= 0 && (off & 15) == 0 && off <= nbytes - (16 + 16L * G);   // wave-uniform; else a zero frame
    const long m0 = live ? off + 16 + 16L * G : 0;               // first mask
    u64 mask = 0;
    long vpos = 0;
    if (live) {
        const u8* entry = blob + off + 16 + 16L * g;
        const u64 l1 = *reinterpret_cast<const u64*>(entry);
        const unsigned mask_base = *reinterpret_cast<const unsigned*>(entry + 8), value_base = *reinterpret_cast<const unsigned*>(entry + 12);
        const unsigned n_masks = *reinterpret_cast<const unsigned*>(blob + off);
        if ((l1 >> lane) & 1ULL) {
            const long p = m0 + 8L * ((long)mask_base + __popcll(l1 & lanes_below(lane)));
            if (p + 8 <= nbytes) mask = *reinterpret_cast<const u64*>(blob + p);
        }
        unsigned total;
        const unsigned before = wave_excl_scan((unsigned)__popcll(mask), lane, total);
        vpos = m0 + 8L * n_masks + (long)value_base + before;
    }
    u8* o = out + slot * E;
    const int sub = lane & 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int src = 16 * k + (lane >> 2);
        const u64 m = __shfl(mask, src, 64);
        long vp = __shfl(vpos, src, 64);
        const unsigned m16 = (unsigned)(m >> (16 * sub)) & 0xffffu;
        vp += __popcll(m & ((1ULL << (16 * sub)) - 1ULL));
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (m16) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if ((m16 >> j) & 1u) {
                    const unsigned v = (vp >= 0 && vp < nbytes) ? blob[vp] : 0u;
                    ++vp;
                    w[j >> 2] |= v << (8 * (j & 3));
                }
            }
        }
        const long e = (long)g * 4096 + k * 1024 + lane * 16;   // first of this lane's 16 elements
        if (e >= E) continue;
        if (!flip && vec) {
            *reinterpret_cast<uint4*>(o + e) = make_uint4(w[0], w[1], w[2], w[3]);
        } else if (flip && vec_flip) {
            const long c = e / HW;
            *reinterpret_cast<uint4*>(o + ((long)(C - 1) - c) * HW + (e - c * HW)) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const long ej = e + j;
                if (ej < E) {
                    long d = ej;
                    if (flip) {
                        const long c = ej / HW;
                        d = ((long)(C - 1) - c) * HW + (ej - c * HW);
                    }
                    o[d] = (u8)(w[j >> 2] >> (8 * (j & 3)));
                }
            }
        }
    }
}

// ---- encoder ----------------------------------------------------------------------------------------------------------------------
// the 4 x 16 bytes of this lane (zeros beyond E) and, returned, the mask of block `lane` of group g
__device__ __forceinline__ u64 load_group(const u8* __restrict__ f, long E, int g, int lane, int vec, uint4 (&v)[4]) {
    u64 mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long e = (long)g * 4096 + k * 1024 + lane * 16;
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (e < E) {
            if (vec) {
                const uint4 q = *reinterpret_cast<const uint4*>(f + e);
                w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (e + j < E) w[j >> 2] |= (unsigned)f[e + j] << (8 * (j & 3));
            }
        }
        v[k] = make_uint4(w[0], w[1], w[2], w[3]);
        const unsigned m16 = nonzero_bytes(w[0]) | (nonzero_bytes(w[1]) << 4) | (nonzero_bytes(w[2]) << 8) | (nonzero_bytes(w[3]) << 12);
        u64 m = (u64)m16 << (16 * (lane & 3));
        m |= __shfl_xor(m, 1, 64);
        m |= __shfl_xor(m, 2, 64);                               // the four quarters of block 16 k + (lane >> 2)
        const u64 t = __shfl(m, 4 * (lane & 15), 64);
        if ((lane >> 4) == k) mine = t;
    }
    return mine;
}

// pass 1: l1 of every group into its entry; the entry's two u32 hold the group's COUNTS until pass 2 turns them into bases
__global__ __launch_bounds__(256) void pack_count_kernel(const u8* __restrict__ frames, long E, int G, u8* __restrict__ ws, long stride, int vec) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const long frame = blockIdx.y;
    uint4 v[4];
    const u64 mask = load_group(frames + frame * E, E, g, lane, vec, v);
    const u64 l1 = __ballot(mask != 0);
    unsigned n_values;
    wave_excl_scan((unsigned)__popcll(mask), lane, n_values);
    if (lane == 0) {
        u8* entry = ws + frame * stride + 16 + 16L * g;
        *reinterpret_cast<u64*>(entry) = l1;
        *reinterpret_cast<uint2*>(entry + 8) = make_uint2((unsigned)__popcll(l1), n_values);
    }
}

// pass 2: one block per frame: counts -> exclusive running sums, the header, the blob's size and its zero padding
__global__ __launch_bounds__(256) void pack_scan_kernel(u8* __restrict__ ws, long stride, int G, long* __restrict__ sizes) {
    __shared__ unsigned sm[256], sv[256];
    const int t = threadIdx.x;
    u8* blob = ws + (long)blockIdx.x * stride;
    const int chunk = (G + 255) / 256, lo = min(t * chunk, G), hi = min(lo + chunk, G);
    unsigned nm = 0, nv = 0;
    for (int g = lo; g < hi; ++g) {
        const uint2 c = *reinterpret_cast<const uint2*>(blob + 16 + 16L * g + 8);
        nm += c.x; nv += c.y;
    }
    sm[t] = nm; sv[t] = nv;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned a = t >= o ? sm[t - o] : 0u, b = t >= o ? sv[t - o] : 0u;
        __syncthreads();
        sm[t] += a; sv[t] += b;
        __syncthreads();
    }
    unsigned bm = sm[t] - nm, bv = sv[t] - nv;                   // exclusive
    for (int g = lo; g < hi; ++g) {
        uint2* p = reinterpret_cast<uint2*>(blob + 16 + 16L * g + 8);
        const uint2 c = *p;
        *p = make_uint2(bm, bv);
        bm += c.x; bv += c.y;
    }
    if (t == 0) {
        const unsigned n_masks = sm[255], n_values = sv[255];
        *reinterpret_cast<uint4*>(blob) = make_uint4(n_masks, n_values, 0u, 0u);
        const long size = 16 + 16L * G + 8L * n_masks + n_values, padded = (size + 15) / 16 * 16;
        for (long p = size; p < padded; ++p) blob[p] = 0;
        sizes[blockIdx.x] = padded;
    }
}

// pass 3: masks and values to their places
__global__ __launch_bounds__(256) void pack_write_kernel(const u8* __restrict__ frames, long E, int G, u8* __restrict__ ws, long stride, int vec) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const long frame = blockIdx.y;
    uint4 v[4];
    const u64 mask = load_group(frames + frame * E, E, g, lane, vec, v);
    const u64 l1 = __ballot(mask != 0);
    u8* blob = ws + frame * stride;
    const uint2 base = *reinterpret_cast<const uint2*>(blob + 16 + 16L * g + 8);
    const unsigned n_masks = *reinterpret_cast<const unsigned*>(blob);
    const long m0 = 16 + 16L * G;
    const long mpos = m0 + 8L * ((long)base.x + __popcll(l1 & lanes_below(lane)));
    if (mask && mpos + 8 <= stride) *reinterpret_cast<u64*>(blob + mpos) = mask;
    unsigned total;
    const unsigned before = wave_excl_scan((unsigned)__popcll(mask), lane, total);
    const long vpos = m0 + 8L * n_masks + (long)base.y + before;
    const int sub = lane & 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int src = 16 * k + (lane >> 2);
        const u64 m = __shfl(mask, src, 64);
        long vp = __shfl(vpos, src, 64) + __popcll(m & ((1ULL << (16 * sub)) - 1ULL));
        const unsigned w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        if ((m >> (16 * sub)) & 0xffffULL) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const unsigned b = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                if (b && vp < stride) blob[vp++] = (u8)b;
            }
        }
    }
}

// blobs from the worst-case stride to their final, back-to-back places: 16 bytes per lane
__global__ __launch_bounds__(256) void pack_compact_kernel(const u8* __restrict__ ws, long stride, const long* __restrict__ offsets,
                                                           u8* __restrict__ out, long out_bytes) {
    const long frame = blockIdx.y;
    const long lo = offsets[frame], hi = offsets[frame + 1];
    if (lo < 0 || hi < lo || hi > out_bytes || hi - lo > stride || (lo & 15) || (hi & 15)) return;
    const uint4* s = reinterpret_cast<const uint4*>(ws + frame * stride);
    uint4* d = reinterpret_cast<uint4*>(out + lo);
    const long n16 = (hi - lo) / 16;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) d[i] = s[i];
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline long worst_bytes(long E, int G) { return (16 + 16L * G + 8 * ((E + 63) / 64) + E + 15) / 16 * 16; }
constexpr int kMaxGridY = 32768;
}  // namespace

LEOD_API int leod_unpack_frames_u8(const unsigned char* blob, long nbytes, const long* slot_off, const int* slot_flags, int n_slots,
                                   unsigned char* out, int C, int H, int W, hipStream_t stream) {
    if (n_slots < 0 || nbytes < 0 || C < 1 || H < 1 || W < 1) return LEOD_ERR_ARG;
    const long HW = (long)H * W, E = HW * C;
    if (E >= (1L << 31)) return LEOD_ERR_UNSUPPORTED;
    if (n_slots == 0) return LEOD_OK;
    if (!slot_off || !out || (nbytes > 0 && !blob) || !aligned16(blob)) return LEOD_ERR_ARG;
    const int G = (int)((E + 4095) / 4096);
    const int vec = (E % 16 == 0 && aligned16(out)) ? 1 : 0, vec_flip = (vec && HW % 16 == 0) ? 1 : 0;
    for (int s0 = 0; s0 < n_slots; s0 += kMaxGridY) {
        const int ns = min(kMaxGridY, n_slots - s0);
        hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((G + 3) / 4), (unsigned)ns), dim3(256), 0, stream, blob, nbytes, slot_off + s0,
                           slot_flags ? slot_flags + s0 : nullptr, out + (long)s0 * E, E, HW, C, G, vec, vec_flip);
    }
    return leod_launch_status();
}

LEOD_API long leod_pack_frame_stride(long E) {
    return E < 1 ? 0 : worst_bytes(E, (int)((E + 4095) / 4096));
}

LEOD_API int leod_pack_frames_u8(const unsigned char* frames, int n, long E, unsigned char* ws, long stride, long* sizes, hipStream_t stream) {
    if (n < 0 || E < 1) return LEOD_ERR_ARG;
    if (E >= (1L << 31)) return LEOD_ERR_UNSUPPORTED;
    if (n == 0) return LEOD_OK;
    const int G = (int)((E + 4095) / 4096);
    if (!frames || !ws || !sizes || !aligned16(ws) || stride % 16 || stride < worst_bytes(E, G)) return LEOD_ERR_ARG;
    const int vec = (E % 16 == 0 && aligned16(frames)) ? 1 : 0;
    for (int f0 = 0; f0 < n; f0 += kMaxGridY) {
        const int nf = min(kMaxGridY, n - f0);
        const dim3 grid((unsigned)((G + 3) / 4), (unsigned)nf);
        hipLaunchKernelGGL(pack_count_kernel, grid, dim3(256), 0, stream, frames + (long)f0 * E, E, G, ws + (long)f0 * stride, stride, vec);
        hipLaunchKernelGGL(pack_scan_kernel, dim3((unsigned)nf), dim3(256), 0, stream, ws + (long)f0 * stride, stride, G, sizes + f0);
        hipLaunchKernelGGL(pack_write_kernel, grid, dim3(256), 0, stream, frames + (long)f0 * E, E, G, ws + (long)f0 * stride, stride, vec);
    }
    return leod_launch_status();
}

LEOD_API int leod_pack_compact_u8(const unsigned char* ws, long stride, const long* offsets, int n, unsigned char* out, long out_bytes,
                                  hipStream_t stream) {
    if (n < 0 || stride < 16 || stride % 16 || out_bytes < 0) return LEOD_ERR_ARG;
    if (n == 0) return LEOD_OK;
    if (!ws || !offsets || !out || !aligned16(ws) || !aligned16(out)) return LEOD_ERR_ARG;
    for (int f0 = 0; f0 < n; f0 += kMaxGridY) {
        const int nf = min(kMaxGridY, n - f0);
        hipLaunchKernelGGL(pack_compact_kernel, dim3((unsigned)max(1L, min(64L, stride / 16 / 256)), (unsigned)nf), dim3(256), 0, stream,
                           ws + (long)f0 * stride, stride, offsets + f0, out, out_bytes);
    }
    return leod_launch_status();
}
