// Baseline JPEG of rendered frames (leod_jpeg_scan / leod_jpeg_emit): rgb [N, H, W, 3] uint8, what leod_render_frames_u8 writes, to N
// complete JFIF files back to back in one byte buffer plus their offsets.  The reference hands its frames to an mp4 writer on the host
// (vis_pred.py:216-227); here the last stage of the video path stays on the device and the files go into a Motion-JPEG AVI.
//
// The stream: SOI, APP0 JFIF 1.01, DQT 0 (luma) and 1 (chroma), SOF0 with three components sampled 1x1 (4:4:4),
// the four Annex K.3 Huffman tables, DRI = blocks per row, SOS, scan, EOI.  An MCU is one 8 x 8 block of Y, Cb, Cr; a row of MCUs is one
// restart interval: DC predictors start at 0, the interval is padded with 1-bits to a byte, RST(row mod 8) follows every row but the last.
// Hence every interval can be coded without knowing any other, and a frame of H rows has ceil(H/8) of them.
//
// Arithmetic, all in integers (tests/jpeg_ref.py restates it):
//   colour   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//            Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,  Cr = (32768 R - 27439 G - 5329 B + ...) >> 16, clipped
//   edges    a partial block repeats the last column / row of the picture
//   DCT      C[k][n] = round(8192 c_k cos((2n+1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2; rows t = (sum C x + 512) >> 10 on x - 128,
//            columns y = (sum C t + 32768) >> 16 (arithmetic shifts)
//   quant    Annex K.1 tables under the IJG quality rule; sign(y) * ((|y| + Q/2) / Q)
//
// One memset and five launches per call, no allocation, no workgroup waits on another:
//   1. transform  one thread per block and component: colour, DCT, quantisation -> 64 int16 in zigzag order (128 bytes, 8 x 16-byte stores)
//   2. pack       one workgroup per interval, 256 units (block x component, in stream order) per step: every thread sizes the code of its
//                 unit, a scan over the workgroup turns the sizes into bit offsets, then the thread codes the unit again and ORs whole
//                 32-bit words into the interval's zeroed bit buffer (atomicOr: the first and the last word of a unit are shared with
//                 its neighbours; OR does not depend on the order, so two runs give the same bytes).  Sizing and coding are ONE function
//                 over two sinks.
//   3. count      one wave per interval: bytes of the interval plus its 0xFF bytes = its length in the file
//   4. offsets    one workgroup: running sum over the intervals of all frames (every interval is followed by two marker bytes, the first
//                 of a frame is preceded by the header) -> position of every interval in the blob, offsets[f] of every frame
//   5. emit       one workgroup per interval: header (first interval of a frame), bytes with a 0x00 behind every 0xFF (ballot + prefix over
//                 256 bytes per step), then RSTm or EOI
// Bounds: a coefficient costs at most 27 bits (16 of code + 11 of magnitude), a block 216 bytes before and 432 after stuffing.
#include <algorithm>

#include "common.hpp"

namespace {
constexpr int HDR_BYTES = 629;
constexpr int BLOCK_BYTES = 216;                                          // 64 coefficients x 27 bits

constexpr unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr unsigned char Q_BASE[2][64] = {                                 // Annex K.1, row-major
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr int DCT[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},   {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                           {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                           {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                           {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// Annex K.3: number of codes of length 1 .. 16, then the symbols in code order.  Index 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma.
struct HuffSpec { unsigned char bits[16]; int n; unsigned char vals[162]; };
constexpr HuffSpec HUFF[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, 162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
      0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
      0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
      0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
      0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
      0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
      0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
      0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, 162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
      0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
      0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
      0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
      0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
      0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
      0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}}};

// symbol -> code | length << 16 (0: no such symbol).  [0] luma, [1] chroma.
struct HuffCodes { uint32_t dc[2][16]; uint32_t ac[2][256]; };
constexpr HuffCodes make_codes() {
    HuffCodes t{};
    for (int s = 0; s < 4; ++s) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < HUFF[s].bits[len - 1]; ++i, ++k, ++code) {
                const uint32_t e = code | (uint32_t)len << 16;
                if (s & 1) t.ac[s >> 1][HUFF[s].vals[k]] = e; else t.dc[s >> 1][HUFF[s].vals[k]] = e;
            }
            code <<= 1;
        }
    }
    return t;
}
__constant__ HuffCodes d_codes = make_codes();

struct Params {                                                           // kernel argument, built on the host per call
    unsigned char q[2][64];                                               // quantisation tables, row-major
    unsigned char hdr[HDR_BYTES + 3];
};

struct Geometry {
    int n, H, W, nbx, nby, units;                                         // units = 3 * nbx: block x component per interval, in stream order
    long n_int, ibuf;                                                     // intervals of the call, bytes of one interval's bit buffer
    long coef, bits, ibytes, isize, apos, total;                          // workspace offsets
};
inline long align16(long v) { return (v + 15) & ~15L; }
inline Geometry geometry(int n, int H, int W) {
    Geometry g;
    g.n = n; g.H = H; g.W = W;
    g.nbx = (W + 7) / 8; g.nby = (H + 7) / 8; g.units = 3 * g.nbx;
    g.n_int = (long)n * g.nby;
    g.ibuf = ((long)g.units * BLOCK_BYTES + 3) / 4 * 4 + 4;               // whole words, one to spare
    g.coef = 0;
    g.bits = align16(g.n_int * g.units * 128);
    g.ibytes = g.bits + align16(g.n_int * g.ibuf);
    g.isize = g.ibytes + align16(g.n_int * 4);
    g.apos = g.isize + align16(g.n_int * 4);
    g.total = g.apos + align16(g.n_int * 8);
    return g;
}

// ---- 1. transform ---------------------------------------------------------------------------------------------------------------------
template <bool WORDS>                                                     // WORDS: rows are whole 32-bit words and the picture starts on one
__global__ __launch_bounds__(256) void jpeg_transform_kernel(const uint8_t* __restrict__ rgb, uint4* __restrict__ coef, const Params P,
                                                             long total, int H, int W, int nbx, int nby) {
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
        const int c = (int)(g % 3);
        const long b = g / 3;
        const int bx = (int)(b % nbx);
        const long r2 = b / nbx;
        const int by = (int)(r2 % nby);
        const long f = r2 / nby;
        const uint8_t* img = rgb + f * H * W * 3;
        const int kr = c == 0 ? 19595 : c == 1 ? -11059 : 32768, kg = c == 0 ? 38470 : c == 1 ? -21709 : -27439;
        const int kb = c == 0 ? 7471 : c == 1 ? 32768 : -5329, add = c == 0 ? 32768 : (128 << 16) + 32767;
        const bool inside = bx * 8 + 8 <= W;
        int t[8][8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint8_t* row = img + (long)min(by * 8 + r, H - 1) * W * 3;
            int x[8];
            if (WORDS && inside) {                                        // 24 bytes = 6 words, the block's offset in the row is a multiple of 24
                const uint32_t* w = reinterpret_cast<const uint32_t*>(row + bx * 24);
                uint32_t v[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) v[i] = w[i];
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    const int R = (v[(3 * n) >> 2] >> (((3 * n) & 3) * 8)) & 255, G = (v[(3 * n + 1) >> 2] >> (((3 * n + 1) & 3) * 8)) & 255;
                    const int B = (v[(3 * n + 2) >> 2] >> (((3 * n + 2) & 3) * 8)) & 255;
                    x[n] = min(max((kr * R + kg * G + kb * B + add) >> 16, 0), 255) - 128;
                }
            } else {
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    const uint8_t* px = row + (long)min(bx * 8 + n, W - 1) * 3;
                    x[n] = min(max((kr * px[0] + kg * px[1] + kb * px[2] + add) >> 16, 0), 255) - 128;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int s = 512;
#pragma unroll
                for (int n = 0; n < 8; ++n) s += DCT[k][n] * x[n];
                t[r][k] = s >> 10;
            }
        }
        const unsigned char* q = P.q[c ? 1 : 0];
        int v[64];                                                        // row-major; every index below is a compile-time constant
#pragma unroll
        for (int col = 0; col < 8; ++col) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int s = 32768;
#pragma unroll
                for (int n = 0; n < 8; ++n) s += DCT[k][n] * t[n][col];
                const int y = s >> 16;
                const uint32_t Q = q[k * 8 + col], m = ((uint32_t)abs(y) + (Q >> 1)) / Q;
                v[k * 8 + col] = y < 0 ? -(int)m : (int)m;
            }
        }
        uint4* dst = coef + g * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint32_t w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                w[e] = ((uint32_t)v[ZIGZAG[8 * j + 2 * e]] & 0xFFFFu) | ((uint32_t)v[ZIGZAG[8 * j + 2 * e + 1]] << 16);
            dst[j] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

// ---- 2. pack --------------------------------------------------------------------------------------------------------------------------
struct CountSink {
    int bits = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { bits += len; }
    __device__ __forceinline__ void flush() {}
};
// Bits go out most significant first; a word of the buffer holds four bytes of the stream, so the 32 bits are byte-swapped before the OR.
struct OrSink {
    uint32_t* buf;                                                        // the interval's bit buffer
    long word;                                                            // index of the word the pending bits start in
    unsigned long long acc = 0;                                           // pending bits, right-aligned; the top (fill - own) of them are a neighbour's: zero
    int fill;                                                             // pending bits, < 32 between calls
    __device__ OrSink(uint32_t* b, long bitpos) : buf(b), word(bitpos >> 5), fill((int)(bitpos & 31)) {}
    __device__ __forceinline__ void put(uint32_t code, int len) {         // len <= 27, so fill + len < 64
        acc = (acc << len) | code;
        fill += len;
        if (fill >= 32) {
            fill -= 32;
            atomicOr(buf + word++, __builtin_bswap32((uint32_t)(acc >> fill)));
            acc &= (1ULL << fill) - 1ULL;
        }
    }
    __device__ __forceinline__ void flush() {
        if (fill > 0 && acc != 0) atomicOr(buf + word, __builtin_bswap32((uint32_t)(acc << (32 - fill))));
    }
};

__device__ __forceinline__ int category(int v) { return v ? 32 - __clz(abs(v)) : 0; }
__device__ __forceinline__ uint32_t magnitude_bits(int v, int cat) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u); }

// The code of one unit (64 coefficients in zigzag order at cp, DC predictor pred, tables sel = 0 luma / 1 chroma) into a sink.
template <class Sink>
__device__ __forceinline__ void code_unit(const uint4* __restrict__ cp, int pred, int sel, Sink& s) {
    uint4 w = cp[0];
    {
        const int diff = (int)(short)(w.x & 0xFFFFu) - pred, cat = category(diff);
        const uint32_t e = d_codes.dc[sel][cat];
        s.put(((e & 0xFFFFu) << cat) | magnitude_bits(diff, cat), (int)(e >> 16) + cat);
    }
    const uint32_t zrl = d_codes.ac[sel][0xF0], eob = d_codes.ac[sel][0x00];
    int run = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j) w = cp[j];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (j == 0 && e == 0) continue;
            const int v = (int)(short)((ws[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu);
            if (v == 0) { ++run; continue; }
            while (run > 15) { s.put(zrl & 0xFFFFu, (int)(zrl >> 16)); run -= 16; }
            const int cat = category(v);
            const uint32_t c = d_codes.ac[sel][(run << 4 | cat) & 255];
            s.put(((c & 0xFFFFu) << cat) | magnitude_bits(v, cat), (int)(c >> 16) + cat);
            run = 0;
        }
    }
    if (run) s.put(eob & 0xFFFFu, (int)(eob >> 16));
    s.flush();
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint4* __restrict__ coef, uint32_t* __restrict__ bits, int* __restrict__ ibytes,
                                                        long n_int, int units, long ibuf_words) {
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long i = blockIdx.x; i < n_int; i += gridDim.x) {
        const uint4* icoef = coef + i * units * 8;
        uint32_t* ibits = bits + i * ibuf_words;
        int carry = 0;                                                    // bits of the interval so far (at most units * 1728 < 2^26)
        for (int u0 = 0; u0 < units; u0 += 256) {
            const int u = u0 + tid;
            const bool live = u < units;
            int pred = 0, sel = 0, len = 0;
            if (live) {
                sel = (u % 3) ? 1 : 0;
                if (u >= 3) pred = (int)(short)(icoef[(long)(u - 3) * 8].x & 0xFFFFu);
                CountSink cs;
                code_unit(icoef + (long)u * 8, pred, sel, cs);
                len = cs.bits;
            }
            int incl = len;                                               // inclusive scan over the wave, then over the four waves
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            __syncthreads();                                              // the previous step's sums have been read
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            int before = carry, all = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                before += w < wave ? s_wave[w] : 0;
                all += s_wave[w];
            }
            if (live) {
                OrSink os(ibits, (long)before + incl - len);
                code_unit(icoef + (long)u * 8, pred, sel, os);
            }
            carry += all;
        }
        if (tid == 0) {
            if (carry & 7) {                                              // pad to a byte with 1-bits
                OrSink os(ibits, carry);
                const int pad = 8 - (carry & 7);
                os.put((1u << pad) - 1u, pad);
                os.flush();
            }
            ibytes[i] = (carry + 7) >> 3;
        }
    }
}

// ---- 3. count -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_count_kernel(const uint8_t* __restrict__ bits, const int* __restrict__ ibytes, int* __restrict__ isize,
                                                         long n_int, long ibuf) {
    const int lane = threadIdx.x & 63;
    for (long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6); i < n_int; i += (long)gridDim.x * 4) {
        const uint8_t* b = bits + i * ibuf;
        const int n = ibytes[i];
        int ff = 0;
        for (int j = lane; j < n; j += 64) ff += b[j] == 0xFF;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ff += __shfl_xor(ff, o, 64);
        if (lane == 0) isize[i] = n + ff;
    }
}

// ---- 4. offsets -----------------------------------------------------------------------------------------------------------------------
// One workgroup.  Interval i takes isize[i] + 2 bytes (RSTm or EOI behind it), the first of a frame HDR_BYTES more in front.
__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const int* __restrict__ isize, long* __restrict__ apos, long* __restrict__ offsets,
                                                           long n_int, int nby, long base) {
    __shared__ long s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long carry = base;
    for (long i0 = 0; i0 < n_int; i0 += 256) {
        const long i = i0 + tid;
        const bool live = i < n_int;
        const bool first = live && i % nby == 0;
        const long mine = live ? (long)isize[i] + 2 + (first ? HDR_BYTES : 0) : 0;
        long incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        __syncthreads();
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        long before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            before += w < wave ? s_wave[w] : 0;
            all += s_wave[w];
        }
        if (live) {
            const long at = before + incl - mine;
            apos[i] = at;
            if (first) offsets[i / nby] = at;
        }
        carry += all;
    }
    if (tid == 0) offsets[n_int / nby] = carry;
}

// ---- 5. emit --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_emit_kernel(const uint8_t* __restrict__ bits, const int* __restrict__ ibytes,
                                                        const int* __restrict__ isize, const long* __restrict__ apos, uint8_t* __restrict__ out,
                                                        long out_bytes, long base, const Params P, long n_int, int nby, long ibuf) {
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long i = blockIdx.x; i < n_int; i += gridDim.x) {
        const int row = (int)(i % nby);
        long at = apos[i] - base;                                         // positions in the workspace count from the start of the blob
        if (at < 0) continue;                                             // (a base other than the scan's: nothing is written)
        if (row == 0) {
            for (int j = tid; j < HDR_BYTES; j += 256)
                if (at + j < out_bytes) out[at + j] = P.hdr[j];
            at += HDR_BYTES;
        }
        const uint8_t* b = bits + i * ibuf;
        const int n = ibytes[i];
        int carry = 0;                                                    // 0xFF bytes so far
        for (int j0 = 0; j0 < n; j0 += 256) {
            const int j = j0 + tid;
            const int byte = j < n ? b[j] : 0;
            const bool ff = byte == 0xFF;
            const unsigned long long m = __ballot(ff);
            __syncthreads();
            if (lane == 0) s_wave[wave] = __popcll(m);
            __syncthreads();
            int before = carry + __popcll(m & ((1ULL << lane) - 1ULL)), all = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                before += w < wave ? s_wave[w] : 0;
                all += s_wave[w];
            }
            if (j < n) {
                const long p = at + j + before;
                if (p < out_bytes) out[p] = (uint8_t)byte;
                if (ff && p + 1 < out_bytes) out[p + 1] = 0;
            }
            carry += all;
        }
        if (tid == 0) {
            const long p = at + isize[i];
            if (p + 1 < out_bytes) {
                out[p] = 0xFF;
                out[p + 1] = row == nby - 1 ? 0xD9 : (uint8_t)(0xD0 + (row & 7));
            }
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
inline unsigned char* put_segment(unsigned char* p, int marker, int body) {
    *p++ = 0xFF; *p++ = (unsigned char)marker;
    *p++ = (unsigned char)((body + 2) >> 8); *p++ = (unsigned char)((body + 2) & 255);
    return p;
}

inline void build_params(Params& P, int H, int W, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) P.q[t][i] = (unsigned char)std::min(std::max((Q_BASE[t][i] * s + 50) / 100, 1), 255);
    unsigned char* p = P.hdr;
    *p++ = 0xFF; *p++ = 0xD8;
    p = put_segment(p, 0xE0, 14);
    const unsigned char jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (unsigned char c : jfif) *p++ = c;
    for (int t = 0; t < 2; ++t) {
        p = put_segment(p, 0xDB, 65);
        *p++ = (unsigned char)t;
        for (int i = 0; i < 64; ++i) *p++ = P.q[t][ZIGZAG[i]];
    }
    p = put_segment(p, 0xC0, 15);
    const unsigned char sof[15] = {8, (unsigned char)(H >> 8), (unsigned char)(H & 255), (unsigned char)(W >> 8), (unsigned char)(W & 255), 3,
                                   1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1};
    for (unsigned char c : sof) *p++ = c;
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        p = put_segment(p, 0xC4, 17 + HUFF[t].n);
        *p++ = (unsigned char)ids[t];
        for (int i = 0; i < 16; ++i) *p++ = HUFF[t].bits[i];
        for (int i = 0; i < HUFF[t].n; ++i) *p++ = HUFF[t].vals[i];
    }
    const int dri = (W + 7) / 8;
    p = put_segment(p, 0xDD, 2);
    *p++ = (unsigned char)(dri >> 8); *p++ = (unsigned char)(dri & 255);
    p = put_segment(p, 0xDA, 10);
    const unsigned char sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (unsigned char c : sos) *p++ = c;
    static_assert(2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 6 + 14 == HDR_BYTES, "header length");
}

inline bool bad_geometry(int n, int H, int W) { return n <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535; }
}  // namespace

LEOD_API int leod_jpeg_query(int n, int H, int W, long* ws_bytes, long* out_bound, int* header_bytes) {
    if (bad_geometry(n, H, W)) return LEOD_ERR_ARG;
    const Geometry g = geometry(n, H, W);
    if (ws_bytes) *ws_bytes = g.total;
    if (out_bound) *out_bound = (long)n * (HDR_BYTES + (long)g.nby * (g.units * 2L * BLOCK_BYTES + 2));
    if (header_bytes) *header_bytes = HDR_BYTES;
    return LEOD_OK;
}

LEOD_API int leod_jpeg_scan(const unsigned char* rgb, int n, int H, int W, int quality, void* ws, long ws_bytes, long* offsets, long base,
                            hipStream_t stream) {
    if (!rgb || !ws || !offsets || bad_geometry(n, H, W) || quality < 1 || quality > 100 || base < 0) return LEOD_ERR_ARG;
    const Geometry g = geometry(n, H, W);
    if (ws_bytes < g.total || (reinterpret_cast<uintptr_t>(ws) & 15)) return LEOD_ERR_ARG;
    Params P;
    build_params(P, H, W, quality);
    uint8_t* w8 = static_cast<uint8_t*>(ws);
    uint4* coef = reinterpret_cast<uint4*>(w8 + g.coef);
    uint32_t* bits = reinterpret_cast<uint32_t*>(w8 + g.bits);
    int* ibytes = reinterpret_cast<int*>(w8 + g.ibytes);
    int* isize = reinterpret_cast<int*>(w8 + g.isize);
    long* apos = reinterpret_cast<long*>(w8 + g.apos);
    if (hipMemsetAsync(bits, 0, g.n_int * g.ibuf, stream) != hipSuccess) return LEOD_ERR_LAUNCH;
    const long total = g.n_int * g.units;
    const dim3 tgrid((unsigned)std::min((total + 255) / 256, 1L << 20));
    if ((W * 3L) % 4 == 0 && (reinterpret_cast<uintptr_t>(rgb) & 3) == 0 && ((long)H * W * 3) % 4 == 0)
        hipLaunchKernelGGL(jpeg_transform_kernel<true>, tgrid, dim3(256), 0, stream, rgb, coef, P, total, H, W, g.nbx, g.nby);
    else
        hipLaunchKernelGGL(jpeg_transform_kernel<false>, tgrid, dim3(256), 0, stream, rgb, coef, P, total, H, W, g.nbx, g.nby);
    if (hipGetLastError() != hipSuccess) return LEOD_ERR_LAUNCH;
    const dim3 igrid((unsigned)std::min(g.n_int, 1L << 20));
    hipLaunchKernelGGL(jpeg_pack_kernel, igrid, dim3(256), 0, stream, coef, bits, ibytes, g.n_int, g.units, g.ibuf / 4);
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)std::min((g.n_int + 3) / 4, 1L << 20)), dim3(256), 0, stream,
                       reinterpret_cast<const uint8_t*>(bits), ibytes, isize, g.n_int, g.ibuf);
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, stream, isize, apos, offsets, g.n_int, g.nby, base);
    return leod_launch_status();
}

LEOD_API int leod_jpeg_emit(const void* ws, long ws_bytes, int n, int H, int W, int quality, unsigned char* out, long out_bytes,
                            long base, hipStream_t stream) {
    if (!ws || !out || bad_geometry(n, H, W) || quality < 1 || quality > 100 || out_bytes < 0 || base < 0) return LEOD_ERR_ARG;
    const Geometry g = geometry(n, H, W);
    if (ws_bytes < g.total || (reinterpret_cast<uintptr_t>(ws) & 15)) return LEOD_ERR_ARG;
    Params P;
    build_params(P, H, W, quality);
    const uint8_t* w8 = static_cast<const uint8_t*>(ws);
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3((unsigned)std::min(g.n_int, 1L << 20)), dim3(256), 0, stream, w8 + g.bits,
                       reinterpret_cast<const int*>(w8 + g.ibytes), reinterpret_cast<const int*>(w8 + g.isize),
                       reinterpret_cast<const long*>(w8 + g.apos), out, out_bytes, base, P, g.n_int, g.nby, g.ibuf);
    return leod_launch_status();
}
