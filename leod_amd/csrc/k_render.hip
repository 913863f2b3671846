// Prediction-video frames (leod_render_frames_u8): the event representation of a recording, [L, 2*bins, H, W] uint8 or fp32, to RGB
// frames [L, up*H, up*W, 3] uint8 (HWC, what a PNG row is) with box outlines and text drawn in the same pass.  The reference does the
// base image with torch ops on the device (vis_pred.py:74-93: sum, mask, fp32 canvas, F.interpolate x2, round) and the drawing on the host
// with OpenCV, frame by frame (vis_pred.py:126-215).
//
// Two launches, no allocation:
//   1. mask pass    ev -> ws[L, H, W] bytes, 1 where any of the 2*bins channels is > 0.  Reads every input byte once: 16-byte words where
//                   H*W and the addresses allow, 4-byte words where those allow, bytes otherwise (a frame's planes are flat arrays here,
//                   so the row length itself does not matter).
//   2. render pass  every output pixel once: base value from the mask, then the overlay items of ITS frame in item order, the later item
//                   winning; one store per output byte, no read-modify-write, no atomics.  Four pixels of one row per thread (three
//                   32-bit words, consecutive lanes consecutive addresses) where the output row is a multiple of four pixels, one pixel
//                   per thread otherwise.  blockIdx.y is the frame; a block first drops the items whose boxes miss the few rows it
//                   covers (one item per thread; ballot + prefix put the survivors into LDS in item order), then every thread visits
//                   the survivors in that order.
//
// Base image, exact in integers.  A pixel with events is 0.25, any other 1.0; bilinear x2 with align_corners=False has the quarter
// weights (4,0) at output index 0, (3,1) on taps (o/2, o/2+1) for odd o and (1,3) on taps (o/2-1, o/2) for even o >= 2, the second tap
// clamped to n-1.  With K = sum wy*wx*m in [0,16]: value*255 = 255 (1 - 0.75 K/16) = (16320 - 765 K)/64.  A tie would need
// 765 K = 32 (mod 64), i.e. K = 32 (mod 64) as 765 is odd, and K <= 16: there is none, so byte = (16320 - 765 K + 32) >> 6 is the
// rounded value whatever the rounding rule.  up = 1: m ? 64 : 255.
//
// Overlay items, int32[8] = {frame, kind, x, y, a, b, c, rgb}, rgb = r | g<<8 | b<<16, coordinates in output pixels:
//   kind 0  rectangle outline, corners (x,y)-(a,b) in any order, thickness c >= 1; with p = c/2, q = (c-1)/2 a pixel is on the outline
//           if it lies in [x-p, a+q] x [y-p, b+q] and not in [x+q+1, a-p-1] x [y+q+1, b-p-1].
//   kind 1  text line, (x,y) = bottom-left, integer scale a >= 1, bytes text[b .. b+c-1]; glyph bit (row r from the top, column k) of
//           character j covers the a x a block at (x + (6j+k)a, y - 7a + r a); a byte outside 0x20-0x7E is a solid 5 x 7 block.
// Everything is clipped to the image by construction (a pixel asks the items, no item writes).  Items with a scale / thickness outside
// [1, 65536] or a text range outside the buffer are skipped / drawn as solid blocks here; ops.render_frames refuses them before upload.
#include "common.hpp"
#include "render_font5x7.hpp"

namespace {
const unsigned char h_font5x7[LEOD_FONT5X7_GLYPHS * 7] = {LEOD_FONT5X7_DATA};
__constant__ unsigned char d_font5x7[LEOD_FONT5X7_GLYPHS * 7] = {LEOD_FONT5X7_DATA};

__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v) {          // 0x01 in every byte lane of v that is not zero
    v |= v >> 4; v |= v >> 2; v |= v >> 1;
    return v & 0x01010101u;
}

// one unit = sizeof(V) consecutive bytes of a frame's flat [H*W] plane; units_per_frame = H*W / sizeof(V)
template <typename V>
__global__ __launch_bounds__(256) void render_mask_u8_kernel(const uint8_t* __restrict__ ev, uint8_t* __restrict__ mask, long units,
                                                             long units_per_frame, int C2, long plane) {
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long)gridDim.x * 256) {
        const long f = u / units_per_frame, p = (u - f * units_per_frame) * (long)sizeof(V);
        const uint8_t* src = ev + f * C2 * plane + p;
        if constexpr (sizeof(V) == 16) {
            uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll 4
            for (int c = 0; c < C2; ++c) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + c * plane);
                acc.x |= v.x; acc.y |= v.y; acc.z |= v.z; acc.w |= v.w;
            }
            *reinterpret_cast<uint4*>(mask + f * plane + p) =
                make_uint4(nonzero_bytes(acc.x), nonzero_bytes(acc.y), nonzero_bytes(acc.z), nonzero_bytes(acc.w));
        } else if constexpr (sizeof(V) == 4) {
            uint32_t acc = 0;
#pragma unroll 4
            for (int c = 0; c < C2; ++c) acc |= *reinterpret_cast<const uint32_t*>(src + c * plane);
            *reinterpret_cast<uint32_t*>(mask + f * plane + p) = nonzero_bytes(acc);
        } else {
            uint32_t acc = 0;
#pragma unroll 4
            for (int c = 0; c < C2; ++c) acc |= src[c * plane];
            mask[f * plane + p] = acc ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(256) void render_mask_f32_kernel(const float* __restrict__ ev, uint8_t* __restrict__ mask, long units,
                                                              int C2, long plane) {
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long)gridDim.x * 256) {
        const long f = u / plane, p = u - f * plane;
        const float* src = ev + f * C2 * plane + p;
        bool any = false;
#pragma unroll 4
        for (int c = 0; c < C2; ++c) any = any || src[c * plane] > 0.0f;
        mask[u] = any ? 1 : 0;
    }
}

// taps of output index o along an axis of n source pixels: sources s0 <= s1, weights (w0, 4 - w0) in quarters
__device__ __forceinline__ void taps_x2(int o, int n, int& s0, int& s1, int& w0) {
    if (o == 0) { s0 = 0; w0 = 4; }
    else if (o & 1) { s0 = o >> 1; w0 = 3; }
    else { s0 = (o >> 1) - 1; w0 = 1; }
    s1 = min(s0 + 1, n - 1);
}

__device__ __forceinline__ uint32_t base_byte(const uint8_t* __restrict__ m, int H, int W, int up, int oy, int ox) {
    if (up == 1) return m[(long)oy * W + ox] ? 64u : 255u;
    int y0, y1, wy, x0, x1, wx;
    taps_x2(oy, H, y0, y1, wy);
    taps_x2(ox, W, x0, x1, wx);
    const uint8_t* r0 = m + (long)y0 * W;
    const uint8_t* r1 = m + (long)y1 * W;
    const int K = wy * (wx * r0[x0] + (4 - wx) * r0[x1]) + (4 - wy) * (wx * r1[x0] + (4 - wx) * r1[x1]);
    return (uint32_t)(16320 - 765 * K + 32) >> 6;
}

struct Item { int frame, kind, x, y, a, b, c, rgb; };

// the item's bounding box in output pixels (inclusive); false: the item draws nothing
__device__ __forceinline__ bool item_bounds(const Item& it, long& bx0, long& by0, long& bx1, long& by1) {
    if (it.kind == 0) {
        if (it.c < 1 || it.c > 65536) return false;
        const int p = it.c / 2, q = (it.c - 1) / 2;
        bx0 = (long)min(it.x, it.a) - p; bx1 = (long)max(it.x, it.a) + q;
        by0 = (long)min(it.y, it.b) - p; by1 = (long)max(it.y, it.b) + q;
        return true;
    }
    if (it.kind == 1) {
        if (it.a < 1 || it.a > 65536 || it.c < 1) return false;           // (one glyph pixel of scale 65536 is larger than any frame)
        bx0 = it.x; bx1 = (long)it.x + 6L * it.a * it.c - 1;
        by0 = (long)it.y - 7L * it.a; by1 = (long)it.y - 1;
        return true;
    }
    return false;
}

// does the item cover pixel (px, py)?  Only called for pixels inside item_bounds.
__device__ __forceinline__ bool item_hits(const Item& it, int px, int py, const uint8_t* __restrict__ text, int n_text) {
    if (it.kind == 0) {
        const int p = it.c / 2, q = (it.c - 1) / 2;
        const long ix0 = (long)min(it.x, it.a) + q + 1, ix1 = (long)max(it.x, it.a) - p - 1;
        const long iy0 = (long)min(it.y, it.b) + q + 1, iy1 = (long)max(it.y, it.b) - p - 1;
        return !(px >= ix0 && px <= ix1 && py >= iy0 && py <= iy1);
    }
    // inside the box 0 <= dx < 6 a c and 0 <= dy < 7 a hold, and a <= 65536 (item_bounds): 32-bit modular arithmetic gives exactly these
    const uint32_t a = (uint32_t)it.a, dx = (uint32_t)px - (uint32_t)it.x, dy = (uint32_t)py - (uint32_t)it.y + 7u * a;
    const uint32_t cell = 6u * a, j = dx / cell, k = (dx - j * cell) / a, r = dy / a;
    if (k >= 5) return false;                                             // the one-column gap between characters
    const long ti = (long)it.b + (long)j;
    const int ch = (ti >= 0 && ti < n_text) ? text[ti] : 0;
    const uint32_t row = (ch >= 0x20 && ch <= 0x7E && r < 7u) ? d_font5x7[(ch - 0x20) * 7 + r] : 0x1Fu;
    return (row >> (4u - k)) & 1u;
}

// A block renders R x 256 groups of PX pixels of one frame per step of its loop: with items (ITEMS) R = RENDER_ROUNDS, enough pixels for
// the item culling below to pay; the instantiations without items have R = 1, no overlay code and no LDS (fewer registers, more waves in
// flight: the pass is then nothing but loads and stores) and are launched only when the call has no items
constexpr int RENDER_ROUNDS = 4;

template <int PX, bool ITEMS>                                             // PX = 4: four pixels of one row per thread (Wo % 4 == 0), PX = 1: one
__global__ __launch_bounds__(256) void render_frames_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, int L, int H, int W,
                                                            int up, const int* __restrict__ frame_off, const Item* __restrict__ items,
                                                            int n_items, const uint8_t* __restrict__ text, int n_text) {
    constexpr int R = ITEMS ? RENDER_ROUNDS : 1;
    const int Ho = up * H, Wo = up * W;
    const long groups = (long)Ho * Wo / PX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int f = blockIdx.y; f < L; f += gridDim.y) {
        const uint8_t* m = mask + (long)f * H * W;
        uint8_t* o = out + (long)f * Ho * Wo * 3;
        int i0 = 0, i1 = 0;
        if (ITEMS && n_items > 0) {
            i0 = min(max(frame_off[f], 0), n_items);
            i1 = min(max(frame_off[f + 1], i0), n_items);
        }
        // every thread of the block takes part in every step (barriers below); a thread past the end computes a pixel again and stores nothing
        for (long g0 = (long)blockIdx.x * (256 * R); g0 < groups; g0 += (long)gridDim.x * (256 * R)) {
            const long g_end = min(g0 + 256 * R, groups);
            int oy[R], ox[R];
            bool active[R];
            uint32_t rgb[R][PX];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const long g = g0 + r * 256 + tid;
                active[r] = g < g_end;
                const uint32_t pix = (uint32_t)(active[r] ? g : groups - 1) * PX;       // < 2^30: a frame is at most 32767 x 32767
                oy[r] = (int)(pix / (uint32_t)Wo);
                ox[r] = (int)(pix - (uint32_t)oy[r] * (uint32_t)Wo);
#pragma unroll
                for (int k = 0; k < PX; ++k) rgb[r][k] = base_byte(m, H, W, up, oy[r], ox[r] + k) * 0x010101u;
            }
            if constexpr (ITEMS) if (i1 > i0) {
                __shared__ Item s_item[256];                              // the items that can touch this block's pixels, in item order
                __shared__ int4 s_box[256];                               // ... and their bounding boxes, clamped to [-1, Wo] x [-1, Ho]
                __shared__ int s_count[4];
                // rows this step of the block covers: an item whose box misses them is dropped for the whole block, 256 items at a time (one
                // per thread; ballot + prefix keep the survivors in item order in LDS), so the later item still wins
                const int row_lo = (int)(g0 * PX / Wo), row_hi = (int)((g_end * PX - 1) / Wo);
                for (int base = i0; base < i1; base += 256) {
                    bool live = false;
                    Item mine;
                    int4 box = make_int4(0, 0, 0, 0);
                    if (base + tid < i1) {
                        mine = items[base + tid];
                        long bx0, by0, bx1, by1;
                        live = item_bounds(mine, bx0, by0, bx1, by1) && by1 >= row_lo && by0 <= row_hi && bx1 >= 0 && bx0 < Wo;
                        if (live)
                            box = make_int4((int)max(bx0, -1L), (int)max(by0, -1L), (int)min(bx1, (long)Wo), (int)min(by1, (long)Ho));
                    }
                    const unsigned long long wave_live = __ballot(live);
                    __syncthreads();                                      // the previous list has been read by everyone
                    if (lane == 0) s_count[wave] = __popcll(wave_live);
                    __syncthreads();
                    int pos = __popcll(wave_live & ((1ULL << lane) - 1ULL)), n_live = 0;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        pos += w < wave ? s_count[w] : 0;
                        n_live += s_count[w];
                    }
                    if (live) { s_item[pos] = mine; s_box[pos] = box; }
                    __syncthreads();
                    for (int n = 0; n < n_live; ++n) {
                        const int4 bx = s_box[n];
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            if (oy[r] < bx.y || oy[r] > bx.w || ox[r] + PX - 1 < bx.x || ox[r] > bx.z) continue;
                            const Item it = s_item[n];
#pragma unroll
                            for (int k = 0; k < PX; ++k)
                                if (ox[r] + k >= bx.x && ox[r] + k <= bx.z && item_hits(it, ox[r] + k, oy[r], text, n_text))
                                    rgb[r][k] = (uint32_t)it.rgb & 0xFFFFFFu;
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (!active[r]) continue;
                const long pix = (g0 + r * 256 + tid) * PX;
                if constexpr (PX == 4) {                                  // 12 bytes r g b r | g b r g | b r g b, little endian
                    uint32_t* dst = reinterpret_cast<uint32_t*>(o + pix * 3);
                    dst[0] = rgb[r][0] | (rgb[r][1] << 24);
                    dst[1] = (rgb[r][1] >> 8) | (rgb[r][2] << 16);
                    dst[2] = (rgb[r][2] >> 16) | (rgb[r][3] << 8);
                } else {
                    o[pix * 3] = (uint8_t)rgb[r][0];
                    o[pix * 3 + 1] = (uint8_t)(rgb[r][0] >> 8);
                    o[pix * 3 + 2] = (uint8_t)(rgb[r][0] >> 16);
                }
            }
        }
    }
}

inline bool aligned(const void* p, unsigned n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
}  // namespace

LEOD_API int leod_render_font(unsigned char* dst) {
    if (!dst) return LEOD_ERR_ARG;
    for (int i = 0; i < LEOD_FONT5X7_GLYPHS * 7; ++i) dst[i] = h_font5x7[i];
    return LEOD_OK;
}

LEOD_API int leod_render_frames_u8(const void* ev, int ev_is_f32, unsigned char* out, int L, int C2, int H, int W, int up,
                                   const int* frame_off, const int* items, int n_items, const unsigned char* text, int n_text,
                                   unsigned char* ws, hipStream_t stream) {
    if (!ev || !out || !ws || L <= 0 || C2 <= 0 || (C2 & 1) || H <= 0 || W <= 0 || (up != 1 && up != 2) || n_items < 0 || n_text < 0)
        return LEOD_ERR_ARG;
    if (n_items > 0 && (!frame_off || !items)) return LEOD_ERR_ARG;
    if ((long)up * H > 32767 || (long)up * W > 32767) return LEOD_ERR_UNSUPPORTED;   // pixel indices of one frame stay far inside int32
    if (!text) n_text = 0;
    const long plane = (long)H * W;
    if (ev_is_f32) {
        const long units = (long)L * plane;
        hipLaunchKernelGGL(render_mask_f32_kernel, dim3(min(cdiv(units, 256), 8192)), dim3(256), 0, stream, (const float*)ev, ws, units, C2,
                           plane);
    } else {
        const uint8_t* e8 = (const uint8_t*)ev;
        if (plane % 16 == 0 && aligned(ev, 16) && aligned(ws, 16)) {
            const long upf = plane / 16, units = L * upf;
            hipLaunchKernelGGL(render_mask_u8_kernel<uint4>, dim3(min(cdiv(units, 256), 8192)), dim3(256), 0, stream, e8, ws, units, upf, C2,
                               plane);
        } else if (plane % 4 == 0 && aligned(ev, 4) && aligned(ws, 4)) {
            const long upf = plane / 4, units = L * upf;
            hipLaunchKernelGGL(render_mask_u8_kernel<uint32_t>, dim3(min(cdiv(units, 256), 8192)), dim3(256), 0, stream, e8, ws, units, upf,
                               C2, plane);
        } else {
            const long units = L * plane;
            hipLaunchKernelGGL(render_mask_u8_kernel<uint8_t>, dim3(min(cdiv(units, 256), 8192)), dim3(256), 0, stream, e8, ws, units, plane,
                               C2, plane);
        }
    }
    if (hipGetLastError() != hipSuccess) return LEOD_ERR_LAUNCH;
    const long opix = (long)up * H * up * W;
    const Item* its = reinterpret_cast<const Item*>(items);
    const unsigned gy = (unsigned)min(L, 65535);
    const bool quads = (up * W) % 4 == 0 && aligned(out, 4);             // every frame then starts on a word as well (12 bytes per group)
    const long groups = quads ? opix / 4 : opix;
    const int rounds = n_items > 0 ? RENDER_ROUNDS : 1;
    const dim3 grid(min(cdiv(groups, 256 * rounds), 1024), gy);
#define LEOD_RENDER_LAUNCH(PX, ITEMS)                                                                                                 \
    hipLaunchKernelGGL((render_frames_kernel<PX, ITEMS>), grid, dim3(256), 0, stream, ws, out, L, H, W, up, frame_off, its, n_items, text, n_text)
    if (quads) {
        if (n_items > 0) LEOD_RENDER_LAUNCH(4, true); else LEOD_RENDER_LAUNCH(4, false);
    } else {
        if (n_items > 0) LEOD_RENDER_LAUNCH(1, true); else LEOD_RENDER_LAUNCH(1, false);
    }
#undef LEOD_RENDER_LAUNCH
    return leod_launch_status();
}
