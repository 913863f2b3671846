// Recording ingestion (leod_voxelize_dat_windows): the raw 8-byte records of a Prophesee .dat file, as they lie in the file, to the
// stacked histograms of MANY windows per call.  leod_voxelize_u8 (k_misc.hip) makes one window per call from four int64 arrays (32
// bytes per event, a clear and two launches per window); a 60 s recording is 1 200 windows.  Here the windows are given as ascending
// event offsets win_off[n_win + 1] and processed in chunks of ws_windows: one clear, one count launch over the chunk's contiguous event
// range, one finalise launch per chunk.
//
// Record layout (Prophesee Event2D, utils/evaluation/prophesee/io/dat_events_tools.py:18-50): u32 t in microseconds, then one i32
// holding x in bits 0-13, y in bits 14-27 and p in bit 28.
//
// Arithmetic per window: exactly StackedHistogram.construct (data/utils/representations.py:78-123) on the window's events, i.e. the
// float expression of voxel_count_kernel (k_misc.hip): bin = floor(fp32(t - t0) / fp32(max(t1 - t0, 1)) * bins) clamped to bins - 1,
// t0 / t1 = first / last event time of the WINDOW.  The count launch finds an event's window by binary search in the chunk's slice of
// win_off (at most log2(ws_windows + 1) probes of a few hundred cached bytes), so the work per thread does not depend on how the events
// spread over the windows.  Counts are int32 global atomics on the chunk's workspace; the finalise pass applies the uint8 wrap (fast
// mode) or the int16 wrap + clamp at 0, then the cutoff.
//
// Bounds: an event whose x >= W or y >= H is skipped and counted in *dropped (leod_voxelize_u8 has no such check).  Offsets are clamped
// to [0, n_events] and the bin to [0, bins - 1] on the device, so that no content of records or win_off can make a thread touch memory
// outside records / the workspace.
#include "common.hpp"

namespace {
struct DatRecord { unsigned t; unsigned xyp; };

__device__ __forceinline__ long clamp_off(long v, long n) { return v < 0 ? 0 : (v > n ? n : v); }

// counts[(w - w_lo), p, bin, y, x] += 1 for every event of windows [w_lo, w_hi)
__global__ __launch_bounds__(256) void dat_count_kernel(const DatRecord* __restrict__ rec, long n_events, const long* __restrict__ win_off,
                                                        int w_lo, int w_hi, int* __restrict__ counts, int bins, int H, int W, int ds2,
                                                        unsigned long long* __restrict__ dropped) {
    const long lo = clamp_off(win_off[w_lo], n_events), hi = clamp_off(win_off[w_hi], n_events);
    const int Ho = ds2 ? H / 2 : H, Wo = ds2 ? W / 2 : W;
    const long plane = (long)Ho * Wo, per_win = 2L * bins * plane;
    for (long i = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (long)gridDim.x * blockDim.x) {
        // the last w in [w_lo, w_hi) with win_off[w] <= i: windows may be empty (equal offsets), the event belongs to the one that ends behind it
        int a = w_lo, b = w_hi - 1;
        while (a < b) {
            const int m = (a + b + 1) >> 1;
            if (win_off[m] <= i) a = m; else b = m - 1;
        }
        const long first = clamp_off(win_off[a], n_events - 1), last = clamp_off(win_off[a + 1], n_events) - 1;
        const DatRecord e = rec[i];
        const long t0 = rec[first].t, t1 = rec[last < first ? first : last].t;
        const int x = (int)(e.xyp & 16383u), y = (int)((e.xyp >> 14) & 16383u), p = (int)((e.xyp >> 28) & 1u);
        if (x >= W || y >= H) {
            if (dropped) atomicAdd(dropped, 1ULL);
            continue;
        }
        int xo = x, yo = y;
        if (ds2) {                                               // full[.., 1::2, 1::2]: what 'nearest-exact' at scale 0.5 selects
            if (!(x & 1) || !(y & 1)) continue;
            xo = x >> 1; yo = y >> 1;
        }
        // voxel_count_kernel (k_misc.hip), as it stands: (time - t0) [int64] / max(t1 - t0, 1) in fp32, * bins, floor, clamp
        const float denom = (float)max(t1 - t0, 1L);
        float tn = (float)((long)e.t - t0) / denom;
        tn = tn * (float)bins;
        long ti = (long)floorf(tn);
        if (ti > bins - 1) ti = bins - 1;
        if (ti < 0) ti = 0;                                      // only for times that run backwards inside a window: stay inside the workspace
        const long idx = xo + (long)Wo * yo + plane * ti + (long)bins * plane * p;
        atomicAdd(counts + (long)(a - w_lo) * per_win + idx, 1);
    }
}

__device__ __forceinline__ unsigned finalize_one(int c, int cutoff, int fastmode) {
    if (fastmode) c &= 255;                                      // uint8 accumulation wraps
    else { c = (int)(short)(c & 0xffff); if (c < 0) c = 0; }      // int16 accumulation, clamp(min=0)
    return (unsigned)min(c, cutoff);
}
// four counts -> four bytes per lane and step (n4 = n / 4; both pointers 16 / 4 byte aligned)
__global__ __launch_bounds__(256) void dat_finalize4_kernel(const int4* __restrict__ counts, unsigned* __restrict__ out, long n4, int cutoff,
                                                            int fastmode) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int4 c = counts[i];
        out[i] = finalize_one(c.x, cutoff, fastmode) | (finalize_one(c.y, cutoff, fastmode) << 8) |
                 (finalize_one(c.z, cutoff, fastmode) << 16) | (finalize_one(c.w, cutoff, fastmode) << 24);
    }
}
__global__ __launch_bounds__(256) void dat_finalize1_kernel(const int* __restrict__ counts, unsigned char* __restrict__ out, long n, int cutoff,
                                                            int fastmode) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = (unsigned char)finalize_one(counts[i], cutoff, fastmode);
}
}  // namespace

LEOD_API int leod_voxelize_dat_windows(const void* records, long n_events, const long* win_off, int n_win, int* counts_ws, int ws_windows,
                                       unsigned char* out, int bins, int H, int W, int ds2, int count_cutoff, int fastmode, long* dropped,
                                       hipStream_t stream) {
    if (n_win < 0 || n_events < 0 || bins < 1 || H < 1 || W < 1 || H > 16384 || W > 16384 || ws_windows < 1) return LEOD_ERR_ARG;
    if (ds2 && ((H | W) & 1)) return LEOD_ERR_ARG;
    if (n_win == 0) return LEOD_OK;
    if (!win_off || !counts_ws || !out || (n_events > 0 && !records)) return LEOD_ERR_ARG;
    const long per_win = 2L * bins * (ds2 ? H / 2 : H) * (ds2 ? W / 2 : W);
    const int cutoff = count_cutoff <= 0 ? 255 : min(count_cutoff, 255);
    const bool vec4 = per_win % 4 == 0 && (reinterpret_cast<uintptr_t>(counts_ws) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    for (int w_lo = 0; w_lo < n_win; w_lo += ws_windows) {
        const int nw = min(ws_windows, n_win - w_lo);
        const long n = per_win * nw;
        if (hipMemsetAsync(counts_ws, 0, n * sizeof(int), stream) != hipSuccess) return LEOD_ERR_LAUNCH;
        if (n_events > 0) {
            // the offsets live on the device: size the grid for the chunk's share of the events, the loop strides over whatever it really holds
            const long share = (n_events + n_win - 1) / n_win * nw;
            hipLaunchKernelGGL(dat_count_kernel, dim3((unsigned)max(1L, min(2048L, (share + 255) / 256))), dim3(256), 0, stream,
                               static_cast<const DatRecord*>(records), n_events, win_off, w_lo, w_lo + nw, counts_ws, bins, H, W, ds2,
                               reinterpret_cast<unsigned long long*>(dropped));
        }
        unsigned char* o = out + per_win * w_lo;
        if (vec4)
            hipLaunchKernelGGL(dat_finalize4_kernel, dim3((unsigned)min(2048L, (n / 4 + 255) / 256)), dim3(256), 0, stream,
                               reinterpret_cast<const int4*>(counts_ws), reinterpret_cast<unsigned*>(o), n / 4, cutoff, fastmode);
        else
            hipLaunchKernelGGL(dat_finalize1_kernel, dim3((unsigned)min(2048L, (n + 255) / 256)), dim3(256), 0, stream, counts_ws, o, n, cutoff,
                               fastmode);
        if (leod_launch_status() != LEOD_OK) return LEOD_ERR_LAUNCH;
    }
    return LEOD_OK;
}
