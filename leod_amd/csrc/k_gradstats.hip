// Per-parameter statistics of the flat gradient buffer in ONE segmented pass (leod_grad_stats): for every segment (= parameter) the sums of
// |g| and g*g and the largest |g| over its FINITE elements, the number of non-finite ones, and the non-finite total over all segments.
// The reference gets the first from one torch reduction + one host read-back per parameter (callbacks/gradflow.py, callbacks/utils/
// visualization.py:5-23: grad.abs().mean() of ~400 tensors) and the last from GradScaler's inf check before the optimiser step
// (train.py:243, precision 16); here the total feeds leod_adamw_clip_step_guarded (k_misc.hip) without leaving the device.
//
// Shape: segments are cut into chunks of GRAD_STATS_CHUNK floats (host-built chunk -> segment map, so a chunk never straddles two
// segments and the padding between parameters is never read into one); one 256-thread workgroup per chunk reads 16 bytes per lane
// (segment starts are 16-byte aligned, the tail is masked), accumulates in double from the first add, reduces by __shfl_down over the 64
// lanes and over its four waves through LDS in a fixed order and writes one record; a second launch folds the records of a segment with
// one wave, again in a fixed order.  No floating-point atomics anywhere: results are bit-identical from run to run.  The pass reads
// 4 bytes per element (the AdamW pass moves 28).
#include "common.hpp"
#include <limits.h>
#pragma clang fp contract(off)

namespace {
constexpr int GRAD_STATS_CHUNK = 8192;                           // floats per chunk: 8 x (256 lanes x 16 bytes)
struct GradRec { double sum_abs, sum_sq, max_abs; long nonfinite; };

struct GradAcc {
    double sa = 0.0, sq = 0.0;
    float mx = 0.f;
    int nf = 0;
    __device__ __forceinline__ void add(float x) {
        const unsigned b = __builtin_bit_cast(unsigned, x);
        const bool fin = (b & 0x7f800000u) != 0x7f800000u;       // exponent bits all ones: inf or NaN
        const float a = __builtin_bit_cast(float, b & 0x7fffffffu);
        const double d = fin ? (double)a : 0.0;
        sa += d;
        sq += d * d;                                             // the product of two fp32 values is exact in double
        mx = fin ? fmaxf(mx, a) : mx;
        nf += fin ? 0 : 1;
    }
};
// lane 0 ends up with the fold of the 64 lanes, always in the same order
__device__ __forceinline__ void wave_fold(double& sa, double& sq, double& mx, long& nf) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_down(sa, o, 64);
        sq += __shfl_down(sq, o, 64);
        mx = fmax(mx, __shfl_down(mx, o, 64));
        nf += __shfl_down(nf, o, 64);
    }
}
}  // namespace

// seg [nseg][3] = {offset, length, index of the segment's first chunk}; chunk [nchunk][2] = {segment, chunk index within the segment}.
// The host entry validated the HOST copy of the segment table; the device tables are re-checked here, so that tables that do not
// belong together give an empty chunk, never an address outside g[0, n).
__global__ __launch_bounds__(256) void grad_stats_chunk_kernel(const float* __restrict__ g, long n, const long* __restrict__ seg, int nseg,
                                                               const int* __restrict__ chunk, long nchunk, GradRec* __restrict__ rec,
                                                               int* __restrict__ total) {
    __shared__ double s_sa[4], s_sq[4], s_mx[4];
    __shared__ long s_nf[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0 && tid == 0) *total = 0;                 // the fold launch behind this one adds the per-segment counts
    for (long c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int s = chunk[2 * c], k = chunk[2 * c + 1];
        long start = 0, len = 0;
        if (s >= 0 && s < nseg && k >= 0) {
            const long off = seg[3 * s], sl = seg[3 * s + 1], rel = (long)k * GRAD_STATS_CHUNK;
            if (off >= 0 && (off & 3) == 0 && off <= n && sl <= n - off && sl > rel) {
                start = off + rel;
                len = min((long)GRAD_STATS_CHUNK, sl - rel);
            }
        }
        const float* p = g + start;
        GradAcc acc;
        for (long i = 4L * tid; i < len; i += 4 * 256) {
            if (i + 4 <= len) {
                const f4 v = ld4(p + i);
                acc.add(v.x); acc.add(v.y); acc.add(v.z); acc.add(v.w);
            } else {
                for (long j = i; j < len; ++j) acc.add(p[j]);    // the segment's last, partial quad: nothing behind `len` is read
            }
        }
        double sa = acc.sa, sq = acc.sq, mx = (double)acc.mx;
        long nf = acc.nf;
        wave_fold(sa, sq, mx, nf);
        if (lane == 0) { s_sa[wave] = sa; s_sq[wave] = sq; s_mx[wave] = mx; s_nf[wave] = nf; }
        __syncthreads();
        if (tid == 0) {
            GradRec r{s_sa[0], s_sq[0], s_mx[0], s_nf[0]};
            for (int w = 1; w < 4; ++w) { r.sum_abs += s_sa[w]; r.sum_sq += s_sq[w]; r.max_abs = fmax(r.max_abs, s_mx[w]); r.nonfinite += s_nf[w]; }
            rec[c] = r;
        }
        __syncthreads();
    }
}

// one wave per segment: lane l folds records l, l + 64, ... of the segment, then the lanes fold in the order of wave_fold
__global__ __launch_bounds__(64) void grad_stats_fold_kernel(const GradRec* __restrict__ rec, const long* __restrict__ seg, int nseg, long nchunk,
                                                             double* __restrict__ stats, int* __restrict__ nonfinite, int* __restrict__ total) {
    const int lane = threadIdx.x;
    for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
        const long sl = seg[3 * s + 1], first = seg[3 * s + 2];
        long cnt = sl >= 1 ? (sl + GRAD_STATS_CHUNK - 1) / GRAD_STATS_CHUNK : 0;
        if (first < 0 || first > nchunk || cnt > nchunk - first) cnt = 0;
        double sa = 0.0, sq = 0.0, mx = 0.0;
        long nf = 0;
        for (long r = lane; r < cnt; r += 64) {
            const GradRec x = rec[first + r];
            sa += x.sum_abs; sq += x.sum_sq; mx = fmax(mx, x.max_abs); nf += x.nonfinite;
        }
        wave_fold(sa, sq, mx, nf);
        if (lane == 0) {
            stats[3 * s] = sa; stats[3 * s + 1] = sq; stats[3 * s + 2] = mx;
            nonfinite[s] = (int)nf;
            if (nf) atomicAdd(total, (int)nf);                   // integer: the order of arrival does not show in the sum
        }
    }
}

LEOD_API int leod_grad_stats_query(long nchunk, int* chunk_floats, long* ws_bytes) {
    if (nchunk < 0) return LEOD_ERR_ARG;
    if (chunk_floats) *chunk_floats = GRAD_STATS_CHUNK;
    if (ws_bytes) *ws_bytes = nchunk * (long)sizeof(GradRec);
    return LEOD_OK;
}

LEOD_API int leod_grad_stats(const float* g, long n, const long* seg_host, const long* seg_dev, int nseg, const int* chunk_dev, long nchunk,
                             void* ws, double* stats, int* nonfinite, int* total, hipStream_t stream) {
    if (!total || nseg < 0) return LEOD_ERR_ARG;
    if (nseg == 0) return hipMemsetAsync(total, 0, sizeof(int), stream) == hipSuccess ? LEOD_OK : LEOD_ERR_LAUNCH;
    if (!g || !seg_host || !seg_dev || !chunk_dev || !ws || !stats || !nonfinite || n < 1 || n > INT_MAX) return LEOD_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(g) & 15) || (reinterpret_cast<uintptr_t>(ws) & 7)) return LEOD_ERR_ARG;
    long end = 0, chunks = 0;
    for (int s = 0; s < nseg; ++s) {                             // ascending, disjoint, 16-byte aligned starts, inside g[0, n), chunks in order
        const long off = seg_host[3 * s], len = seg_host[3 * s + 1];
        if (off < end || (off & 3) || len < 1 || off > n || len > n - off || seg_host[3 * s + 2] != chunks) return LEOD_ERR_ARG;
        end = off + len;
        chunks += (len + GRAD_STATS_CHUNK - 1) / GRAD_STATS_CHUNK;
    }
    if (chunks != nchunk) return LEOD_ERR_ARG;
    hipLaunchKernelGGL(grad_stats_chunk_kernel, dim3((unsigned)min(nchunk, 8192L)), dim3(256), 0, stream, g, n, seg_dev, nseg, chunk_dev, nchunk,
                       reinterpret_cast<GradRec*>(ws), total);
    if (leod_launch_status() != LEOD_OK) return LEOD_ERR_LAUNCH;
    hipLaunchKernelGGL(grad_stats_fold_kernel, dim3((unsigned)min(nseg, 4096)), dim3(64), 0, stream, reinterpret_cast<const GradRec*>(ws), seg_dev,
                       nseg, nchunk, stats, nonfinite, total);
    return leod_launch_status();
}
