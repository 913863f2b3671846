// What the record filters of the ingestion and the filter survey share (k_filter.hip, k_pixfilter.hip, k_survey.hip): the .dat record, the marks layout that
// leod_event_filter_emit reads (one class byte per record, padded to 8, then one u64 per tile: the offset of the tile's kept records;
// class 0 is "kept"), the io block of a scan call, the wave / workgroup sums, and the three steps both filters take alike (classify,
// tally_classes, scan_tiles).  Their __global__ kernels stay in the .hip files: separate translation units, no relocatable device code.
#pragma once
#include "common.hpp"

namespace filt {
constexpr int BLOCK = 256;
constexpr int TILE = BLOCK;                                      // one record per lane
constexpr int PASS = BLOCK;                                      // tile counts per pass of the scan workgroup
enum { C_KEPT = 0, C_OUTSIDE = 1, C_MASKED = 2 };                // the classes both filters know; each adds its own from 3 on
enum { IO_EMITTED = 0, IO_BAD, IO_T_BEFORE, IO_T_AT };

struct Rec { unsigned t, xyp; };

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// exclusive prefix sum over the workgroup's lanes + the total; every lane must call it
__device__ __forceinline__ unsigned long long block_scan_sum(unsigned long long mine, unsigned long long& total, unsigned long long* lds /* [4] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long q = __shfl_up(inc, o, 64);
        if (lane >= o) inc += q;
    }
    __syncthreads();                                             // the previous use of lds is over
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned long long before = 0;
    total = 0;
    for (int w = 0; w < BLOCK / 64; ++w) {
        if (w < wave) before += lds[w];
        total += lds[w];
    }
    return before + inc - mine;
}

// What both filters decide about record i of a chunk before their own rule: its class -- outside the sensor, on a masked pixel, or a
// candidate (C_KEPT) -- its pixel (x, y), and the order check: a time below the one before it (rec[i - 1]; for i = 0 *t_last, the last
// time of the chunk before, -1: nothing seen yet) lowers io[IO_BAD] to i.  x, y are compared with W, H before they index the mask.
__device__ __forceinline__ int classify(const Rec* __restrict__ rec, long i, const long* __restrict__ t_last, int H, int W,
                                        const unsigned char* __restrict__ mask, long* __restrict__ io, Rec& e, int& x, int& y) {
    e = rec[i];
    const long before = i > 0 ? (long)rec[i - 1].t : *t_last;
    if ((long)e.t < before) atomicMin(reinterpret_cast<long long*>(io + IO_BAD), (long long)i);
    x = (int)(e.xyp & 16383u), y = (int)((e.xyp >> 14) & 16383u);
    return x >= W || y >= H ? C_OUTSIDE : mask && mask[(long)y * W + x] ? C_MASKED : C_KEPT;
}

// Records per class of a tile, classes 0 .. N - 1 (c = -1: a lane without a record): wave sums, N counts in LDS; the tile's kept count
// goes to *tile_kept (the scan turns the counts into offsets) and every count is added to counters[class].  Every lane must call it.
template <int N>
__device__ __forceinline__ void tally_classes(int c, unsigned long long* __restrict__ tile_kept, long* __restrict__ counters) {
    __shared__ unsigned lds_c[N];
    if (threadIdx.x < N) lds_c[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const unsigned n = wave_sum_u32(c == k ? 1u : 0u);
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(&lds_c[k], n);
    }
    __syncthreads();
    if (threadIdx.x == 0) *tile_kept = lds_c[C_KEPT];
    if (threadIdx.x < N && lds_c[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(counters + threadIdx.x), (unsigned long long)lds_c[threadIdx.x]);
}

// What ONE lane does last for the piece [lo, hi): the times around a decrease in the piece, state[SEEN] += hi - lo, state[T_LAST] = the
// last time.
template <int SEEN, int T_LAST>
__device__ __forceinline__ void close_piece(const Rec* __restrict__ rec, long lo, long hi, long* __restrict__ state, long* __restrict__ io) {
    const long bad = io[IO_BAD];
    if (bad >= lo && bad < hi) {
        io[IO_T_BEFORE] = bad > 0 ? (long)rec[bad - 1].t : state[T_LAST];
        io[IO_T_AT] = (long)rec[bad].t;
    }
    state[SEEN] += hi - lo;
    if (hi > lo) state[T_LAST] = (long)rec[hi - 1].t;
}

// The body of a scan kernel, ONE workgroup, for the piece [lo, hi): the tiles' kept counts -> offsets behind the records emitted so far,
// PASS tiles per pass; lane 0 then closes the piece (close_piece).
template <int SEEN, int T_LAST>
__device__ __forceinline__ void scan_tiles(const Rec* __restrict__ rec, long lo, long hi, long* __restrict__ state,
                                           unsigned long long* __restrict__ tile_off, long* __restrict__ io) {
    __shared__ unsigned long long lds_s[BLOCK / 64];
    unsigned long long base = (unsigned long long)io[IO_EMITTED];
    const long first = lo / TILE, end = (hi + TILE - 1) / TILE;
    __syncthreads();                                             // every lane has read io before lane 0 writes it
    for (long t0 = first; t0 < end; t0 += PASS) {
        const long tile = t0 + threadIdx.x;
        const unsigned long long n = tile < end ? tile_off[tile] : 0ULL;
        unsigned long long sum;
        const unsigned long long off = base + block_scan_sum(n, sum, lds_s);
        if (tile < end) tile_off[tile] = off;
        base += sum;
    }
    if (threadIdx.x == 0) {
        io[IO_EMITTED] = (long)base;
        close_piece<SEEN, T_LAST>(rec, lo, hi, state, io);
    }
}

inline long marks_need(long n_events) {                          // class bytes, padded to 8, + one u64 per tile
    return (n_events + 7) / 8 * 8 + (n_events + TILE - 1) / TILE * 8L;
}
inline bool records_ok(const void* records, long n_events) {
    if (n_events < 0 || n_events > 0x7fffffffL) return false;
    return n_events == 0 || (records && (reinterpret_cast<uintptr_t>(records) & 7) == 0);
}
}  // namespace filt
