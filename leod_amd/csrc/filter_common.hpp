// What the record filters of the ingestion share (k_filter.hip, k_pixfilter.hip): the .dat record, the marks layout that
// leod_event_filter_emit reads (one class byte per record, padded to 8, then one u64 per tile: the offset of the tile's kept records;
// class 0 is "kept"), the io block of a scan call, and the wave / workgroup sums.
#pragma once
#include "common.hpp"

namespace filt {
constexpr int BLOCK = 256;
constexpr int TILE = BLOCK;                                      // one record per lane
constexpr int PASS = BLOCK;                                      // tile counts per pass of the scan workgroup
constexpr int C_KEPT = 0;
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

inline long marks_need(long n_events) {                          // class bytes, padded to 8, + one u64 per tile
    return (n_events + 7) / 8 * 8 + (n_events + TILE - 1) / TILE * 8L;
}
inline bool records_ok(const void* records, long n_events) {
    if (n_events < 0 || n_events > 0x7fffffffL) return false;
    return n_events == 0 || (records && (reinterpret_cast<uintptr_t>(records) & 7) == 0);
}
}  // namespace filt
