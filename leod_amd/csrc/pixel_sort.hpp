// The stable per-pixel sort that the per-pixel filter (k_pixfilter.hip) and the filter survey (k_survey.hip) share: a least-significant-
// digit radix sort of (key, index) pairs on `bits` key bits, DIGIT bits a pass, three launches a pass:
//   pix_hist_kernel (digit counts per sort tile -- SORT_TILES tiles of records, a workgroup takes them a tile a round -- stored
//   digit-major), pix_hist_scan_kernel (ONE workgroup: the exclusive sum over [digit][sort tile], which is where each sort tile's run of
//   each digit starts), pix_scatter_kernel (rank of a record among its sort tile's earlier records of the same digit: the rounds before
//   it, the waves before it in its round, and a wave ballot -- no rank is the return value of an atomic, so the permutation is the same
//   in every run).
// Stable: records of one key stay in the order they came in, so with index = stream position a pixel's run is in stream order.
// The kernels have internal linkage: each .hip file that includes this header carries its own copy (separate translation units, no
// relocatable device code).  The workspace of a piece of `per` records (whole tiles): keys and indices, twice (ping-pong), then RADIX
// digit counts per sort tile; ws_of_tiles / tiles_of_ws are the piecewise policy both users apply to the ws_bytes they are given.
//
// Bounds: keys and indices are read below n only; a scatter position is compared with n before it is stored to.
#pragma once
#include "filter_common.hpp"

namespace filt {
namespace {
constexpr int DIGIT = 8;                                         // key bits per sort pass
constexpr int RADIX = 1 << DIGIT;                                // = BLOCK: lane d owns digit d of its tile's histogram
constexpr int SCAN_PER_LANE = 16;                                // histogram entries a lane of the scan workgroup takes per pass
constexpr int SORT_TILES = 8;                                    // tiles of records per workgroup of the sort: one digit count per 8 x 256 records
constexpr long WS_TILE = (long)TILE * 16;                        // keys and indices, twice (ping-pong)
constexpr long WS_HIST = (long)RADIX * 4;                        // the digit counts of one sort tile
static_assert(RADIX == BLOCK, "one lane per digit");

// digit counts of sort tile blockIdx.x -> hist[digit * n_stiles + sort tile]
__global__ __launch_bounds__(BLOCK) void pix_hist_kernel(const unsigned* __restrict__ key, long n, int shift, long n_stiles,
                                                         unsigned* __restrict__ hist) {
    __shared__ unsigned lds_h[RADIX];
    lds_h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_TILES; ++r) {
        const long j = ((long)blockIdx.x * SORT_TILES + r) * TILE + threadIdx.x;
        if (j < n) atomicAdd(&lds_h[(key[j] >> shift) & (RADIX - 1)], 1u);        // a count: the sum is the same in any order
    }
    __syncthreads();
    hist[(long)threadIdx.x * n_stiles + blockIdx.x] = lds_h[threadIdx.x];
}

// one workgroup: exclusive sum over the `total` entries of hist, in place
__global__ __launch_bounds__(BLOCK) void pix_hist_scan_kernel(unsigned* __restrict__ hist, long total) {
    __shared__ unsigned long long lds_s[BLOCK / 64];
    unsigned long long base = 0;
    for (long e0 = 0; e0 < total; e0 += (long)BLOCK * SCAN_PER_LANE) {
        const long mine = e0 + (long)threadIdx.x * SCAN_PER_LANE;
        unsigned v[SCAN_PER_LANE];
        unsigned long long s = 0;
#pragma unroll
        for (int k = 0; k < SCAN_PER_LANE; ++k) {
            v[k] = mine + k < total ? hist[mine + k] : 0u;
            s += v[k];
        }
        unsigned long long sum;
        unsigned long long off = base + block_scan_sum(s, sum, lds_s);
#pragma unroll
        for (int k = 0; k < SCAN_PER_LANE; ++k) {
            if (mine + k < total) hist[mine + k] = (unsigned)off;                // below the piece's size, which is below 2^31
            off += v[k];
        }
        base += sum;
    }
}

// a record goes to: the start of its sort tile's run of its digit + its rank among the sort tile's earlier records of that digit
__global__ __launch_bounds__(BLOCK) void pix_scatter_kernel(const unsigned* __restrict__ key_in, const unsigned* __restrict__ idx_in, long n,
                                                            int shift, long n_stiles, const unsigned* __restrict__ hist,
                                                            unsigned* __restrict__ key_out, unsigned* __restrict__ idx_out) {
    __shared__ unsigned lds_w[BLOCK / 64][RADIX];                                // records of digit d in wave w, this round
    __shared__ unsigned lds_run[RADIX];                                          // where the next record of digit d goes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lds_run[threadIdx.x] = hist[(long)threadIdx.x * n_stiles + blockIdx.x];
    for (int w = 0; w < BLOCK / 64; ++w) lds_w[w][threadIdx.x] = 0;
    for (int r = 0; r < SORT_TILES; ++r) {                                       // every lane takes every round: the barriers are uniform
        __syncthreads();
        const long j = ((long)blockIdx.x * SORT_TILES + r) * TILE + threadIdx.x;
        const bool valid = j < n;
        const unsigned k = valid ? key_in[j] : 0u, v = valid ? idx_in[j] : 0u;
        const unsigned d = (k >> shift) & (RADIX - 1);
        unsigned long long same = __ballot(valid);                               // the wave's lanes that hold a record of my digit
#pragma unroll
        for (int b = 0; b < DIGIT; ++b) {
            const unsigned long long has = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? has : ~has;
        }
        const unsigned rank = (unsigned)__popcll(same & ((1ULL << lane) - 1ULL));
        if (valid && rank == 0) lds_w[wave][d] = (unsigned)__popcll(same);       // the first lane of each digit: one store per digit
        __syncthreads();
        if (valid) {
            unsigned before = 0;
            for (int w = 0; w < wave; ++w) before += lds_w[w][d];
            const long pos = (long)lds_run[d] + before + rank;
            if (pos < n) {
                key_out[pos] = k;
                idx_out[pos] = v;
            }
        }
        __syncthreads();
        unsigned took = 0;                                                       // lane d owns column d: advance its run, clear its counts
        for (int w = 0; w < BLOCK / 64; ++w) {
            took += lds_w[w][threadIdx.x];
            lds_w[w][threadIdx.x] = 0;
        }
        lds_run[threadIdx.x] += took;
    }
}

inline int key_bits(long n_keys) {                               // ceil(log2(n_keys)): 0 for one key
    int bits = 0;
    while ((1L << bits) < n_keys) ++bits;
    return bits;
}
inline long ws_of_tiles(long tiles) {                            // a piece of so many tiles of records
    return tiles * WS_TILE + (tiles + SORT_TILES - 1) / SORT_TILES * WS_HIST;
}
inline long ws_need(long n_events) {                             // one piece that takes n_events records
    const long tiles = (n_events + TILE - 1) / TILE;
    return ws_of_tiles(tiles > 0 ? tiles : 1);
}
inline long tiles_of_ws(long ws_bytes) {                         // the largest piece the workspace takes: ws_of_tiles(it) <= ws_bytes
    const long groups = ws_bytes / (SORT_TILES * WS_TILE + WS_HIST), rest = ws_bytes - groups * (SORT_TILES * WS_TILE + WS_HIST);
    return groups * SORT_TILES + (rest >= WS_HIST ? (rest - WS_HIST) / WS_TILE : 0);
}

// The workspace of a piece of `per` records (a whole number of tiles), laid out: key[0], idx[0], key[1], idx[1], the digit counts.
struct SortWs {
    unsigned* key[2];
    unsigned* idx[2];
    unsigned* hist;
    SortWs(void* ws, long per) {
        unsigned* buf = static_cast<unsigned*>(ws);
        key[0] = buf; idx[0] = buf + per; key[1] = buf + 2 * per; idx[1] = buf + 3 * per;
        hist = buf + 4 * per;                                    // RADIX entries per sort tile of the piece
    }
};
// Sorts the n pairs in key[0] / idx[0] on `bits` key bits; -> which of the two buffers holds the result (0 or 1).
inline int sort_pairs(const SortWs& s, long n, int bits, hipStream_t stream) {
    const long n_tiles = (n + TILE - 1) / TILE, n_stiles = (n_tiles + SORT_TILES - 1) / SORT_TILES;
    const dim3 sgrid((unsigned)n_stiles), block(BLOCK);
    int cur = 0;
    for (int shift = 0; shift < bits; shift += DIGIT, cur ^= 1) {
        hipLaunchKernelGGL(pix_hist_kernel, sgrid, block, 0, stream, s.key[cur], n, shift, n_stiles, s.hist);
        hipLaunchKernelGGL(pix_hist_scan_kernel, dim3(1), block, 0, stream, s.hist, (long)RADIX * n_stiles);
        hipLaunchKernelGGL(pix_scatter_kernel, sgrid, block, 0, stream, s.key[cur], s.idx[cur], n, shift, n_stiles, s.hist, s.key[cur ^ 1],
                           s.idx[cur ^ 1]);
    }
    return cur;
}
}  // namespace
}  // namespace filt
