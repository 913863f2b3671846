// Per-pixel event filters at ingestion (rule: DESIGN.md section 1): trail / STC (position of an event in a burst of same-polarity events
// of its pixel) and anti-flicker (consecutive in-band periods between a pixel's rising edges), on the 8-byte records of a .dat file in
// stream order with t non-decreasing.  Both rules are SEQUENTIAL per pixel -- the verdict on an event depends on the state its pixel's
// earlier candidates left -- and independent between pixels.  Since t is sorted, a pixel's order is index order, so a piece of records
// [lo, hi) of a chunk takes
//   (a) pix_classify_kernel: class per record (outside / masked / candidate), sortedness, and the sort's input: key = the pixel y * W + x
//       of a candidate (0 for any other record; the walk skips those by their class), value = the record's index;
//   (b) a STABLE least-significant-digit radix sort of (key, index) on ceil(log2(H * W)) key bits, DIGIT bits a pass, three launches a
//       pass: pix_hist_kernel (digit counts per sort tile -- SORT_TILES tiles of records, a workgroup takes them a tile a round --
//       stored digit-major), pix_hist_scan_kernel (ONE workgroup: the exclusive sum over [digit][sort tile], which is where each sort
//       tile's run of each digit starts), pix_scatter_kernel (rank of a record among its sort tile's earlier records of the same
//       digit: the rounds before it, the waves before it in its round, and a wave ballot -- no rank is the return value of an atomic,
//       so the permutation is the same in every run);
//   (c) pix_walk_kernel: the lane at the first sorted position of a pixel walks that pixel's run in index order with the pixel's state in
//       registers, writes the class byte of every candidate and stores the state.  One lane walks a whole run: the cost is linear in
//       the run, also when every event of the piece lies on one pixel;
//   (d) pix_count_kernel: kept records per tile and the five counters; (e) pix_scan_kernel, ONE workgroup: offsets of the tiles' kept
//       records, PASS tiles per pass; seen, the last time, the times around a decrease.
// The marks are those of k_filter.hip (class 0 = kept), so leod_event_filter_emit stores the kept records.  Launches run in stream order; no
// workgroup waits on another; every loop is bounded by the piece.  A chunk larger than the workspace allows is cut into pieces of whole
// tiles: the state block in memory carries the pixels from piece to piece as it does from chunk to chunk.
//
// Bounds: records are read below n_events only; x, y are compared with W, H before they index the mask or form a key, so a key is below
// H * W and indexes the state block; the sort's values are the indices the classify pass wrote (lo <= index < hi); a scatter position
// is compared with the piece's size before it is stored to; the entry points refuse buffers smaller than leod_pixel_filter_query reports.
#include "filter_common.hpp"

namespace {
using namespace filt;
constexpr int DIGIT = 8;                                         // key bits per sort pass
constexpr int RADIX = 1 << DIGIT;                                // = BLOCK: lane d owns digit d of its tile's histogram
constexpr int SCAN_PER_LANE = 16;                                // histogram entries a lane of the scan workgroup takes per pass
constexpr int SORT_TILES = 8;                                    // tiles of records per workgroup of the sort: one digit count per 8 x 256 records
constexpr long WS_TILE = (long)TILE * 16;                        // keys and indices, twice (ping-pong)
constexpr long WS_HIST = (long)RADIX * 4;                        // the digit counts of one sort tile
enum { C_FLICKER = 3, C_BURST = 4, N_CLASS = 5 };                // behind C_KEPT (a candidate until the walk decides), C_OUTSIDE, C_MASKED
enum { S_SEEN = 0, S_KEPT, S_OUTSIDE, S_MASKED, S_FLICKER, S_BURST, S_T_LAST, S_HEAD = 8 };      // state block: include/leod_hip.h
enum { P_T_PREV = 0, P_T_EDGE, P_PK, P_N_PER, P_LONGS };         // per pixel, behind the head
enum { KEEP_FIRST = 0, KEEP_SECOND = 1, KEEP_FROM_SECOND = 2 };
static_assert(RADIX == BLOCK, "one lane per digit");

struct Rule { long tau; int keep; long p_min, p_max; int lock; };         // tau -1: the burst family is off; lock 0: flicker is off

// (a)
__global__ __launch_bounds__(BLOCK) void pix_classify_kernel(const Rec* __restrict__ rec, long lo, long hi, int H, int W,
                                                             const unsigned char* __restrict__ mask, const long* __restrict__ state,
                                                             unsigned char* __restrict__ cls, unsigned* __restrict__ key,
                                                             unsigned* __restrict__ idx, long* __restrict__ io) {
    const long i = lo + (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= hi) return;
    Rec e; int x, y;
    const int c = classify(rec, i, state + S_T_LAST, H, W, mask, io, e, x, y);
    cls[i] = (unsigned char)c;
    key[i - lo] = c == C_KEPT ? (unsigned)y * (unsigned)W + (unsigned)x : 0u;     // H * W <= 2^28
    idx[i - lo] = (unsigned)i;
}

// (b) digit counts of sort tile blockIdx.x -> hist[digit * n_stiles + sort tile]
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

// (c) the rule, steps (a) to (f) of DESIGN.md section 1, for the run of one pixel
__global__ __launch_bounds__(BLOCK) void pix_walk_kernel(const Rec* __restrict__ rec, long lo, long hi, const unsigned* __restrict__ key,
                                                         const unsigned* __restrict__ idx, Rule r, unsigned char* __restrict__ cls,
                                                         long* __restrict__ state) {
    const long n = hi - lo, j0 = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (j0 >= n) return;
    const unsigned pix = key[j0];
    if (j0 > 0 && key[j0 - 1] == pix) return;                                    // not the head of a run
    long* st = state + S_HEAD + (long)pix * P_LONGS;
    long t_prev = st[P_T_PREV], t_edge = st[P_T_EDGE], n_per = st[P_N_PER];
    int p_prev = (int)(st[P_PK] & 1), k_prev = (int)(st[P_PK] >> 1);
    bool any = false;
    for (long j = j0; j < n && key[j] == pix; ++j) {
        const long i = (long)idx[j];
        if (i < lo || i >= hi || cls[i] != C_KEPT) continue;                     // an outside or masked record: it touches no state
        const Rec e = rec[i];
        const long t = (long)e.t;
        const int p = (int)((e.xyp >> 28) & 1u);
        const bool first = t_prev == -1;
        const bool connected = r.tau >= 0 && !first && p == p_prev && t - t_prev <= r.tau;
        const int k = connected ? (k_prev + 1 < 3 ? k_prev + 1 : 3) : 1;
        if (r.lock) {
            if (t_edge != -1 && t - t_edge > r.p_max) n_per = 0;
            if (p == 1 && (first || p_prev == 0)) {
                if (t_edge != -1) {
                    const long d = t - t_edge;
                    n_per = (r.p_min <= d && d <= r.p_max) ? (n_per + 1 < r.lock ? n_per + 1 : r.lock) : 0;
                }
                t_edge = t;
            }
        }
        t_prev = t; p_prev = p; k_prev = k;
        any = true;
        int c = C_KEPT;
        if (r.lock && n_per >= r.lock) c = C_FLICKER;
        else if (r.tau >= 0 && !(r.keep == KEEP_FIRST ? k == 1 : r.keep == KEEP_SECOND ? k == 2 : k >= 2)) c = C_BURST;
        if (c != C_KEPT) cls[i] = (unsigned char)c;
    }
    if (any) {
        st[P_T_PREV] = t_prev; st[P_T_EDGE] = t_edge; st[P_PK] = (long)(p_prev + 2 * k_prev); st[P_N_PER] = n_per;
    }
}

// (d) kept records per tile; the five counters
__global__ __launch_bounds__(BLOCK) void pix_count_kernel(long lo, long hi, const unsigned char* __restrict__ cls, long* __restrict__ state,
                                                          unsigned long long* __restrict__ tile_off) {
    const long i = lo + (long)blockIdx.x * BLOCK + threadIdx.x;
    tally_classes<N_CLASS>(i < hi ? (int)cls[i] : -1, tile_off + lo / TILE + blockIdx.x, state + S_KEPT);
}

// (e) the scan of the tile counts, on this state block
__global__ __launch_bounds__(BLOCK) void pix_scan_kernel(const Rec* __restrict__ rec, long lo, long hi, long* __restrict__ state,
                                                         unsigned long long* __restrict__ tile_off, long* __restrict__ io) {
    scan_tiles<S_SEEN, S_T_LAST>(rec, lo, hi, state, tile_off, io);
}

int key_bits(int H, int W) {                                     // ceil(log2(H * W)): 0 for one pixel
    int bits = 0;
    while ((1L << bits) < (long)H * W) ++bits;
    return bits;
}
long ws_of_tiles(long tiles) {                                   // a piece of so many tiles of records
    return tiles * WS_TILE + (tiles + SORT_TILES - 1) / SORT_TILES * WS_HIST;
}
long ws_need(long n_events) {                                    // one piece that takes n_events records
    const long tiles = (n_events + TILE - 1) / TILE;
    return ws_of_tiles(tiles > 0 ? tiles : 1);
}
long tiles_of_ws(long ws_bytes) {                                // the largest piece the workspace takes: ws_of_tiles(it) <= ws_bytes
    const long groups = ws_bytes / (SORT_TILES * WS_TILE + WS_HIST), rest = ws_bytes - groups * (SORT_TILES * WS_TILE + WS_HIST);
    return groups * SORT_TILES + (rest >= WS_HIST ? (rest - WS_HIST) / WS_TILE : 0);
}
}  // namespace

LEOD_API int leod_pixel_filter_query(long n_events, int H, int W, int* tile_events, int* tiles_per_pass, int* digit_bits, long* ws_bytes,
                                     long* marks_bytes) {
    if (n_events < 0 || n_events > 0x7fffffffL || H < 1 || W < 1 || H > 16384 || W > 16384) return LEOD_ERR_ARG;
    if (tile_events) *tile_events = TILE;
    if (tiles_per_pass) *tiles_per_pass = PASS;
    if (digit_bits) *digit_bits = DIGIT;
    if (ws_bytes) *ws_bytes = ws_need(n_events);
    if (marks_bytes) *marks_bytes = marks_need(n_events);
    return LEOD_OK;
}

LEOD_API int leod_pixel_filter_scan(const void* records, long n_events, int H, int W, long burst_us, int burst_keep, long p_min_us,
                                    long p_max_us, int lock, const unsigned char* mask, long* state, void* ws, long ws_bytes, void* marks,
                                    long marks_bytes, long* io, hipStream_t stream) {
    if (!records_ok(records, n_events) || H < 1 || W < 1 || H > 16384 || W > 16384) return LEOD_ERR_ARG;
    if (burst_us < -1 || burst_us > 0x7fffffffL || burst_keep < KEEP_FIRST || burst_keep > KEEP_FROM_SECOND) return LEOD_ERR_ARG;
    if (lock < 0 || lock > 255 || (lock && (p_min_us < 1 || p_min_us > p_max_us || p_max_us > 0x7fffffffL))) return LEOD_ERR_ARG;
    if (!state || !io || ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(io)) & 7)) return LEOD_ERR_ARG;
    if (n_events == 0) return LEOD_OK;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || !marks || (reinterpret_cast<uintptr_t>(marks) & 7)) return LEOD_ERR_ARG;
    if (marks_bytes < marks_need(n_events)) return LEOD_ERR_ARG;
    // the records per piece that the workspace allows: whole tiles
    const long total_tiles = (n_events + TILE - 1) / TILE;
    long piece_tiles = tiles_of_ws(ws_bytes);
    if (piece_tiles > total_tiles) piece_tiles = total_tiles;
    if (piece_tiles < 1) return LEOD_ERR_ARG;
    const long per = piece_tiles * TILE;
    const Rec* rec = static_cast<const Rec*>(records);
    unsigned char* cls = static_cast<unsigned char*>(marks);
    unsigned long long* tile_off = reinterpret_cast<unsigned long long*>(cls + (n_events + 7) / 8 * 8);
    unsigned* buf = static_cast<unsigned*>(ws);
    unsigned* key[2] = {buf, buf + 2 * per};
    unsigned* idx[2] = {buf + per, buf + 3 * per};
    unsigned* hist = buf + 4 * per;                              // RADIX entries per sort tile of the piece
    const Rule rule = {burst_us, burst_keep, p_min_us, p_max_us, lock};
    const int bits = key_bits(H, W);
    for (long lo = 0; lo < n_events; lo += per) {
        const long hi = lo + per < n_events ? lo + per : n_events;
        const long n = hi - lo, n_tiles = (n + TILE - 1) / TILE, n_stiles = (n_tiles + SORT_TILES - 1) / SORT_TILES;
        const dim3 sgrid((unsigned)n_stiles);
        const dim3 grid((unsigned)n_tiles), block(BLOCK);
        hipLaunchKernelGGL(pix_classify_kernel, grid, block, 0, stream, rec, lo, hi, H, W, mask, state, cls, key[0], idx[0], io);
        int cur = 0;
        for (int shift = 0; shift < bits; shift += DIGIT, cur ^= 1) {
            hipLaunchKernelGGL(pix_hist_kernel, sgrid, block, 0, stream, key[cur], n, shift, n_stiles, hist);
            hipLaunchKernelGGL(pix_hist_scan_kernel, dim3(1), block, 0, stream, hist, (long)RADIX * n_stiles);
            hipLaunchKernelGGL(pix_scatter_kernel, sgrid, block, 0, stream, key[cur], idx[cur], n, shift, n_stiles, hist, key[cur ^ 1],
                               idx[cur ^ 1]);
        }
        hipLaunchKernelGGL(pix_walk_kernel, grid, block, 0, stream, rec, lo, hi, key[cur], idx[cur], rule, cls, state);
        hipLaunchKernelGGL(pix_count_kernel, grid, block, 0, stream, lo, hi, cls, state, tile_off);
        hipLaunchKernelGGL(pix_scan_kernel, dim3(1), block, 0, stream, rec, lo, hi, state, tile_off, io);
        if (leod_launch_status() != LEOD_OK) return LEOD_ERR_LAUNCH;
    }
    return LEOD_OK;
}
