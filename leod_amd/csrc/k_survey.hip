// Filter survey (the definitions and identities: DESIGN.md section 1): ONE pass over the 8-byte .dat records of a recording, in stream
// order with t non-decreasing, that gives the exact count each ingestion filter would remove for a whole list of thresholds at once.
// Nothing is filtered: the pass adds to integer histograms of the intervals the filters' rules look at, binned by a strictly increasing
// list of K <= 64 edges (bin(d) = the number of edges < d; bin K: above the last edge), and the cumulative sums of those histograms are
// the filters' counters.  A candidate is an event inside the sensor and not masked, as in both filters.
//   nb[K + 2]      d = t - the latest EARLIER (stream position) candidate on one of the 8 in-sensor neighbours; [K + 1]: there is none
//   same[K + 1]    d = t - t_prev of a candidate whose pixel's previous candidate has its polarity
//   sec_on / sec_off[K + 1]   with c = bin(d) of `same` (INF without a same-polarity predecessor) and c' = the c of the pixel's previous
//                  candidate: when c < c' and c < K, sec_on[c] += 1 and, if c' <= K, sec_off[c'] += 1
//   period[K + 1]  d = t - t_edge at every rising edge (an ON candidate that is the pixel's first or follows an OFF one) with an edge before
//   run[256]       (only with a band) n_per of the anti-flicker rule with lock = 255, after every candidate
// A piece of records [lo, hi) of a chunk takes
//   (a) survey_classify_kernel: class per record, sortedness, the three class counters, and the sort's input: key = the pixel y * W + x
//       of a candidate, H * W for any other record (those sort behind every pixel and nothing looks at them again), value = the index;
//   (b) the stable per-pixel sort of pixel_sort.hpp on ceil(log2(H * W + 1)) key bits: a pixel's run is in stream order;
//   (c) survey_nb_kernel, one lane per sorted position: for each of the 8 neighbours q ONE binary search over the sorted (key, index)
//       pairs for the last pair below (q, own index): if its key is q it is the latest earlier candidate of q in the piece, else the
//       carried per-pixel time answers for the records before the piece (the walk has not touched it yet).  Exact times, no time slots;
//   (d) survey_walk_kernel: the lane at the first sorted position of a pixel walks that pixel's run with the pixel's state in registers
//       (same, sec_on, sec_off, period, run) and stores the state;
//   (e) survey_close_kernel, one lane: seen, the first and the last time, the times around a decrease.
// Histograms: integer atomics into per-workgroup LDS bins, then one integer atomic per non-empty bin and workgroup into the int64 state:
// sums of integers, the same in any order, so two runs give the same bytes.  An event's bin is a binary search over the edges in LDS.
// Launches run in stream order; no workgroup waits on another; every loop is bounded by the piece.  A chunk larger than the workspace
// allows is cut into pieces of whole tiles: the state block carries the pixels from piece to piece as it does from chunk to chunk.
//
// State block (int64, include/leod_hip.h): [0] seen [1] candidates [2] outside [3] masked [4] time of the first event seen (-1: none)
// [5] time of the last event seen (-1: none) [6] [7] 0; then nb[K + 2], same[K + 1], sec_on[K + 1], sec_off[K + 1], period[K + 1],
// run[256]; then per pixel q four words: t_prev (time of the last candidate, which is also the activity filter's surface; -1: never),
// t_edge (time of the last rising edge; -1: none), p_prev + 2 * c_prev (c_prev = the bin of the last candidate's same-polarity interval,
// 255 = INF: it had none), n_per (0 .. 255).  A recording starts from {-1, -1, 510, 0} in every pixel.
//
// Bounds: records are read below n_events only; x, y are compared with W, H before they index the mask or form a key, so a key below
// H * W indexes the per-pixel block and neighbours are compared with the sensor before they form one; the sort's values are the indices
// the classify pass wrote and are compared with [lo, hi) before they index the records; a bin is at most K (K + 1 for nb) and n_per
// at most 255 by construction, for any record contents; the entry point refuses a workspace smaller than one tile's.
#include "pixel_sort.hpp"

namespace {
using namespace filt;
constexpr int MAX_EDGES = 64;
constexpr int RUN_BINS = 256;
constexpr int C_INF = 255;                                       // "no same-polarity predecessor": above every bin
enum { S_SEEN = 0, S_CAND, S_OUTSIDE, S_MASKED, S_T_FIRST, S_T_LAST, S_HEAD = 8 };
enum { P_T_PREV = 0, P_T_EDGE, P_PC, P_N_PER, P_LONGS };         // per pixel, behind the histograms
static_assert(S_OUTSIDE == S_CAND + C_OUTSIDE && S_MASKED == S_CAND + C_MASKED, "the class counters lie in class order");

struct Edges { int n; unsigned e[MAX_EDGES]; };                  // strictly increasing, below 2^31
struct Band { long p_min, p_max; };                              // p_min 0: no band, run[] is not touched

inline long hist_longs(int K) { return (long)(K + 2) + 4L * (K + 1) + RUN_BINS; }

// the number of edges < d (d < 0 for records out of order: bin 0)
__device__ __forceinline__ int bin_of(const long* __restrict__ lds_e, int K, long d) {
    int a = 0, b = K;
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (lds_e[mid] < d) a = mid + 1; else b = mid;
    }
    return a;
}

// (a)
__global__ __launch_bounds__(BLOCK) void survey_classify_kernel(const Rec* __restrict__ rec, long lo, long hi, int H, int W,
                                                                const unsigned char* __restrict__ mask, long* __restrict__ state,
                                                                unsigned* __restrict__ key, unsigned* __restrict__ idx,
                                                                long* __restrict__ io) {
    const long i = lo + (long)blockIdx.x * BLOCK + threadIdx.x;
    int c = -1;                                                  // a lane without a record; every lane takes the wave sums
    if (i < hi) {
        Rec e; int x, y;
        c = classify(rec, i, state + S_T_LAST, H, W, mask, io, e, x, y);
        key[i - lo] = c == C_KEPT ? (unsigned)y * (unsigned)W + (unsigned)x : (unsigned)H * (unsigned)W;         // H * W <= 2^28
        idx[i - lo] = (unsigned)i;
    }
#pragma unroll
    for (int k = C_KEPT; k <= C_MASKED; ++k) {
        const unsigned n = wave_sum_u32(c == k ? 1u : 0u);
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(reinterpret_cast<unsigned long long*>(state + S_CAND + k), (unsigned long long)n);
    }
}

// the time of the latest candidate of pixel q before stream position i: in the piece's sorted pairs, else what the state carries
__device__ __forceinline__ long latest_before(const Rec* __restrict__ rec, long lo, long hi, const unsigned* __restrict__ key,
                                              const unsigned* __restrict__ idx, long n, unsigned q, unsigned i,
                                              const long* __restrict__ pixels) {
    long a = 0, b = n;                                           // -> the number of pairs below (q, i)
    while (a < b) {
        const long mid = (a + b) >> 1;
        const unsigned k = key[mid];
        if (k < q || (k == q && idx[mid] < i)) a = mid + 1; else b = mid;
    }
    if (a > 0 && key[a - 1] == q) {
        const long j = (long)idx[a - 1];
        if (j >= lo && j < hi) return (long)rec[j].t;
    }
    return pixels[(long)q * P_LONGS + P_T_PREV];
}

// (c)
__global__ __launch_bounds__(BLOCK) void survey_nb_kernel(const Rec* __restrict__ rec, long lo, long hi, int H, int W,
                                                          const unsigned* __restrict__ key, const unsigned* __restrict__ idx, Edges ed,
                                                          const long* __restrict__ pixels, long* __restrict__ nb) {
    __shared__ unsigned lds_h[MAX_EDGES + 2];
    __shared__ long lds_e[MAX_EDGES];
    const int K = ed.n;
    if (threadIdx.x < K + 2) lds_h[threadIdx.x] = 0;
    if (threadIdx.x < K) lds_e[threadIdx.x] = (long)ed.e[threadIdx.x];
    __syncthreads();
    const long n = hi - lo, j = (long)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned pixel_count = (unsigned)H * (unsigned)W;
    if (j < n) {
        const unsigned pix = key[j];
        const long i = (long)idx[j];
        if (pix < pixel_count && i >= lo && i < hi) {
            const long t = (long)rec[i].t;
            const int x = (int)(pix % (unsigned)W), y = (int)(pix / (unsigned)W);
            long m = -1;
            for (int dy = -1; dy <= 1; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= H) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qx = x + dx;
                    if (qx < 0 || qx >= W || (dx == 0 && dy == 0)) continue;
                    const long tq = latest_before(rec, lo, hi, key, idx, n, (unsigned)qy * (unsigned)W + (unsigned)qx, (unsigned)i, pixels);
                    m = tq > m ? tq : m;
                }
            }
            atomicAdd(&lds_h[m < 0 ? K + 1 : bin_of(lds_e, K, t - m)], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < K + 2 && lds_h[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(nb + threadIdx.x), (unsigned long long)lds_h[threadIdx.x]);
}

// (d) lds_h and hist: same, sec_on, sec_off, period (K + 1 bins each), run
__global__ __launch_bounds__(BLOCK) void survey_walk_kernel(const Rec* __restrict__ rec, long lo, long hi, int H, int W,
                                                            const unsigned* __restrict__ key, const unsigned* __restrict__ idx, Edges ed,
                                                            Band band, long* __restrict__ pixels, long* __restrict__ hist) {
    __shared__ unsigned lds_h[4 * (MAX_EDGES + 1) + RUN_BINS];
    __shared__ long lds_e[MAX_EDGES];
    const int K = ed.n, bins = 4 * (K + 1) + RUN_BINS;
    for (int b = threadIdx.x; b < bins; b += BLOCK) lds_h[b] = 0;
    if (threadIdx.x < K) lds_e[threadIdx.x] = (long)ed.e[threadIdx.x];
    __syncthreads();
    unsigned* h_same = lds_h;
    unsigned* h_on = lds_h + (K + 1);
    unsigned* h_off = lds_h + 2 * (K + 1);
    unsigned* h_period = lds_h + 3 * (K + 1);
    unsigned* h_run = lds_h + 4 * (K + 1);
    const long n = hi - lo, j0 = (long)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned pixel_count = (unsigned)H * (unsigned)W;
    const unsigned pix = j0 < n ? key[j0] : pixel_count;
    if (pix < pixel_count && (j0 == 0 || key[j0 - 1] != pix)) {                  // the head of a pixel's run
        long* st = pixels + (long)pix * P_LONGS;
        long t_prev = st[P_T_PREV], t_edge = st[P_T_EDGE];
        int p_prev = (int)(st[P_PC] & 1), c_prev = (int)((st[P_PC] >> 1) & 255), n_per = (int)(st[P_N_PER] & 255);
        bool any = false;
        for (long j = j0; j < n && key[j] == pix; ++j) {
            const long i = (long)idx[j];
            if (i < lo || i >= hi) continue;
            const Rec e = rec[i];
            const long t = (long)e.t;
            const int p = (int)((e.xyp >> 28) & 1u);
            const bool first = t_prev == -1;
            int c = C_INF;
            if (!first && p == p_prev) {
                c = bin_of(lds_e, K, t - t_prev);
                atomicAdd(&h_same[c], 1u);
            }
            if (c < c_prev && c < K) {
                atomicAdd(&h_on[c], 1u);
                if (c_prev <= K) atomicAdd(&h_off[c_prev], 1u);
            }
            if (band.p_min && t_edge != -1 && t - t_edge > band.p_max) n_per = 0;
            if (p == 1 && (first || p_prev == 0)) {
                if (t_edge != -1) {
                    const long d = t - t_edge;
                    atomicAdd(&h_period[bin_of(lds_e, K, d)], 1u);
                    if (band.p_min) n_per = (band.p_min <= d && d <= band.p_max) ? (n_per + 1 < 255 ? n_per + 1 : 255) : 0;
                }
                t_edge = t;
            }
            if (band.p_min) atomicAdd(&h_run[n_per], 1u);
            t_prev = t; p_prev = p; c_prev = c;
            any = true;
        }
        if (any) {
            st[P_T_PREV] = t_prev; st[P_T_EDGE] = t_edge; st[P_PC] = (long)(p_prev + 2 * c_prev); st[P_N_PER] = (long)n_per;
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += BLOCK)
        if (lds_h[b]) atomicAdd(reinterpret_cast<unsigned long long*>(hist + b), (unsigned long long)lds_h[b]);
}

// (e)
__global__ void survey_close_kernel(const Rec* __restrict__ rec, long lo, long hi, long* __restrict__ state, long* __restrict__ io) {
    if (blockIdx.x || threadIdx.x) return;
    if (hi > lo && state[S_T_FIRST] == -1) state[S_T_FIRST] = (long)rec[lo].t;
    close_piece<S_SEEN, S_T_LAST>(rec, lo, hi, state, io);
}
}  // namespace

LEOD_API int leod_survey_query(long n_events, int H, int W, int n_edges, int* tile_events, int* digit_bits, long* ws_bytes,
                               long* state_longs) {
    if (n_events < 0 || n_events > 0x7fffffffL || H < 1 || W < 1 || H > 16384 || W > 16384) return LEOD_ERR_ARG;
    if (n_edges < 1 || n_edges > MAX_EDGES) return LEOD_ERR_ARG;
    if (tile_events) *tile_events = TILE;
    if (digit_bits) *digit_bits = DIGIT;
    if (ws_bytes) *ws_bytes = ws_need(n_events);
    if (state_longs) *state_longs = S_HEAD + hist_longs(n_edges) + (long)P_LONGS * H * W;
    return LEOD_OK;
}

LEOD_API int leod_survey_events(const void* records, long n_events, int H, int W, const long* edges_us, int n_edges, long p_min_us,
                                long p_max_us, const unsigned char* mask, long* state, void* ws, long ws_bytes, long* io,
                                hipStream_t stream) {
    if (!records_ok(records, n_events) || H < 1 || W < 1 || H > 16384 || W > 16384) return LEOD_ERR_ARG;
    if (!edges_us || n_edges < 1 || n_edges > MAX_EDGES) return LEOD_ERR_ARG;
    Edges ed;
    ed.n = n_edges;
    for (int k = 0; k < MAX_EDGES; ++k) {
        if (k < n_edges && (edges_us[k] < 0 || edges_us[k] > 0x7fffffffL || (k > 0 && edges_us[k] <= edges_us[k - 1]))) return LEOD_ERR_ARG;
        ed.e[k] = k < n_edges ? (unsigned)edges_us[k] : 0u;
    }
    if (p_min_us < 0 || (p_min_us == 0 && p_max_us != 0) || (p_min_us && (p_min_us > p_max_us || p_max_us > 0x7fffffffL))) return LEOD_ERR_ARG;
    if (!state || !io || ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(io)) & 7)) return LEOD_ERR_ARG;
    if (n_events == 0) return LEOD_OK;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7)) return LEOD_ERR_ARG;
    // the records per piece that the workspace allows: whole tiles
    const long total_tiles = (n_events + TILE - 1) / TILE;
    long piece_tiles = tiles_of_ws(ws_bytes);
    if (piece_tiles > total_tiles) piece_tiles = total_tiles;
    if (piece_tiles < 1) return LEOD_ERR_ARG;
    const long per = piece_tiles * TILE;
    const Rec* rec = static_cast<const Rec*>(records);
    const SortWs s(ws, per);
    const Band band = {p_min_us, p_max_us};
    const int K = n_edges, bits = key_bits((long)H * W + 1);
    long* nb = state + S_HEAD;
    long* hist = nb + (K + 2);                                   // same, sec_on, sec_off, period, run
    long* pixels = state + S_HEAD + hist_longs(K);
    for (long lo = 0; lo < n_events; lo += per) {
        const long hi = lo + per < n_events ? lo + per : n_events;
        const long n = hi - lo, n_tiles = (n + TILE - 1) / TILE;
        const dim3 grid((unsigned)n_tiles), block(BLOCK);
        hipLaunchKernelGGL(survey_classify_kernel, grid, block, 0, stream, rec, lo, hi, H, W, mask, state, s.key[0], s.idx[0], io);
        const int cur = sort_pairs(s, n, bits, stream);
        hipLaunchKernelGGL(survey_nb_kernel, grid, block, 0, stream, rec, lo, hi, H, W, s.key[cur], s.idx[cur], ed, pixels, nb);
        hipLaunchKernelGGL(survey_walk_kernel, grid, block, 0, stream, rec, lo, hi, H, W, s.key[cur], s.idx[cur], ed, band, pixels, hist);
        hipLaunchKernelGGL(survey_close_kernel, dim3(1), dim3(64), 0, stream, rec, lo, hi, state, io);
        if (leod_launch_status() != LEOD_OK) return LEOD_ERR_LAUNCH;
    }
    return LEOD_OK;
}
