// Per-pixel event filters at ingestion (rule: DESIGN.md section 1): trail / STC (position of an event in a burst of same-polarity events
// of its pixel) and anti-flicker (consecutive in-band periods between a pixel's rising edges), on the 8-byte records of a .dat file in
// stream order with t non-decreasing.  Both rules are SEQUENTIAL per pixel -- the verdict on an event depends on the state its pixel's
// earlier candidates left -- and independent between pixels.  Since t is sorted, a pixel's order is index order, so a piece of records
// [lo, hi) of a chunk takes
//   (a) pix_classify_kernel: class per record (outside / masked / candidate), sortedness, and the sort's input: key = the pixel y * W + x
//       of a candidate (0 for any other record; the walk skips those by their class), value = the record's index;
//   (b) a STABLE least-significant-digit radix sort of (key, index) on ceil(log2(H * W)) key bits, DIGIT bits a pass, three launches a
//       pass (pixel_sort.hpp, shared with the filter survey of k_survey.hip: pix_hist_kernel, pix_hist_scan_kernel, pix_scatter_kernel);
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
#include "pixel_sort.hpp"

namespace {
using namespace filt;
enum { C_FLICKER = 3, C_BURST = 4, N_CLASS = 5 };                // behind C_KEPT (a candidate until the walk decides), C_OUTSIDE, C_MASKED
enum { S_SEEN = 0, S_KEPT, S_OUTSIDE, S_MASKED, S_FLICKER, S_BURST, S_T_LAST, S_HEAD = 8 };      // state block: include/leod_hip.h
enum { P_T_PREV = 0, P_T_EDGE, P_PK, P_N_PER, P_LONGS };         // per pixel, behind the head
enum { KEEP_FIRST = 0, KEEP_SECOND = 1, KEEP_FROM_SECOND = 2 };

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
    const SortWs s(ws, per);
    const Rule rule = {burst_us, burst_keep, p_min_us, p_max_us, lock};
    const int bits = key_bits((long)H * W);
    for (long lo = 0; lo < n_events; lo += per) {
        const long hi = lo + per < n_events ? lo + per : n_events;
        const long n = hi - lo, n_tiles = (n + TILE - 1) / TILE;
        const dim3 grid((unsigned)n_tiles), block(BLOCK);
        hipLaunchKernelGGL(pix_classify_kernel, grid, block, 0, stream, rec, lo, hi, H, W, mask, state, cls, s.key[0], s.idx[0], io);
        const int cur = sort_pairs(s, n, bits, stream);
        hipLaunchKernelGGL(pix_walk_kernel, grid, block, 0, stream, rec, lo, hi, s.key[cur], s.idx[cur], rule, cls, state);
        hipLaunchKernelGGL(pix_count_kernel, grid, block, 0, stream, lo, hi, cls, state, tile_off);
        hipLaunchKernelGGL(pix_scan_kernel, dim3(1), block, 0, stream, rec, lo, hi, state, tile_off, io);
        if (leod_launch_status() != LEOD_OK) return LEOD_ERR_LAUNCH;
    }
    return LEOD_OK;
}
