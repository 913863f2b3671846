// Sensor fit at ingestion (rule: DESIGN.md section 1): the 8-byte records of a .dat file, in stream order with t non-decreasing, from the
// camera's own geometry (Hs, Ws) onto the frame geometry (Hd, Wd) of a dataset: mirror, orient (0 / 90 / 180 / 270 degrees clockwise),
// scale by an integer k (cell = k x k source pixels), place at an offset (ox, oy).  What happens to the events of a cell is the reduce:
// `pick` keeps those of the cell's centre pixel (x' % k == k / 2 and y' % k == k / 2), `sum` keeps all, `fire` integrates and fires:
// each destination pixel holds an accumulator a; its events, in stream order, add +1 (ON) or -1 (OFF); the event that brings a to
// +theta or -theta is kept and a returns to 0, any other is merged.  pick and sum decide every record on its own.  fire is SEQUENTIAL per
// destination pixel and independent between pixels, so it groups the records as the per-pixel filter does (k_pixfilter.hip).  A piece of
// records [lo, hi) of a chunk takes
//   (a) fit_classify_kernel: class per record (outside the source sensor / cropped / skipped / candidate), sortedness; for pick and sum
//       the candidates are the kept records and the same launch counts them (d); for fire it writes the sort's input: key = the
//       destination pixel yd * Wd + xd of a candidate, value = the index.  Any other record has no pixel; the walk skips it by its class
//       wherever it sorts, so it gets the key (position in the piece) % (Hd * Wd): spread evenly over the pixels, such records lengthen
//       every run a little.  With one key for them all (0, as in k_pixfilter.hip) the cropped events of a recording -- 5 % of a VGA one
//       on Gen1 frames -- are ONE run that ONE lane walks while the device idles, and that walk is most of the stage's time;
//   fire only: (b) the STABLE least-significant-digit radix sort of (key, index) on ceil(log2(Hd * Wd)) key bits (pixel_sort.hpp);
//   (c) fit_walk_kernel: the lane at the first sorted position of a pixel walks that pixel's run in index order with the accumulator in a
//       register, writes the class byte (kept / merged) of every candidate and stores the accumulator.  One lane walks a whole run: the
//       cost is linear in the run, also when every event of the piece lies on one pixel;  (d) fit_count_kernel: kept records per tile
//       and the five counters;
//   (e) fit_scan_kernel, ONE workgroup: offsets of the tiles' kept records, PASS tiles per pass; seen, the last time, the times around
//       a decrease.
// The marks are those of k_filter.hip (class 0 = kept).  leod_event_fit_emit stores the kept records of the whole chunk in one launch,
// with x, y replaced by xd, yd (t and bits 28-31 unchanged): the map is evaluated again from the source record, so the marks stay one
// byte a record.  Launches run in stream order; no workgroup waits on another; every loop is bounded by the piece.  With fire a chunk
// larger than the workspace allows is cut into pieces of whole tiles: the accumulators in the state block carry the pixels from piece to
// piece as they do from chunk to chunk.  pick and sum need no workspace and take a chunk in one piece.
//
// Bounds: records are read below n_events only; x, y are compared with Ws, Hs before they are mapped, the mapped cell with the scaled
// image and xd, yd with Wd, Hd before they form a key, and the key of a record without a pixel is a remainder of Hd * Wd, so a key is
// below Hd * Wd and indexes the state block; the sort's values are the indices the classify pass wrote (lo <= index < hi); a scatter
// position is compared with the piece's size, an emit position with the capacity, before it is stored to; the entry points refuse
// buffers smaller than leod_event_fit_query reports.
#include "pixel_sort.hpp"

namespace {
using namespace filt;
enum { C_CROPPED = 2, C_SKIPPED = 3, C_MERGED = 4, N_CLASS = 5 };          // behind C_KEPT (with fire: a candidate until the walk decides), C_OUTSIDE
enum { S_SEEN = 0, S_KEPT, S_OUTSIDE, S_CROPPED, S_SKIPPED, S_MERGED, S_T_LAST, S_HEAD = 8 };      // state block: include/leod_hip.h
enum { R_PICK = 0, R_SUM = 1, R_FIRE = 2 };

struct Fit { int Hs, Ws, Hd, Wd, orient, mirror, k, ox, oy, reduce; };

// steps 1 to 4 of the rule for a pixel INSIDE the source sensor, and the pick test -> C_KEPT (xd, yd are set and inside the frame),
// C_CROPPED or C_SKIPPED
__device__ __forceinline__ int fit_map(const Fit& f, int x, int y, int& xd, int& yd) {
    if (f.mirror) x = f.Ws - 1 - x;
    int xo, yo, Ho, Wo;
    switch (f.orient) {
        case 1:  xo = f.Hs - 1 - y; yo = x;            Ho = f.Ws; Wo = f.Hs; break;
        case 2:  xo = f.Ws - 1 - x; yo = f.Hs - 1 - y; Ho = f.Hs; Wo = f.Ws; break;
        case 3:  xo = y;            yo = f.Ws - 1 - x; Ho = f.Ws; Wo = f.Hs; break;
        default: xo = x;            yo = y;            Ho = f.Hs; Wo = f.Ws; break;
    }
    const int cx = xo / f.k, cy = yo / f.k;
    if (cx >= Wo / f.k || cy >= Ho / f.k) return C_CROPPED;                  // an incomplete edge cell
    xd = cx + f.ox; yd = cy + f.oy;
    if (xd < 0 || xd >= f.Wd || yd < 0 || yd >= f.Hd) return C_CROPPED;
    if (f.reduce == R_PICK && (xo - cx * f.k != f.k / 2 || yo - cy * f.k != f.k / 2)) return C_SKIPPED;
    return C_KEPT;
}

// (a); FIRE false: and (d)
template <bool FIRE>
__global__ __launch_bounds__(BLOCK) void fit_classify_kernel(const Rec* __restrict__ rec, long lo, long hi, Fit f, long* __restrict__ state,
                                                             unsigned char* __restrict__ cls, unsigned* __restrict__ key,
                                                             unsigned* __restrict__ idx, unsigned long long* __restrict__ tile_off,
                                                             long* __restrict__ io) {
    const long i = lo + (long)blockIdx.x * BLOCK + threadIdx.x;
    int c = -1;
    if (i < hi) {
        Rec e; int x, y, xd = 0, yd = 0;
        c = classify(rec, i, state + S_T_LAST, f.Hs, f.Ws, nullptr, io, e, x, y);
        if (c == C_KEPT) c = fit_map(f, x, y, xd, yd);
        cls[i] = (unsigned char)c;
        if (FIRE) {
            key[i - lo] = c == C_KEPT ? (unsigned)yd * (unsigned)f.Wd + (unsigned)xd                 // Hd * Wd <= 2^28
                                      : (unsigned)((i - lo) % ((long)f.Hd * f.Wd));                  // below Hd * Wd, too
            idx[i - lo] = (unsigned)i;
        }
    }
    if (!FIRE) tally_classes<N_CLASS>(c, tile_off + lo / TILE + blockIdx.x, state + S_KEPT);
}

// (c) integrate and fire for the run of one destination pixel
__global__ __launch_bounds__(BLOCK) void fit_walk_kernel(const Rec* __restrict__ rec, long lo, long hi, const unsigned* __restrict__ key,
                                                         const unsigned* __restrict__ idx, long theta, unsigned char* __restrict__ cls,
                                                         long* __restrict__ state) {
    const long n = hi - lo, j0 = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (j0 >= n) return;
    const unsigned pix = key[j0];
    if (j0 > 0 && key[j0 - 1] == pix) return;                                    // not the head of a run
    long* st = state + S_HEAD + (long)pix;
    long a = *st;
    bool any = false;
    for (long j = j0; j < n && key[j] == pix; ++j) {
        const long i = (long)idx[j];
        if (i < lo || i >= hi || cls[i] != C_KEPT) continue;                     // outside, cropped or skipped: it touches no state
        a += (rec[i].xyp >> 28) & 1u ? 1 : -1;
        any = true;
        if (a == theta || a == -theta) a = 0;
        else cls[i] = (unsigned char)C_MERGED;
    }
    if (any) *st = a;
}

// (d) kept records per tile; the five counters
__global__ __launch_bounds__(BLOCK) void fit_count_kernel(long lo, long hi, const unsigned char* __restrict__ cls, long* __restrict__ state,
                                                          unsigned long long* __restrict__ tile_off) {
    const long i = lo + (long)blockIdx.x * BLOCK + threadIdx.x;
    tally_classes<N_CLASS>(i < hi ? (int)cls[i] : -1, tile_off + lo / TILE + blockIdx.x, state + S_KEPT);
}

// (e) the scan of the tile counts, on this state block
__global__ __launch_bounds__(BLOCK) void fit_scan_kernel(const Rec* __restrict__ rec, long lo, long hi, long* __restrict__ state,
                                                         unsigned long long* __restrict__ tile_off, long* __restrict__ io) {
    scan_tiles<S_SEEN, S_T_LAST>(rec, lo, hi, state, tile_off, io);
}

// the ordered compaction of filter_emit_kernel, with the transformed coordinates
__global__ __launch_bounds__(BLOCK) void fit_emit_kernel(const Rec* __restrict__ rec, long n_events, Fit f, const unsigned char* __restrict__ cls,
                                                         const unsigned long long* __restrict__ tile_off, Rec* __restrict__ out,
                                                         long capacity) {
    __shared__ unsigned long long lds_s[BLOCK / 64];
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    const bool keep = i < n_events && cls[i] == C_KEPT;
    unsigned long long sum;
    const long pos = (long)(tile_off[blockIdx.x] + block_scan_sum(keep ? 1ULL : 0ULL, sum, lds_s));
    if (!keep || pos < 0 || pos >= capacity) return;
    Rec e = rec[i];
    const int x = (int)(e.xyp & 16383u), y = (int)((e.xyp >> 14) & 16383u);
    int xd = 0, yd = 0;
    if (x >= f.Ws || y >= f.Hs || fit_map(f, x, y, xd, yd) != C_KEPT) return;    // marks of another call: nothing is stored
    e.xyp = (e.xyp & 0xf0000000u) | ((unsigned)yd << 14) | (unsigned)xd;          // xd < Wd, yd < Hd <= 2^14
    out[pos] = e;
}

bool fit_ok(int Hs, int Ws, int Hd, int Wd, int orient, int mirror, int k, int ox, int oy) {
    for (int v : {Hs, Ws, Hd, Wd})
        if (v < 1 || v > 16384) return false;
    if (orient != 0 && orient != 90 && orient != 180 && orient != 270) return false;
    return (mirror == 0 || mirror == 1) && k >= 1 && k <= 64 && ox >= -16384 && ox <= 16384 && oy >= -16384 && oy <= 16384;
}
}  // namespace

LEOD_API int leod_event_fit_query(long n_events, int Hd, int Wd, int reduce, int* tile_events, int* tiles_per_pass, int* digit_bits,
                                  long* ws_bytes, long* marks_bytes) {
    if (n_events < 0 || n_events > 0x7fffffffL || Hd < 1 || Wd < 1 || Hd > 16384 || Wd > 16384) return LEOD_ERR_ARG;
    if (reduce < R_PICK || reduce > R_FIRE) return LEOD_ERR_ARG;
    if (tile_events) *tile_events = TILE;
    if (tiles_per_pass) *tiles_per_pass = PASS;
    if (digit_bits) *digit_bits = DIGIT;
    if (ws_bytes) *ws_bytes = reduce == R_FIRE ? ws_need(n_events) : 0;
    if (marks_bytes) *marks_bytes = marks_need(n_events);
    return LEOD_OK;
}

LEOD_API int leod_event_fit_scan(const void* records, long n_events, int Hs, int Ws, int Hd, int Wd, int orient, int mirror, int k, int ox,
                                 int oy, int reduce, int threshold, long* state, void* ws, long ws_bytes, void* marks, long marks_bytes,
                                 long* io, hipStream_t stream) {
    if (!records_ok(records, n_events) || !fit_ok(Hs, Ws, Hd, Wd, orient, mirror, k, ox, oy)) return LEOD_ERR_ARG;
    if (reduce < R_PICK || reduce > R_FIRE || (reduce == R_FIRE && (threshold < 1 || threshold > 32767))) return LEOD_ERR_ARG;
    if (!state || !io || ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(io)) & 7)) return LEOD_ERR_ARG;
    if (n_events == 0) return LEOD_OK;
    if (!marks || (reinterpret_cast<uintptr_t>(marks) & 7) || marks_bytes < marks_need(n_events)) return LEOD_ERR_ARG;
    const Rec* rec = static_cast<const Rec*>(records);
    unsigned char* cls = static_cast<unsigned char*>(marks);
    unsigned long long* tile_off = reinterpret_cast<unsigned long long*>(cls + (n_events + 7) / 8 * 8);
    const Fit f = {Hs, Ws, Hd, Wd, orient / 90, mirror, k, ox, oy, reduce};
    const long total_tiles = (n_events + TILE - 1) / TILE;
    const dim3 block(BLOCK);
    if (reduce != R_FIRE) {
        hipLaunchKernelGGL(fit_classify_kernel<false>, dim3((unsigned)total_tiles), block, 0, stream, rec, 0L, n_events, f, state, cls,
                           (unsigned*)nullptr, (unsigned*)nullptr, tile_off, io);
        hipLaunchKernelGGL(fit_scan_kernel, dim3(1), block, 0, stream, rec, 0L, n_events, state, tile_off, io);
        return leod_launch_status() != LEOD_OK ? LEOD_ERR_LAUNCH : LEOD_OK;
    }
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 7)) return LEOD_ERR_ARG;
    // the records per piece that the workspace allows: whole tiles
    long piece_tiles = tiles_of_ws(ws_bytes);
    if (piece_tiles > total_tiles) piece_tiles = total_tiles;
    if (piece_tiles < 1) return LEOD_ERR_ARG;
    const long per = piece_tiles * TILE;
    const SortWs s(ws, per);
    const int bits = key_bits((long)Hd * Wd);
    for (long lo = 0; lo < n_events; lo += per) {
        const long hi = lo + per < n_events ? lo + per : n_events;
        const long n = hi - lo, n_tiles = (n + TILE - 1) / TILE;
        const dim3 grid((unsigned)n_tiles);
        hipLaunchKernelGGL(fit_classify_kernel<true>, grid, block, 0, stream, rec, lo, hi, f, state, cls, s.key[0], s.idx[0], tile_off, io);
        const int cur = sort_pairs(s, n, bits, stream);
        hipLaunchKernelGGL(fit_walk_kernel, grid, block, 0, stream, rec, lo, hi, s.key[cur], s.idx[cur], (long)threshold, cls, state);
        hipLaunchKernelGGL(fit_count_kernel, grid, block, 0, stream, lo, hi, cls, state, tile_off);
        hipLaunchKernelGGL(fit_scan_kernel, dim3(1), block, 0, stream, rec, lo, hi, state, tile_off, io);
        if (leod_launch_status() != LEOD_OK) return LEOD_ERR_LAUNCH;
    }
    return LEOD_OK;
}

LEOD_API int leod_event_fit_emit(const void* records, long n_events, int Hs, int Ws, int Hd, int Wd, int orient, int mirror, int k, int ox,
                                 int oy, int reduce, const void* marks, long marks_bytes, void* out, long capacity, hipStream_t stream) {
    if (!records_ok(records, n_events) || capacity < 0 || !fit_ok(Hs, Ws, Hd, Wd, orient, mirror, k, ox, oy)) return LEOD_ERR_ARG;
    if (reduce < R_PICK || reduce > R_FIRE) return LEOD_ERR_ARG;
    if (capacity > 0 && (!out || (reinterpret_cast<uintptr_t>(out) & 7))) return LEOD_ERR_ARG;
    if (n_events == 0) return LEOD_OK;
    if (!marks || (reinterpret_cast<uintptr_t>(marks) & 7) || marks_bytes < marks_need(n_events)) return LEOD_ERR_ARG;
    const unsigned char* cls = static_cast<const unsigned char*>(marks);
    const unsigned long long* tile_off = reinterpret_cast<const unsigned long long*>(cls + (n_events + 7) / 8 * 8);
    const Fit f = {Hs, Ws, Hd, Wd, orient / 90, mirror, k, ox, oy, reduce};
    hipLaunchKernelGGL(fit_emit_kernel, dim3((unsigned)((n_events + TILE - 1) / TILE)), dim3(BLOCK), 0, stream,
                       static_cast<const Rec*>(records), n_events, f, cls, tile_off, static_cast<Rec*>(out), capacity);
    return leod_launch_status();
}
