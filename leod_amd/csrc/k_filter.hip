// Event noise filters at ingestion (rule: DESIGN.md section 1): the 8-byte records of a Prophesee .dat file (u32 t; x in bits 0-13, y in
// bits 14-27, p in bit 28), in stream order with t non-decreasing, to the records that survive
//   1. the sensor bounds (x < W, y < H), 2. a pixel mask, 3. the background-activity rule: an event is kept iff an EARLIER event of the
//   stream that passed 1 and 2 lies on one of its 8 neighbour pixels, at most tau microseconds before it (tau_us = -1: rule 3 is off).
// An event that rule 3 removes still supports later ones, so whether event i is kept depends only on WHICH events lie before it, never
// on what was decided about them: the rule has an order-independent parallel form.
//
// slot(t) = t / (tau + 1).  Two events of one slot are at most tau apart, and a supporter lies in the event's own slot or in the one
// before it.  Per (slot, pixel) that holds an event the chunk keeps F = the smallest record index and M = the largest time; both are
// built with atomicMax (F as ~index) and do not depend on the order of execution.  Event i of slot s at time t is kept iff for one of
// its neighbours q:  F[s][q] < i,  or  M[s-1][q] >= t - tau,  or the carried surface holds last[q] >= t - tau.
// The (slot, pixel) maps are ONE open-addressing hash table keyed by (slot, y, x) -- 16 bytes per entry, at most one entry per event,
// never more than half full -- instead of dense [slots, H, W] planes: a silent gap of any length between two events costs nothing, tau = 0
// (one slot per microsecond) costs nothing, and the workspace is bounded by the number of events alone.  A chunk larger than the table
// allows is cut into sub-chunks at record boundaries (the rule is a stream rule: any cut gives the same result), each with
//   memset of the table; (a) filter_build_kernel: class per record (outside / masked / candidate), insert, sortedness;
//   (b) filter_decide_kernel: candidates look their neighbours up (surface, own slot, slot before), per-tile kept counts, counters;
//   (c) filter_surface_kernel: last[pixel] = max(last[pixel], t) over the candidates; (d) filter_scan_kernel, ONE workgroup: offsets of
//   the tiles' kept records, PASS tiles per pass.
// leod_event_filter_emit then stores the kept records of the whole chunk in one launch (per-tile prefix sum + the tile's offset): the
// ordered compaction of k_evt.hip.  Launches run in stream order; no workgroup waits on another.
//
// Bounds: records are read below n_events only; x, y are compared with W, H before they index the mask or the surface; the table is
// indexed through `& (capacity - 1)` and a probe sequence ends after `capacity` steps at the latest (records crafted to collide cost
// time, never an access outside the table); a record is stored only at a
// position below `capacity`; the entry points refuse buffers smaller than leod_event_filter_query reports.
#include "filter_common.hpp"

namespace {
using namespace filt;                 // Rec, BLOCK / TILE / PASS, the io block, the sums, classify / tally_classes / scan_tiles: filter_common.hpp
constexpr long MIN_ENTRIES = 64;
enum { C_UNSUPPORTED = 3, N_CLASS = 4 };                         // behind C_KEPT, C_OUTSIDE, C_MASKED
enum { S_SEEN = 0, S_KEPT, S_OUTSIDE, S_MASKED, S_UNSUPPORTED, S_T_LAST, S_HEAD = 8 };      // state block: include/leod_hip.h

struct Entry { unsigned long long key; unsigned fneg, m; };      // key 0: empty; fneg = ~(smallest record index); m = largest time

__device__ __forceinline__ unsigned long long make_key(unsigned slot, int x, int y) {
    return (((unsigned long long)slot << 28) | ((unsigned long long)y << 14) | (unsigned long long)x) + 1ULL;      // < 2^60 + 1, never 0
}
__device__ __forceinline__ unsigned long long mix(unsigned long long k) {        // the finaliser of splitmix64
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ULL;
    k ^= k >> 27; k *= 0x94d049bb133111ebULL;
    return k ^ (k >> 31);
}
// the entry of `key`, claimed if it is not there yet; nullptr only if the table is full (the entry points size it so that it never is).
// Other workgroups claim words of the same table meanwhile.  A key word only ever goes from 0 (the memset) to one key and stays: a
// stale 0 is repaired by the compare-and-swap, which returns what is there, and a non-zero value read is final.  The read is a relaxed
// atomic load so that no compiler keeps the word in a register across probes.
__device__ __forceinline__ Entry* table_insert(Entry* tab, unsigned long long cap, unsigned long long key) {
    unsigned long long h = mix(key) & (cap - 1);
    for (unsigned long long step = 0; step < cap; ++step) {
        unsigned long long k = __atomic_load_n(&tab[h].key, __ATOMIC_RELAXED);
        if (k == 0) k = atomicCAS(&tab[h].key, 0ULL, key);
        if (k == 0 || k == key) return tab + h;
        h = (h + 1) & (cap - 1);
    }
    return nullptr;
}
__device__ __forceinline__ const Entry* table_find(const Entry* tab, unsigned long long cap, unsigned long long key) {
    unsigned long long h = mix(key) & (cap - 1);
    for (unsigned long long step = 0; step < cap; ++step) {
        const unsigned long long k = tab[h].key;
        if (k == key) return tab + h;
        if (k == 0) return nullptr;
        h = (h + 1) & (cap - 1);
    }
    return nullptr;
}

// (a) records [lo, hi): class, insert of the candidates, first position where the time decreases
__global__ __launch_bounds__(BLOCK) void filter_build_kernel(const Rec* __restrict__ rec, long lo, long hi, int H, int W, unsigned width,
                                                             const unsigned char* __restrict__ mask, const long* __restrict__ state,
                                                             Entry* __restrict__ tab, unsigned long long cap,
                                                             unsigned char* __restrict__ cls, long* __restrict__ io) {
    const long i = lo + (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= hi) return;
    Rec e; int x, y;
    const int c = classify(rec, i, state + S_T_LAST, H, W, mask, io, e, x, y);
    if (c == C_KEPT && width) {                                  // width 0: rule 3 is off, nothing is looked up
        Entry* en = table_insert(tab, cap, make_key(e.t / width, x, y));
        if (en) { atomicMax(&en->fneg, ~(unsigned)i); atomicMax(&en->m, e.t); }
    }
    cls[i] = (unsigned char)c;
}

// (b) rule 3 for the candidates of [lo, hi); kept records per tile; the four counters
__global__ __launch_bounds__(BLOCK) void filter_decide_kernel(const Rec* __restrict__ rec, long lo, long hi, int H, int W, unsigned width,
                                                              long* __restrict__ state, const Entry* __restrict__ tab,
                                                              unsigned long long cap, unsigned char* __restrict__ cls,
                                                              unsigned long long* __restrict__ tile_off) {
    const long i = lo + (long)blockIdx.x * BLOCK + threadIdx.x;
    int c = -1;
    if (i < hi) {
        c = cls[i];
        if (c == C_KEPT && width) {
            const Rec e = rec[i];
            const int x = (int)(e.xyp & 16383u), y = (int)((e.xyp >> 14) & 16383u);
            const unsigned tau = width - 1, slot = e.t / width;
            const long since = e.t > tau ? (long)(e.t - tau) : 0L;               // a supporter's time is >= since (and >= 0: -1 is "never")
            const long* last = state + S_HEAD;
            bool ok = false;
            for (int dy = -1; dy <= 1 && !ok; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= H) continue;
                for (int dx = -1; dx <= 1 && !ok; ++dx) {
                    const int qx = x + dx;
                    if (qx < 0 || qx >= W || (dx == 0 && dy == 0)) continue;
                    if (last[(long)qy * W + qx] >= since) { ok = true; break; }
                    const Entry* own = table_find(tab, cap, make_key(slot, qx, qy));
                    if (own && (long)(~own->fneg) < i) { ok = true; break; }
                    if (slot > 0) {
                        const Entry* prev = table_find(tab, cap, make_key(slot - 1, qx, qy));
                        if (prev && (long)prev->m >= since) { ok = true; break; }
                    }
                }
            }
            if (!ok) { c = C_UNSUPPORTED; cls[i] = (unsigned char)c; }
        }
    }
    tally_classes<N_CLASS>(c, tile_off + lo / TILE + blockIdx.x, state + S_KEPT);
}

// (c) the surface takes every event that passed rules 1 and 2, kept or not
__global__ __launch_bounds__(BLOCK) void filter_surface_kernel(const Rec* __restrict__ rec, long lo, long hi, int W,
                                                               const unsigned char* __restrict__ cls, long* __restrict__ state) {
    const long i = lo + (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= hi) return;
    const int c = cls[i];
    if (c != C_KEPT && c != C_UNSUPPORTED) return;
    const Rec e = rec[i];                                        // in the sensor: the build pass classified it
    const long pix = (long)((e.xyp >> 14) & 16383u) * W + (long)(e.xyp & 16383u);
    atomicMax(reinterpret_cast<long long*>(state + S_HEAD + pix), (long long)e.t);
}

// (d) one workgroup: tile counts -> offsets behind the records emitted so far; seen, last time, the times around a decrease
__global__ __launch_bounds__(BLOCK) void filter_scan_kernel(const Rec* __restrict__ rec, long lo, long hi, long* __restrict__ state,
                                                            unsigned long long* __restrict__ tile_off, long* __restrict__ io) {
    scan_tiles<S_SEEN, S_T_LAST>(rec, lo, hi, state, tile_off, io);
}

__global__ __launch_bounds__(BLOCK) void filter_emit_kernel(const Rec* __restrict__ rec, long n_events, const unsigned char* __restrict__ cls,
                                                            const unsigned long long* __restrict__ tile_off, Rec* __restrict__ out,
                                                            long capacity) {
    __shared__ unsigned long long lds_s[BLOCK / 64];
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    const bool keep = i < n_events && cls[i] == C_KEPT;
    unsigned long long sum;
    const long pos = (long)(tile_off[blockIdx.x] + block_scan_sum(keep ? 1ULL : 0ULL, sum, lds_s));
    if (keep && pos >= 0 && pos < capacity) out[pos] = rec[i];
}

__global__ __launch_bounds__(BLOCK) void pixel_counts_kernel(const Rec* __restrict__ rec, long n_events, int H, int W,
                                                             long* __restrict__ counts, long* __restrict__ outside) {
    unsigned out = 0;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n_events; i += (long)gridDim.x * BLOCK) {
        const unsigned w = rec[i].xyp;
        const int x = (int)(w & 16383u), y = (int)((w >> 14) & 16383u);
        if (x >= W || y >= H) { ++out; continue; }
        atomicAdd(reinterpret_cast<unsigned long long*>(counts + (long)y * W + x), 1ULL);
    }
    out = wave_sum_u32(out);
    if ((threadIdx.x & 63) == 0 && out) atomicAdd(reinterpret_cast<unsigned long long*>(outside), (unsigned long long)out);
}

long table_entries(long n_events) {                              // a power of two, at least twice the events
    long cap = MIN_ENTRIES;
    while (cap < 2 * n_events) cap <<= 1;
    return cap;
}
}  // namespace

LEOD_API int leod_event_filter_query(long n_events, int* tile_events, int* tiles_per_pass, long* table_bytes, long* marks_bytes) {
    if (n_events < 0 || n_events > 0x7fffffffL) return LEOD_ERR_ARG;
    if (tile_events) *tile_events = TILE;
    if (tiles_per_pass) *tiles_per_pass = PASS;
    if (table_bytes) *table_bytes = table_entries(n_events) * (long)sizeof(Entry);
    if (marks_bytes) *marks_bytes = marks_need(n_events);
    return LEOD_OK;
}

LEOD_API int leod_event_filter_scan(const void* records, long n_events, int H, int W, long tau_us, const unsigned char* mask, long* state,
                                    void* table, long table_bytes, void* marks, long marks_bytes, long* io, hipStream_t stream) {
    if (!records_ok(records, n_events) || H < 1 || W < 1 || H > 16384 || W > 16384 || tau_us < -1 || tau_us > 0x7fffffffL) return LEOD_ERR_ARG;
    if (!state || !io || ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(io)) & 7)) return LEOD_ERR_ARG;
    if (n_events == 0) return LEOD_OK;
    if (!table || (reinterpret_cast<uintptr_t>(table) & 15) || !marks || (reinterpret_cast<uintptr_t>(marks) & 7)) return LEOD_ERR_ARG;
    if (marks_bytes < marks_need(n_events)) return LEOD_ERR_ARG;
    // the largest table the buffer holds, and the records per sub-chunk it allows: whole tiles, unless the chunk fits as it is
    long cap = MIN_ENTRIES;
    if (table_bytes < cap * (long)sizeof(Entry)) return LEOD_ERR_ARG;
    while (cap * 2 * (long)sizeof(Entry) <= table_bytes && cap < table_entries(n_events)) cap <<= 1;
    long per = cap / 2;
    if (per < n_events) {
        per = per / TILE * TILE;
        if (per < TILE) return LEOD_ERR_ARG;
    }
    const Rec* rec = static_cast<const Rec*>(records);
    unsigned char* cls = static_cast<unsigned char*>(marks);
    unsigned long long* tile_off = reinterpret_cast<unsigned long long*>(cls + (n_events + 7) / 8 * 8);
    Entry* tab = static_cast<Entry*>(table);
    const unsigned width = (unsigned)(tau_us + 1);                // slot width; 0 for tau_us = -1
    for (long lo = 0; lo < n_events; lo += per) {
        const long hi = lo + per < n_events ? lo + per : n_events;
        const unsigned grid = (unsigned)((hi - lo + BLOCK - 1) / BLOCK);
        if (hipMemsetAsync(tab, 0, (size_t)cap * sizeof(Entry), stream) != hipSuccess) return LEOD_ERR_LAUNCH;
        hipLaunchKernelGGL(filter_build_kernel, dim3(grid), dim3(BLOCK), 0, stream, rec, lo, hi, H, W, width, mask, state, tab,
                           (unsigned long long)cap, cls, io);
        hipLaunchKernelGGL(filter_decide_kernel, dim3(grid), dim3(BLOCK), 0, stream, rec, lo, hi, H, W, width, state, tab,
                           (unsigned long long)cap, cls, tile_off);
        hipLaunchKernelGGL(filter_surface_kernel, dim3(grid), dim3(BLOCK), 0, stream, rec, lo, hi, W, cls, state);
        hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(BLOCK), 0, stream, rec, lo, hi, state, tile_off, io);
        if (leod_launch_status() != LEOD_OK) return LEOD_ERR_LAUNCH;
    }
    return LEOD_OK;
}

LEOD_API int leod_event_filter_emit(const void* records, long n_events, const void* marks, long marks_bytes, void* out, long capacity,
                                    hipStream_t stream) {
    if (!records_ok(records, n_events) || capacity < 0) return LEOD_ERR_ARG;
    if (capacity > 0 && (!out || (reinterpret_cast<uintptr_t>(out) & 7))) return LEOD_ERR_ARG;
    if (n_events == 0) return LEOD_OK;
    if (!marks || (reinterpret_cast<uintptr_t>(marks) & 7) || marks_bytes < marks_need(n_events)) return LEOD_ERR_ARG;
    const unsigned char* cls = static_cast<const unsigned char*>(marks);
    const unsigned long long* tile_off = reinterpret_cast<const unsigned long long*>(cls + (n_events + 7) / 8 * 8);
    hipLaunchKernelGGL(filter_emit_kernel, dim3((unsigned)((n_events + TILE - 1) / TILE)), dim3(BLOCK), 0, stream,
                       static_cast<const Rec*>(records), n_events, cls, tile_off, static_cast<Rec*>(out), capacity);
    return leod_launch_status();
}

LEOD_API int leod_event_pixel_counts(const void* records, long n_events, int H, int W, long* counts, long* outside, hipStream_t stream) {
    if (!records_ok(records, n_events) || H < 1 || W < 1 || H > 16384 || W > 16384 || !counts || !outside) return LEOD_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(outside)) & 7) return LEOD_ERR_ARG;
    if (n_events == 0) return LEOD_OK;
    const long blocks = (n_events + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(pixel_counts_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(BLOCK), 0, stream,
                       static_cast<const Rec*>(records), n_events, H, W, counts, outside);
    return leod_launch_status();
}
