// The 8-byte records of a Prophesee .dat file (u32 t; x in bits 0-13, y in bits 14-27, p in bit 28), in stream order, to the words of a
// Metavision RAW payload (EVT2: u32 words, EVT3: u16 words; layout and the project's rules: DESIGN.md section 1), a chunk of records per
// call.  The words of a recording are those of raw_events.encode_evt2 / encode_evt3 (data/utils/raw_events.py) applied to all its events
// at once, however it was cut into chunks.
//
// What a GROUP of events emits (a group is one event; with `vectors` up to 12 events of one t, y, p with strictly ascending x inside the 12
// columns of the first) depends on the group before it (its time high / low and row) and on its index in the recording (the periodic
// TIME_HIGH).  A call works on E = the records the state holds back ++ the chunk's records, m events, in tiles of TILE:
//   (m) enc_mark_kernel (vectors only): flags[i] = 1 where a group starts.  A run is a maximal stretch of equal t, y, p and strictly
//       ascending x; the lane of every run start walks its run and cuts it greedily where x leaves the 12 columns of the group's first
//       event.  x < 16384 ascends strictly, so a walk ends;
//   (g) enc_groups_kernel (vectors only): group starts per tile;
//   (a) enc_count_kernel: a tile sums the group starts of the tiles before it itself (without vectors the index of an event is its group
//       index), then words and vector groups per tile; the order of the times and the 11-bit range of x and y of the chunk's records;
//   (b) enc_scan_kernel, ONE workgroup: exclusive scan of the tile word counts, PASS tiles per pass; the state after the chunk;
//   (c) enc_emit_kernel, one workgroup per tile: every lane recounts its groups and stores their words behind the workgroup prefix sum.
// Launches in stream order; no workgroup waits on another.  With vectors and without `final` the last group of E is held back in the
// state (the next chunk may extend it); its start is a true cut of the greedy rule, which starts afresh at every group start.
//
// Bounds: records are read below n only, held records below 12; flags and the tile tables are indexed below m <= n + 12 and below the
// tile count of n + 12, and the entry points refuse a workspace smaller than leod_evtenc_query reports; a word is stored only at a
// position below `capacity`.
#include "common.hpp"

namespace {
constexpr int BLOCK = 256;
constexpr int LANE_EVENTS = 8;                                   // consecutive events per lane
constexpr int TILE = BLOCK * LANE_EVENTS;                        // 2048 events per tile
constexpr int PASS = BLOCK;
constexpr int HOLD = 12;                                         // the most events of a group
constexpr int HEAD_BYTES = 64;                                   // bad count, first bad position, first unordered position (both as POS_TOP - position)
constexpr long POS_TOP = 1L << 62;
constexpr int HIGH_STEP = 1024;
enum { S_STARTED = 0, S_HI, S_LO, S_Y, S_GROUPS, S_EVENTS, S_WORDS, S_VGROUPS, S_HELD, S_T_LAST, S_CHUNK_WORDS, S_BAD, S_BAD_POS, S_ORDER_POS,
       S_T_BEFORE, S_T_AT, S_FMT, S_VECTORS, S_PERIOD, S_FIRST_HIGH, S_HELD_REC, S_LONGS = S_HELD_REC + HOLD };

struct Params {
    const uint2* rec; long n;                                    // the chunk's records
    const long* state_in;
    int vectors, final_, period; long first_high;
};
struct Ws { unsigned long long* head; unsigned char* flags; unsigned* tile_groups; unsigned* tile_vg; unsigned long long* tile_words; };

__host__ __device__ inline long tiles_of(long m) { return (m + TILE - 1) / TILE; }
__host__ __device__ inline long flags_bytes(long n) { return (n + HOLD + 15) / 16 * 16; }
__host__ __device__ inline Ws carve(void* ws, long n) {
    Ws w;
    char* p = static_cast<char*>(ws);
    const long T = tiles_of(n + HOLD);
    w.head = reinterpret_cast<unsigned long long*>(p); p += HEAD_BYTES;
    w.flags = reinterpret_cast<unsigned char*>(p); p += flags_bytes(n);
    w.tile_words = reinterpret_cast<unsigned long long*>(p); p += T * 8;
    w.tile_groups = reinterpret_cast<unsigned*>(p); p += T * 4;
    w.tile_vg = reinterpret_cast<unsigned*>(p);
    return w;
}
inline long ws_bytes_of(long n) { return HEAD_BYTES + flags_bytes(n) + tiles_of(n + HOLD) * 16; }

__device__ __forceinline__ int held_of(const long* state_in) {
    const long h = state_in[S_HELD];
    return h < 0 ? 0 : (h > HOLD ? HOLD : (int)h);
}
// event i of E (0 <= i < held + n)
__device__ __forceinline__ uint2 event(const Params& P, int held, long i) {
    if (i < held) { const unsigned long long v = (unsigned long long)P.state_in[S_HELD_REC + i]; return make_uint2((unsigned)v, (unsigned)(v >> 32)); }
    return P.rec[i - held];
}
__device__ __forceinline__ unsigned ex(uint2 r) { return r.y & 16383u; }
__device__ __forceinline__ unsigned ey(uint2 r) { return (r.y >> 14) & 16383u; }
__device__ __forceinline__ unsigned ep(uint2 r) { return (r.y >> 28) & 1u; }
// b continues the run of a, the event before it
__device__ __forceinline__ bool same_run(uint2 a, uint2 b) { return a.x == b.x && ((a.y ^ b.y) & 0x1fffc000u) == 0 && ex(b) > ex(a); }

__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* lds /* [BLOCK / 64] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                             // the previous use of lds is over
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
    for (int w = 0; w < BLOCK / 64; ++w) s += lds[w];
    return s;
}
// exclusive prefix in lane order + the workgroup's total; every lane must call it
__device__ __forceinline__ unsigned long long block_scan_sum(unsigned long long mine, unsigned long long& total, unsigned long long* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long q = __shfl_up(inc, o, 64);
        if (lane >= o) inc += q;
    }
    __syncthreads();
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

// where the emitted events of E end: m, or with a hold the start of its last group (every lane gets it; one barrier)
__device__ __forceinline__ long emit_end(const Params& P, const unsigned char* flags, long m, long* lds) {
    if (threadIdx.x < 64) {
        const long i = m - 1 - (long)threadIdx.x;
        const bool f = P.vectors && !P.final_ && threadIdx.x < HOLD && i >= 0 && flags[i] != 0;
        const unsigned long long b = __ballot(f);
        if (threadIdx.x == 0) *lds = b ? m - (long)__ffsll((long long)b) : m;
    }
    __syncthreads();
    return *lds;
}

// ---- (m) -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void enc_mark_kernel(Params P, unsigned char* __restrict__ flags) {
    const int held = held_of(P.state_in);
    const long m = held + P.n;
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    uint2 b = event(P, held, i);
    if (i > 0 && same_run(event(P, held, i - 1), b)) return;
    flags[i] = 1;                                                // a run starts here; flags were cleared before the launch
    uint2 prev = b;
    for (long j = i + 1; j < m; ++j) {
        const uint2 r = event(P, held, j);
        if (!same_run(prev, r)) break;
        if (ex(r) - ex(b) >= (unsigned)HOLD) { flags[j] = 1; b = r; }
        prev = r;
    }
}

// ---- (g) -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void enc_groups_kernel(Params P, const unsigned char* __restrict__ flags, unsigned* __restrict__ tile_groups) {
    __shared__ unsigned long long lds[BLOCK / 64];
    __shared__ long lds_end;
    const long m = held_of(P.state_in) + P.n;
    const long end = emit_end(P, flags, m, &lds_end);
    const long i0 = (long)blockIdx.x * TILE + (long)threadIdx.x * LANE_EVENTS;
    unsigned n = 0;
#pragma unroll
    for (int e = 0; e < LANE_EVENTS; ++e)
        if (i0 + e < end) n += flags[i0 + e] != 0;
    const unsigned long long s = block_sum(n, lds);
    if (threadIdx.x == 0) tile_groups[blockIdx.x] = (unsigned)s;
}

// ---- what a group emits ----------------------------------------------------------------------------------------------------------
struct Before { long hi; unsigned lo, y; };                      // of the group before
struct Emit { unsigned k, tl, wy, vect; long hi; unsigned lo; }; // k TIME_HIGH words, TIME_LOW?, ADDR_Y?, a vector?
template <int FMT> __device__ __forceinline__ long time_of(const Params& P, uint2 r) { return (long)r.x + (P.first_high << (FMT == 3 ? 12 : 6)); }
template <int FMT> __device__ __forceinline__ Before before_of(const Params& P, uint2 r) {
    const long a = time_of<FMT>(P, r);
    return FMT == 3 ? Before{a >> 12, (unsigned)(a & 4095), ey(r)} : Before{a >> 6, 0u, 0u};
}
__device__ __forceinline__ Before before_of_state(const Params& P) {
    if (!P.state_in[S_STARTED]) return Before{P.first_high, 0u, 0u};
    return Before{P.state_in[S_HI], (unsigned)P.state_in[S_LO], (unsigned)P.state_in[S_Y]};
}
template <int FMT> __device__ __forceinline__ Emit emit_of(const Params& P, uint2 r, const Before& b, long g, bool vect) {
    Emit o;
    const long a = time_of<FMT>(P, r);
    const bool periodic = g % P.period == 0;
    if (FMT == 3) {
        o.hi = a >> 12; o.lo = (unsigned)(a & 4095);
        const long gap = o.hi - b.hi;
        o.k = gap > 0 ? (unsigned)((gap + HIGH_STEP - 1) / HIGH_STEP) : (periodic ? 1u : 0u);
        o.tl = (g == 0 || o.lo != b.lo || gap > 0) ? 1u : 0u;
        o.wy = (g == 0 || ey(r) != b.y) ? 1u : 0u;
        o.vect = vect ? 1u : 0u;
    } else {
        o.hi = a >> 6; o.lo = (unsigned)(a & 63);
        o.k = (o.hi != b.hi || periodic) ? 1u : 0u;
        o.tl = o.wy = o.vect = 0;
    }
    return o;
}
__device__ __forceinline__ unsigned words_of(const Emit& o) { return o.k + o.tl + o.wy + 1u + o.vect; }

// the lane's events of tile `tile`: r[0] is the event before the lane's first (if any), r[1 + e] event i0 + e; start[e]: a group that is
// emitted starts there
template <int VEC> __device__ __forceinline__ void load_lane(const Params& P, int held, long m, long end, const unsigned char* flags, long i0,
                                                              uint2 (&r)[LANE_EVENTS + 1], bool (&start)[LANE_EVENTS]) {
    r[0] = (i0 > 0 && i0 - 1 < m) ? event(P, held, i0 - 1) : make_uint2(0, 0);
#pragma unroll
    for (int e = 0; e < LANE_EVENTS; ++e) {
        const long i = i0 + e;
        r[1 + e] = i < m ? event(P, held, i) : make_uint2(0, 0);
        start[e] = i < end && (!VEC || flags[i] != 0);
    }
}
// groups the tiles before `tile` emit
template <int VEC> __device__ __forceinline__ long groups_before(long tile, const unsigned* tile_groups, unsigned long long* lds) {
    if (!VEC) return tile * TILE;
    unsigned long long n = 0;
    for (long t = threadIdx.x; t < tile; t += BLOCK) n += tile_groups[t];
    return (long)block_sum(n, lds);
}

// ---- (a) -------------------------------------------------------------------------------------------------------------------------
template <int FMT, int VEC> __global__ __launch_bounds__(BLOCK) void enc_count_kernel(Params P, Ws W) {
    __shared__ unsigned long long lds[BLOCK / 64];
    __shared__ long lds_end;
    const int held = held_of(P.state_in);
    const long m = held + P.n;
    const long end = emit_end(P, W.flags, m, &lds_end);
    const long tile = blockIdx.x;
    const long i0 = tile * TILE + (long)threadIdx.x * LANE_EVENTS;
    uint2 r[LANE_EVENTS + 1];
    bool start[LANE_EVENTS];
    load_lane<VEC>(P, held, m, end, W.flags, i0, r, start);
    unsigned ns = 0;
#pragma unroll
    for (int e = 0; e < LANE_EVENTS; ++e) ns += start[e];
    unsigned long long total;
    long g = P.state_in[S_GROUPS] + groups_before<VEC>(tile, W.tile_groups, lds) + (long)block_scan_sum(ns, total, lds);
    const Before b0 = before_of_state(P);
    unsigned long long words = 0, vg = 0;
    unsigned bad = 0;
#pragma unroll
    for (int e = 0; e < LANE_EVENTS; ++e) {
        const long i = i0 + e;
        if (i >= held && i < m) {                                // a record of this chunk: its order and its range
            const long t_before = i > 0 ? (long)r[e].x : P.state_in[S_T_LAST];
            if ((long)r[1 + e].x < t_before) atomicMax(&W.head[2], (unsigned long long)(POS_TOP - (i - held)));
            if (ex(r[1 + e]) >= 2048u || ey(r[1 + e]) >= 2048u) {
                ++bad;
                atomicMax(&W.head[1], (unsigned long long)(POS_TOP - (i - held)));
            }
        }
        if (start[e]) {
            const bool vect = VEC && i + 1 < m && W.flags[i + 1] == 0;
            const Emit o = emit_of<FMT>(P, r[1 + e], i > 0 ? before_of<FMT>(P, r[e]) : b0, g, vect);
            words += words_of(o); vg += o.vect; ++g;
        }
    }
    const unsigned long long tw = block_sum(words, lds), tv = block_sum(vg, lds), tb = block_sum(bad, lds);
    if (threadIdx.x == 0) {
        W.tile_words[tile] = tw; W.tile_vg[tile] = (unsigned)tv;
        if (tb) atomicAdd(&W.head[0], tb);
    }
}

// ---- (b) -------------------------------------------------------------------------------------------------------------------------
// tile_words[t] becomes the position of the tile's first word in the chunk's output
template <int FMT> __global__ __launch_bounds__(BLOCK) void enc_scan_kernel(Params P, Ws W, long n_tiles, long* __restrict__ state_out) {
    __shared__ unsigned long long lds[BLOCK / 64];
    __shared__ long lds_end;
    const int held = held_of(P.state_in);
    const long m = held + P.n;
    const long end = emit_end(P, W.flags, m, &lds_end);
    const long started = P.state_in[S_STARTED];
    unsigned long long words = started ? 0 : 1, vgroups = 0, groups = 0;      // the opening TIME_HIGH is the first call's first word
    for (long t0 = 0; t0 < n_tiles; t0 += PASS) {
        const long tile = t0 + threadIdx.x;
        const bool have = tile < n_tiles;
        unsigned long long sum;
        const unsigned long long off = words + block_scan_sum(have ? W.tile_words[tile] : 0ULL, sum, lds);
        if (have) W.tile_words[tile] = off;
        words += sum;
        vgroups += block_sum(have ? W.tile_vg[tile] : 0u, lds);
        if (P.vectors) groups += block_sum(have ? W.tile_groups[tile] : 0u, lds);
    }
    if (!P.vectors) groups = (unsigned long long)end;
    if (threadIdx.x == 0) {
        const long bad_pos = (long)W.head[1], order_pos = (long)W.head[2];
        state_out[S_STARTED] = 1;
        if (end > 0) {
            const Before b = before_of<FMT>(P, event(P, held, end - 1));
            state_out[S_HI] = b.hi; state_out[S_LO] = b.lo; state_out[S_Y] = b.y;
        } else {
            const Before b = before_of_state(P);
            state_out[S_HI] = b.hi; state_out[S_LO] = b.lo; state_out[S_Y] = b.y;
        }
        state_out[S_GROUPS] = P.state_in[S_GROUPS] + (long)groups;
        state_out[S_EVENTS] = P.state_in[S_EVENTS] + P.n;
        state_out[S_WORDS] = P.state_in[S_WORDS] + (long)words;
        state_out[S_VGROUPS] = P.state_in[S_VGROUPS] + (long)vgroups;
        state_out[S_HELD] = m - end;
        state_out[S_T_LAST] = m > 0 ? (long)event(P, held, m - 1).x : P.state_in[S_T_LAST];
        state_out[S_CHUNK_WORDS] = (long)words;
        state_out[S_BAD] = (long)W.head[0];
        state_out[S_BAD_POS] = bad_pos ? POS_TOP - bad_pos : -1;
        state_out[S_ORDER_POS] = order_pos ? POS_TOP - order_pos : -1;
        state_out[S_T_BEFORE] = state_out[S_T_AT] = 0;
        if (order_pos) {
            const long i = held + (POS_TOP - order_pos);
            state_out[S_T_BEFORE] = i > 0 ? (long)event(P, held, i - 1).x : P.state_in[S_T_LAST];
            state_out[S_T_AT] = (long)event(P, held, i).x;
        }
        state_out[S_FMT] = FMT; state_out[S_VECTORS] = P.vectors; state_out[S_PERIOD] = P.period; state_out[S_FIRST_HIGH] = P.first_high;
    }
    if (threadIdx.x < HOLD) {
        const long i = end + threadIdx.x;
        long v = 0;
        if (i < m) { const uint2 r = event(P, held, i); v = (long)((unsigned long long)r.x | ((unsigned long long)r.y << 32)); }
        state_out[S_HELD_REC + threadIdx.x] = v;
    }
}

// ---- (c) -------------------------------------------------------------------------------------------------------------------------
template <int FMT> __device__ __forceinline__ void put(void* out, long capacity, long pos, unsigned w) {
    if (pos < 0 || pos >= capacity) return;
    if (FMT == 3) static_cast<unsigned short*>(out)[pos] = (unsigned short)w;
    else static_cast<unsigned*>(out)[pos] = w;
}
template <int FMT, int VEC> __global__ __launch_bounds__(BLOCK) void enc_emit_kernel(Params P, Ws W, long n_tiles, void* __restrict__ out,
                                                                                    long capacity) {
    __shared__ unsigned long long lds[BLOCK / 64];
    __shared__ long lds_end;
    const int held = held_of(P.state_in);
    const long m = held + P.n;
    const long tile = blockIdx.x;
    if (tile == 0 && threadIdx.x == 0 && !P.state_in[S_STARTED])
        put<FMT>(out, capacity, 0, FMT == 3 ? 0x8000u | (unsigned)(P.first_high & 4095) : 0x80000000u | (unsigned)(P.first_high & 0x0fffffff));
    if (tile >= n_tiles) return;                                 // the whole workgroup: a call without events has no tile
    const long end = emit_end(P, W.flags, m, &lds_end);
    const long i0 = tile * TILE + (long)threadIdx.x * LANE_EVENTS;
    uint2 r[LANE_EVENTS + 1];
    bool start[LANE_EVENTS];
    load_lane<VEC>(P, held, m, end, W.flags, i0, r, start);
    unsigned ns = 0;
#pragma unroll
    for (int e = 0; e < LANE_EVENTS; ++e) ns += start[e];
    unsigned long long total;
    const long g0 = P.state_in[S_GROUPS] + groups_before<VEC>(tile, W.tile_groups, lds) + (long)block_scan_sum(ns, total, lds);
    const Before b0 = before_of_state(P);
    unsigned long long words = 0;
    long g = g0;
#pragma unroll
    for (int e = 0; e < LANE_EVENTS; ++e)
        if (start[e]) {
            const long i = i0 + e;
            const bool vect = VEC && i + 1 < m && W.flags[i + 1] == 0;
            words += words_of(emit_of<FMT>(P, r[1 + e], i > 0 ? before_of<FMT>(P, r[e]) : b0, g, vect));
            ++g;
        }
    long pos = (long)(W.tile_words[tile] + block_scan_sum(words, total, lds));
    g = g0;
#pragma unroll
    for (int e = 0; e < LANE_EVENTS; ++e)
        if (start[e]) {
            const long i = i0 + e;
            const uint2 ev = r[1 + e];
            const bool vect = VEC && i + 1 < m && W.flags[i + 1] == 0;
            const Before b = i > 0 ? before_of<FMT>(P, r[e]) : b0;
            const Emit o = emit_of<FMT>(P, ev, b, g, vect);
            ++g;
            if (FMT == 3) {
                for (unsigned j = 0; j < o.k; ++j)
                    put<3>(out, capacity, pos++, 0x8000u | (unsigned)((j == o.k - 1 ? o.hi : b.hi + (long)HIGH_STEP * (j + 1)) & 4095));
                if (o.tl) put<3>(out, capacity, pos++, 0x6000u | o.lo);
                if (o.wy) put<3>(out, capacity, pos++, ey(ev) & 2047u);
                const unsigned px = (ep(ev) << 11) | (ex(ev) & 2047u);
                if (!vect) put<3>(out, capacity, pos++, 0x2000u | px);
                else {
                    unsigned mask = 1;
                    for (long j = i + 1; j < m && j < i + HOLD && W.flags[j] == 0; ++j) mask |= 1u << ((ex(event(P, held, j)) - ex(ev)) & 15u);
                    mask &= 4095u;
                    put<3>(out, capacity, pos++, 0x3000u | px);
                    put<3>(out, capacity, pos++, mask >= 256u ? 0x4000u | mask : 0x5000u | mask);
                }
            } else {
                if (o.k) put<2>(out, capacity, pos++, 0x80000000u | (unsigned)(o.hi & 0x0fffffff));
                put<2>(out, capacity, pos++, (ep(ev) << 28) | (o.lo << 22) | ((ex(ev) & 2047u) << 11) | (ey(ev) & 2047u));
            }
        }
}

bool enc_args_ok(const void* records, long n, int fmt, int vectors, int final_, long period, long first_high, const long* state_in,
                 const void* ws, long ws_bytes) {
    if ((fmt != 2 && fmt != 3) || n < 0 || n >= (1L << 31) || period < 1 || period > (1L << 30) || first_high < 0) return false;
    if ((vectors != 0 && vectors != 1) || (final_ != 0 && final_ != 1) || (vectors && fmt != 3)) return false;
    if (first_high >= (fmt == 3 ? 4096L : (1L << 27))) return false;  // EVT2: (t >> 6) + first_high stays below 2^28
    if (n > 0 && (!records || (reinterpret_cast<uintptr_t>(records) & 7))) return false;
    if (!state_in || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < ws_bytes_of(n)) return false;
    return true;
}
}  // namespace

LEOD_API int leod_evtenc_query(long n_events, int fmt, int* tile_events, long* ws_bytes, long* max_words) {
    if (n_events < 0 || n_events >= (1L << 31) || (fmt != 2 && fmt != 3)) return LEOD_ERR_ARG;
    if (tile_events) *tile_events = TILE;
    if (ws_bytes) *ws_bytes = ws_bytes_of(n_events);
    // EVT3: a group takes TIME_LOW, ADDR_Y, a TIME_HIGH, and two words of its own; the fillers of all pauses together cover at most the
    // 2^20 + 4096 TIME_HIGH units a u32 time and the first TIME_HIGH span, 1024 per word.  EVT2: a TIME_HIGH and the event.
    if (max_words) *max_words = fmt == 3 ? 1 + 5 * (n_events + HOLD) + ((1L << 20) + 4096) / HIGH_STEP + 1 : 1 + 2 * n_events;
    return LEOD_OK;
}

LEOD_API int leod_evtenc_scan(const void* records, long n_events, int fmt, int vectors, int final_chunk, long high_period, long first_time_high,
                              const long* state_in, long* state_out, void* ws, long ws_bytes, hipStream_t stream) {
    if (!enc_args_ok(records, n_events, fmt, vectors, final_chunk, high_period, first_time_high, state_in, ws, ws_bytes) || !state_out ||
        state_out == state_in)
        return LEOD_ERR_ARG;
    const Params P{static_cast<const uint2*>(records), n_events, state_in, vectors, final_chunk, (int)high_period, first_time_high};
    const Ws W = carve(ws, n_events);
    const long m_max = n_events + HOLD;                          // the held events are known on the device only
    const unsigned n_tiles = (unsigned)tiles_of(m_max);
    if (hipMemsetAsync(ws, 0, HEAD_BYTES + (vectors ? flags_bytes(n_events) : 0), stream) != hipSuccess) return LEOD_ERR_LAUNCH;
    if (vectors) {
        hipLaunchKernelGGL(enc_mark_kernel, dim3((unsigned)((m_max + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, P, W.flags);
        hipLaunchKernelGGL(enc_groups_kernel, dim3(n_tiles), dim3(BLOCK), 0, stream, P, W.flags, W.tile_groups);
        hipLaunchKernelGGL((enc_count_kernel<3, 1>), dim3(n_tiles), dim3(BLOCK), 0, stream, P, W);
        hipLaunchKernelGGL(enc_scan_kernel<3>, dim3(1), dim3(BLOCK), 0, stream, P, W, (long)n_tiles, state_out);
    } else if (fmt == 3) {
        hipLaunchKernelGGL((enc_count_kernel<3, 0>), dim3(n_tiles), dim3(BLOCK), 0, stream, P, W);
        hipLaunchKernelGGL(enc_scan_kernel<3>, dim3(1), dim3(BLOCK), 0, stream, P, W, (long)n_tiles, state_out);
    } else {
        hipLaunchKernelGGL((enc_count_kernel<2, 0>), dim3(n_tiles), dim3(BLOCK), 0, stream, P, W);
        hipLaunchKernelGGL(enc_scan_kernel<2>, dim3(1), dim3(BLOCK), 0, stream, P, W, (long)n_tiles, state_out);
    }
    return leod_launch_status();
}

LEOD_API int leod_evtenc_emit(const void* records, long n_events, int fmt, int vectors, int final_chunk, long high_period, long first_time_high,
                              const long* state_in, const void* ws, long ws_bytes, void* out, long capacity, hipStream_t stream) {
    if (!enc_args_ok(records, n_events, fmt, vectors, final_chunk, high_period, first_time_high, state_in, ws, ws_bytes) || capacity < 0)
        return LEOD_ERR_ARG;
    if (capacity > 0 && (!out || (reinterpret_cast<uintptr_t>(out) & 3))) return LEOD_ERR_ARG;
    const Params P{static_cast<const uint2*>(records), n_events, state_in, vectors, final_chunk, (int)high_period, first_time_high};
    const Ws W = carve(const_cast<void*>(ws), n_events);
    const unsigned n_tiles = (unsigned)tiles_of(n_events + HOLD);
    if (vectors) hipLaunchKernelGGL((enc_emit_kernel<3, 1>), dim3(n_tiles), dim3(BLOCK), 0, stream, P, W, (long)n_tiles, out, capacity);
    else if (fmt == 3) hipLaunchKernelGGL((enc_emit_kernel<3, 0>), dim3(n_tiles), dim3(BLOCK), 0, stream, P, W, (long)n_tiles, out, capacity);
    else hipLaunchKernelGGL((enc_emit_kernel<2, 0>), dim3(n_tiles), dim3(BLOCK), 0, stream, P, W, (long)n_tiles, out, capacity);
    return leod_launch_status();
}
