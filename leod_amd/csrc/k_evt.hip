// Metavision RAW payloads (EVT2: u32 words, EVT3: u16 words; layout and the project's rules: DESIGN.md section 1) to the 8-byte records of
// a Prophesee .dat file (u32 t; x in bits 0-13, y in bits 14-27, p in bit 28), in stream order, a chunk of words per call.
//
// EVT3 is a stateful stream: row, vector base / polarity and the two halves of the time are set by words of their own, one word emits up to
// 12 events.  What a run of words does to the decoder state is a transform T = {which fields it sets, their last values, the first / last
// TIME_HIGH and the clock wraps between them, the vector base as a value (set inside) or as an offset (not set)}.  compose() is
// associative, "unset" included, so a chunk decodes as a scan:
//   (a) evt_reduce_kernel, one workgroup per tile of TILE words: the tile's transform, its ignored / unknown words and its events as a
//       histogram over what they still NEED from before the tile (time high, time low, row, base: 16 classes) -- how many of them are
//       emitted depends on which fields the incoming state has, which no tile knows yet;
//   (b) evt_scan_kernel, ONE workgroup: exclusive scan of the tile transforms from the carried state, PASS tiles per pass, as many passes
//       as it takes; per tile the incoming state, the events it emits under that state and their offset; the state after the chunk;
//   (c) evt_emit_kernel, one workgroup per tile: every lane rescans its words from the tile's incoming state and stores its records behind
//       the workgroup prefix sum of the lanes' event counts.
// Three launches in stream order; no workgroup waits on another.  EVT2 runs through the same skeleton: one last-writer field (TIME_HIGH),
// at most one event per word, no wraps.
//
// A decoder state and a transform are the same thing (the state is the transform of everything read so far, applied to "nothing set").
// The caller's state block is 16 longs (include/leod_hip.h).
//
// Bounds: words are read below n_words only; a record is stored only at a position below `capacity`; the tile tables are indexed by
// blockIdx / a loop below n_tiles, and the entry points refuse a workspace smaller than leod_evt_query reports.
#include "common.hpp"

namespace {
constexpr int LANE_WORDS = 16;                                   // consecutive words per lane
constexpr int BLOCK = 256;
constexpr int TILE = BLOCK * LANE_WORDS;                         // 4096 words per tile
constexpr int PASS = BLOCK;                                      // tile summaries per pass of the scan workgroup
constexpr unsigned F_HIGH = 1, F_LOW = 2, F_Y = 4, F_BASE = 8;
constexpr int SUMMARY_U32 = 24;                                  // T (5), ignored, unknown, pad, need histogram (16)
constexpr int TILE_IN_U32 = 8;                                   // T (5), pad, u64 record offset
enum { S_VALID = 0, S_HIGH, S_WRAPS, S_LOW, S_Y, S_BASE, S_VPOL, S_TIME_BASE, S_EVENTS, S_EARLY, S_IGNORED, S_UNKNOWN, S_OVERFLOW, S_FMT,
       S_CHUNK_EVENTS, S_RESERVED, S_LONGS };

struct T {
    unsigned set, vpol, low, y;                                  // last writers (valid where the bit of `set` is)
    unsigned first, last, wraps;                                 // TIME_HIGH: first and last value, wraps between them
    unsigned base;                                               // F_BASE set: the base after the run; else the columns the run adds to it
};
__device__ __forceinline__ T t_identity() { return T{0, 0, 0, 0, 0, 0, 0, 0}; }

template <int FMT> __device__ __forceinline__ T compose(const T& l, const T& r) {
    T o;
    o.set = l.set | r.set;
    o.low = (r.set & F_LOW) ? r.low : l.low;
    o.y = (r.set & F_Y) ? r.y : l.y;
    o.vpol = (r.set & F_BASE) ? r.vpol : l.vpol;
    o.base = (r.set & F_BASE) ? r.base : l.base + r.base;
    if (!(r.set & F_HIGH)) { o.first = l.first; o.last = l.last; o.wraps = l.wraps; }
    else if (!(l.set & F_HIGH)) { o.first = r.first; o.last = r.last; o.wraps = r.wraps; }
    else {
        o.first = l.first; o.last = r.last;
        o.wraps = l.wraps + r.wraps + ((FMT == 3 && (int)l.last - (int)r.first >= 2048) ? 1u : 0u);
    }
    return o;
}

// five dwords on the wire (shuffles, LDS, the tile tables)
struct P { unsigned w[5]; };
__device__ __forceinline__ P pack(const T& t) {
    return P{{t.set | (t.vpol << 4) | (t.low << 5) | (t.y << 17), t.first, t.last, t.wraps, t.base}};
}
__device__ __forceinline__ T unpack(const P& p) {
    return T{p.w[0] & 15u, (p.w[0] >> 4) & 1u, (p.w[0] >> 5) & 4095u, (p.w[0] >> 17) & 2047u, p.w[1], p.w[2], p.w[3], p.w[4]};
}

// what one word is: events it may emit, the fields they need, and its class for the counters
struct Word { unsigned n, need, mask; int kind; };               // kind: 0 state / event word, 1 ignored, 2 unknown
template <int FMT> __device__ __forceinline__ Word classify(unsigned w) {
    Word o{0, 0, 0, 0};
    if (FMT == 3) {
        const unsigned ty = w >> 12;
        switch (ty) {
            case 0x2: o.n = 1; o.mask = 1; o.need = F_HIGH | F_LOW | F_Y; break;
            case 0x4: o.mask = w & 4095u; o.n = __popc(o.mask); o.need = F_HIGH | F_LOW | F_Y | F_BASE; break;
            case 0x5: o.mask = w & 255u; o.n = __popc(o.mask); o.need = F_HIGH | F_LOW | F_Y | F_BASE; break;
            case 0x0: case 0x3: case 0x6: case 0x8: break;
            case 0x7: case 0xA: case 0xE: case 0xF: o.kind = 1; break;
            default: o.kind = 2;
        }
    } else {
        const unsigned ty = w >> 28;
        if (ty <= 1) { o.n = 1; o.mask = 1; o.need = F_HIGH; }
        else if (ty == 0x8) {}
        else if (ty == 0xA || ty == 0xE || ty == 0xF) o.kind = 1;
        else o.kind = 2;
    }
    return o;
}
// the word's effect on a state or on a transform under construction (= compose with the word's own transform)
template <int FMT> __device__ __forceinline__ void apply(T& s, unsigned w) {
    if (FMT == 3) {
        const unsigned ty = w >> 12, v = w & 4095u;
        if (ty == 0x8) {
            if (!(s.set & F_HIGH)) { s.first = v; s.set |= F_HIGH; }
            else if ((int)s.last - (int)v >= 2048) s.wraps += 1;
            s.last = v;
        } else if (ty == 0x6) { s.low = v; s.set |= F_LOW; }
        else if (ty == 0x0) { s.y = v & 2047u; s.set |= F_Y; }
        else if (ty == 0x3) { s.base = v & 2047u; s.vpol = v >> 11; s.set |= F_BASE; }
        else if (ty == 0x4) s.base += 12;
        else if (ty == 0x5) s.base += 8;
    } else if ((w >> 28) == 0x8) {
        const unsigned v = w & 0x0fffffffu;
        if (!(s.set & F_HIGH)) { s.first = v; s.set |= F_HIGH; }
        s.last = v;
    }
}

// ---- workgroup scans (256 lanes = 4 waves of 64) ---------------------------------------------------------------------------------
// exclusive prefix of the lanes' transforms in lane order + the workgroup's total; every lane must call it
template <int FMT> __device__ __forceinline__ T block_scan(const T& mine, T& total, P* lds /* [4] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        P p = pack(inc), q;
#pragma unroll
        for (int k = 0; k < 5; ++k) q.w[k] = __shfl_up(p.w[k], o, 64);
        if (lane >= o) inc = compose<FMT>(unpack(q), inc);
    }
    P pi = pack(inc), pe;
#pragma unroll
    for (int k = 0; k < 5; ++k) pe.w[k] = __shfl_up(pi.w[k], 1, 64);
    T exc = lane == 0 ? t_identity() : unpack(pe);
    __syncthreads();                                             // the previous use of lds is over
    if (lane == 63) lds[wave] = pi;
    __syncthreads();
    T before = t_identity();
    total = t_identity();
    for (int w = 0; w < BLOCK / 64; ++w) {
        const T tw = unpack(lds[w]);
        if (w < wave) before = compose<FMT>(before, tw);
        total = compose<FMT>(total, tw);
    }
    return compose<FMT>(before, exc);
}
__device__ __forceinline__ unsigned long long block_scan_sum(unsigned long long mine, unsigned long long& total, unsigned long long* lds /* [4] */) {
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

// the lane's words of tile `tile`: w[0 .. nw)
template <int FMT> __device__ __forceinline__ int load_words(const void* words, long n_words, long tile, unsigned (&w)[LANE_WORDS]) {
    const long start = tile * TILE + (long)threadIdx.x * LANE_WORDS;
    const long left = n_words - start;
    const int nw = left >= LANE_WORDS ? LANE_WORDS : (left > 0 ? (int)left : 0);
    if (FMT == 3) {
        const unsigned short* p = static_cast<const unsigned short*>(words) + start;
        if (nw == LANE_WORDS) {                                   // 32 bytes, 16-byte aligned (the entry points demand it of `words`)
            const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
            const unsigned d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) { w[2 * i] = d[i] & 0xffffu; w[2 * i + 1] = d[i] >> 16; }
        } else {
#pragma unroll
            for (int i = 0; i < LANE_WORDS; ++i) w[i] = i < nw ? p[i] : 0u;
        }
    } else {
        const unsigned* p = static_cast<const unsigned*>(words) + start;
        if (nw == LANE_WORDS) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 a = reinterpret_cast<const uint4*>(p)[i];
                w[4 * i] = a.x; w[4 * i + 1] = a.y; w[4 * i + 2] = a.z; w[4 * i + 3] = a.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < LANE_WORDS; ++i) w[i] = i < nw ? p[i] : 0u;
        }
    }
    return nw;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// (a) ------------------------------------------------------------------------------------------------------------------------------
template <int FMT> __global__ __launch_bounds__(BLOCK) void evt_reduce_kernel(const void* __restrict__ words, long n_words,
                                                                              unsigned* __restrict__ summary) {
    __shared__ P lds_t[BLOCK / 64];
    __shared__ unsigned lds_c[19];                               // need histogram [16], ignored, unknown, events that need nothing more
    const long tile = blockIdx.x;
    unsigned w[LANE_WORDS];
    const int nw = load_words<FMT>(words, n_words, tile, w);
    if (threadIdx.x < 19) lds_c[threadIdx.x] = 0;
    T mine = t_identity();
    unsigned ign = 0, unk = 0;
#pragma unroll
    for (int i = 0; i < LANE_WORDS; ++i)
        if (i < nw) {
            const Word c = classify<FMT>(w[i]);
            ign += c.kind == 1; unk += c.kind == 2;
            apply<FMT>(mine, w[i]);
        }
    T total;
    const T exc = block_scan<FMT>(mine, total, lds_t);            // its barriers also order the clear of lds_c before the adds below
    unsigned set = exc.set, n0 = 0;
#pragma unroll
    for (int i = 0; i < LANE_WORDS; ++i)
        if (i < nw) {
            const Word c = classify<FMT>(w[i]);
            const unsigned r = c.need & ~set;
            if (c.n) {
                if (r == 0) n0 += c.n;
                else atomicAdd(&lds_c[r], c.n);                   // only until the tile has set every field: the head of a stream
            }
            T s = t_identity();
            apply<FMT>(s, w[i]);
            set |= s.set;
        }
    n0 = wave_sum_u32(n0); ign = wave_sum_u32(ign); unk = wave_sum_u32(unk);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&lds_c[0], n0); atomicAdd(&lds_c[16], ign); atomicAdd(&lds_c[17], unk); }
    __syncthreads();
    unsigned* s = summary + tile * SUMMARY_U32;
    if (threadIdx.x < 16) s[8 + threadIdx.x] = lds_c[threadIdx.x];
    if (threadIdx.x == 16) {
        const P p = pack(total);
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = p.w[k];
        s[5] = lds_c[16]; s[6] = lds_c[17]; s[7] = 0;
    }
}

// (b) ------------------------------------------------------------------------------------------------------------------------------
template <int FMT> __global__ __launch_bounds__(BLOCK) void evt_scan_kernel(const unsigned* __restrict__ summary, long n_tiles,
                                                                            unsigned* __restrict__ tile_in, const long* state_in,
                                                                            long* state_out) {
    __shared__ P lds_t[BLOCK / 64];
    __shared__ unsigned long long lds_s[BLOCK / 64];
    T carry = t_identity();                                      // every lane keeps the same carried state
    carry.set = (unsigned)state_in[S_VALID] & 15u;
    carry.last = (unsigned)state_in[S_HIGH]; carry.wraps = (unsigned)state_in[S_WRAPS];
    carry.low = (unsigned)state_in[S_LOW] & 4095u; carry.y = (unsigned)state_in[S_Y] & 2047u;
    carry.base = (unsigned)state_in[S_BASE]; carry.vpol = (unsigned)state_in[S_VPOL] & 1u;
    carry.first = (unsigned)(state_in[S_TIME_BASE] >> (FMT == 3 ? 12 : 6));
    unsigned long long events = 0, early = 0, ign = 0, unk = 0;  // of this chunk
    const long c_events = state_in[S_EVENTS], c_early = state_in[S_EARLY], c_ign = state_in[S_IGNORED], c_unk = state_in[S_UNKNOWN];
    const long c_over = state_in[S_OVERFLOW];
    __syncthreads();                                             // state_out may be state_in: every lane has read it before lane 0 writes
    for (long t0 = 0; t0 < n_tiles; t0 += PASS) {
        const long tile = t0 + threadIdx.x;
        const bool have = tile < n_tiles;
        const unsigned* s = summary + tile * SUMMARY_U32;
        T mine = t_identity();
        if (have) { P p; for (int k = 0; k < 5; ++k) p.w[k] = s[k]; mine = unpack(p); }
        T total;
        const T in = compose<FMT>(carry, block_scan<FMT>(mine, total, lds_t));
        unsigned long long n = 0, n_all = 0;
        if (have)
            for (unsigned r = 0; r < 16; ++r) {
                const unsigned h = s[8 + r];
                n_all += h;
                if ((r & ~in.set) == 0) n += h;
            }
        unsigned long long sum;
        const unsigned long long off = events + block_scan_sum(n, sum, lds_s);
        if (have) {
            unsigned* o = tile_in + tile * TILE_IN_U32;
            const P p = pack(in);
            for (int k = 0; k < 5; ++k) o[k] = p.w[k];
            o[5] = 0;
            *reinterpret_cast<unsigned long long*>(o + 6) = off;
        }
        events += sum;
        unsigned long long tot;
        block_scan_sum(n_all - n, tot, lds_s); early += tot;
        block_scan_sum(have ? s[5] : 0u, tot, lds_s); ign += tot;
        block_scan_sum(have ? s[6] : 0u, tot, lds_s); unk += tot;
        carry = compose<FMT>(carry, total);
    }
    if (threadIdx.x == 0) {
        state_out[S_VALID] = carry.set; state_out[S_HIGH] = carry.last; state_out[S_WRAPS] = carry.wraps; state_out[S_LOW] = carry.low;
        state_out[S_Y] = carry.y; state_out[S_BASE] = carry.base; state_out[S_VPOL] = carry.vpol;
        state_out[S_TIME_BASE] = (carry.set & F_HIGH) ? (long)carry.first << (FMT == 3 ? 12 : 6) : 0;
        state_out[S_EVENTS] = c_events + (long)events; state_out[S_EARLY] = c_early + (long)early;
        state_out[S_IGNORED] = c_ign + (long)ign; state_out[S_UNKNOWN] = c_unk + (long)unk;
        state_out[S_OVERFLOW] = c_over; state_out[S_FMT] = FMT; state_out[S_CHUNK_EVENTS] = (long)events; state_out[S_RESERVED] = 0;
    }
}

// (c) ------------------------------------------------------------------------------------------------------------------------------
// shifted time of an event under state s; *bad when it does not fit the record's u32
template <int FMT> __device__ __forceinline__ unsigned event_time(const T& s, unsigned w, bool* bad) {
    long t;
    if (FMT == 3) t = ((((long)s.wraps * 4096 + s.last) << 12) | s.low) - ((long)s.first << 12);
    else t = (((long)s.last << 6) | ((w >> 22) & 63u)) - ((long)s.first << 6);
    if (t < 0 || t > 0xffffffffL) *bad = true;
    return (unsigned)t;
}
template <int FMT> __global__ __launch_bounds__(BLOCK) void evt_emit_kernel(const void* __restrict__ words, long n_words,
                                                                            const unsigned* __restrict__ tile_in, uint2* __restrict__ out,
                                                                            long capacity, long* state_out) {
    __shared__ P lds_t[BLOCK / 64];
    __shared__ unsigned long long lds_s[BLOCK / 64];
    const long tile = blockIdx.x;
    unsigned w[LANE_WORDS];
    const int nw = load_words<FMT>(words, n_words, tile, w);
    T mine = t_identity();
#pragma unroll
    for (int i = 0; i < LANE_WORDS; ++i)
        if (i < nw) apply<FMT>(mine, w[i]);
    const unsigned* ti = tile_in + tile * TILE_IN_U32;
    P p;
#pragma unroll
    for (int k = 0; k < 5; ++k) p.w[k] = ti[k];
    T total;
    const T start = compose<FMT>(unpack(p), block_scan<FMT>(mine, total, lds_t));
    T s = start;
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < LANE_WORDS; ++i)
        if (i < nw) {
            const Word c = classify<FMT>(w[i]);
            if ((c.need & ~s.set) == 0) n += c.n;
            apply<FMT>(s, w[i]);
        }
    unsigned long long sum;
    long pos = (long)(*reinterpret_cast<const unsigned long long*>(ti + 6) + block_scan_sum(n, sum, lds_s));
    s = start;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < LANE_WORDS; ++i)
        if (i < nw) {
            const Word c = classify<FMT>(w[i]);
            if (c.n && (c.need & ~s.set) == 0) {
                const unsigned t = event_time<FMT>(s, w[i], &bad);
                if (FMT == 3) {
                    const bool vect = (w[i] >> 12) != 0x2;
                    const unsigned x0 = vect ? s.base : (w[i] & 2047u), pol = vect ? s.vpol : ((w[i] >> 11) & 1u);
                    for (unsigned m = c.mask; m; m &= m - 1) {   // ascending columns
                        const unsigned x = (x0 + (unsigned)__ffs(m) - 1u) & 16383u;
                        if (pos < capacity) out[pos] = make_uint2(t, x | (s.y << 14) | (pol << 28));
                        ++pos;
                    }
                } else {
                    if (pos < capacity) out[pos] = make_uint2(t, ((w[i] >> 11) & 2047u) | ((w[i] & 2047u) << 14) | ((w[i] >> 28) << 28));
                    ++pos;
                }
            }
            apply<FMT>(s, w[i]);
        }
    if (bad) atomicOr(reinterpret_cast<unsigned long long*>(state_out + S_OVERFLOW), 1ULL);
}

bool evt_args_ok(const void* words, long n_words, int fmt, const void* ws, long ws_bytes) {
    if ((fmt != 2 && fmt != 3) || n_words < 0 || n_words > (1L << 40)) return false;
    if (n_words > 0 && (!words || (reinterpret_cast<uintptr_t>(words) & 15))) return false;
    const long n_tiles = (n_words + TILE - 1) / TILE;
    if (n_tiles > 0 && (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || ws_bytes < n_tiles * (SUMMARY_U32 + TILE_IN_U32) * 4L)) return false;
    return true;
}
}  // namespace

LEOD_API int leod_evt_query(long n_words, int* tile_words, int* tiles_per_pass, long* ws_bytes) {
    if (n_words < 0) return LEOD_ERR_ARG;
    if (tile_words) *tile_words = TILE;
    if (tiles_per_pass) *tiles_per_pass = PASS;
    if (ws_bytes) *ws_bytes = (n_words + TILE - 1) / TILE * (SUMMARY_U32 + TILE_IN_U32) * 4L;
    return LEOD_OK;
}

LEOD_API int leod_evt_scan(const void* words, long n_words, int fmt, const long* state_in, long* state_out, void* ws, long ws_bytes,
                           hipStream_t stream) {
    if (!evt_args_ok(words, n_words, fmt, ws, ws_bytes) || !state_in || !state_out) return LEOD_ERR_ARG;
    const long n_tiles = (n_words + TILE - 1) / TILE;
    unsigned* summary = static_cast<unsigned*>(ws);
    unsigned* tile_in = summary + n_tiles * SUMMARY_U32;
    if (fmt == 3) {
        if (n_tiles) hipLaunchKernelGGL(evt_reduce_kernel<3>, dim3((unsigned)n_tiles), dim3(BLOCK), 0, stream, words, n_words, summary);
        hipLaunchKernelGGL(evt_scan_kernel<3>, dim3(1), dim3(BLOCK), 0, stream, summary, n_tiles, tile_in, state_in, state_out);
    } else {
        if (n_tiles) hipLaunchKernelGGL(evt_reduce_kernel<2>, dim3((unsigned)n_tiles), dim3(BLOCK), 0, stream, words, n_words, summary);
        hipLaunchKernelGGL(evt_scan_kernel<2>, dim3(1), dim3(BLOCK), 0, stream, summary, n_tiles, tile_in, state_in, state_out);
    }
    return leod_launch_status();
}

LEOD_API int leod_evt_emit(const void* words, long n_words, int fmt, const void* ws, long ws_bytes, void* out, long capacity, long* state_out,
                           hipStream_t stream) {
    if (!evt_args_ok(words, n_words, fmt, ws, ws_bytes) || !state_out || capacity < 0) return LEOD_ERR_ARG;
    if (capacity > 0 && (!out || (reinterpret_cast<uintptr_t>(out) & 7))) return LEOD_ERR_ARG;
    const long n_tiles = (n_words + TILE - 1) / TILE;
    if (n_tiles == 0) return LEOD_OK;
    const unsigned* tile_in = static_cast<const unsigned*>(ws) + n_tiles * SUMMARY_U32;
    if (fmt == 3)
        hipLaunchKernelGGL(evt_emit_kernel<3>, dim3((unsigned)n_tiles), dim3(BLOCK), 0, stream, words, n_words, tile_in, static_cast<uint2*>(out),
                           capacity, state_out);
    else
        hipLaunchKernelGGL(evt_emit_kernel<2>, dim3((unsigned)n_tiles), dim3(BLOCK), 0, stream, words, n_words, tile_in, static_cast<uint2*>(out),
                           capacity, state_out);
    return leod_launch_status();
}
