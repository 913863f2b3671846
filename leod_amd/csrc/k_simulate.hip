// Video-to-events simulator (rule: DESIGN.md section 1): luma frames uint8 [K, H, W] with their times -> the 8-byte records of a .dat
// file, in the rule's order (time, then pixel y * W + x, then the candidate's number).  A pixel holds a reference level m, the time t_keep
// of its last kept event and the byte of the last frame; between two frames the table value of its byte moves linearly from l0 to l1, and
// every multiple of the pixel's threshold that the value passes on its way from m is a candidate, at the time the line reaches it
// (integer division, rounded down, but never the earlier frame's own time); a candidate less than refractory_us behind the pixel's last
// kept event is dropped and still moves m.  The rule is SEQUENTIAL per pixel and independent between pixels, and a pixel's frames are
// few: one lane takes one pixel and walks the frames of the call with the pixel's state in registers.
//   leod_simulate_count: (a) sim_walk_kernel<false>: the walk, storing nothing but counts: kept events per pixel (the lane's own word),
//       per tile of TILE pixels (one store per workgroup) and per interval (wave sums added with integer atomics: the same in any order).
//       The state is read, never written.
//   leod_simulate_emit:  (b) sim_scan_kernel, ONE workgroup: the exclusive sum of the tile counts, PASS tiles per pass;
//       (c) sim_walk_kernel<true>: the same walk; a lane's first event goes to its tile's offset + the sum of the counts of the tile's
//       earlier pixels, the next ones behind it: pixel-major, as the sort's pairs key = t - t_base - 1, value = 2 * pixel + polarity.
//       It stores the pixel's state and adds to the counters;  (d) the STABLE sort of pixel_sort.hpp on ceil(log2(t_end - t_base)) key
//       bits: ties in time keep the pixel-major order, which is the rule's (no pass at all for a span of 1 us);  (e) sim_gather_kernel:
//       the records in sorted order;  (f) sim_close_kernel, one lane: frames seen, the time of the last frame.
// Launches run in stream order; no workgroup waits on another.  Every loop is bounded: a walk by n_frames * MAX_CAND, the scan by the
// tile count.  No rank or offset is the return value of an atomic, so two runs give identical bytes.  The head of the state ([0], [5]) is
// read by every workgroup of (a) and (c) and written by (f) alone, behind them.
//
// Bounds: frames are read below n_frames * H * W only, times below n_frames, thresholds and the state's pixel words below H * W, the
// table below 256 (its index is a byte); a pair is stored below n_events only, a record below n_events and below the capacity, a
// scatter position of the sort below n_events; the entry points refuse buffers smaller than leod_simulate_query reports.
#include "pixel_sort.hpp"

namespace {
using namespace filt;
enum { S_FRAMES = 0, S_KEPT, S_ON, S_OFF, S_DROPPED, S_T_LAST, S_HEAD = 8 };     // state block: include/leod_hip.h
constexpr long MAX_CAND = 4097;          // candidates per pixel and interval: 4096 by the limit on the table and the thresholds, + 1 as m lags the value
constexpr int MAX_FRAMES = 65536;        // per call: a lane's kept count (MAX_FRAMES * MAX_CAND) fits 32 bits

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct Sim {
    const unsigned char* frames; int n_frames; long P; const long* times; const int* lut; const int* th_on; const int* th_off; long refr;
};

// (a) EMIT false, (c) EMIT true.  counts layout: tile_cnt [n_tiles] u64, pix_cnt [P] u32, ival_cnt [n_frames] u64 (interval k ends at
// frame k of the call; the first frame of a recording has none)
template <bool EMIT>
__global__ __launch_bounds__(BLOCK) void sim_walk_kernel(Sim s, long* __restrict__ state, unsigned long long* __restrict__ tile_cnt,
                                                         unsigned* __restrict__ pix_cnt, unsigned long long* __restrict__ ival_cnt,
                                                         long t_base, long n_events, unsigned* __restrict__ key, unsigned* __restrict__ idx) {
    __shared__ int lds_lut[256];
    __shared__ unsigned long long lds_s[BLOCK / 64];
    static_assert(BLOCK == 256, "one lane per table entry");
    lds_lut[threadIdx.x] = s.lut[threadIdx.x];
    __syncthreads();
    const long pix = (long)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = pix < s.P;                                                 // a lane without a pixel takes every barrier and wave sum
    const bool fresh = state[S_FRAMES] == 0;
    long* st = state + S_HEAD + 2 * pix;
    unsigned char* last = reinterpret_cast<unsigned char*>(state + S_HEAD + 2 * s.P);
    long m = 0, t_keep = -1, t0;
    int v0 = 0, k = 0;
    if (fresh) {                                                                 // the first frame of a recording sets m and emits nothing
        t0 = s.times[0];
        if (live) { v0 = s.frames[pix]; m = lds_lut[v0]; }
        k = 1;
    } else {
        t0 = state[S_T_LAST];
        if (live) { m = st[0]; t_keep = st[1]; v0 = last[pix]; }
    }
    const long th1 = live ? (long)s.th_on[pix] : 1, th0 = live ? (long)s.th_off[pix] : 1;
    unsigned long long pos = 0;
    if (EMIT) {
        unsigned long long sum;
        pos = tile_cnt[blockIdx.x] + block_scan_sum(live ? (unsigned long long)pix_cnt[pix] : 0ULL, sum, lds_s);
    }
    unsigned kept = 0, n_on = 0, dropped = 0;
    for (; k < s.n_frames; ++k) {
        const long t1 = s.times[k];
        unsigned c = 0;
        if (live) {
            const int v1 = s.frames[(long)k * s.P + pix];
            const long l0 = lds_lut[v0], l1 = lds_lut[v1];
            if (l1 != l0) {
                const bool on = l1 > l0;
                const long th = on ? th1 : th0, dl = on ? l1 - l0 : l0 - l1, gap = on ? l1 - m : m - l1;
                long n = gap >= th && th > 0 ? gap / th : 0;
                if (n > MAX_CAND) n = MAX_CAND;
                if (!EMIT && s.refr == 0) {
                    c = (unsigned)n;                                             // nothing is dropped: the times are not needed to count
                } else {
                    const unsigned long long D = (unsigned long long)(t1 - t0), a0 = (unsigned long long)(on ? m - l0 : l0 - m);
                    for (long j = 1; j <= n; ++j) {                              // level j lies a0 + j * th from l0, which is in (0, dl]
                        unsigned long long dt = D * (a0 + (unsigned long long)(j * th)) / (unsigned long long)dl;
                        if (dt < 1) dt = 1;
                        const long t = t0 + (long)dt;
                        if (t_keep >= 0 && t - t_keep < s.refr) { ++dropped; continue; }
                        t_keep = t;
                        ++c;
                        if (EMIT) {
                            if (pos < (unsigned long long)n_events) {
                                key[pos] = (unsigned)(t - t_base - 1);
                                idx[pos] = 2u * (unsigned)pix + (on ? 1u : 0u);  // H * W < 2^30
                            }
                            ++pos;
                        }
                    }
                }
                m += on ? n * th : -(n * th);
                if (on) n_on += c;
            }
            v0 = v1;
        }
        t0 = t1;
        if (!EMIT && __ballot(c != 0)) {                                         // uniform in the wave
            const unsigned sum = wave_sum_u32(c);                                // 64 * MAX_CAND fits
            if ((threadIdx.x & 63) == 0) atomicAdd(ival_cnt + k, (unsigned long long)sum);
        }
        kept += c;
    }
    if (!EMIT) {
        if (live) pix_cnt[pix] = kept;
        unsigned long long sum;
        block_scan_sum((unsigned long long)kept, sum, lds_s);
        if (threadIdx.x == 0) tile_cnt[blockIdx.x] = sum;
        return;
    }
    if (live) {
        st[0] = m;
        st[1] = t_keep;
        last[pix] = (unsigned char)v0;
    }
    const unsigned long long w_kept = wave_sum_u64(kept), w_on = wave_sum_u64(n_on), w_drop = wave_sum_u64(dropped);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* cnt = reinterpret_cast<unsigned long long*>(state);
        if (w_kept) atomicAdd(cnt + S_KEPT, w_kept);
        if (w_on) atomicAdd(cnt + S_ON, w_on);
        if (w_kept - w_on) atomicAdd(cnt + S_OFF, w_kept - w_on);
        if (w_drop) atomicAdd(cnt + S_DROPPED, w_drop);
    }
}

// (b) one workgroup: exclusive sum of the tile counts, in place
__global__ __launch_bounds__(BLOCK) void sim_scan_kernel(unsigned long long* __restrict__ tile_cnt, long n_tiles) {
    __shared__ unsigned long long lds_s[BLOCK / 64];
    unsigned long long base = 0;
    for (long t0 = 0; t0 < n_tiles; t0 += PASS) {
        const long tile = t0 + threadIdx.x;
        const unsigned long long n = tile < n_tiles ? tile_cnt[tile] : 0ULL;
        unsigned long long sum;
        const unsigned long long off = base + block_scan_sum(n, sum, lds_s);
        if (tile < n_tiles) tile_cnt[tile] = off;
        base += sum;
    }
}

// (e) sorted pairs -> records
__global__ __launch_bounds__(BLOCK) void sim_gather_kernel(const unsigned* __restrict__ key, const unsigned* __restrict__ idx, long n_events,
                                                           long t_base, int W, long P, Rec* __restrict__ out, long capacity) {
    const long j = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_events || j >= capacity) return;
    const unsigned v = idx[j], pix = v >> 1;
    if ((long)pix >= P) return;                                                  // pairs of another call: nothing is stored
    Rec e;
    e.t = (unsigned)((long)key[j] + t_base + 1);
    e.xyp = (pix % (unsigned)W) | ((pix / (unsigned)W) << 14) | ((v & 1u) << 28);
    out[j] = e;
}

// (f)
__global__ void sim_close_kernel(long* __restrict__ state, const long* __restrict__ times, int n_frames) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state[S_FRAMES] += n_frames;
        state[S_T_LAST] = times[n_frames - 1];
    }
}

inline long n_tiles_of(long P) { return (P + TILE - 1) / TILE; }
inline long count_longs(long P) { return n_tiles_of(P) + (P + 1) / 2; }          // tile counts, pixel counts (two to a long)
inline long state_longs(long P) { return S_HEAD + 2 * P + (P + 7) / 8; }
inline bool aligned8(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

bool sim_ok(const void* frames, int n_frames, int H, int W, const void* times, const void* lut, const void* th_on, const void* th_off,
            long refr, const void* state, const void* counts) {
    if (H < 1 || W < 1 || H > 16384 || W > 16384 || (long)H * W >= (1L << 30)) return false;
    if (n_frames < 0 || n_frames > MAX_FRAMES || refr < 0 || refr > 0xffffffffL) return false;
    if (!frames || !aligned8(times) || !lut || !th_on || !th_off || !aligned8(state) || !aligned8(counts)) return false;
    return ((reinterpret_cast<uintptr_t>(lut) | reinterpret_cast<uintptr_t>(th_on) | reinterpret_cast<uintptr_t>(th_off)) & 3) == 0;
}
}  // namespace

LEOD_API int leod_simulate_query(long n_events, int H, int W, int* tile_pixels, int* digit_bits, long* state_longs_out,
                                 long* count_longs_out, long* ws_bytes) {
    if (n_events < 0 || n_events > 0x7fffffffL || H < 1 || W < 1 || H > 16384 || W > 16384 || (long)H * W >= (1L << 30)) return LEOD_ERR_ARG;
    if (tile_pixels) *tile_pixels = TILE;
    if (digit_bits) *digit_bits = DIGIT;
    if (state_longs_out) *state_longs_out = state_longs((long)H * W);
    if (count_longs_out) *count_longs_out = count_longs((long)H * W);
    if (ws_bytes) *ws_bytes = ws_need(n_events);
    return LEOD_OK;
}

LEOD_API int leod_simulate_count(const unsigned char* frames, int n_frames, int H, int W, const long* times_us, const int* lut,
                                 const int* theta_on, const int* theta_off, long refractory_us, const long* state, long* counts,
                                 hipStream_t stream) {
    if (!sim_ok(frames, n_frames, H, W, times_us, lut, theta_on, theta_off, refractory_us, state, counts)) return LEOD_ERR_ARG;
    if (n_frames == 0) return LEOD_OK;
    const long P = (long)H * W, n_tiles = n_tiles_of(P);
    unsigned long long* tile_cnt = reinterpret_cast<unsigned long long*>(counts);
    unsigned* pix_cnt = reinterpret_cast<unsigned*>(counts + n_tiles);
    unsigned long long* ival_cnt = reinterpret_cast<unsigned long long*>(counts + count_longs(P));
    if (hipMemsetAsync(ival_cnt, 0, (size_t)n_frames * 8, stream) != hipSuccess) return LEOD_ERR_LAUNCH;
    const Sim s = {frames, n_frames, P, times_us, lut, theta_on, theta_off, refractory_us};
    hipLaunchKernelGGL(sim_walk_kernel<false>, dim3((unsigned)n_tiles), dim3(BLOCK), 0, stream, s, const_cast<long*>(state), tile_cnt, pix_cnt,
                       ival_cnt, 0L, 0L, (unsigned*)nullptr, (unsigned*)nullptr);
    return leod_launch_status();
}

LEOD_API int leod_simulate_emit(const unsigned char* frames, int n_frames, int H, int W, const long* times_us, const int* lut,
                                const int* theta_on, const int* theta_off, long refractory_us, long* state, long* counts, long t_base,
                                long t_end, long n_events, void* ws, long ws_bytes, void* out, long capacity, hipStream_t stream) {
    if (!sim_ok(frames, n_frames, H, W, times_us, lut, theta_on, theta_off, refractory_us, state, counts)) return LEOD_ERR_ARG;
    if (n_events < 0 || n_events > 0x7fffffffL || capacity < n_events) return LEOD_ERR_ARG;
    if (t_base < 0 || t_end < t_base || t_end > 0xffffffffL) return LEOD_ERR_ARG;
    if (n_frames == 0) return n_events == 0 ? LEOD_OK : LEOD_ERR_ARG;
    if (n_events > 0 && (!aligned8(ws) || ws_bytes < ws_need(n_events) || !aligned8(out) || t_end == t_base)) return LEOD_ERR_ARG;
    const long P = (long)H * W, n_tiles = n_tiles_of(P);
    unsigned long long* tile_cnt = reinterpret_cast<unsigned long long*>(counts);
    unsigned* pix_cnt = reinterpret_cast<unsigned*>(counts + n_tiles);
    const dim3 block(BLOCK);
    const Sim s = {frames, n_frames, P, times_us, lut, theta_on, theta_off, refractory_us};
    const long per = (n_events + TILE - 1) / TILE * TILE;
    const SortWs sw(n_events > 0 ? ws : nullptr, per);
    hipLaunchKernelGGL(sim_scan_kernel, dim3(1), block, 0, stream, tile_cnt, n_tiles);
    hipLaunchKernelGGL(sim_walk_kernel<true>, dim3((unsigned)n_tiles), block, 0, stream, s, state, tile_cnt, pix_cnt,
                       (unsigned long long*)nullptr, t_base, n_events, sw.key[0], sw.idx[0]);
    if (n_events > 0) {
        const int cur = sort_pairs(sw, n_events, key_bits(t_end - t_base), stream);
        hipLaunchKernelGGL(sim_gather_kernel, dim3((unsigned)(per / TILE)), block, 0, stream, sw.key[cur], sw.idx[cur], n_events, t_base, W, P,
                           static_cast<Rec*>(out), capacity);
    }
    hipLaunchKernelGGL(sim_close_kernel, dim3(1), dim3(64), 0, stream, state, times_us, n_frames);
    return leod_launch_status();
}
