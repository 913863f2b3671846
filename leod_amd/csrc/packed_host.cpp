// Packed event frames on the host (format: leod_amd/data/utils/packed.py): the validator the frame store runs on
// every blob before a decoder sees it, and the dense decoder of the loaders' host path.  Both are called through ctypes, i.e. with
// the GIL released, from the loaders' reader threads.  The numpy codec in packed.py states the format; these two accept, refuse and
// produce exactly what it does (tests/test_packed_cpu.py).
#include <cstdint>
#include <cstring>

#define LEOD_HOST_API extern "C" __attribute__((visibility("default")))

namespace {
inline uint32_t ld32(const unsigned char* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline uint64_t ld64(const unsigned char* p) { uint64_t v; std::memcpy(&v, p, 8); return v; }
// branch-free population count (this file is built without -mpopcnt, where the builtin is a library call)
inline int popc(uint64_t x) {
    x -= (x >> 1) & 0x5555555555555555ULL;
    x = (x & 0x3333333333333333ULL) + ((x >> 2) & 0x3333333333333333ULL);
    x = (x + (x >> 4)) & 0x0f0f0f0f0f0f0f0fULL;
    return (int)((x * 0x0101010101010101ULL) >> 56);
}
}  // namespace

// 0 = the blob is THE encoding of a frame of E elements; else the first failed check, in the order of packed.validate_frame:
// 1 size (header + group entries, multiple of 16), 2 header padding, 3 size against the counts, 4 padding behind the values,
// 5 marked blocks != n_masks, 6 mask_base, 7 a block beyond the frame, 8 an empty mask, 9 mask bits beyond the frame,
// 10 marked elements != n_values, 11 value_base, 12 a stored zero.
LEOD_HOST_API int leod_evp_validate(const unsigned char* b, long nbytes, long E) {
    if (!b || E < 1) return 1;
    const long G = (E + 4095) / 4096, n_blocks = (E + 63) / 64;
    if (nbytes < 16 + 16 * G || nbytes % 16) return 1;
    for (int i = 8; i < 16; ++i) if (b[i]) return 2;
    const long n_masks = ld32(b), n_values = ld32(b + 4);
    const long size = 16 + 16 * G + 8 * n_masks + n_values;
    if (nbytes != (size + 15) / 16 * 16) return 3;
    for (long p = size; p < nbytes; ++p) if (b[p]) return 4;
    long marked = 0;
    for (long g = 0; g < G; ++g) marked += popc(ld64(b + 16 + 16 * g));
    if (marked != n_masks) return 5;
    long run = 0;
    for (long g = 0; g < G; ++g) {
        if ((long)ld32(b + 16 + 16 * g + 8) != run) return 6;
        run += popc(ld64(b + 16 + 16 * g));
    }
    for (long g = 0; g < G; ++g) {
        const uint64_t l1 = ld64(b + 16 + 16 * g);
        const long first = 64 * g;                               // blocks first .. first + 63
        if (first + 64 > n_blocks) {
            const long keep = n_blocks - first;                  // 1 .. 63 blocks of this group exist
            if (keep < 64 && (l1 >> keep)) return 7;
        }
    }
    const unsigned char* masks = b + 16 + 16 * G;
    const unsigned char* values = masks + 8 * n_masks;
    for (long m = 0; m < n_masks; ++m) if (!ld64(masks + 8 * m)) return 8;
    if (E % 64 && n_masks > 0 && ((ld64(b + 16 + 16 * (G - 1)) >> ((n_blocks - 1) % 64)) & 1) && (ld64(masks + 8 * (n_masks - 1)) >> (E % 64)))
        return 9;
    long m = 0, vrun = 0;
    bool bases_ok = true;
    for (long g = 0; g < G; ++g) {
        bases_ok = bases_ok && (long)ld32(b + 16 + 16 * g + 12) == vrun;
        for (int k = popc(ld64(b + 16 + 16 * g)); k > 0; --k) vrun += popc(ld64(masks + 8 * m++));
    }
    if (vrun != n_values) return 10;
    if (!bases_ok) return 11;
    unsigned char any_zero = 0;
    for (long v = 0; v < n_values; ++v) any_zero |= (unsigned char)(values[v] == 0);
    if (any_zero) return 12;
    return 0;
}

// A blob that passed leod_evp_validate -> out[C * HW] (contiguous); flip != 0 writes the channel planes in reverse order.  Every index is
// still compared with its extent (a blob that was not validated gives a wrong frame, no access outside b or out).  0, or -1 for bad
// arguments.
LEOD_HOST_API int leod_evp_decode(const unsigned char* b, long nbytes, int C, long HW, int flip, unsigned char* out) {
    if (!b || !out || C < 1 || HW < 1) return -1;
    const long E = (long)C * HW, G = (E + 4095) / 4096;
    if (nbytes < 16 + 16 * G) return -1;
    std::memset(out, 0, (size_t)E);
    const long n_masks = ld32(b), n_values = ld32(b + 4);
    const unsigned char* masks = b + 16 + 16 * G;
    if (16 + 16 * G + 8 * n_masks + n_values > nbytes) return -1;
    const unsigned char* values = masks + 8 * n_masks;
    long m = 0, v = 0;
    for (long g = 0; g < G; ++g) {
        uint64_t l1 = ld64(b + 16 + 16 * g);
        while (l1 && m < n_masks) {
            const int i = __builtin_ctzll(l1);
            l1 &= l1 - 1;
            uint64_t mask = ld64(masks + 8 * m++);
            const long e0 = 4096 * g + 64 * i;
            while (mask && v < n_values) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1;
                const long e = e0 + j;
                if (e >= E) break;
                long d = e;
                if (flip) {
                    const long c = e / HW;
                    d = ((long)(C - 1) - c) * HW + (e - c * HW);
                }
                out[d] = values[v++];
            }
        }
    }
    return 0;
}
