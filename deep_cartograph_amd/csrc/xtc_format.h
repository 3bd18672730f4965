// What the XTC decoder (xtc.hip) and the XTC encoder (xtc_encode.hip) share: the constants and the table of the format,
// the bit lengths of its fields, the limb type of its packed integers and the host-side range checks of both entry
// points.  The format itself is written out in include/dcv.h.
#pragma once
#include "common.h"

namespace dcv {

constexpr int kXtcThreads = 64;   // one wave a workgroup, a lane a frame
constexpr int kXtcFirstIdx = 9, kXtcLastIdx = 72;

// three integers packed into up to 72 bits live in three of these, least significant first
typedef uint32_t xtc_limb;

// magic[i], 0 <= i <= 72; a function so that a host build of the frame coders (a stand-alone check) reads the same table
__host__ __device__ __forceinline__ int32_t xtc_magic(int i) {
    constexpr int32_t kMagic[kXtcLastIdx + 1] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 10, 12, 16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512, 645, 812, 1024, 1290, 1625,
    2048, 2580, 3250, 4096, 5060, 6501, 8192, 10321, 13003, 16384, 20642, 26007, 32768, 41285, 52015, 65536, 82570, 104031, 131072, 165140,
    208063, 262144, 330280, 416127, 524287, 660561, 832255, 1048576, 1321122, 1664510, 2097152, 2642245, 3329021, 4194304, 5284491, 6658042,
    8388607, 10568983, 13316085, 16777216};
    return kMagic[i];
}

__host__ __device__ __forceinline__ int xtc_bits_of(uint32_t size) {   // smallest b with 2^b > size, at most 32
    return size == 0 ? 0 : 32 - __builtin_clz(size);
}

// bit length of a * b * c, each below 2^24
__host__ __device__ __forceinline__ int xtc_product_bits(uint32_t a, uint32_t b, uint32_t c) {
    const uint64_t ab = (uint64_t)a * b;                   // < 2^48
    const uint64_t lo = (ab & 0xffffffffu) * c;            // < 2^56
    const uint64_t hi = (ab >> 32) * c + (lo >> 32);       // < 2^40 + 2^24
    return hi ? 96 - __builtin_clzll(hi) : 32 - __builtin_clz((uint32_t)lo | 1u);   // a, b, c >= 1: the product is not 0
}

// last element a coordinate layout reaches, false when that does not fit 60 bits
inline bool xtc_extent(int64_t n_frames, int64_t n_atoms, int64_t fs, int64_t as, int64_t cs, int64_t& last) {
    int64_t x, y, z;
    if (__builtin_mul_overflow(n_frames - 1, fs, &x) || __builtin_mul_overflow(n_atoms - 1, as, &y) || __builtin_mul_overflow((int64_t)2, cs, &z))
        return false;
    if (__builtin_add_overflow(x, y, &last) || __builtin_add_overflow(last, z, &last)) return false;
    return last < (int64_t)1 << 60;
}

inline bool xtc_disjoint(uintptr_t a_lo, uintptr_t a_hi, uintptr_t b_lo, uintptr_t b_hi) { return a_hi <= b_lo || b_hi <= a_lo; }

}  // namespace dcv
