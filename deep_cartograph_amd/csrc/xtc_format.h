// What the XTC decoder (xtc.hip) and the XTC encoder (xtc_encode.hip) share: the constants and the table of the format,
// the bit lengths of its fields, the limb type of its packed integers and the walk in which a wave exchanges a block of
// atoms of its 64 frames between LDS and global memory.  The format itself is written out in include/dcv.h.
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

// Block `block` of kBlock atoms of the 64 frames of a wave, moved by the WAVE between LDS and global memory (the decoder's
// stores, the encoder's loads): lane j of pass i takes element 64 i + j of [frame][atom][component] -- component fastest
// where the layout in global memory has it fastest (comp_fast), atom fastest for planes --, so a pass covers contiguous
// pieces of 12 kBlock bytes (dense rows) or 4 kBlock bytes (planes) instead of 64 single floats in 64 different lines.
// fn(frame of the wave, atom, component) guards and moves one element; atoms are counted in the type of `block`.
template <int kBlock, typename Block, typename Fn>
__device__ __forceinline__ void xtc_block_walk(Block block, bool comp_fast, Fn&& fn) {
    constexpr int kPer = 3 * kBlock;   // floats of one frame's block
#pragma unroll 4
    for (int i = 0; i < kPer; ++i) {
        const int e = i * kXtcThreads + (int)threadIdx.x;
        const int L = e / kPer, k = e - L * kPer;
        const int s = comp_fast ? k / 3 : k % kBlock, c = comp_fast ? k - 3 * s : k / kBlock;
        fn(L, block * kBlock + s, c);
    }
}

}  // namespace dcv
