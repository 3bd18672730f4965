// The frame encoder of the XTC writer: quantisation, the policy that chooses the groups, pack3 and the bit writer, host
// and device.  xtc_encode.hip runs it a lane a frame; a stand-alone host program (tools/xtc_encode_host.cpp) runs the same
// code on host memory.  The contract -- quantisation, policy, capacity -- is written out in include/dcv.h.
#pragma once
#include <cmath>

#include "xtc_format.h"

namespace dcv {

constexpr int kXtcLookahead = 8;   // a group is its first atom and at most this many behind it

// bytes of a frame's slot: 102 bits an atom (96 of a full-range atom, 6 of flag and run; a small atom costs at most 72),
// rounded up to whole 4-byte words.  A raw frame (at most 9 atoms, 12 bytes each) fits as well.
__host__ __device__ __forceinline__ int64_t xtc_slot_bytes(int32_t natoms) { return (((int64_t)102 * natoms + 7) / 8 + 3) / 4 * 4; }

// the payload of one frame written as a stream of bits, most significant first, in finished big-endian 32-bit words
struct XtcBitWriter {
    uint32_t* words;     // the frame's slot, 4-byte aligned
    uint32_t n_words;    // words of the slot: nothing is stored at or behind this index
    uint32_t next;       // the next word to store
    uint64_t win;        // the `have` bits not yet stored, at the top
    int have;            // < 32 between calls
    uint64_t total;      // bits written
    bool overflow;       // a word did not fit the slot (the capacity bound makes that impossible; checked all the same)

    __host__ __device__ __forceinline__ void open(uint32_t* p, uint32_t n_words_) {
        words = p; n_words = n_words_;
        next = 0; win = 0; have = 0; total = 0; overflow = false;
    }
    __host__ __device__ __forceinline__ void store(uint32_t w) {
        if (next < n_words) words[next] = __builtin_bswap32(w);
        else overflow = true;
        ++next;
    }
    // the low n bits of v, n in [0, 32]; v has no bits above them
    __host__ __device__ __forceinline__ void put(uint32_t v, int n) {
        if (n == 0) return;
        win |= (uint64_t)v << (64 - have - n);   // have + n <= 63
        have += n;
        total += (uint64_t)n;
        if (have >= 32) {
            store((uint32_t)(win >> 32));
            win <<= 32;
            have -= 32;
        }
    }
    // the last word, padded with zero bits; returns the payload's bytes
    __host__ __device__ __forceinline__ uint32_t close() {
        if (have > 0) store((uint32_t)(win >> 32));
        have = 0;
        return (uint32_t)((total + 7) >> 3);
    }
};

// (n0 * s1 + n1) * s2 + n2 in nbits <= 72 bits, the inverse of unpack3 (dcv.h): whole bytes least significant first, then
// the remaining bits.  n0, n1, n2 and the sizes below 2^24 (or the product below 2^nbits in any case)
__host__ __device__ __forceinline__ void xtc_pack3(XtcBitWriter& out, int nbits, uint32_t s1, uint32_t s2, const uint32_t (&n)[3]) {
    const uint64_t t = (uint64_t)n[0] * s1 + n[1];              // < 2^48
    const uint64_t lo = (t & 0xffffffffu) * s2 + n[2];          // < 2^56 + 2^24
    const uint64_t hi = (t >> 32) * s2 + (lo >> 32);            // < 2^40 + 2^25
    const xtc_limb v[3] = {(xtc_limb)lo, (xtc_limb)hi, (xtc_limb)(hi >> 32)};
    const int full = nbits >> 3, rest = nbits & 7;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int b = full - 4 * j;   // whole bytes of this limb and the ones above it
        if (b >= 4) out.put(__builtin_bswap32(v[j]), 32);
        else if (b > 0) out.put(__builtin_bswap32(v[j]) >> (32 - 8 * b), 8 * b);
    }
    if (rest) out.put((v[full >> 2] >> (8 * (full & 3))) & ((1u << rest) - 1u), rest);
}

// One coordinate quantised (dcv.h): lf = (x * inv_scale) * precision, i = trunc(lf + copysign(0.5, lf)), float32, never
// contracted.  `bad` collects DCV_XTC_ENC_NONFINITE (bit 0) and DCV_XTC_ENC_RANGE (bit 1); a bad value gives 0.
__host__ __device__ __forceinline__ int32_t xtc_quantise(float x, float inv_scale, float precision, int& bad) {
#pragma clang fp contract(off)
    const float lf = (x * inv_scale) * precision;
    if (!std::isfinite(x)) { bad |= 1; return 0; }
    if (!(fabsf(lf) < 2147483520.0f)) { bad |= 2; return 0; }
    return (int32_t)truncf(lf + copysignf(0.5f, lf));
}

// One compressed frame of natoms > 9 atoms.  fetch(a, x) gives the three coordinates of atom a; stage(pass, p) is called
// at the top of iteration p of pass 0 (minima, maxima, the smallest step between neighbours) and of pass 1 (the stream):
// every lane of a wave calls it with the same p, and fetch is then used for atoms p .. min(p + kXtcLookahead, natoms - 1)
// only.  Every iteration of pass 1 consumes ONE atom and writes one packed triple -- the full-range atom of a group or
// one of its small atoms -- so the lanes of a wave stay in step.  The descriptor fields nbytes, smallidx, precision, raw,
// minint and maxint of `d` are filled (zeros for a marked frame; offset is the caller's); returns the status.  `live`
// = false (a lane behind the last frame) fetches and writes nothing.
template <class Fetch, class Stage>
__host__ __device__ __forceinline__ int xtc_encode_frame(int32_t natoms, float inv_scale, float precision, bool live, uint32_t* slot,
                                                         uint32_t slot_words, dcv_xtc_frame& d, Fetch&& fetch, Stage&& stage) {
    auto quant = [&](int32_t a, int32_t (&q)[3], int& bad) {
        float x[3];
        fetch(a, x);
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = xtc_quantise(x[c], inv_scale, precision, bad);
    };
    d.nbytes = 0; d.smallidx = 0; d.precision = precision; d.raw = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) d.minint[c] = d.maxint[c] = 0;

    // ---- pass 0
    int bad = 0;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN}, last[3] = {0, 0, 0};
    int64_t mindiff = INT64_MAX;
    for (int32_t p = 0; p < natoms; ++p) {
        stage(0, p);
        if (live) {
            int32_t q[3];
            quant(p, q, bad);
            int64_t diff = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lo[c] = q[c] < lo[c] ? q[c] : lo[c];
                hi[c] = q[c] > hi[c] ? q[c] : hi[c];
                const int64_t e = (int64_t)q[c] - last[c];
                diff += e < 0 ? -e : e;
                last[c] = q[c];
            }
            if (p > 0 && diff < mindiff) mindiff = diff;
        }
    }
    const int status = (bad & 1) ? DCV_XTC_ENC_NONFINITE : (bad & 2) ? DCV_XTC_ENC_RANGE : DCV_XTC_OK;
    const bool active = live && status == DCV_XTC_OK;

    int smallidx = kXtcFirstIdx;
    uint32_t sizeint[3] = {1, 1, 1};
    if (active) {
        while (smallidx < kXtcLastIdx && (int64_t)xtc_magic(smallidx) < mindiff) ++smallidx;
#pragma unroll
        for (int c = 0; c < 3; ++c) sizeint[c] = (uint32_t)hi[c] - (uint32_t)lo[c] + 1u;
    } else {
        lo[0] = lo[1] = lo[2] = 0;
    }
    const int smallidx0 = smallidx;
    int bitsize, bitsizeint[3] = {0, 0, 0};
    if ((sizeint[0] | sizeint[1] | sizeint[2]) > 0xffffffu) {
        bitsize = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) bitsizeint[c] = xtc_bits_of(sizeint[c]);
    } else {
        bitsize = xtc_product_bits(sizeint[0], sizeint[1], sizeint[2]);
    }

    // ---- pass 1
    XtcBitWriter out;
    out.open(slot, active ? slot_words : 0u);
    int run = 0;              // the run value written last
    int left = 0;             // small atoms of the current group still to write
    bool first = false;       // the next small atom is the group's first: atom p - 1 coded against the full-range atom p
    int step_idx = 0;         // the step of smallidx at the end of the current group
    int32_t prev[3] = {0, 0, 0}, held[3] = {0, 0, 0};   // the atom small atoms are coded against; the group's first atom
    for (int32_t p = 0; p < natoms; ++p) {
        stage(1, p);
        if (!active) continue;
        const int32_t smallnum = xtc_magic(smallidx) / 2;
        const uint32_t sizesmall = (uint32_t)xtc_magic(smallidx);
        int ignore = 0;
        if (left == 0) {   // a group starts at p: how far does it reach?
            const int64_t smaller = xtc_magic(smallidx - 1 > kXtcFirstIdx ? smallidx - 1 : kXtcFirstIdx) / 2;
            int32_t q0[3], q1[3];
            quant(p, q0, ignore);
            int r = 0;
            bool all_smaller = true;
            auto reach = [&](const int32_t (&a)[3], const int32_t (&b)[3]) {
                bool ok = true, small = true;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int64_t e = (int64_t)a[c] - b[c];
                    ok = ok && e + smallnum >= 0 && e + smallnum < (int64_t)sizesmall;
                    small = small && (e < 0 ? -e : e) < smaller;
                }
                if (ok) all_smaller = all_smaller && small;
                return ok;
            };
            if (p + 1 < natoms) {
                quant(p + 1, q1, ignore);
                if (reach(q0, q1)) {
                    r = 1;
                    int32_t pv[3] = {q0[0], q0[1], q0[2]};
                    while (r < kXtcLookahead && p + 1 + r < natoms) {
                        int32_t qn[3];
                        quant(p + 1 + r, qn, ignore);
                        if (!reach(qn, pv)) break;
#pragma unroll
                        for (int c = 0; c < 3; ++c) pv[c] = qn[c];
                        ++r;
                    }
                }
            }
            if (r == 0) step_idx = smallidx < kXtcLastIdx ? 1 : 0;
            else step_idx = (smallidx > kXtcFirstIdx && all_smaller) ? -1 : 0;
            const int32_t (&big)[3] = r ? q1 : q0;   // the water swap: the full-range atom of a run is the SECOND atom
            uint32_t n[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = (uint32_t)big[c] - (uint32_t)lo[c];
            if (bitsize == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) out.put(n[c], bitsizeint[c]);
            } else {
                xtc_pack3(out, bitsize, sizeint[1], sizeint[2], n);
            }
            if (3 * r == run && step_idx == 0) {
                out.put(0u, 1);
            } else {
                out.put(1u, 1);
                out.put((uint32_t)(3 * r + step_idx + 1), 5);
                run = 3 * r;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { prev[c] = big[c]; held[c] = q0[c]; }
            left = r;
            first = true;
            if (r == 0) smallidx += step_idx;
        } else {           // a small atom: the group's first atom against the full-range one, then the atoms behind it in order
            int32_t cur[3];
            if (first) {
#pragma unroll
                for (int c = 0; c < 3; ++c) cur[c] = held[c];
            } else {
                quant(p, cur, ignore);
            }
            first = false;
            uint32_t n[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                n[c] = (uint32_t)cur[c] - (uint32_t)prev[c] + (uint32_t)smallnum;
                prev[c] = cur[c];
            }
            xtc_pack3(out, smallidx, sizesmall, sizesmall, n);
            if (--left == 0) smallidx += step_idx;
        }
    }
    if (!active) return status;
    d.nbytes = (int32_t)out.close();
    d.smallidx = smallidx0;
#pragma unroll
    for (int c = 0; c < 3; ++c) { d.minint[c] = lo[c]; d.maxint[c] = hi[c]; }
    return out.overflow ? DCV_XTC_ENC_RANGE : status;   // unreachable by the capacity bound
}

}  // namespace dcv
