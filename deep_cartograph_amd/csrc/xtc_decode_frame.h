// The frame decoder of the XTC reader: the bit reader, unpack3 and xtc_decode_frame, host and device.  xtc.hip runs it a
// lane a frame; a stand-alone host program (tools/xtc_encode_host.cpp) runs the same code on host memory.  The format is
// written out in include/dcv.h.
#pragma once
#include <cmath>

#include "xtc_format.h"

namespace dcv {

// the payload of one frame as a stream of bits, most significant first
struct XtcBits {
    const uint32_t* words;   // 4-byte aligned
    uint32_t n_words;        // nbytes rounded up to whole words: no word at or behind this index is ever loaded
    uint32_t nbytes;
    uint32_t next;           // the next word to load
    uint64_t win;            // the `have` bits not yet handed out, at the top
    int have;
    uint64_t taken, total;   // bits handed out, bits the payload holds

    __host__ __device__ __forceinline__ void open(const uint8_t* p, uint32_t nbytes_) {
        words = reinterpret_cast<const uint32_t*>(p);
        nbytes = nbytes_;
        n_words = (nbytes_ + 3u) >> 2;
        next = 0; win = 0; have = 0; taken = 0;
        total = (uint64_t)nbytes_ * 8u;
    }
    // n in [0, 32]; behind the payload the bits are zero
    __host__ __device__ __forceinline__ uint32_t get(int n) {
        if (have < n) {
            uint32_t w = 0;
            if (next < n_words) {
                w = __builtin_bswap32(words[next]);
                const uint32_t left = nbytes - 4u * next;   // payload bytes in this word, >= 1
                if (left < 4u) w &= ~(0xffffffffu >> (8u * left));
            }
            ++next;
            win |= (uint64_t)w << (32 - have);
            have += 32;
        }
        taken += (uint64_t)n;
        if (n == 0) return 0;
        const uint32_t v = (uint32_t)(win >> (64 - n));
        win <<= n;
        have -= n;
        return v;
    }
    __host__ __device__ __forceinline__ bool overrun() const { return taken > total; }
};

// v / d in place and v % d, v in three 32-bit limbs (least significant first), 1 <= d
__host__ __device__ __forceinline__ uint32_t xtc_divmod(xtc_limb (&v)[3], uint32_t d) {
    uint64_t rem = 0;
#pragma unroll
    for (int j = 2; j >= 0; --j) {
        const uint64_t cur = (rem << 32) | v[j];
        const uint64_t q = cur / d;
        rem = cur - q * d;
        v[j] = (uint32_t)q;
    }
    return (uint32_t)rem;
}

// three integers packed into nbits <= 72 bits (dcv.h: unpack3)
__host__ __device__ __forceinline__ void xtc_unpack3(XtcBits& in, int nbits, uint32_t s1, uint32_t s2, uint32_t (&n)[3]) {
    xtc_limb v[3] = {0, 0, 0};
    const int full = nbits >> 3, rest = nbits & 7;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int b = full - 4 * j;   // whole bytes of this limb and the ones above it
        if (b >= 4) v[j] = __builtin_bswap32(in.get(32));
        else if (b > 0) v[j] = __builtin_bswap32(in.get(8 * b) << (32 - 8 * b));
    }
    if (rest) v[full >> 2] |= in.get(rest) << (8 * (full & 3));
    n[2] = xtc_divmod(v, s2);
    n[1] = xtc_divmod(v, s1);
    n[0] = v[0];
}

// One compressed frame: descriptor `d`, payload inside `bytes`; returns the frame's status.  `live` = false (a lane behind
// the last frame) decodes nothing.  Every coordinate goes through emit(atom, x, y, z), atom < natoms checked here; after
// every iteration -- all frames of a launch have the same natoms, so the trip count is the same in every lane, and a
// frame that is marked idles through the rest -- step(decoded, emitted) is called with the numbers of atoms read and
// written so far: decoded is the same in every live lane, emitted is decoded or one less (the atom in front of a run
// waits for the run's first small atom).  Host and device: the kernel runs it one lane a frame, a stand-alone host
// program can run the same code on host memory.
template <class Emit, class Step>
__host__ __device__ __forceinline__ int xtc_decode_frame(const uint8_t* bytes, const dcv_xtc_frame& d, int32_t natoms, float scale, bool live,
                                                         Emit&& emit_atom, Step&& step) {
#pragma clang fp contract(off)
    int status = DCV_XTC_OK;
    int smallidx = d.smallidx;
    uint32_t sizeint[3] = {1, 1, 1};
    if (live) {
        bool header_ok = std::isfinite(d.precision) && d.precision > 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            header_ok = header_ok && d.maxint[k] >= d.minint[k];
            sizeint[k] = (uint32_t)d.maxint[k] - (uint32_t)d.minint[k] + 1u;
            header_ok = header_ok && sizeint[k] != 0;   // the whole int32 range: 2^32 sizes, which the format cannot hold
        }
        if (!header_ok) status = DCV_XTC_HEADER;
        else if (smallidx < kXtcFirstIdx || smallidx > kXtcLastIdx) status = DCV_XTC_SMALLIDX;
    }
    bool active = live && status == DCV_XTC_OK;
    if (!active) {   // nothing of a marked frame's descriptor is used
        smallidx = kXtcFirstIdx;
        sizeint[0] = sizeint[1] = sizeint[2] = 1;
    }
    int bitsize, bitsizeint[3] = {0, 0, 0};
    if ((sizeint[0] | sizeint[1] | sizeint[2]) > 0xffffffu) {
        bitsize = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) bitsizeint[k] = xtc_bits_of(sizeint[k]);
    } else {
        bitsize = xtc_product_bits(sizeint[0], sizeint[1], sizeint[2]);
    }
    const float inv = 1.0f / d.precision;

    XtcBits in;
    in.open(bytes + (active ? d.offset : 0), active ? (uint32_t)d.nbytes : 0u);
    int32_t smaller = xtc_magic(smallidx - 1 > kXtcFirstIdx ? smallidx - 1 : kXtcFirstIdx) / 2;
    int32_t smallnum = xtc_magic(smallidx) / 2;
    uint32_t sizesmall = (uint32_t)xtc_magic(smallidx);

    int32_t emitted = 0;                     // atoms written
    int run = 0, left = 0, is_smaller = 0;   // small atoms of the current run still to read
    bool first = false;                      // the next small atom is the first of its run
    uint32_t prev[3] = {0, 0, 0};            // the atom decoded last (32-bit wrapping sums)

    auto emit = [&](const uint32_t (&v)[3]) {
        if (emitted < natoms) {
            float x[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = ((float)(int32_t)v[c] * inv) * scale;
            emit_atom(emitted, x[0], x[1], x[2]);
        }
        ++emitted;
    };

    for (int32_t decoded = 0; decoded < natoms;) {
        if (active) {
            const bool small = left > 0;
            uint32_t n[3];
            if (!small && bitsize == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] = in.get(bitsizeint[k]);
            } else {
                xtc_unpack3(in, small ? smallidx : bitsize, small ? sizesmall : sizeint[1], small ? sizesmall : sizeint[2], n);
            }
            bool update = false;   // the end of an atom group: smallidx moves
            if (!small) {
#pragma unroll
                for (int k = 0; k < 3; ++k) prev[k] = n[k] + (uint32_t)d.minint[k];
                is_smaller = 0;
                if (in.get(1)) {
                    run = (int)in.get(5);
                    is_smaller = run % 3;
                    run -= is_smaller;
                    is_smaller -= 1;
                }
                if (run > 0) {
                    left = run / 3;
                    first = true;
                    if (decoded + 1 + left > natoms) {   // the run would pass natoms: nothing of it is read
                        status = DCV_XTC_RUN;
                        active = false;
                    }
                } else {
                    emit(prev);
                    update = true;
                }
            } else {
                uint32_t cur[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) cur[k] = n[k] + prev[k] - (uint32_t)smallnum;
                emit(cur);
                if (first) emit(prev);   // the water swap: the atom in front of the run is written behind its first small atom
                first = false;
#pragma unroll
                for (int k = 0; k < 3; ++k) prev[k] = cur[k];
                update = --left == 0;
            }
            if (active && in.overrun()) {
                status = DCV_XTC_SHORT;
                active = false;
            }
            if (active && update) {
                smallidx += is_smaller;
                if (smallidx < kXtcFirstIdx || smallidx > kXtcLastIdx) {
                    if (decoded + 1 < natoms) status = DCV_XTC_SMALLIDX;   // behind the last atom the value is never used
                    active = false;
                    smallidx = kXtcFirstIdx;
                } else {
                    if (is_smaller < 0) {
                        smallnum = smaller;
                        smaller = smallidx > kXtcFirstIdx ? xtc_magic(smallidx - 1) / 2 : 0;
                    } else if (is_smaller > 0) {
                        smaller = smallnum;
                        smallnum = xtc_magic(smallidx) / 2;
                    }
                    sizesmall = (uint32_t)xtc_magic(smallidx);
                }
            }
        }
        ++decoded;
        step(decoded, emitted);
    }
    return status;
}

}  // namespace dcv
