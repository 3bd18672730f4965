// GROMACS XTC frames decoded on the device (import_trajectories): the compressed bytes of a chunk of frames in, float32
// coordinates out, straight into a dense (n, A, 3) array or the planes of a DCD record image.  The format and the
// algorithm are written out in include/dcv.h.
//
// A LANE owns a frame.  Inside a frame the bit stream is strictly sequential -- the position of every field depends on
// the fields before it -- so there is nothing to spread over lanes; frames are independent, so there are as many streams
// as frames.  A workgroup is one wave (64 frames): a wave lasts as long as its longest frame, and with one-wave
// workgroups a finished wave frees its slot at once.
//
// The loop decodes ONE atom per iteration, a full-range one or a small one of a run, through the same unpack3 call:
// lanes that stand at different places of the format still execute the limb divisions -- nearly all of the arithmetic --
// together, and every lane of a wave has read the same number of atoms after every iteration.  The bit reader keeps a
// 64-bit window, most significant bit first, refilled by aligned 4-byte loads with a byte swap; it never loads a word at
// or behind nbytes rounded up to 4 (the host has checked that this much lies inside the uploaded bytes), masks the bytes
// of the last word that lie behind nbytes and marks the frame when more bits are asked for than the payload holds.
//
// Stores.  A lane that stored its own coordinates as it produced them would make every store of the wave touch 64 lines,
// one per frame (measured, 1M frames x 256 atoms: 8.3 ms into dense rows, 14.7 ms into the planes of DCD records, for
// the same arithmetic).  Because the lanes stay within one atom of each other, a lane instead keeps its
// last nine atoms in LDS and the WAVE stores blocks of eight atoms of its 64 frames in contiguous pieces (xtc_flush
// below); the atom counter of every frame is checked before each of those stores.  7.3 KB of LDS a wave, no atomics.
#include <cmath>

#include "common.h"

namespace dcv {

constexpr int kXtcThreads = 64;
constexpr int kXtcFirstIdx = 9, kXtcLastIdx = 72;

// magic[i], 0 <= i <= 72; a function so that the host build of the decoder (a stand-alone check) reads the same table
__host__ __device__ __forceinline__ int32_t xtc_magic(int i) {
    constexpr int32_t kMagic[kXtcLastIdx + 1] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 10, 12, 16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512, 645, 812, 1024, 1290, 1625,
    2048, 2580, 3250, 4096, 5060, 6501, 8192, 10321, 13003, 16384, 20642, 26007, 32768, 41285, 52015, 65536, 82570, 104031, 131072, 165140,
    208063, 262144, 330280, 416127, 524287, 660561, 832255, 1048576, 1321122, 1664510, 2097152, 2642245, 3329021, 4194304, 5284491, 6658042,
    8388607, 10568983, 13316085, 16777216};
    return kMagic[i];
}

struct XtcArgs {
    const uint8_t* bytes;
    const dcv_xtc_frame* frames;   // in the workspace
    float* out;
    int32_t* status;
    int64_t n_frames;
    int64_t ofs, oas, ocs;
    int32_t n_atoms;
    float scale;
};

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
__host__ __device__ __forceinline__ uint32_t xtc_divmod(uint32_t (&v)[3], uint32_t d) {
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
    uint32_t v[3] = {0, 0, 0};
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

// The staging of a wave (64 frames) in LDS: a lane keeps its last kXtcRing atoms, word ((slot*3 + c)*65 + lane) -- lanes on
// consecutive banks when they write, and the 24 words of a frame's block on different banks when the wave reads them
// back --, and when every live lane has written the atoms of a block of kXtcBlock the WAVE stores the 64 blocks: lane j
// of store i takes element 64 i + j of [frame][atom][component] (component fastest where the output has it fastest,
// atom fastest for planes), so a store covers contiguous pieces of 96 bytes (dense rows) or 32 bytes (planes) instead
// of 64 single floats in 64 different lines.  A block is flushed when decoded == kXtcBlock (b + 1) + 1: every live lane
// has then written at least kXtcBlock (b + 1) atoms and at most one more, kXtcBlock + 1 atoms from the block's first:
// the ring.  The atoms a marked frame did not write are not stored (cnt[] holds every lane's count).
constexpr int kXtcBlock = 8, kXtcRing = kXtcBlock + 1, kXtcPitch = kXtcThreads + 1;

__device__ __forceinline__ void xtc_flush(const XtcArgs& a, const float* ring, const int32_t* cnt, int64_t f0, int32_t block, bool comp_fast) {
    constexpr int kPer = 3 * kXtcBlock;   // floats of one frame's block
#pragma unroll 4
    for (int i = 0; i < kPer; ++i) {
        const int e = i * kXtcThreads + (int)threadIdx.x;
        const int L = e / kPer, k = e - L * kPer;
        const int s = comp_fast ? k / 3 : k % kXtcBlock, c = comp_fast ? k - 3 * s : k / kXtcBlock;
        const int32_t atom = block * kXtcBlock + s;
        if (f0 + L < a.n_frames && atom < cnt[L])
            a.out[(f0 + L) * a.ofs + (int64_t)atom * a.oas + c * a.ocs] = ring[((atom % kXtcRing) * 3 + c) * kXtcPitch + L];
    }
}

__global__ __launch_bounds__(kXtcThreads) void xtc_decode_kernel(const XtcArgs a) {
    __shared__ float ring[kXtcRing * 3 * kXtcPitch];
    __shared__ int32_t cnt[kXtcThreads];
    const int lane = (int)threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * kXtcThreads, f = f0 + lane;
    const bool live = f < a.n_frames;
    dcv_xtc_frame d{};
    if (live) d = a.frames[f];
    if (a.n_atoms <= 9) {   // the raw form (the host has checked that every descriptor says so): big-endian floats as they are
#pragma clang fp contract(off)
        if (live) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(a.bytes + d.offset);
            float* out = a.out + f * a.ofs;
            for (int32_t i = 0; i < a.n_atoms; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) out[i * a.oas + c * a.ocs] = __builtin_bit_cast(float, __builtin_bswap32(w[3 * i + c])) * a.scale;
            a.status[f] = DCV_XTC_OK;
        }
        return;
    }
    const bool comp_fast = a.ocs < a.oas;
    int32_t flushed = 0, written = 0;   // blocks stored, atoms this lane has written
    const int status = xtc_decode_frame(
        a.bytes, d, a.n_atoms, a.scale, live,
        [&](int32_t atom, float x, float y, float z) {
            float* p = ring + (atom % kXtcRing) * 3 * kXtcPitch + lane;
            p[0] = x; p[kXtcPitch] = y; p[2 * kXtcPitch] = z;
        },
        [&](int32_t decoded, int32_t emitted) {
            written = emitted < a.n_atoms ? emitted : a.n_atoms;
            if (decoded == kXtcBlock * (flushed + 1) + 1) {   // the same in every lane
                cnt[lane] = written;
                __syncthreads();
                xtc_flush(a, ring, cnt, f0, flushed, comp_fast);
                __syncthreads();
                ++flushed;
            }
        });
    cnt[lane] = written;
    __syncthreads();
    for (; flushed * kXtcBlock < a.n_atoms; ++flushed) xtc_flush(a, ring, cnt, f0, flushed, comp_fast);
    if (live) a.status[f] = status;
}

// last element an output layout reaches, false when that does not fit 60 bits
static bool xtc_extent(int64_t n_frames, int64_t n_atoms, int64_t fs, int64_t as, int64_t cs, int64_t& last) {
    int64_t x, y, z;
    if (__builtin_mul_overflow(n_frames - 1, fs, &x) || __builtin_mul_overflow(n_atoms - 1, as, &y) || __builtin_mul_overflow((int64_t)2, cs, &z))
        return false;
    if (__builtin_add_overflow(x, y, &last) || __builtin_add_overflow(last, z, &last)) return false;
    return last < (int64_t)1 << 60;
}

static bool xtc_disjoint(uintptr_t a_lo, uintptr_t a_hi, uintptr_t b_lo, uintptr_t b_hi) { return a_hi <= b_lo || b_hi <= a_lo; }

}  // namespace dcv

using namespace dcv;

extern "C" size_t dcv_xtc_decode_workspace(int64_t n_frames) {
    if (n_frames < 0 || n_frames > ((int64_t)1 << 40)) return 0;
    return align_up((size_t)n_frames * sizeof(dcv_xtc_frame), 256);
}

extern "C" int dcv_xtc_decode(const void* bytes_d, int64_t n_bytes, const dcv_xtc_frame* frames_h, int64_t n_frames, int32_t n_atoms,
                              float scale, float* out_d, int64_t out_frame_stride, int64_t out_atom_stride, int64_t out_comp_stride,
                              int32_t* status_d, void* ws_d, size_t ws_bytes, void* stream) {
    // ---- validate everything before anything is launched
    DCV_REQUIRE(n_atoms > 0 && n_frames >= 0 && n_frames <= ((int64_t)1 << 40) && n_bytes >= 0 && n_bytes < ((int64_t)1 << 60),
                "dcv_xtc_decode: bad arguments (n_atoms=%d n_frames=%lld n_bytes=%lld)", n_atoms, (long long)n_frames, (long long)n_bytes);
    DCV_REQUIRE(n_frames == 0 || (bytes_d && frames_h && out_d && status_d), "dcv_xtc_decode: a NULL pointer with %lld frames", (long long)n_frames);
    DCV_REQUIRE(out_frame_stride >= 1 && out_atom_stride >= 1 && out_comp_stride >= 1,
                "dcv_xtc_decode: output strides (%lld, %lld, %lld) must all be >= 1", (long long)out_frame_stride, (long long)out_atom_stride,
                (long long)out_comp_stride);
    DCV_REQUIRE((reinterpret_cast<uintptr_t>(bytes_d) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_d) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(status_d) & 3) == 0 && (reinterpret_cast<uintptr_t>(ws_d) & 7) == 0,
                "dcv_xtc_decode: the bytes, the output and the status must be 4-byte aligned, the workspace 8-byte aligned");
    const bool raw = n_atoms <= 9;
    for (int64_t f = 0; f < n_frames; ++f) {
        const dcv_xtc_frame& d = frames_h[f];
        DCV_REQUIRE((d.raw != 0) == raw, "dcv_xtc_decode: frame %lld is %s, which %d atoms are not (raw form: at most 9 atoms)", (long long)f,
                    d.raw ? "raw" : "compressed", n_atoms);
        const int64_t len = raw ? (int64_t)12 * n_atoms : ((int64_t)d.nbytes + 3) / 4 * 4;
        DCV_REQUIRE(d.offset >= 0 && d.offset % 4 == 0 && (raw || d.nbytes >= 0) && d.offset <= n_bytes && len <= n_bytes - d.offset,
                    "dcv_xtc_decode: frame %lld: %lld bytes at offset %lld do not lie on the 4-byte grid inside the %lld bytes given",
                    (long long)f, (long long)len, (long long)d.offset, (long long)n_bytes);
    }
    const size_t need = dcv_xtc_decode_workspace(n_frames);
    if (n_frames > 0 && (!ws_d || ws_bytes < need)) {
        set_error("dcv_xtc_decode: workspace too small (%zu bytes, need %zu)", ws_bytes, need);
        return DCV_ENOMEM;
    }
    if (n_frames == 0) return DCV_OK;
    int64_t out_last;
    DCV_REQUIRE(xtc_extent(n_frames, n_atoms, out_frame_stride, out_atom_stride, out_comp_stride, out_last),
                "dcv_xtc_decode: %lld frames of %d atoms with these strides do not fit the address space", (long long)n_frames, n_atoms);
    const uintptr_t in_lo = reinterpret_cast<uintptr_t>(bytes_d), in_hi = in_lo + (uintptr_t)n_bytes;
    const uintptr_t out_lo = reinterpret_cast<uintptr_t>(out_d), out_hi = out_lo + 4 * (uintptr_t)out_last + 4;
    const uintptr_t st_lo = reinterpret_cast<uintptr_t>(status_d), st_hi = st_lo + 4 * (uintptr_t)n_frames;
    const uintptr_t ws_lo = reinterpret_cast<uintptr_t>(ws_d), ws_hi = ws_lo + need;
    DCV_REQUIRE(xtc_disjoint(in_lo, in_hi, out_lo, out_hi),
                "dcv_xtc_decode: the %lld input bytes and the output elements [0, %lld] overlap in memory", (long long)n_bytes, (long long)out_last);
    DCV_REQUIRE(xtc_disjoint(in_lo, in_hi, st_lo, st_hi) && xtc_disjoint(out_lo, out_hi, st_lo, st_hi) && xtc_disjoint(in_lo, in_hi, ws_lo, ws_hi) &&
                    xtc_disjoint(out_lo, out_hi, ws_lo, ws_hi) && xtc_disjoint(st_lo, st_hi, ws_lo, ws_hi),
                "dcv_xtc_decode: the input bytes, the output, the status words and the workspace must not overlap");
    DCV_REQUIRE(cdiv(n_frames, kXtcThreads) <= 0x7fffffffLL, "dcv_xtc_decode: %lld frames need more than 2^31 - 1 workgroups", (long long)n_frames);

    hipStream_t s = as_stream(stream);
    // a pageable source: the runtime has taken its copy of the descriptors when this call returns
    DCV_CHECK_HIP(hipMemcpyAsync(ws_d, frames_h, (size_t)n_frames * sizeof(dcv_xtc_frame), hipMemcpyHostToDevice, s));
    XtcArgs a{};
    a.bytes = static_cast<const uint8_t*>(bytes_d);
    a.frames = static_cast<const dcv_xtc_frame*>(ws_d);
    a.out = out_d;
    a.status = status_d;
    a.n_frames = n_frames;
    a.ofs = out_frame_stride; a.oas = out_atom_stride; a.ocs = out_comp_stride;
    a.n_atoms = n_atoms;
    a.scale = scale;
    hipLaunchKernelGGL(xtc_decode_kernel, dim3((unsigned)cdiv(n_frames, kXtcThreads)), dim3(kXtcThreads), 0, s, a);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}
