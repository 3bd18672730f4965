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

#include "coords.h"
#include "xtc_decode_frame.h"

namespace dcv {

struct XtcArgs {
    const uint8_t* bytes;
    const dcv_xtc_frame* frames;   // in the workspace
    float* out;
    int32_t* status;
    int64_t n_frames;
    CoordStrides outs;
    int32_t n_atoms;
    float scale;
};

// The staging of a wave (64 frames) in LDS: a lane keeps its last kXtcRing atoms, word ((slot*3 + c)*65 + lane) -- lanes on
// consecutive banks when they write, and the 24 words of a frame's block on different banks when the wave reads them
// back --, and when every live lane has written the atoms of a block of kXtcBlock the WAVE stores the 64 blocks in
// xtc_format.h's block walk: contiguous pieces of 96 bytes (dense rows) or 32 bytes (planes).  A block is flushed when
// decoded == kXtcBlock (b + 1) + 1: every live lane has then written at least kXtcBlock (b + 1) atoms and at most one
// more, kXtcBlock + 1 atoms from the block's first: the ring.  The atoms a marked frame did not write are not stored
// (cnt[] holds every lane's count).
constexpr int kXtcBlock = 8, kXtcRing = kXtcBlock + 1, kXtcPitch = kXtcThreads + 1;

__device__ __forceinline__ void xtc_flush(const XtcArgs& a, const float* ring, const int32_t* cnt, int64_t f0, int32_t block, bool comp_fast) {
    xtc_block_walk<kXtcBlock>(block, comp_fast, [&](int L, int32_t atom, int c) {
        if (f0 + L < a.n_frames && atom < cnt[L])
            a.out[(f0 + L) * a.outs.f + (int64_t)atom * a.outs.a + c * a.outs.c] = ring[((atom % kXtcRing) * 3 + c) * kXtcPitch + L];
    });
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
            float* out = a.out + f * a.outs.f;
            for (int32_t i = 0; i < a.n_atoms; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) out[i * a.outs.a + c * a.outs.c] = __builtin_bit_cast(float, __builtin_bswap32(w[3 * i + c])) * a.scale;
            a.status[f] = DCV_XTC_OK;
        }
        return;
    }
    const bool comp_fast = coord_comp_fast(a.outs);
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
    const CoordStrides outs{out_frame_stride, out_atom_stride, out_comp_stride};
    DCV_REQUIRE_STRIDES_GE1("dcv_xtc_decode", "output strides", outs);
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
    if (n_frames > 0) DCV_REQUIRE_WORKSPACE("dcv_xtc_decode", ws_d, ws_bytes, need);
    if (n_frames == 0) return DCV_OK;
    int64_t out_last;
    DCV_REQUIRE_COORDS_FIT("dcv_xtc_decode", coord_extent(n_frames, n_atoms, outs, out_last), n_frames, n_atoms);
    const Span spans[4] = {span_of(bytes_d, (uintptr_t)n_bytes), coord_span(out_d, out_last), span_of(status_d, 4 * (uintptr_t)n_frames),
                           span_of(ws_d, need)};
    DCV_REQUIRE(spans_disjoint(spans, 2),
                "dcv_xtc_decode: the %lld input bytes and the output elements [0, %lld] overlap in memory", (long long)n_bytes, (long long)out_last);
    DCV_REQUIRE(spans_disjoint(spans, 4), "dcv_xtc_decode: the input bytes, the output, the status words and the workspace must not overlap");
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
    a.outs = outs;
    a.n_atoms = n_atoms;
    a.scale = scale;
    hipLaunchKernelGGL(xtc_decode_kernel, dim3((unsigned)cdiv(n_frames, kXtcThreads)), dim3(kXtcThreads), 0, s, a);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}
