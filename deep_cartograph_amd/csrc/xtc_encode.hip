// GROMACS XTC frames written on the device (traj_cluster's cluster ensembles): float32 coordinates in -- a dense
// (n, A, 3) array or the planes of DCD frame records, read in place, optionally gathered through a list of frame indices
// -- the finished big-endian file image out.  Two launches: dcv_xtc_encode compresses every frame into a slot of its own
// (the length of a frame's stream is known only when it is written), dcv_xtc_pack copies the slots behind their headers
// into one contiguous image once the host has summed the lengths.  The format, the quantisation and the policy are
// written out in include/dcv.h; the frame encoder itself is xtc_encode_frame.h.
//
// A LANE owns a frame, as in the decoder (xtc.hip): the stream of a frame is strictly sequential, frames are independent.
// One-wave workgroups; every iteration consumes one atom in every lane and writes one packed triple, so the lanes of a
// wave stay in step and execute the limb arithmetic together.
//
// Loads.  A lane that read its own frame from global memory would make every load of the wave touch 64 lines, one per
// frame -- the decoder's first store pattern in mirror image.  The WAVE instead stages blocks of
// kXtcEncBlock atoms of its 64 frames in LDS (xtc_stage below) in xtc_format.h's block walk, the one the decoder stores
// with: contiguous pieces of 192 bytes (dense rows) or 64 bytes (planes).  Two blocks are resident: at atom p the
// encoder looks at most kXtcLookahead = 8 atoms ahead, which never leaves the block of p and the one behind it.  The
// coordinates are staged as floats and quantised where they are used; both passes stage the same way.  24.4 KB of LDS a
// wave, no atomics.
#include <cmath>
#include <vector>

#include "coords.h"
#include "xtc_encode_frame.h"

namespace dcv {

constexpr int kXtcEncBlock = 16, kXtcEncRing = 2 * kXtcEncBlock, kXtcEncPitch = kXtcThreads + 1;
static_assert(kXtcEncBlock >= kXtcLookahead, "atoms p .. p + lookahead must lie in two consecutive blocks");

struct XtcEncArgs {
    const float* xyz;
    const int64_t* index;   // in the workspace; NULL: frame f is source frame f
    uint8_t* slots;
    dcv_xtc_frame* desc;
    int32_t* status;
    int64_t n_frames;
    CoordStrides in;
    int64_t slot_bytes;
    int32_t n_atoms;
    float inv_scale, precision;
};

// block `block` of the atoms of the wave's 64 frames, global memory -> LDS word ((atom % ring) * 3 + c) * pitch + frame
__device__ __forceinline__ void xtc_stage(const XtcEncArgs& a, float* ring, const int64_t* src, int64_t f0, int32_t block, bool comp_fast) {
    xtc_block_walk<kXtcEncBlock>((int64_t)block, comp_fast, [&](int L, int64_t atom, int c) {
        if (f0 + L < a.n_frames && atom < a.n_atoms)
            ring[((int)(atom % kXtcEncRing) * 3 + c) * kXtcEncPitch + L] = a.xyz[src[L] * a.in.f + atom * a.in.a + c * a.in.c];
    });
}

__global__ __launch_bounds__(kXtcThreads) void xtc_encode_kernel(const XtcEncArgs a) {
    __shared__ float ring[kXtcEncRing * 3 * kXtcEncPitch];
    __shared__ int64_t src[kXtcThreads];
    const int lane = (int)threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * kXtcThreads, f = f0 + lane;
    const bool live = f < a.n_frames;
    const int64_t from = live ? (a.index ? a.index[f] : f) : 0;
    dcv_xtc_frame d{};
    d.offset = f * a.slot_bytes;
    uint32_t* slot = reinterpret_cast<uint32_t*>(a.slots + (live ? d.offset : 0));
    if (a.n_atoms <= 9) {   // the raw form: big-endian floats of x * inv_scale, nothing else
#pragma clang fp contract(off)
        if (live) {
            const float* x = a.xyz + from * a.in.f;
            bool finite = true;
            for (int32_t i = 0; i < a.n_atoms; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) finite = finite && std::isfinite(x[i * a.in.a + c * a.in.c]);
            if (finite)
                for (int32_t i = 0; i < a.n_atoms; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) slot[3 * i + c] = __builtin_bswap32(__builtin_bit_cast(uint32_t, x[i * a.in.a + c * a.in.c] * a.inv_scale));
            d.raw = 1;
            a.desc[f] = d;
            a.status[f] = finite ? DCV_XTC_OK : DCV_XTC_ENC_NONFINITE;
        }
        return;
    }
    src[lane] = from;
    const bool comp_fast = coord_comp_fast(a.in);
    const int status = xtc_encode_frame(
        a.n_atoms, a.inv_scale, a.precision, live, slot, (uint32_t)(a.slot_bytes / 4), d,
        [&](int32_t atom, float (&x)[3]) {
            const float* p = ring + (atom % kXtcEncRing) * 3 * kXtcEncPitch + lane;
            x[0] = p[0]; x[1] = p[kXtcEncPitch]; x[2] = p[2 * kXtcEncPitch];
        },
        [&](int pass, int32_t p) {   // the same p in every lane
            if (p % kXtcEncBlock) return;
            __syncthreads();         // every lane is done with the block this one replaces (and src[] is written)
            if (p == 0) xtc_stage(a, ring, src, f0, 0, comp_fast);
            xtc_stage(a, ring, src, f0, p / kXtcEncBlock + 1, comp_fast);
            __syncthreads();
        });
    if (live) {
        a.desc[f] = d;
        a.status[f] = status;
    }
}

// ---------------------------------------------------------------------------------------------------------- pack
struct XtcPackRec {
    int64_t slot;      // bytes from the slots to the frame's payload
    int64_t image;     // bytes from the image to the frame's header; < 0: the frame is not packed
    int32_t words;     // payload words: nbytes rounded up, or 3 natoms for a raw frame
    int32_t raw;
    uint32_t head[23]; // the header (14 words) and the nine fields of a compressed frame, host order
    int32_t pad;
};
static_assert(sizeof(XtcPackRec) == 120, "records are copied as they are");

constexpr int kXtcPackThreads = 256, kXtcPackWaves = kXtcPackThreads / kWave;

// a wave a frame, in 4-byte words: the header words byte-swapped, the payload as it is (it is big-endian already)
__global__ __launch_bounds__(kXtcPackThreads) void xtc_pack_kernel(const uint8_t* slots, const XtcPackRec* recs, int64_t n_frames, uint8_t* image) {
    const int lane = (int)threadIdx.x % kWave;
    const int64_t f = (int64_t)blockIdx.x * kXtcPackWaves + (int)threadIdx.x / kWave;
    if (f >= n_frames) return;
    const XtcPackRec& r = recs[f];
    if (r.image < 0) return;
    uint32_t* dst = reinterpret_cast<uint32_t*>(image + r.image);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(slots + r.slot);
    const int n_head = r.raw ? 14 : 23;
    if (lane < n_head) dst[lane] = __builtin_bswap32(r.head[lane]);
    for (int32_t w = lane; w < r.words; w += kWave) dst[n_head + w] = src[w];
}

}  // namespace dcv

using namespace dcv;

extern "C" size_t dcv_xtc_encode_slot_bytes(int32_t n_atoms) { return n_atoms < 1 ? 0 : (size_t)xtc_slot_bytes(n_atoms); }

extern "C" size_t dcv_xtc_encode_workspace(int64_t n_frames) {
    if (n_frames < 0 || n_frames > ((int64_t)1 << 40)) return 0;
    return align_up((size_t)n_frames * sizeof(int64_t), 256);
}

extern "C" int dcv_xtc_encode(const float* xyz_d, int64_t n_src_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                              int32_t n_atoms, const int64_t* frames_h, int64_t n_frames, float inv_scale, float precision,
                              void* slots_d, size_t slots_bytes, dcv_xtc_frame* desc_d, int32_t* status_d, void* ws_d, size_t ws_bytes,
                              void* stream) {
    // ---- validate everything before anything is launched
    DCV_REQUIRE(n_atoms > 0 && n_frames >= 0 && n_frames <= ((int64_t)1 << 40) && n_src_frames >= 0 && n_src_frames <= ((int64_t)1 << 40),
                "dcv_xtc_encode: bad arguments (n_atoms=%d n_frames=%lld n_src_frames=%lld)", n_atoms, (long long)n_frames, (long long)n_src_frames);
    DCV_REQUIRE(std::isfinite(precision) && precision > 0.0f && std::isfinite(inv_scale),
                "dcv_xtc_encode: the precision (%g) must be finite and positive, inv_scale (%g) finite", (double)precision, (double)inv_scale);
    DCV_REQUIRE(n_frames == 0 || (xyz_d && slots_d && desc_d && status_d), "dcv_xtc_encode: a NULL pointer with %lld frames", (long long)n_frames);
    const CoordStrides in{frame_stride, atom_stride, comp_stride};
    DCV_REQUIRE_STRIDES_GE1("dcv_xtc_encode", "strides", in);
    DCV_REQUIRE((reinterpret_cast<uintptr_t>(xyz_d) & 3) == 0 && (reinterpret_cast<uintptr_t>(slots_d) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(status_d) & 3) == 0 && (reinterpret_cast<uintptr_t>(desc_d) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(ws_d) & 7) == 0,
                "dcv_xtc_encode: the coordinates, the slots and the status must be 4-byte aligned, the descriptors and the workspace 8-byte aligned");
    if (frames_h) {
        for (int64_t f = 0; f < n_frames; ++f)
            DCV_REQUIRE(frames_h[f] >= 0 && frames_h[f] < n_src_frames, "dcv_xtc_encode: frame index %lld (entry %lld) outside the %lld frames given",
                        (long long)frames_h[f], (long long)f, (long long)n_src_frames);
    } else {
        DCV_REQUIRE(n_frames <= n_src_frames, "dcv_xtc_encode: %lld frames asked for, %lld given", (long long)n_frames, (long long)n_src_frames);
    }
    const size_t need = frames_h ? dcv_xtc_encode_workspace(n_frames) : 0;
    const size_t slot = (size_t)xtc_slot_bytes(n_atoms);
    if (n_frames > 0 && need > 0) DCV_REQUIRE_WORKSPACE("dcv_xtc_encode", ws_d, ws_bytes, need);
    if (n_frames > 0 && slots_bytes / slot < (size_t)n_frames) {
        set_error("dcv_xtc_encode: slot buffer too small (%zu bytes, need %lld slots of %zu)", slots_bytes, (long long)n_frames, slot);
        return DCV_ENOMEM;
    }
    if (n_frames == 0) return DCV_OK;
    int64_t in_last;
    DCV_REQUIRE_COORDS_FIT("dcv_xtc_encode", coord_extent(n_src_frames, n_atoms, in, in_last), n_src_frames, n_atoms);
    const Span spans[5] = {coord_span(xyz_d, in_last), span_of(slots_d, (uintptr_t)n_frames * slot),
                           span_of(desc_d, (uintptr_t)n_frames * sizeof(dcv_xtc_frame)), span_of(status_d, 4 * (uintptr_t)n_frames),
                           span_of(ws_d, need)};   // without indices the workspace is empty
    DCV_REQUIRE(spans_disjoint(spans, 5),
                "dcv_xtc_encode: the coordinates, the slots, the descriptors, the status words and the workspace must not overlap");
    DCV_REQUIRE(cdiv(n_frames, kXtcThreads) <= 0x7fffffffLL, "dcv_xtc_encode: %lld frames need more than 2^31 - 1 workgroups", (long long)n_frames);

    hipStream_t s = as_stream(stream);
    // a pageable source: the runtime has taken its copy of the indices when this call returns
    if (frames_h) DCV_CHECK_HIP(hipMemcpyAsync(ws_d, frames_h, (size_t)n_frames * sizeof(int64_t), hipMemcpyHostToDevice, s));
    XtcEncArgs a{};
    a.xyz = xyz_d;
    a.index = frames_h ? static_cast<const int64_t*>(ws_d) : nullptr;
    a.slots = static_cast<uint8_t*>(slots_d);
    a.desc = desc_d;
    a.status = status_d;
    a.n_frames = n_frames;
    a.in = in;
    a.slot_bytes = (int64_t)slot;
    a.n_atoms = n_atoms;
    a.inv_scale = inv_scale;
    a.precision = precision;
    hipLaunchKernelGGL(xtc_encode_kernel, dim3((unsigned)cdiv(n_frames, kXtcThreads)), dim3(kXtcThreads), 0, s, a);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

extern "C" size_t dcv_xtc_pack_workspace(int64_t n_frames) {
    if (n_frames < 0 || n_frames > ((int64_t)1 << 40)) return 0;
    return align_up((size_t)n_frames * sizeof(XtcPackRec), 256);
}

extern "C" int dcv_xtc_pack(const void* slots_d, size_t slots_bytes, const dcv_xtc_frame* desc_h, const int64_t* image_offset_h,
                            const int32_t* step_h, const float* time_h, const float* box_h, int64_t n_frames, int32_t n_atoms,
                            void* image_d, size_t image_bytes, void* ws_d, size_t ws_bytes, void* stream) {
    DCV_REQUIRE(n_atoms > 0 && n_frames >= 0 && n_frames <= ((int64_t)1 << 40), "dcv_xtc_pack: bad arguments (n_atoms=%d n_frames=%lld)", n_atoms,
                (long long)n_frames);
    DCV_REQUIRE(n_frames == 0 || (slots_d && desc_h && image_offset_h && step_h && time_h && image_d),
                "dcv_xtc_pack: a NULL pointer with %lld frames", (long long)n_frames);
    DCV_REQUIRE((reinterpret_cast<uintptr_t>(slots_d) & 3) == 0 && (reinterpret_cast<uintptr_t>(image_d) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(ws_d) & 7) == 0,
                "dcv_xtc_pack: the slots and the image must be 4-byte aligned, the workspace 8-byte aligned");
    const bool raw = n_atoms <= 9;
    int64_t end = 0;   // the frames follow each other in the image: a frame begins at or behind the end of the one before
    for (int64_t f = 0; f < n_frames; ++f) {
        const dcv_xtc_frame& d = desc_h[f];
        if (image_offset_h[f] < 0) continue;
        DCV_REQUIRE((d.raw != 0) == raw, "dcv_xtc_pack: frame %lld is %s, which %d atoms are not (raw form: at most 9 atoms)", (long long)f,
                    d.raw ? "raw" : "compressed", n_atoms);
        DCV_REQUIRE(raw || (d.nbytes >= 0 && d.nbytes <= xtc_slot_bytes(n_atoms)), "dcv_xtc_pack: frame %lld: a payload of %d bytes", (long long)f, d.nbytes);
        const int64_t len = raw ? (int64_t)12 * n_atoms : ((int64_t)d.nbytes + 3) / 4 * 4;
        DCV_REQUIRE(d.offset >= 0 && d.offset % 4 == 0 && (uint64_t)d.offset <= slots_bytes && (uint64_t)len <= slots_bytes - (uint64_t)d.offset,
                    "dcv_xtc_pack: frame %lld: %lld bytes at offset %lld do not lie on the 4-byte grid inside the %zu bytes of slots", (long long)f,
                    (long long)len, (long long)d.offset, slots_bytes);
        const int64_t whole = (raw ? 56 : 92) + len;
        DCV_REQUIRE(image_offset_h[f] % 4 == 0 && image_offset_h[f] >= end && (uint64_t)image_offset_h[f] <= image_bytes &&
                        (uint64_t)whole <= image_bytes - (uint64_t)image_offset_h[f],
                    "dcv_xtc_pack: frame %lld: %lld bytes at image offset %lld overlap the frame before, leave the 4-byte grid or the %zu bytes of the image",
                    (long long)f, (long long)whole, (long long)image_offset_h[f], image_bytes);
        end = image_offset_h[f] + whole;
    }
    const size_t need = dcv_xtc_pack_workspace(n_frames);
    if (n_frames > 0) DCV_REQUIRE_WORKSPACE("dcv_xtc_pack", ws_d, ws_bytes, need);
    if (n_frames == 0) return DCV_OK;
    const Span spans[3] = {span_of(slots_d, slots_bytes), span_of(image_d, image_bytes), span_of(ws_d, need)};
    DCV_REQUIRE(spans_disjoint(spans, 3), "dcv_xtc_pack: the slots, the image and the workspace must not overlap");
    DCV_REQUIRE(cdiv(n_frames, kXtcPackWaves) <= 0x7fffffffLL, "dcv_xtc_pack: %lld frames need more than 2^31 - 1 workgroups", (long long)n_frames);

    std::vector<XtcPackRec> recs((size_t)n_frames);
    for (int64_t f = 0; f < n_frames; ++f) {
        const dcv_xtc_frame& d = desc_h[f];
        XtcPackRec& r = recs[(size_t)f];
        r = XtcPackRec{};
        r.slot = d.offset;
        r.image = image_offset_h[f];
        r.raw = raw;
        r.words = raw ? 3 * n_atoms : (d.nbytes + 3) / 4;
        r.head[0] = 1995u;
        r.head[1] = r.head[13] = (uint32_t)n_atoms;
        r.head[2] = (uint32_t)step_h[f];
        r.head[3] = __builtin_bit_cast(uint32_t, time_h[f]);
        for (int k = 0; k < 9; ++k) r.head[4 + k] = box_h ? __builtin_bit_cast(uint32_t, box_h[9 * f + k]) : 0u;
        r.head[14] = __builtin_bit_cast(uint32_t, d.precision);
        for (int k = 0; k < 3; ++k) {
            r.head[15 + k] = (uint32_t)d.minint[k];
            r.head[18 + k] = (uint32_t)d.maxint[k];
        }
        r.head[21] = (uint32_t)d.smallidx;
        r.head[22] = (uint32_t)d.nbytes;
    }
    hipStream_t s = as_stream(stream);
    DCV_CHECK_HIP(hipMemcpyAsync(ws_d, recs.data(), recs.size() * sizeof(XtcPackRec), hipMemcpyHostToDevice, s));
    DCV_CHECK_HIP(hipStreamSynchronize(s));   // `recs` dies with this call; the caller has just read the descriptors, the stream is idle
    hipLaunchKernelGGL(xtc_pack_kernel, dim3((unsigned)cdiv(n_frames, kXtcPackWaves)), dim3(kXtcPackThreads), 0, s,
                       static_cast<const uint8_t*>(slots_d), static_cast<const XtcPackRec*>(ws_d), n_frames, static_cast<uint8_t*>(image_d));
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}
