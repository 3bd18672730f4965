// Rigid transform of every atom of every frame (align_trajectories): out = (x - c_mob) . R + c_ref with the per-frame
// R, c_mob, c_ref of dcv_superpose's transform rows.  n x A x 3 float32 in, the same out, float64 arithmetic in between
// and one rounding on the store (the formula: include/dcv.h).  A streaming map: 12 bytes read and 12 written per atom
// and frame, nothing staged in LDS, so there is no limit on the number of atoms.
//
// A THREAD owns a group of four consecutive atoms of one frame.  With atoms contiguous (DCD planes, atom stride 1) that
// is one 16-byte access per component, with dense rows (atom stride 3, component stride 1) it is 12 contiguous floats,
// three 16-byte accesses; any other strides take one 4-byte access per coordinate.  Input and output forms are
// independent (nine instantiations of one kernel).  The work items of a launch are (frame, group) pairs in one flat
// index, `slots` groups per frame, so with few atoms a workgroup of 256 threads holds several frames (104 atoms: 27
// groups a frame, nine frames a workgroup) and lanes are idle only in the last group of a frame.
//
// Alignment.  Rows start anywhere on the 4-byte grid: the planes of a DCD record image start at 1 + f 3(A + 2) + c (A + 2)
// floats, so the three planes of one frame disagree with each other whenever (A + 2) % 4 != 0, the frames disagree
// whenever 3 (A + 2) % 4 != 0, and the input's misalignment is independent of the output's.  stage.h puts every row
// on the 16-byte grid of its own address because LDS sits between its loads and its consumers; here a thread needs the
// SAME four atoms from up to six rows, so at most one of them decides.  The groups of frame f start at atom 4k - m_f,
// m_f chosen so that the STORES of the first output row of the frame (plane X, or the dense row) fall on the 16-byte
// grid of the address.  Every other row of the thread is read or written with 16-byte accesses that are 4-byte aligned
// only (legal for global memory on gfx950), which the memory pipeline splits at 128-byte lines: one more line per 1 KiB
// a wave touches.  Stores got the grid on the expectation that a line left partly written by one wave is the dearer
// of the two at the memory side (the opposite choice was not measured).  stage.h's guarded 4-byte head and tail are
// NOT reused: a lane on that path issues twelve loads and twelve stores and its whole wave waits for them, and with 65
// groups a frame (256 atoms) nearly every wave holds such a lane (measured in consecutive runs: 2.23 ms against 1.71 -
// 1.80 ms for 1M x 256 from planes into a record image).  Instead the first and the last group of a
// row are moved inside the row (atoms [0, 4) and [A - 4, A)): the same three 16-byte accesses as everybody, off the
// grid, and the atoms shared with the neighbouring group are computed and stored by both lanes -- the same expression
// on the same inputs, so the same bits, whichever store lands last.  Rows of fewer than four atoms take guarded 4-byte
// accesses.
//
// The transform row of a frame is read with scalar loads: a wave makes one pass of the arithmetic per frame it holds
// lanes of (the lanes of the other frames masked off), one pass wherever the wave is inside one frame; loads and stores
// are issued once, outside that loop.  No LDS, no atomics, no workspace; at most kXfMaxGroups workgroups stride over
// the items.
#include "coords.h"

namespace dcv {

constexpr int kXfThreads = 256;
constexpr int64_t kXfMaxGroups = 2048;   // 256 CUs x 8 workgroups

// a 16-byte non-temporal access that is only promised 4-byte alignment
typedef float xf_float4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void xf_load4(const float* p, float (&v)[4]) {
    const xf_float4 q = __builtin_nontemporal_load(reinterpret_cast<const xf_float4*>(p));
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void xf_store4(float* p, float a, float b, float c, float d) {
    xf_float4 q;
    q.x = a; q.y = b; q.z = c; q.w = d;
    __builtin_nontemporal_store(q, reinterpret_cast<xf_float4*>(p));
}

struct XfArgs {   // the three pointers are kernel arguments of their own: __restrict__ there lets the transform rows take scalar loads
    CoordStrides in;
    int64_t ldt;
    CoordStrides outs;
    int64_t n_frames, n_atoms;
    int64_t slots, total;   // groups per frame (worst alignment), n_frames * slots
    uint32_t x_word, out_word;   // the bases in floats, mod 4
    int32_t grid_on;        // whose address the groups are laid on: 1 output, 2 input, 0 nobody (no 16-byte form)
};

// atoms before the first whole group of a row whose first element sits r floats past a 16-byte boundary
template <int FORM>
__device__ __forceinline__ int xf_shift(uint32_t base_word, int64_t f, int64_t frame_stride) {
    const int r = (int)((base_word + (uint32_t)f * (uint32_t)frame_stride) & 3u);
    return FORM == kCoordPlanes ? r : (3 * r) & 3;   // dense: element 3 (4k - m) of the row, and 3 . 3 = 1 (mod 4)
}

// the coordinates of the four atoms [j, j + 4) of a frame that starts at `in`; `vec`: the group lies inside the row
template <int IN>
__device__ __forceinline__ void xf_load(const XfArgs& a, const float* in, int64_t j, bool vec, float (&v)[3][4]) {
    if (vec && IN == kCoordPlanes) {
#pragma unroll
        for (int c = 0; c < 3; ++c) xf_load4(in + c * a.in.c + j, v[c]);
    } else if (vec && IN == kCoordDense) {
        float q[3][4];
#pragma unroll
        for (int i = 0; i < 3; ++i) xf_load4(in + 3 * j + 4 * i, q[i]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][e] = q[(3 * e + c) >> 2][(3 * e + c) & 3];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                v[c][e] = j + e >= 0 && j + e < a.n_atoms ? __builtin_nontemporal_load(in + (j + e) * a.in.a + c * a.in.c) : 0.0f;
    }
}

template <int OUT>
__device__ __forceinline__ void xf_store(const XfArgs& a, float* out, int64_t j, bool vec, const float (&o)[3][4]) {
    if (vec && OUT == kCoordPlanes) {
#pragma unroll
        for (int c = 0; c < 3; ++c) xf_store4(out + c * a.outs.c + j, o[c][0], o[c][1], o[c][2], o[c][3]);
    } else if (vec && OUT == kCoordDense) {
        float* p = out + 3 * j;
        xf_store4(p, o[0][0], o[1][0], o[2][0], o[0][1]);
        xf_store4(p + 4, o[1][1], o[2][1], o[0][2], o[1][2]);
        xf_store4(p + 8, o[2][2], o[0][3], o[1][3], o[2][3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (j + e >= 0 && j + e < a.n_atoms) __builtin_nontemporal_store(o[c][e], out + (j + e) * a.outs.a + c * a.outs.c);
    }
}

// four atoms through the transform row `t`: the float64 expression of the header, operation by operation
__device__ __forceinline__ void xf_apply(const double* __restrict__ t, const float (&v)[3][4], float (&o)[3][4]) {
#pragma clang fp contract(off)
    double R[9], cm[3], cr[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = t[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) { cm[c] = t[9 + c]; cr[c] = t[12 + c]; }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double p0 = (double)v[0][e] - cm[0], p1 = (double)v[1][e] - cm[1], p2 = (double)v[2][e] - cm[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c][e] = (float)(p0 * R[c] + p1 * R[3 + c] + p2 * R[6 + c] + cr[c]);
    }
}

__device__ __forceinline__ int64_t xf_first_lane(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <int IN, int OUT>
__global__ __launch_bounds__(kXfThreads) void transform_frames_kernel(const XfArgs a, const float* __restrict__ x, const double* __restrict__ T,
                                                                   float* __restrict__ out) {
    const uint32_t slots = (uint32_t)a.slots;   // <= 2^29 + 1
    const bool vec = a.n_atoms >= 4;            // a group can be moved inside its row
    for (int64_t w0 = (int64_t)blockIdx.x * kXfThreads; w0 < a.total; w0 += (int64_t)gridDim.x * kXfThreads) {
        // the workgroup's first item, by scalar arithmetic; a lane is at most 255 items further
        const int64_t fb = w0 / a.slots;
        const uint32_t r = (uint32_t)(w0 - fb * a.slots) + threadIdx.x;
        const uint32_t q = r / slots, k = r - q * slots;
        const int64_t f = fb + q;
        if (f >= a.n_frames) continue;   // no barrier and no shuffle below
        int m = 0;
        if (a.grid_on == 1) m = xf_shift<OUT>(a.out_word, f, a.outs.f);
        else if (a.grid_on == 2) m = xf_shift<IN>(a.x_word, f, a.in.f);
        int64_t j = 4 * (int64_t)k - m;
        if (j >= a.n_atoms) continue;
        // the ragged first and last group of a row move inside it: their lanes take the same 16-byte accesses as every other
        // lane (off the grid), and the one to three atoms they share with their neighbour are written twice with the same bits
        if (vec) j = j < 0 ? 0 : (j + 4 > a.n_atoms ? a.n_atoms - 4 : j);
        // one pass per frame that has lanes in this wave, its transform row read with scalar loads (the first one beside the
        // coordinates); one pass wherever the wave is inside one frame
        int64_t fc = xf_first_lane(f);
        double t[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) t[i] = T[fc * a.ldt + i];
        float v[3][4], o[3][4];
        xf_load<IN>(a, x + f * a.in.f, j, vec, v);
        for (;;) {
            if (f == fc) {
                xf_apply(t, v, o);
                break;
            }
            fc = xf_first_lane(f);
#pragma unroll
            for (int i = 0; i < 15; ++i) t[i] = T[fc * a.ldt + i];
        }
        xf_store<OUT>(a, out + f * a.outs.f, j, vec, o);
    }
}

template <int IN>
static void xf_launch(int out_form, dim3 grid, hipStream_t s, const XfArgs& a, const float* x, const double* T, float* out) {
    if (out_form == kCoordPlanes) hipLaunchKernelGGL((transform_frames_kernel<IN, kCoordPlanes>), grid, dim3(kXfThreads), 0, s, a, x, T, out);
    else if (out_form == kCoordDense) hipLaunchKernelGGL((transform_frames_kernel<IN, kCoordDense>), grid, dim3(kXfThreads), 0, s, a, x, T, out);
    else hipLaunchKernelGGL((transform_frames_kernel<IN, kCoordStrided>), grid, dim3(kXfThreads), 0, s, a, x, T, out);
}

}  // namespace dcv

using namespace dcv;

extern "C" int dcv_transform_frames(const float* xyz_d, int64_t n_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                                    int32_t n_atoms, const double* transform_d, int64_t ldt, float* out_d, int64_t out_frame_stride,
                                    int64_t out_atom_stride, int64_t out_comp_stride, void* stream) {
    // ---- validate everything before anything is launched
    DCV_REQUIRE(xyz_d && transform_d && out_d && n_atoms > 0 && n_frames >= 0, "dcv_transform_frames: bad arguments (n_atoms=%d n_frames=%lld)",
                n_atoms, (long long)n_frames);
    DCV_REQUIRE_COORD_STRIDES("dcv_transform_frames", frame_stride, atom_stride, comp_stride);
    const CoordStrides in{frame_stride, atom_stride, comp_stride}, outs{out_frame_stride, out_atom_stride, out_comp_stride};
    DCV_REQUIRE_STRIDES_GE1("dcv_transform_frames", "output strides", outs);
    DCV_REQUIRE((reinterpret_cast<uintptr_t>(xyz_d) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_d) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(transform_d) & 7) == 0,
                "dcv_transform_frames: the coordinates must be 4-byte aligned and the transforms 8-byte aligned");
    DCV_REQUIRE(ldt >= 15,"dcv_transform_frames: a transform row holds 15 doubles, ldt is %lld", (long long)ldt);
    if (n_frames == 0) return DCV_OK;
    int64_t in_last, out_last;
    DCV_REQUIRE_COORDS_FIT("dcv_transform_frames", coord_extent(n_frames, n_atoms, in, in_last) && coord_extent(n_frames, n_atoms, outs, out_last),
                           n_frames, n_atoms);
    const Span in_out[2] = {coord_span(xyz_d, in_last), coord_span(out_d, out_last)};
    DCV_REQUIRE(spans_disjoint(in_out, 2),
                "dcv_transform_frames: the input elements [0, %lld] and the output elements [0, %lld] overlap in memory: the map is not in place",
                (long long)in_last, (long long)out_last);
    int64_t t_last;   // the kernel reads the rows through a __restrict__ pointer: they must not be written either
    DCV_REQUIRE(!__builtin_mul_overflow(n_frames - 1, ldt, &t_last) && t_last < (int64_t)1 << 59,
                "dcv_transform_frames: %lld transform rows %lld doubles apart do not fit the address space", (long long)n_frames, (long long)ldt);
    const Span t_out[2] = {span_of(transform_d, 8 * ((uintptr_t)t_last + 15)), in_out[1]};
    DCV_REQUIRE(spans_disjoint(t_out, 2), "dcv_transform_frames: the transform rows and the output elements [0, %lld] overlap in memory",
                (long long)out_last);
    const int64_t slots = ((int64_t)n_atoms + 6) >> 2;
    DCV_REQUIRE(n_frames <= (((int64_t)1 << 62) / slots), "dcv_transform_frames: %lld frames x %d atoms are too many work items",
                (long long)n_frames, n_atoms);

    XfArgs a{};
    a.in = in;
    a.ldt = ldt;
    a.outs = outs;
    a.n_frames = n_frames; a.n_atoms = n_atoms;
    a.slots = slots; a.total = n_frames * slots;
    a.x_word = (uint32_t)((in_out[0].lo >> 2) & 3); a.out_word = (uint32_t)((in_out[1].lo >> 2) & 3);
    const CoordForm in_form = coord_form(in), out_form = coord_form(outs);
    a.grid_on = out_form != kCoordStrided ? 1 : (in_form != kCoordStrided ? 2 : 0);
    const int64_t want = cdiv(a.total, kXfThreads);
    const dim3 grid((unsigned)(want < kXfMaxGroups ? want : kXfMaxGroups));
    hipStream_t s = as_stream(stream);
    if (in_form == kCoordPlanes) xf_launch<kCoordPlanes>(out_form, grid, s, a, xyz_d, transform_d, out_d);
    else if (in_form == kCoordDense) xf_launch<kCoordDense>(out_form, grid, s, a, xyz_d, transform_d, out_d);
    else xf_launch<kCoordStrided>(out_form, grid, s, a, xyz_d, transform_d, out_d);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}
