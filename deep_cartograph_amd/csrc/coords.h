// What the coordinate entries share on the host (dcv_featurize, dcv_featurize_project, dcv_superpose, dcv_interpolate,
// dcv_transform_frames, dcv_xtc_decode, dcv_xtc_encode / dcv_xtc_pack): the stride triple of a layout, its
// classification, the last element it reaches, byte spans and their overlap, and the requirements every entry states in
// the same words.  Coordinate c of atom a of frame f of a layout is base[f * s.f + a * s.a + c * s.c].  Usable from plain
// host code; the kernels take the struct and the two classifications and keep their own index expressions.
#pragma once
#include "common.h"

namespace dcv {

struct CoordStrides {
    int64_t f, a, c;   // frame, atom, component; in elements
};

// planes: the atoms of a component are contiguous (the X / Y / Z rows of a DCD frame record); dense: (n, A, 3) rows
enum CoordForm { kCoordStrided = 0, kCoordPlanes = 1, kCoordDense = 2 };
__host__ __device__ inline CoordForm coord_form(const CoordStrides& s) { return s.a == 1 ? kCoordPlanes : (s.a == 3 && s.c == 1 ? kCoordDense : kCoordStrided); }
// which of atom and component runs fastest over consecutive addresses
__host__ __device__ inline bool coord_comp_fast(const CoordStrides& s) { return s.c < s.a; }

// last element a layout of n_frames >= 1 frames reaches, false when that overflows or does not lie below 2^60
inline bool coord_extent(int64_t n_frames, int64_t n_atoms, const CoordStrides& s, int64_t& last) {
    int64_t x, y, z;
    if (__builtin_mul_overflow(n_frames - 1, s.f, &x) || __builtin_mul_overflow(n_atoms - 1, s.a, &y) || __builtin_mul_overflow((int64_t)2, s.c, &z))
        return false;
    if (__builtin_add_overflow(x, y, &last) || __builtin_add_overflow(last, z, &last)) return false;
    return last < (int64_t)1 << 60;
}

struct Span {   // the bytes [lo, hi)
    uintptr_t lo, hi;
};
inline Span span_of(const void* p, uintptr_t bytes) { return {reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes}; }
// the elements [0, last] of a float32 layout
inline Span coord_span(const float* p, int64_t last) { return span_of(p, 4 * (uintptr_t)last + 4); }
// no two of the n spans share a byte; an empty span overlaps nothing
inline bool spans_disjoint(const Span* s, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (s[i].lo != s[i].hi && s[j].lo != s[j].hi && s[i].hi > s[j].lo && s[j].hi > s[i].lo) return false;
    return true;
}

// the strides every coordinate entry accepts for its input; `entry` is the entry's name, a string literal
#define DCV_REQUIRE_COORD_STRIDES(entry, frame_stride, atom_stride, comp_stride)                                                  \
    DCV_REQUIRE((frame_stride) >= 0 && (atom_stride) >= 1 && (comp_stride) >= 1,                                                  \
                entry ": strides (%lld, %lld, %lld): the frame stride must be >= 0, the atom and component strides >= 1",         \
                (long long)(frame_stride), (long long)(atom_stride), (long long)(comp_stride))

// a layout that is written, or gathered from by frame index: `noun` is "output strides" or "strides", a string literal
#define DCV_REQUIRE_STRIDES_GE1(entry, noun, s)                                                                                   \
    DCV_REQUIRE((s).f >= 1 && (s).a >= 1 && (s).c >= 1, entry ": " noun " (%lld, %lld, %lld) must all be >= 1", (long long)(s).f, \
                (long long)(s).a, (long long)(s).c)

// `fits`: the conjunction of the coord_extent() calls on the layouts of n_frames x n_atoms
#define DCV_REQUIRE_COORDS_FIT(entry, fits, n_frames, n_atoms)                                                                    \
    DCV_REQUIRE(fits, entry ": %lld frames of %d atoms with these strides do not fit the address space", (long long)(n_frames), (n_atoms))

}  // namespace dcv
