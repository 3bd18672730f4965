// Host-side check of the layout rules of the coordinate entries under sanitizers: coord_extent, coord_form,
// coord_comp_fast and spans_disjoint (csrc/coords.h) over their corners -- one frame, one atom, strides of 0, 1, 2^60 and
// INT64_MAX, an overflow in each of the three products and in each of the two sums, the 2^60 bound from both sides,
// empty, touching and nested spans -- against answers worked out with 128-bit integers.  No GPU call is made.  Build and
// run (from the repository root):
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/coords_host.cpp -o /tmp/coords_host && /tmp/coords_host
//
// Exit status 0 and "coords_host: ok" mean every answer was right and no sanitizer spoke.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../deep_cartograph_amd/csrc/coords.h"

using namespace dcv;

namespace {

int failures = 0;

void expect(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0, long long e = 0) {
    if (ok) return;
    ++failures;
    std::fprintf(stderr, "coords_host: WRONG %s (%lld, %lld, %lld, %lld, %lld)\n", what, a, b, c, d, e);
}

constexpr int64_t kMax = INT64_MAX, kLimit = (int64_t)1 << 60;

// the definition, in integers that cannot overflow: the last element and whether every step of the int64 evaluation
// (three products, two sums) stays in range and the result lies below 2^60
bool extent_ref(int64_t n, int64_t A, const CoordStrides& s, int64_t& last) {
    const __int128 lo = INT64_MIN, hi = INT64_MAX;
    const __int128 x = (__int128)(n - 1) * s.f, y = (__int128)(A - 1) * s.a, z = (__int128)2 * s.c;
    if (x < lo || x > hi || y < lo || y > hi || z < lo || z > hi) return false;
    if (x + y < lo || x + y > hi || x + y + z < lo || x + y + z > hi) return false;
    last = (int64_t)(x + y + z);
    return last < kLimit;
}

void check_extent(int64_t n, int64_t A, CoordStrides s, int want = -1) {
    int64_t got_last = -1, ref_last = -1;
    const bool got = coord_extent(n, A, s, got_last), ref = extent_ref(n, A, s, ref_last);
    expect(got == ref && (!ref || got_last == ref_last), "coord_extent against the 128-bit definition", n, A, s.f, s.a, s.c);
    if (want >= 0) expect(got == (want != 0), "coord_extent against the expected answer", n, A, s.f, s.a, s.c);
}

void extents() {
    // the valid base shapes
    check_extent(4, 10, {30, 3, 1}, 1);
    check_extent(4, 10, {3 * 12 + 14, 1, 12}, 1);
    // one frame: n_frames - 1 = 0 annihilates any frame stride
    for (int64_t f : {(int64_t)0, (int64_t)1, kLimit, kMax}) check_extent(1, 10, {f, 3, 1}, 1);
    // one atom: the same for the atom stride
    for (int64_t a : {(int64_t)1, kLimit, kMax}) check_extent(4, 1, {30, a, 1}, 1);
    check_extent(1, 1, {kMax, kMax, 1}, 1);
    // a frame stride of 0 (every frame the same: allowed on the input side)
    check_extent(1000, 10, {0, 3, 1}, 1);
    // the bound from both sides: last == 2^60 - 1 fits, 2^60 does not
    check_extent(2, 1, {kLimit - 3, 1, 1}, 1);
    check_extent(2, 1, {kLimit - 2, 1, 1}, 0);
    check_extent(1, 2, {1, kLimit - 3, 1}, 1);
    check_extent(1, 2, {1, kLimit - 2, 1}, 0);
    check_extent(1, 1, {1, 1, kLimit / 2 - 1}, 1);   // 2 c = 2^60 - 2
    check_extent(1, 1, {1, 1, kLimit / 2}, 0);
    // strides of 2^60 and INT64_MAX with more than one frame / atom
    check_extent(2, 10, {kLimit, 3, 1}, 0);
    check_extent(4, 10, {(int64_t)1 << 61, 3, 1}, 0);
    check_extent(2, 10, {kMax, 3, 1}, 0);      // the product fits, the sum does not
    check_extent(3, 10, {kMax, 3, 1}, 0);      // overflow in the first product
    check_extent(4, 3, {30, kMax, 1}, 0);      // overflow in the second product
    check_extent(4, 10, {30, 3, kMax}, 0);     // overflow in the third product
    check_extent(4, 10, {30, 3, kMax / 2 + 1}, 0);
    check_extent(2, 2, {kMax, kMax, 1}, 0);    // overflow in the first sum
    check_extent(2, 2, {kMax - 5, 3, 1}, 0);   // both sums fit, INT64_MAX is above the bound
    check_extent(2, 2, {kMax - 5, 5, 1}, 0);   // the first sum is INT64_MAX, the second overflows
    check_extent(2, 1, {kMax - 1, 1, 1}, 0);   // overflow in the second sum only
    check_extent(1, 1, {0, 1, kMax / 2}, 0);   // 2 c = INT64_MAX - 1: no overflow anywhere, above the bound
    // a sweep around every corner value
    const std::vector<int64_t> vals = {0, 1, 2, 3, kLimit - 1, kLimit, kLimit + 1, kMax / 2, kMax / 2 + 1, kMax - 1, kMax};
    for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)1 << 40})
        for (int64_t A : {(int64_t)1, (int64_t)2, (int64_t)INT32_MAX})
            for (int64_t f : vals)
                for (int64_t a : vals)
                    for (int64_t c : vals) check_extent(n, A, {f, a, c});
}

void forms() {
    expect(coord_form({30, 3, 1}) == kCoordDense, "dense rows");
    expect(coord_form({0, 3, 1}) == kCoordDense, "dense rows, frame stride 0");
    expect(coord_form({50, 1, 12}) == kCoordPlanes, "planes");
    expect(coord_form({3, 1, 1}) == kCoordPlanes, "atom stride 1 is planes whatever the component stride");
    expect(coord_form({3, 1, kMax}) == kCoordPlanes, "planes, component stride INT64_MAX");
    expect(coord_form({40, 4, 1}) == kCoordStrided, "atom stride 4");
    expect(coord_form({60, 3, 2}) == kCoordStrided, "atom stride 3, component stride 2");
    expect(coord_form({1, kLimit, 1}) == kCoordStrided && coord_form({1, kMax, kMax}) == kCoordStrided, "huge strides");
    expect(coord_comp_fast({30, 3, 1}) && coord_comp_fast({40, 4, 1}) && coord_comp_fast({1, kMax, kMax - 1}), "component fastest");
    expect(!coord_comp_fast({50, 1, 12}) && !coord_comp_fast({3, 1, 1}) && !coord_comp_fast({3, 3, 3}) && !coord_comp_fast({0, kMax, kMax}),
           "atom fastest, ties included");
}

bool disjoint2(Span a, Span b) {
    const Span s[2] = {a, b}, r[2] = {b, a};
    const bool x = spans_disjoint(s, 2), y = spans_disjoint(r, 2);
    expect(x == y, "spans_disjoint is symmetric", (long long)a.lo, (long long)a.hi, (long long)b.lo, (long long)b.hi);
    return x;
}

void spans() {
    alignas(8) static char buf[256];
    const Span whole = span_of(buf, 256), head = span_of(buf, 64), next = span_of(buf + 64, 64), inner = span_of(buf + 32, 8);
    expect(whole.lo == reinterpret_cast<uintptr_t>(buf) && whole.hi == whole.lo + 256, "span_of");
    const Span xyz = coord_span(reinterpret_cast<const float*>(buf), 9);
    expect(xyz.lo == whole.lo && xyz.hi == whole.lo + 40, "coord_span: the elements [0, last]");
    expect(disjoint2(head, next), "touching spans are disjoint");
    expect(!disjoint2(head, span_of(buf + 63, 64)), "one shared byte overlaps");
    expect(!disjoint2(whole, inner) && !disjoint2(head, inner), "a nested span overlaps");
    expect(!disjoint2(head, head), "a span overlaps itself");
    // an empty span overlaps nothing: at the start, inside, at the end, and another empty span at the same address
    for (int off : {0, 32, 64}) expect(disjoint2(head, span_of(buf + off, 0)), "an empty span overlaps nothing", off);
    expect(disjoint2(span_of(buf + 8, 0), span_of(buf + 8, 0)), "two empty spans");
    expect(disjoint2(span_of(nullptr, 0), whole), "a NULL workspace of no bytes");
    expect(spans_disjoint(&whole, 1) && spans_disjoint(&whole, 0), "fewer than two spans");
    // n spans: one bad pair anywhere is found
    const Span ok[5] = {head, next, span_of(buf + 128, 64), span_of(buf + 192, 64), span_of(buf + 100, 0)};
    expect(spans_disjoint(ok, 5), "five spans, one of them empty and inside another");
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            if (i == j) continue;
            Span bad[5] = {ok[0], ok[1], ok[2], ok[3], ok[4]};
            bad[i] = Span{ok[j].lo + 8, ok[j].lo + 16};   // i moves inside j: i's own place is free now, j is hit
            expect(!spans_disjoint(bad, 5), "a nested pair among five", i, j);
        }
    // the top of the address space: hi may be the last address
    const Span top{UINTPTR_MAX - 16, UINTPTR_MAX}, below{UINTPTR_MAX - 32, UINTPTR_MAX - 16};
    expect(disjoint2(top, below) && !disjoint2(top, Span{UINTPTR_MAX - 17, UINTPTR_MAX - 15}), "spans at the top of the address space");
}

}  // namespace

int main() {
    extents();
    forms();
    spans();
    if (failures) {
        std::fprintf(stderr, "coords_host: %d wrong answers\n", failures);
        return 1;
    }
    std::printf("coords_host: ok\n");
    return 0;
}
