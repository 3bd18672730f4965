// Host-side check of the XTC frame encoder under sanitizers: the __host__ __device__ frame encoder
// (csrc/xtc_encode_frame.h) runs over generated frames whose slots lie inside guard bands, every result is decoded with the
// frame decoder (csrc/xtc_decode_frame.h) on the host, and the integers, the payload length against the capacity bound
// and the bands are compared.  No GPU call is made.  Build and run (from the repository root):
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/xtc_encode_host.cpp -o /tmp/xtc_encode_host && /tmp/xtc_encode_host
//
// Exit status 0 and "xtc_encode_host: ok" mean every case round-tripped with the bands intact.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../deep_cartograph_amd/csrc/xtc_decode_frame.h"
#include "../deep_cartograph_amd/csrc/xtc_encode_frame.h"

using namespace dcv;

namespace {

constexpr size_t kBand = 64;   // guard words on either side of a slot
constexpr uint32_t kFill = 0xffffffffu;

enum Case { kChain, kWater, kScattered, kTight, kIdentical, kNegative, kBigSize, kBits72, kCases };
const char* kNames[kCases] = {"chain", "water", "scattered", "tight", "identical", "negative", "bigsize", "bits72"};

std::vector<float> make_frame(Case c, int natoms, std::mt19937_64& rng) {
    std::normal_distribution<double> normal(0.0, 1.0);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    std::vector<float> x(3 * (size_t)natoms);
    double cur[3] = {uni(rng) * 80 - 20, uni(rng) * 80 - 20, uni(rng) * 80 - 20};
    for (int a = 0; a < natoms; ++a)
        for (int k = 0; k < 3; ++k) {
            double v = 0;
            switch (c) {
                case kChain: cur[k] += 2.2 * normal(rng); v = cur[k]; break;
                case kNegative: cur[k] += 2.2 * normal(rng); v = cur[k] - 400.0; break;
                case kWater:
                    if (a % 3 == 0) cur[k] = uni(rng) * 40;
                    v = cur[k] + (a % 3 ? 0.6 * normal(rng) : 0.0);
                    break;
                case kScattered: v = uni(rng) * 600 - 300; break;
                case kTight: v = cur[k] + 0.01 * normal(rng); break;
                case kIdentical: v = cur[k]; break;
                case kBigSize: v = uni(rng) * 4000 - 2000; break;
                case kBits72: v = a == 0 ? -83886.0 + 0.5 * uni(rng) : a == 1 ? 83885.5 + 0.5 * uni(rng) : uni(rng) * 167760 - 83880; break;
                default: break;
            }
            x[3 * (size_t)a + k] = (float)v;
        }
    return x;
}

int fail(const char* what, Case c, int natoms, int frame) {
    std::fprintf(stderr, "xtc_encode_host: %s (case %s, %d atoms, frame %d)\n", what, kNames[c], natoms, frame);
    return 1;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20240607);
    const int atom_counts[] = {10, 11, 16, 17, 37, 104};
    long frames = 0, bytes = 0;
    for (int ci = 0; ci < kCases; ++ci) {
        const Case c = (Case)ci;
        const float precision = c == kBigSize ? 1.0e5f : 1000.0f;
        for (int natoms : atom_counts)
            for (int f = 0; f < 24; ++f) {
                const std::vector<float> x = make_frame(c, natoms, rng);
                const size_t slot_words = (size_t)xtc_slot_bytes(natoms) / 4;
                std::vector<uint32_t> buf(slot_words + 2 * kBand, kFill);
                dcv_xtc_frame d{};
                const int status = xtc_encode_frame(
                    natoms, 0.1f, precision, true, buf.data() + kBand, (uint32_t)slot_words, d,
                    [&](int32_t a, float (&v)[3]) {
                        for (int k = 0; k < 3; ++k) v[k] = x[3 * (size_t)a + k];
                    },
                    [](int, int32_t) {});
                if (status != DCV_XTC_OK) return fail("a frame was marked", c, natoms, f);
                const size_t used = ((size_t)d.nbytes + 3) / 4;
                if (d.nbytes <= 0 || used > slot_words) return fail("nbytes outside the slot", c, natoms, f);
                for (size_t i = 0; i < buf.size(); ++i)
                    if ((i < kBand || i >= kBand + used) && buf[i] != kFill) return fail("a word outside the payload was written", c, natoms, f);
                // decode what was written and compare with the quantised input
                // (precision 1 and scale 1 make the decoder hand out (float)i itself: exact below 2^24, compared as floats above)
                dcv_xtc_frame dd = d;
                dd.offset = 0;
                dd.precision = 1.0f;
                std::vector<float> got(3 * (size_t)natoms, -1.0f);
                int emitted = 0;
                const int dstatus = xtc_decode_frame(
                    reinterpret_cast<const uint8_t*>(buf.data() + kBand), dd, natoms, 1.0f, true,
                    [&](int32_t a, float vx, float vy, float vz) {
                        got[3 * (size_t)a] = vx; got[3 * (size_t)a + 1] = vy; got[3 * (size_t)a + 2] = vz;
                        ++emitted;
                    },
                    [](int32_t, int32_t) {});
                if (dstatus != DCV_XTC_OK || emitted != natoms) return fail("the stream did not decode", c, natoms, f);
                for (int a = 0; a < natoms; ++a)
                    for (int k = 0; k < 3; ++k) {
                        int bad = 0;
                        const int32_t want = xtc_quantise(x[3 * (size_t)a + k], 0.1f, precision, bad);
                        if (bad || got[3 * (size_t)a + k] != (float)want) return fail("decoded integers differ from the quantised input", c, natoms, f);
                        if (want < d.minint[k] || want > d.maxint[k]) return fail("minint / maxint do not bound the frame", c, natoms, f);
                    }
                ++frames;
                bytes += d.nbytes;
            }
    }
    // marked frames: nothing is written
    for (int kind = 0; kind < 2; ++kind) {
        std::vector<float> x = make_frame(kChain, 20, rng);
        x[31] = kind ? 3.0e9f : std::nanf("");
        std::vector<uint32_t> buf((size_t)xtc_slot_bytes(20) / 4 + 2 * kBand, kFill);
        dcv_xtc_frame d{};
        const int status = xtc_encode_frame(
            20, 0.1f, 1000.0f, true, buf.data() + kBand, (uint32_t)(buf.size() - 2 * kBand), d,
            [&](int32_t a, float (&v)[3]) {
                for (int k = 0; k < 3; ++k) v[k] = x[3 * (size_t)a + k];
            },
            [](int, int32_t) {});
        if (status != (kind ? DCV_XTC_ENC_RANGE : DCV_XTC_ENC_NONFINITE) || d.nbytes != 0) return fail("a bad frame was not marked", kChain, 20, kind);
        for (uint32_t w : buf)
            if (w != kFill) return fail("a marked frame wrote to its slot", kChain, 20, kind);
    }
    std::printf("xtc_encode_host: ok (%ld frames, %ld payload bytes, bands intact)\n", frames, bytes);
    return 0;
}
