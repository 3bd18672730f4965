// The float64 arithmetic of one feature record on one staged frame, ONE copy for the kernels that evaluate records
// (featurize.hip stores the values, featurize_project.hip contracts them): distance, torsion angle or its sine and
// cosine as include/dcv.h documents them -- p = (double)x * unit, no fused multiply-adds, the degenerate cases
// (coincident middle atoms, collinear atoms) as PLUMED resolves them.  Nothing is rounded here.
#pragma once
#include "common.h"

namespace dcv {

struct FeatValue {
    double v0, v1;   // distance | angle | sine, and the cosine of a DCV_FEAT_TORSION_SINCOS record (0 otherwise)
};

// lf: the frame in LDS; s0 .. s3: the atoms' LDS offsets (slot * las); lcs: the LDS stride of a component
__device__ __forceinline__ FeatValue feature_value(const float* lf, int kind, int s0, int s1, int s2, int s3, int lcs, double unit) {
#pragma clang fp contract(off)   // a*b - c*d of identical products must be exactly 0 (collinear atoms), as in NumPy / PLUMED
    const double p0x = (double)lf[s0] * unit, p0y = (double)lf[s0 + lcs] * unit, p0z = (double)lf[s0 + 2 * lcs] * unit;
    const double p1x = (double)lf[s1] * unit, p1y = (double)lf[s1 + lcs] * unit, p1z = (double)lf[s1 + 2 * lcs] * unit;
    const double b0x = p1x - p0x, b0y = p1y - p0y, b0z = p1z - p0z;
    if (kind == DCV_FEAT_DISTANCE) return {sqrt(b0x * b0x + b0y * b0y + b0z * b0z), 0.0};
    const double p2x = (double)lf[s2] * unit, p2y = (double)lf[s2 + lcs] * unit, p2z = (double)lf[s2 + 2 * lcs] * unit;
    const double p3x = (double)lf[s3] * unit, p3y = (double)lf[s3 + lcs] * unit, p3z = (double)lf[s3 + 2 * lcs] * unit;
    const double b1x = p2x - p1x, b1y = p2y - p1y, b1z = p2z - p1z;
    const double b2x = p3x - p2x, b2y = p3y - p2y, b2z = p3z - p2z;
    const double n1x = b0y * b1z - b0z * b1y, n1y = b0z * b1x - b0x * b1z, n1z = b0x * b1y - b0y * b1x;
    const double n2x = b1y * b2z - b1z * b2y, n2y = b1z * b2x - b1x * b2z, n2z = b1x * b2y - b1y * b2x;
    const double x = n1x * n2x + n1y * n2y + n1z * n2z;
    const double mx = n1y * n2z - n1z * n2y, my = n1z * n2x - n1x * n2z, mz = n1x * n2y - n1y * n2x;
    const double l1 = sqrt(b1x * b1x + b1y * b1y + b1z * b1z);
    const double q = mx * b1x + my * b1y + mz * b1z;
    const double y = l1 == 0.0 ? 0.0 : q / l1;   // coincident middle atoms: atan2(0, 0)
    if (kind == DCV_FEAT_TORSION) return {atan2(y, x), 0.0};
    const double r = hypot(x, y);
    return {r == 0.0 ? 0.0 : y / r, r == 0.0 ? 1.0 : x / r};
}

}  // namespace dcv
