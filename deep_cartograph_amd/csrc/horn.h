// Optimal rotation of a weighted point set onto another from their 3 x 3 correlation (Horn 1987): the unit quaternion
// of the rotation is the eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix built from the correlation.
// The eigenvector is found by cyclic Jacobi rotations with a convergence test and a fixed sweep cap: no polynomial
// root finding (a Newton iteration on the characteristic polynomial stalls where the two largest eigenvalues meet:
// coplanar, collinear and mirror-image sets), and the eigenvectors stay orthonormal whatever the spectrum is, so a
// unit quaternion -- a proper rotation -- comes back in every case, also for an all-zero correlation (the identity).
// Every loop has compile-time bounds so the 4 x 4 matrices stay in registers.
#pragma once

#include <math.h>

namespace dcv {

constexpr int kJacobiSweeps = 16;   // a 4 x 4 matrix converges in 4 - 7 sweeps; the cap only bounds non-finite input

// S[3 * a + b] = sum_i w_i x_ia y_ib over CENTRED mobile points x and reference points y.  R (row-major, row-vector
// convention) minimises sum_i w_i |x_i . R - y_i|^2 over proper rotations.
__device__ __forceinline__ void horn_rotation(const double* S, double* R) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[4][4], V[4][4];
    A[0][0] = Sxx + Syy + Szz;
    A[1][1] = Sxx - Syy - Szz;
    A[2][2] = -Sxx + Syy - Szz;
    A[3][3] = -Sxx - Syy + Szz;
    A[0][1] = A[1][0] = Syz - Szy;
    A[0][2] = A[2][0] = Szx - Sxz;
    A[0][3] = A[3][0] = Sxy - Syx;
    A[1][2] = A[2][1] = Sxy + Syx;
    A[1][3] = A[3][1] = Szx + Sxz;
    A[2][3] = A[3][2] = Syz + Szy;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;

    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            diag += A[p][p] * A[p][p];
#pragma unroll
            for (int q = p + 1; q < 4; ++q) off += A[p][q] * A[p][q];
        }
        // converged: the off-diagonal norm is below one rounding of the matrix norm.  Written so that NaN ends the loop.
        if (!(off > 1e-32 * (diag + 2.0 * off))) break;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // theta^2 = inf gives t = 0
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r != p && r != q) {
                        const double arp = A[r][p], arq = A[r][q];
                        A[r][p] = A[p][r] = arp - s * (arq + tau * arp);
                        A[r][q] = A[q][r] = arq + s * (arp - tau * arq);
                    }
                    const double vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = vrp - s * (vrq + tau * vrp);
                    V[r][q] = vrq + s * (vrp - tau * vrq);
                }
            }
        }
    }
    // the eigenvector of the largest eigenvalue, picked with selects (no indexed register access)
    double lam = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool b = A[k][k] > lam;
        lam = b ? A[k][k] : lam;
        q0 = b ? V[0][k] : q0; q1 = b ? V[1][k] : q1; q2 = b ? V[2][k] : q2; q3 = b ? V[3][k] : q3;
    }
    const double nrm = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    q0 *= nrm; q1 *= nrm; q2 *= nrm; q3 *= nrm;
    // column-vector rotation C that takes x to y; R = C^T
    const double C00 = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, C01 = 2.0 * (q1 * q2 - q0 * q3), C02 = 2.0 * (q1 * q3 + q0 * q2);
    const double C10 = 2.0 * (q1 * q2 + q0 * q3), C11 = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, C12 = 2.0 * (q2 * q3 - q0 * q1);
    const double C20 = 2.0 * (q1 * q3 - q0 * q2), C21 = 2.0 * (q2 * q3 + q0 * q1), C22 = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
    R[0] = C00; R[1] = C10; R[2] = C20;
    R[3] = C01; R[4] = C11; R[5] = C21;
    R[6] = C02; R[7] = C12; R[8] = C22;
}

}  // namespace dcv
