// normals_solve.h — the part of the normal estimation that every lane computes alike: the unit eigenvector of the smallest eigenvalue of
// a 3 x 3 covariance (a fixed number of cyclic Jacobi sweeps in double, the 3 x 3 sibling of icp_solve.h's 4 x 4 pattern) and the sign of
// the result.  Stated in include/dnsplat.h and restated in torch_normals.py.  Plain C++ of + - * / sqrt fabs, so that a host compiler reads
// the same text.  Compile without contraction.
#pragma once

#include <math.h>

#ifdef __HIPCC__
#define NM_FN __host__ __device__ inline __attribute__((always_inline))
#define NM_UNROLL _Pragma("unroll")
#else
#define NM_FN inline
#define NM_UNROLL
#endif

namespace {

constexpr int NM_SWEEPS = 8;

// One rotation of the cyclic Jacobi on the symmetric A (both triangles kept) and the accumulated V, in the plane (P, Q); R is the third
// axis.  An off-diagonal entry that changes neither diagonal entry when added to its magnitude is set to zero without a rotation.
template <int P, int Q>
NM_FN void nm_rotate(double (&A)[3][3], double (&V)[3][3])
{
    constexpr int R = 3 - P - Q;
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double app = A[P][P], aqq = A[Q][Q], g = fabs(apq);
    if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
        A[P][Q] = 0.0; A[Q][P] = 0.0;
        return;
    }
    const double theta = (aqq - app) / (2.0 * apq);
    const double mag = fabs(theta) + sqrt(theta * theta + 1.0);                     // inf for a huge theta: t = 0
    const double tt = (theta < 0.0 ? -1.0 : 1.0) / mag;
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
    A[P][P] = app - tt * apq;
    A[Q][Q] = aqq + tt * apq;
    A[P][Q] = 0.0; A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = c * arp - s * arq; A[P][R] = A[R][P];
    A[R][Q] = s * arp + c * arq; A[Q][R] = A[R][Q];
    NM_UNROLL
    for (int r = 0; r < 3; ++r) {
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// The normal of n neighbours with the covariance C (xx, xy, xz, yy, yz, zz), before its sign is chosen.
NM_FN void nm_normal(const double C[6], int n, double out[3])
{
    out[0] = 0.0; out[1] = 0.0; out[2] = 1.0;                                       // Open3D's fallback
    const bool zero = C[0] == 0.0 && C[1] == 0.0 && C[2] == 0.0 && C[3] == 0.0 && C[4] == 0.0 && C[5] == 0.0;
    if (n < 3 || zero) return;
    double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < NM_SWEEPS; ++sweep) {
        nm_rotate<0, 1>(A, V); nm_rotate<0, 2>(A, V); nm_rotate<1, 2>(A, V);
    }
    // the smallest eigenvalue; equal ones go to the lowest column
    const bool one = A[1][1] < A[0][0];
    const double l01 = one ? A[1][1] : A[0][0];
    const bool two = A[2][2] < l01;
    double e[3];
    NM_UNROLL
    for (int r = 0; r < 3; ++r) e[r] = two ? V[r][2] : (one ? V[r][1] : V[r][0]);
    const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    out[0] = e[0] / len; out[1] = e[1] / len; out[2] = e[2] / len;
}

// The sign: towards `toward` from p (flip iff the dot product is negative), or canonical: the component of largest magnitude positive,
// the lowest axis on equal magnitudes.
NM_FN void nm_orient(double nrm[3], bool orient, const double toward[3], const double p[3])
{
    bool flip;
    if (orient) {
        const double dot = (nrm[0] * (toward[0] - p[0]) + nrm[1] * (toward[1] - p[1])) + nrm[2] * (toward[2] - p[2]);
        flip = dot < 0.0;
    } else {
        const double ax = fabs(nrm[0]), ay = fabs(nrm[1]), az = fabs(nrm[2]);
        const bool one = ay > ax;
        const double m01 = one ? ay : ax;
        const bool two = az > m01;
        const double lead = two ? nrm[2] : (one ? nrm[1] : nrm[0]);
        flip = lead < 0.0;
    }
    if (flip) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
}

}  // namespace

#undef NM_FN
#undef NM_UNROLL
