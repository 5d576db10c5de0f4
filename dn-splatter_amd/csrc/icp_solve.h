// icp_solve.h — the part of the mesh alignment that one thread computes: the partial of the moments and the rigid update solved from
// them (Horn's 4 x 4 quaternion matrix, a fixed-order cyclic Jacobi in double), stated in include/dnsplat.h and restated in torch_icp.py.
// Plain C++ of + - * / sqrt, so that a host compiler reads the same text: tools/icp_solve_host_check.cpp and tests/test_icp_reference.py
// hold it bit for bit to the restatement without a device.  Compile without contraction.
#pragma once

#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#define __forceinline__ inline
#endif

namespace {

constexpr int ICP_SWEEPS = 10;

struct IcpPartial {                                       // 136 bytes
    long long n;
    double d2, q[3], g[3], gq[9];                         // gq[3 a + b] = sum of (g - c)[a] (q - c)[b]
    static __host__ __device__ IcpPartial identity()
    {
        IcpPartial p;
        p.n = 0; p.d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { p.q[k] = 0.0; p.g[k] = 0.0; }
#pragma unroll
        for (int k = 0; k < 9; ++k) p.gq[k] = 0.0;
        return p;
    }
    __host__ __device__ void join(const IcpPartial &o)
    {
        n += o.n; d2 += o.d2;
#pragma unroll
        for (int k = 0; k < 3; ++k) { q[k] += o.q[k]; g[k] += o.g[k]; }
#pragma unroll
        for (int k = 0; k < 9; ++k) gq[k] += o.gq[k];
    }
};
static_assert(sizeof(IcpPartial) == 136, "a partial is 17 words of 8 bytes");

// One rotation of the cyclic Jacobi on the symmetric A (both triangles kept) and the accumulated V, in the plane (p, q)
__host__ __device__ __forceinline__ void icp_rotate(double A[4][4], double V[4][4], int p, int q)
{
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double mag = (theta < 0.0 ? -theta : theta) + sqrt(theta * theta + 1.0);     // inf for a huge theta: t = 0
    const double tt = (theta < 0.0 ? -1.0 : 1.0) / mag;
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
    A[p][p] = A[p][p] - tt * apq;
    A[q][q] = A[q][q] + tt * apq;
    A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != p && r != q) {
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = c * arp - s * arq; A[p][r] = A[r][p];
            A[r][q] = s * arp + c * arq; A[q][r] = A[r][q];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double vrp = V[r][p], vrq = V[r][q];
        V[r][p] = c * vrp - s * vrq;
        V[r][q] = s * vrp + c * vrq;
    }
}

// The rigid update U (rotation R, translation t) of the moments, and whether the rotation is determined.  Stated in dnsplat.h.
__host__ __device__ __forceinline__ bool icp_solve(const IcpPartial &v, const double c[3], double R[9], double tr[3])
{
    const double n = (double)v.n;
    double mq[3], mg[3], S[3][3];                         // S[a][b] = Sigma[a][b]: g along a, q along b
#pragma unroll
    for (int k = 0; k < 3; ++k) { mq[k] = v.q[k] / n; mg[k] = v.g[k] / n; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[i][j] = v.gq[3 * i + j] / n - mg[i] * mq[j];
    // Horn's matrix of the quaternion (w, x, y, z); his S_xy pairs the source's x with the target's y: Sigma[1][0]
    const double Sxx = S[0][0], Sxy = S[1][0], Sxz = S[2][0], Syx = S[0][1], Syy = S[1][1], Syz = S[2][1], Szx = S[0][2], Szy = S[1][2],
                 Szz = S[2][2];
    double A[4][4], V[4][4];
    A[0][0] = (Sxx + Syy) + Szz;
    A[1][1] = (Sxx - Syy) - Szz;
    A[2][2] = (Syy - Sxx) - Szz;
    A[3][3] = (Szz - Sxx) - Syy;
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
    for (int sweep = 0; sweep < ICP_SWEEPS; ++sweep) {
        icp_rotate(A, V, 0, 1); icp_rotate(A, V, 0, 2); icp_rotate(A, V, 0, 3);
        icp_rotate(A, V, 1, 2); icp_rotate(A, V, 1, 3); icp_rotate(A, V, 2, 3);
    }
    // the largest eigenvalue and the one below it; ties go to the lower column
    int i1 = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) if (A[k][k] > A[i1][i1]) i1 = k;
    int i2 = i1 == 0 ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k != i1 && k != i2 && A[k][k] > A[i2][i2]) i2 = k;
    double l1 = 0.0, l2 = 0.0, e[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {                         // static indices only
        l1 = k == i1 ? A[k][k] : l1;
        l2 = k == i2 ? A[k][k] : l2;
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = k == i1 ? V[r][k] : e[r];
    }
    const double len = sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]);
    const double w = e[0] / len, x = e[1] / len, y = e[2] / len, z = e[3] / len;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
    double fq[3], fg[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { fq[k] = mq[k] + c[k]; fg[k] = mg[k] + c[k]; }
#pragma unroll
    for (int a = 0; a < 3; ++a) tr[a] = fg[a] - ((R[3 * a] * fq[0] + R[3 * a + 1] * fq[1]) + R[3 * a + 2] * fq[2]);
    // l1 - l2 = 2 (sigma_2 + s sigma_3) and l1 + l2 = 2 sigma_1
    return (l1 - l2) * 0.5 <= 0x1p-26 * ((l1 + l2) * 0.5);
}

}  // namespace
