// icp_solve_host_check.cpp — the solve of the mesh alignment (csrc/icp_solve.h, the very text icp_solve_kernel compiles) as a host program:
// it reads one pass's moments — n, then the 16 sums d2, q[3], g[3], gq[9] and the centre c[3] as C99 hexadecimal doubles — from standard
// input and prints R[9], t[3] in the same notation and the DEGENERATE flag.  tests/test_icp_reference.py builds it with g++ and holds its
// output bit for bit to torch_icp.solve.  A stand-alone program: it touches no device and loads nothing into Python.
//
//   g++ -O2 -std=c++17 -ffp-contract=off tools/icp_solve_host_check.cpp -o /tmp/icp_solve_host_check
#include <cstdio>

#include "../dn-splatter_amd/csrc/icp_solve.h"

int main()
{
    IcpPartial v = IcpPartial::identity();
    double c[3], R[9], t[3];
    if (std::scanf("%lld", &v.n) != 1) return 2;
    double *sums[16] = {&v.d2, &v.q[0], &v.q[1], &v.q[2], &v.g[0], &v.g[1], &v.g[2], &v.gq[0], &v.gq[1], &v.gq[2], &v.gq[3], &v.gq[4], &v.gq[5],
                        &v.gq[6], &v.gq[7], &v.gq[8]};
    for (double *s : sums)
        if (std::scanf("%la", s) != 1) return 2;
    for (double &x : c)
        if (std::scanf("%la", &x) != 1) return 2;
    const bool degenerate = icp_solve(v, c, R, t);
    for (double x : R) std::printf("%a ", x);
    for (double x : t) std::printf("%a ", x);
    std::printf("%d\n", degenerate ? 1 : 0);
    return 0;
}
