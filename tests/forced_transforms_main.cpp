// A stand-alone program over the forced transforms of csrc/common/pmx_dense.h
// (p2plane_transform_4dof, p2plane_transform_force2d) and the forced step's
// solve, for a host build with -fsanitize=address,undefined
// (tests/test_forced_chain.py builds and runs it).  Exit status 0: every check held.
#include <cmath>
#include <cstdio>
#include <limits>

#include "common/pmx_dense.h"

namespace d = pmx_dense;

template <typename T>
static int run(const char* name) {
    int bad = 0;
    const T angles[] = {(T)0, (T)1.3e-3, (T)-0.4, (T)1.0};
    for (T a : angles) {
        const T x4[4] = {a, (T)0.25, (T)-0.5, (T)0.75};
        T m[16];
        for (T& v : m) v = std::numeric_limits<T>::quiet_NaN();  // (every entry must be written)
        d::p2plane_transform_4dof(x4, m);
        const T c = std::cos(a), s = std::sin(a);
        const T want[16] = {c, -s, 0, x4[1], s, c, 0, x4[2], 0, 0, 1, x4[3], 0, 0, 0, 1};
        for (int i = 0; i < 16; ++i)
            if (!(m[i] == want[i])) ++bad, std::printf("%s 4dof angle %g entry %d: %g != %g\n", name, (double)a, i, (double)m[i], (double)want[i]);
        const T x3[3] = {a, (T)0.25, (T)-0.5};
        for (T& v : m) v = std::numeric_limits<T>::quiet_NaN();
        d::p2plane_transform_force2d(x3, m);
        const T want2[16] = {c, -s, 0, x3[1], s, c, 0, x3[2], 0, 0, 1, 0, 0, 0, 0, 1};
        for (int i = 0; i < 16; ++i)
            if (!(m[i] == want2[i])) ++bad, std::printf("%s 2d angle %g entry %d: %g != %g\n", name, (double)a, i, (double)m[i], (double)want2[i]);
    }
    // the NaN guard of the 4-DOF branch: the rotation becomes the identity, the translation stays
    const T xn[4] = {std::numeric_limits<T>::quiet_NaN(), (T)1, (T)2, (T)3};
    T m[16];
    d::p2plane_transform_4dof(xn, m);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            if (m[r * 4 + c] != (r == c ? (T)1 : (T)0)) ++bad, std::printf("%s NaN guard (%d, %d)\n", name, r, c);
    if (m[3] != 1 || m[7] != 2 || m[11] != 3 || m[15] != 1) ++bad, std::printf("%s NaN guard translation\n", name);
    // the forced systems' sizes through the solver: a full-rank 4 x 4 and a rank-2 3 x 3 (t_y free)
    const T A4[16] = {4, 1, 0, 0, 1, 3, 0, 0, 0, 0, 2, 1, 0, 0, 1, 2}, b4[4] = {1, 2, 3, 4};
    T x[6];
    d::solve_underdetermined(A4, b4, 4, x);
    for (int r = 0; r < 4; ++r) {
        T s = 0;
        for (int c = 0; c < 4; ++c) s += A4[r * 4 + c] * x[c];
        if (std::fabs(s - b4[r]) > (T)1e-4) ++bad, std::printf("%s 4 x 4 solve row %d\n", name, r);
    }
    const T A3[9] = {2, 1, 0, 1, 2, 0, 0, 0, 0}, b3[3] = {1, 1, 0};
    d::solve_underdetermined(A3, b3, 3, x);
    if (x[2] != 0 || std::fabs(x[0] - (T)(1.0 / 3)) > (T)1e-5 || std::fabs(x[1] - (T)(1.0 / 3)) > (T)1e-5)
        ++bad, std::printf("%s rank-2 3 x 3 solve: %g %g %g\n", name, (double)x[0], (double)x[1], (double)x[2]);
    return bad;
}

int main() {
    const int bad = run<float>("float") + run<double>("double");
    std::printf("forced transforms: %d failures\n", bad);
    return bad != 0;
}
