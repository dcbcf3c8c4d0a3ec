// The closed forms of the Min-Max / Min-Sum attacks (include/byzagg.h states the rule operation for operation): the largest gamma
// with |mu + gamma p - g_i|^2 = a_i + 2 gamma b_i + gamma^2 c <= T for one row, and the largest gamma with the sum of those over
// the r known rows <= r max a + A.  Each is the positive root of one quadratic, written in the form that does not cancel: the
// root's numerator is s - b where b <= 0 and q / (s + b) where b > 0, with s = sqrt(b^2 + c q) >= |b|.  minmax.hip's solve kernel
// supplies the moments and the reductions.  It compiles as plain C++17 too (tests/minmax_solve_check.cpp runs it on the host
// against long double).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define BYZ_MINMAX_FN __host__ __device__ __forceinline__
#else
#define BYZ_MINMAX_FN inline
#endif

namespace byz {
namespace minmax {

constexpr int kKindMinMax = 0, kKindMinSum = 1;
constexpr int kPerturbUnit = 0, kPerturbStd = 1, kPerturbSign = 2, kPerturbCustom = 3;

// finite: the exponent's bits (no compiler flag changes this test)
BYZ_MINMAX_FN bool is_finite(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// the larger root of c g^2 + 2 b g - q = 0 for c > 0, q >= 0: never negative, 0 when q = 0 and b >= 0
BYZ_MINMAX_FN double root(double b, double c, double q) {
    const double bb = b * b, cq = c * q;
    const double s = std::sqrt(bb + cq);
    return b <= 0.0 ? (s - b) / c : q / (s + b);
}

// Min-Max, one known row: the slack q = max(T - a, 0) (a row farther from mu than T allows binds at gamma = 0 or wherever its
// b < 0 brings it back), then the root
BYZ_MINMAX_FN double row_gamma(double a, double b, double c, double T) {
    const double slack = T - a;
    return root(b, c, slack > 0.0 ? slack : 0.0);
}

// Min-Sum: sum_i (a_i + 2 g b_i + g^2 c) = A + 2 g B + g^2 r c <= r a_max + A
BYZ_MINMAX_FN double sum_gamma(double a_max, double B, double c, double r) {
    const double rc = r * c;
    return root(B, rc, r * a_max);
}
BYZ_MINMAX_FN double sum_bound(double a_max, double A, double r) {
    const double ra = r * a_max;
    return ra + A;
}

}  // namespace minmax
}  // namespace byz

#undef BYZ_MINMAX_FN
