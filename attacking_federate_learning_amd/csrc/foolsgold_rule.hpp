// FoolsGold's rule on an fp64 Gram (include/byzagg.h states it operation for operation, (R) 1 to 8): what decides is here -- which
// rows are usable, the norm, a cosine, the running maximum, the pardoned cosine, the raw weight, the rescaled weight and the
// clipped logit -- and foolsgold.hip's kernels supply the loops.  Every function is one or two fp64 operations in a stated order;
// the file that includes it is compiled with -ffp-contract=off.  It compiles as plain C++17 too (tests/foolsgold_rule_check.cpp
// runs it on the host against the numpy restatement's numbers).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define BYZ_FOOLSGOLD_FN __host__ __device__ __forceinline__
#else
#define BYZ_FOOLSGOLD_FN inline
#endif

namespace byz {
namespace foolsgold {

constexpr int kNormaliseCount = 0;     // T = the number of usable rows
constexpr int kNormaliseSum = 1;       // T = the weights summed in ascending row order

// (1) a row is usable when its diagonal entry is finite and not negative (the exponent's bits: no compiler flag changes this test)
BYZ_FOOLSGOLD_FN bool usable(double diag) {
    uint64_t b;
    std::memcpy(&b, &diag, sizeof b);
    const bool finite = (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
    return finite && diag >= 0.0;
}

// (2) the norm; -1 marks an excluded row, so "takes part in a cosine" is r > 0 and "usable" is r >= 0
BYZ_FOOLSGOLD_FN double norm(double diag) { return usable(diag) ? std::sqrt(diag) : -1.0; }

// (3) both norms > 0 and i != j are the caller's business; a NaN is taken as 0, nothing is clamped
BYZ_FOOLSGOLD_FN double cosine(double c, double ri, double rj) {
    const double cs = c / (ri * rj);
    return cs != cs ? 0.0 : cs;
}

// (4), (5) the running maximum from +0.0: a NaN and a -0.0 never replace what is there
BYZ_FOOLSGOLD_FN double take_max(double acc, double x) { return x > acc ? x : acc; }

// (5) m_j > m_i >= 0 where the quotient is formed: the divisor is never 0
BYZ_FOOLSGOLD_FN double pardoned(double cs, double mi, double mj) { return mi < mj ? (cs * mi) / mj : cs; }

// (6)
BYZ_FOOLSGOLD_FN double raw_weight(double a) {
    const double v = 1.0 - a;
    const double lo = v > 0.0 ? v : 0.0;
    return lo < 1.0 ? lo : 1.0;
}

// (8) top > 0
BYZ_FOOLSGOLD_FN double rescaled(double v, double top) {
    const double w = v / top;
    return w == 1.0 ? 0.99 : w;
}
BYZ_FOOLSGOLD_FN double clipped_logit(double w, double kappa) {
    if (w == 0.0) return 0.0;
    const double l = kappa * (std::log(w / (1.0 - w)) + 0.5);
    const double lo = l > 0.0 ? l : 0.0;
    return lo < 1.0 ? lo : 1.0;
}

}  // namespace foolsgold
}  // namespace byz

#undef BYZ_FOOLSGOLD_FN
