// csrc/minmax_solve.hpp on the host, as plain C++17: the roots of the Min-Max / Min-Sum attacks against long double on a grid that
// holds what breaks the textbook formula -- b of both signs at 1e8 times sqrt(c q) (the difference s - |b| cancels there), q = 0,
// a denormal c -- and the row and sum forms against the same reference.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "minmax_solve.hpp"

namespace {

int failures = 0;

// the larger root of c g^2 + 2 b g - q = 0 in long double, by the same two branches
long double root_ref(long double b, long double c, long double q) {
    const long double s = sqrtl(b * b + c * q);
    return b <= 0.0L ? (s - b) / c : q / (s + b);
}

void expect_close(double got, long double want, const char* what, double b, double c, double q) {
    // sqrt, two products, a sum, a difference or sum and a quotient: 6 roundings of 2^-53, doubled
    if (want > static_cast<long double>(std::numeric_limits<double>::max())) {      // beyond fp64: inf, which the kernel reports as broken
        if (!std::isinf(got)) {
            std::printf("%s: b = %a, c = %a, q = %a: got %a, want inf\n", what, b, c, q, got);
            ++failures;
        }
        return;
    }
    const long double tol = 12.0L * 0x1p-53L * fabsl(want) + std::numeric_limits<double>::denorm_min();
    if (!(fabsl(static_cast<long double>(got) - want) <= tol) || !(got >= 0.0)) {
        std::printf("%s: b = %a, c = %a, q = %a: got %a, want %La\n", what, b, c, q, got, want);
        ++failures;
    }
}

}  // namespace

int main() {
    using namespace byz::minmax;
    const double denormal = std::numeric_limits<double>::denorm_min() * 16.0;        // 2^-1070
    const std::vector<double> cs = {denormal, 0x1p-600, 1e-3, 1.0, 3.0, 1e6, 0x1p300};
    const std::vector<double> qs = {0.0, 0x1p-40, 0.7, 1.0, 0x1p27, 1e12};
    const std::vector<double> ks = {0.0, 1e-8, 0.5, 1.0, 3.0, 1e8};
    long long checked = 0;
    for (double c : cs)
        for (double q : qs) {
            if (c < 0x1p-1000 && q != 0.0 && q < 1.0) continue;                        // c q would underflow: not a case of the rule
            const double scale = q == 0.0 ? 1.0 : std::sqrt(c) * std::sqrt(q);
            for (double k : ks)
                for (double sign : {-1.0, 1.0}) {
                    const double b = sign * k * scale;
                    if (b != 0.0 && std::fabs(b) < 0x1p-500) continue;                 // b^2 would underflow: s = sqrt(b^2 + c q) as stated loses b
                    const double g = root(b, c, q);
                    expect_close(g, root_ref(b, c, q), "root", b, c, q);
                    if (q == 0.0 && b >= 0.0 && g != 0.0) {
                        std::printf("root: q = 0, b = %a >= 0 must give 0, got %a\n", b, g);
                        ++failures;
                    }
                    // the row form: T - a = q exactly (a = 0), and a row beyond T has no slack
                    expect_close(row_gamma(0.0, b, c, q), root_ref(b, c, q), "row_gamma", b, c, q);
                    expect_close(row_gamma(2.0 * q + 1.0, b, c, q), root_ref(b, c, 0.0L), "row_gamma (a > T)", b, c, q);
                    // the sum form over r rows: (r c) g^2 + 2 B g - r a_max = 0
                    for (double r : {2.0, 50.0, 4000.0}) {
                        if (c > 0x1p200) continue;
                        const long double want = root_ref(b, static_cast<long double>(r * c), static_cast<long double>(r * q));
                        expect_close(sum_gamma(q, b, c, r), want, "sum_gamma", b, c, q);
                    }
                    ++checked;
                }
        }
    if (sum_bound(2.0, 5.0, 3.0) != 11.0) ++failures;
    const double inf = std::numeric_limits<double>::infinity();
    if (!is_finite(0.0) || !is_finite(denormal) || !is_finite(-1e308) || is_finite(inf) || is_finite(-inf) || is_finite(std::nan(""))) ++failures;
    if (failures != 0) {
        std::printf("minmax_solve: %d failures\n", failures);
        return 1;
    }
    std::printf("minmax_solve ok: %lld roots\n", checked);
    return 0;
}
