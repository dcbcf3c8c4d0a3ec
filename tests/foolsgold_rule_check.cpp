// csrc/foolsgold_rule.hpp on the host, built with the host sanitizers by tests/test_foolsgold.py: the rule (R) of include/byzagg.h
// run in plain loops -- the kernels' loops, one row at a time -- on the Grams of a file the numpy restatement
// (tests/foolsgold_rule.py: write_rule_cases) wrote beside its own numbers.  m, a, top, the rescaled w, the flags and T under
// 'count' are compared as bits; the weight l within kappa * 4 * 2^-53 (this libm's log and numpy's are each within 1 ulp, not
// equal), and T under 'sum' within n times that.
//   foolsgold_rule_check <cases file>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "foolsgold_rule.hpp"

namespace fg = byz::foolsgold;

static int failures = 0;

static double read_double(FILE* f) {
    uint64_t b = 0;
    if (std::fscanf(f, "%" SCNx64, &b) != 1) {
        std::fprintf(stderr, "short file\n");
        std::exit(2);
    }
    double d;
    std::memcpy(&d, &b, sizeof d);
    return d;
}
static void read_vector(FILE* f, std::vector<double>& v) {
    for (double& x : v) x = read_double(f);
}
static uint64_t bits(double d) {
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}
static void same_bits(const char* what, int c, int i, double got, double want) {
    if (bits(got) != bits(want)) {
        if (++failures <= 20) std::fprintf(stderr, "case %d, %s[%d]: %.17g, expected %.17g\n", c, what, i, got, want);
    }
}
static void near(const char* what, int c, int i, double got, double want, double bound) {
    if (!(std::fabs(got - want) <= bound)) {
        if (++failures <= 20) std::fprintf(stderr, "case %d, %s[%d]: %.17g, expected %.17g within %.3g\n", c, what, i, got, want, bound);
    }
}

// the maximum over j != i with r_j > 0, from +0.0
template <typename F>
static double row_max(const std::vector<double>& r, int n, int i, F f) {
    double acc = 0.0;
    for (int j = 0; j < n; ++j)
        if (j != i && r[j] > 0.0) acc = fg::take_max(acc, f(j));
    return acc;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: foolsgold_rule_check <cases file>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (f == nullptr) {
        std::perror(argv[1]);
        return 2;
    }
    int n_cases = 0;
    if (std::fscanf(f, "%d", &n_cases) != 1) return 2;
    for (int c = 0; c < n_cases; ++c) {
        int n = 0, normalise = 0, want_degenerate = 0;
        if (std::fscanf(f, "%d", &n) != 1 || n < 1) return 2;
        const double kappa = read_double(f);
        if (std::fscanf(f, "%d", &normalise) != 1) return 2;
        const double want_top = read_double(f), want_total = read_double(f);
        if (std::fscanf(f, "%d", &want_degenerate) != 1) return 2;
        std::vector<double> C(static_cast<size_t>(n) * n), want_m(n), want_a(n), want_w(n), want_l(n);
        std::vector<int> want_usable(n);
        read_vector(f, C);
        for (int& u : want_usable)
            if (std::fscanf(f, "%d", &u) != 1) return 2;
        read_vector(f, want_m), read_vector(f, want_a), read_vector(f, want_w), read_vector(f, want_l);

        std::vector<double> r(n), m(n), a(n);
        for (int i = 0; i < n; ++i) r[i] = fg::norm(C[static_cast<size_t>(i) * n + i]);
        for (int i = 0; i < n; ++i) {
            const double* row = &C[static_cast<size_t>(i) * n];
            const double ri = r[i];
            m[i] = ri > 0.0 ? row_max(r, n, i, [&](int j) { return fg::cosine(row[j], ri, r[j]); }) : 0.0;
        }
        for (int i = 0; i < n; ++i) {
            const double* row = &C[static_cast<size_t>(i) * n];
            const double ri = r[i], mi = m[i];
            a[i] = ri > 0.0 ? row_max(r, n, i, [&](int j) { return fg::pardoned(fg::cosine(row[j], ri, r[j]), mi, m[j]); }) : 0.0;
        }
        double top = 0.0;
        int usable = 0;
        for (int i = 0; i < n; ++i)
            if (r[i] >= 0.0) ++usable, top = fg::take_max(top, fg::raw_weight(a[i]));
        const bool few = usable < 2, degenerate = !few && top == 0.0;
        double total = 0.0;
        for (int i = 0; i < n; ++i) {
            const bool in = r[i] >= 0.0;
            double w = 0.0, l = 0.0;
            if (in && few) w = 1.0, l = 1.0;
            else if (in && !degenerate) w = fg::rescaled(fg::raw_weight(a[i]), top), l = fg::clipped_logit(w, kappa);
            total = total + l;
            if ((in ? 1 : 0) != want_usable[i] && ++failures <= 20) std::fprintf(stderr, "case %d, usable[%d]: %d\n", c, i, in ? 1 : 0);
            same_bits("m", c, i, m[i], want_m[i]);
            same_bits("a", c, i, a[i], want_a[i]);
            same_bits("w", c, i, w, want_w[i]);
            near("l", c, i, l, want_l[i], kappa * 4.0 * 0x1p-53);
        }
        same_bits("top", c, 0, top, want_top);
        if (normalise == fg::kNormaliseCount) same_bits("T", c, 0, static_cast<double>(usable), want_total);
        else near("T", c, 0, total, want_total, n * kappa * 4.0 * 0x1p-53);
        if ((degenerate ? 1 : 0) != want_degenerate && ++failures <= 20) std::fprintf(stderr, "case %d: degenerate %d\n", c, degenerate ? 1 : 0);
    }
    std::fclose(f);
    if (failures != 0) {
        std::fprintf(stderr, "foolsgold_rule: %d differences\n", failures);
        return 1;
    }
    std::printf("foolsgold_rule ok: %d cases\n", n_cases);
    return 0;
}
