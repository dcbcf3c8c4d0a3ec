// csrc/two_means.hpp on the host: the per-column rule of Auror driven the way auror.hip's kernel drives it (a first pass for
// the extremes, sweeps that hand (m1, S1, S0) to step(), the votes of the final assignment), held to a brute-force 2-means that
// knows nothing of the header: the values sorted, every assignment a split point of the sorted list, the sums taken afresh.
// Quarter-integer values make every sum exact, so the two agree bit for bit whatever the order of the sums.
// Built and run by tests/test_auror.py with the host sanitizers; plain C++17, no HIP.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "two_means.hpp"

namespace rule = byz::two_means;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("line %d: %s\n", __LINE__, #cond);                 \
            if (++failures > 20) std::exit(1);                             \
        }                                                                  \
    } while (0)

struct Result {
    rule::Column col;
    std::vector<int> voted;      // the rows that got a vote
    int sweeps;
};

// the kernel's walk over one column: rows split over `groups` row groups, a group's rows ascending, the groups ascending
static Result run_header(const std::vector<float>& x, double alpha, int max_iter, int groups) {
    Result r{};
    const int n = static_cast<int>(x.size());
    float mn = std::numeric_limits<float>::infinity(), mx = -mn;
    int m = 0;
    for (float v : x)
        if (rule::takes_part(v)) {
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
            ++m;
        }
    rule::start(r.col, m, mn, mx);
    for (int k = 1; !r.col.stopped; ++k) {
        CHECK(k <= max_iter);
        int m1 = 0;
        double s1 = 0.0, s0 = 0.0;
        for (int g = 0; g < groups; ++g) {
            int gm = 0;
            double g1 = 0.0, g0 = 0.0;
            for (int i = g; i < n; i += groups) {
                if (!rule::takes_part(x[i])) continue;
                if (rule::upper(x[i], r.col.t)) {
                    ++gm;
                    g1 += static_cast<double>(x[i]);
                } else {
                    g0 += static_cast<double>(x[i]);
                }
            }
            m1 += gm;
            s1 += g1;
            s0 += g0;
        }
        rule::step(r.col, k, max_iter, m1, s1, s0);
        r.sweeps = k;
    }
    const int side = rule::suspicious_side(r.col, alpha);
    for (int i = 0; i < n; ++i)
        if (rule::votes(x[i], r.col.t, side)) r.voted.push_back(i);
    return r;
}

// the rule again from its statement, on the sorted finite values: cluster 1 is a suffix of the sorted list
struct Brute {
    bool clustered = false, capped = false, indicative = false;
    double gap = 0.0, t = 0.0;
    int m = 0, m1 = -1, side = -1, sweeps = 0;
};
static Brute run_brute(const std::vector<float>& x, double alpha, int max_iter) {
    Brute b;
    std::vector<double> s;
    for (float v : x)
        if (std::isfinite(v)) s.push_back(static_cast<double>(v));
    std::sort(s.begin(), s.end());
    b.m = static_cast<int>(s.size());
    if (b.m < 2 || s.front() == s.back()) return b;
    b.clustered = true;
    double c0 = s.front(), c1 = s.back();
    int prev = -1;
    for (int k = 1; k <= max_iter; ++k) {
        b.t = 0.5 * (c0 + c1);
        const int first_upper = static_cast<int>(std::upper_bound(s.begin(), s.end(), b.t) - s.begin());
        const int m1 = b.m - first_upper;
        double s0 = 0.0, s1 = 0.0;
        for (int i = 0; i < first_upper; ++i) s0 += s[i];
        for (int i = first_upper; i < b.m; ++i) s1 += s[i];
        c1 = s1 / m1;
        c0 = s0 / (b.m - m1);
        b.sweeps = k;
        b.m1 = m1;
        if (k >= 2 && m1 == prev) break;
        if (k == max_iter) {
            b.capped = true;
            break;
        }
        prev = m1;
    }
    b.gap = c1 - c0;
    b.indicative = b.gap > alpha;
    if (b.indicative && b.m1 != b.m - b.m1) b.side = b.m1 < b.m - b.m1 ? 1 : 0;
    return b;
}

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

static void compare(const std::vector<float>& x, double alpha, int max_iter) {
    const Brute want = run_brute(x, alpha, max_iter);
    for (int groups : {1, 16, 64}) {
        const Result got = run_header(x, alpha, max_iter, groups);
        CHECK(got.col.m == want.m);
        CHECK((got.col.clustered != 0) == want.clustered);
        CHECK((got.col.capped != 0) == want.capped);
        CHECK(got.col.stopped == 1);
        CHECK(bits(rule::gap(got.col)) == bits(want.gap));
        CHECK(rule::indicative(got.col, alpha) == want.indicative);
        CHECK(rule::suspicious_side(got.col, alpha) == want.side);
        if (want.clustered) {
            CHECK(got.sweeps == want.sweeps);
            CHECK(got.col.m1 == want.m1);
            CHECK(bits(got.col.t) == bits(want.t));
            CHECK(got.col.m1 >= 1 && got.col.m1 < got.col.m);
        }
        std::vector<int> voted;
        for (int i = 0; i < static_cast<int>(x.size()); ++i)
            if (want.side >= 0 && std::isfinite(x[i]) && ((static_cast<double>(x[i]) > want.t) ? 1 : 0) == want.side) voted.push_back(i);
        CHECK(voted == got.voted);
        if (want.side >= 0) CHECK(static_cast<int>(voted.size()) == std::min(want.m1, want.m - want.m1));
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the columns that are not clustered
    compare({}, 0.0, 32);
    compare({1.0f}, 0.0, 32);
    compare({nan, inf, -inf}, 0.0, 32);
    compare({nan, 2.0f, inf}, 0.0, 32);
    compare({3.0f, 3.0f, 3.0f, 3.0f}, 0.0, 32);
    compare({-0.0f, 0.0f, 0.0f, -0.0f}, 0.0, 32);               // -0 == +0: constant
    // two values, a value on the threshold, equal clusters, denormals
    compare({0.0f, 1.0f}, 0.5, 32);                             // one each: nobody is suspicious
    compare({0.0f, 1.0f, 2.0f}, 0.5, 32);                       // t = 1 exactly: the 1 stays below
    compare({-0.0f, 0.0f, 1.0f}, 0.25, 32);
    compare({1e-45f, 2e-45f, 3e-45f, 1e-40f}, 0.0, 32);
    compare({-2.0f, -2.0f, 2.0f, 2.0f}, 1.0, 32);
    compare({0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 4.0f, nan}, 3.9, 32);
    compare({0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 4.0f, inf}, 4.0, 32);    // the gap equals alpha: not indicative
    // the cap
    for (int cap : {1, 2, 3}) compare({0.0f, 0.25f, 0.5f, 0.75f, 1.0f, 1.25f, 1.5f, 8.0f}, 1.0, cap);
    // quarter-integer columns: every sum exact, values land on the threshold
    std::mt19937 rng(20161205);
    for (int trial = 0; trial < 400; ++trial) {
        const int n = 1 + static_cast<int>(rng() % 300);
        std::vector<float> x(n);
        for (float& v : x) {
            v = static_cast<float>(static_cast<int>(rng() % 17) - 8) / 4.0f;
            const unsigned odd = rng() % 64;
            if (odd == 0) v = nan;
            if (odd == 1) v = (rng() & 1) ? inf : -inf;
            if (odd == 2) v = -0.0f;
        }
        if (trial % 3 == 0)
            for (int i = 0; i < n / 5; ++i) x[i] = 16.0f + static_cast<float>(rng() % 5) / 4.0f;     // a planted minority
        compare(x, static_cast<double>(rng() % 9) / 4.0, 1 + static_cast<int>(rng() % 6) * (trial % 2 ? 1 : 8));
    }
    if (failures != 0) return 1;
    std::printf("two_means ok\n");
    return 0;
}
