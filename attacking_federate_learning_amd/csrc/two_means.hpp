// Auror's per-column rule (include/byzagg.h states it operation for operation): Lloyd's 2-means of one column's finite values from
// the start c0 = min, c1 = max.  What decides is here -- which values take part, the threshold, the side of a value, when a column
// stops, which side is suspicious -- and auror.hip's kernel supplies the sums.  It compiles as plain C++17 too
// (tests/two_means_check.cpp runs it on the host against a sort-based 2-means).
#pragma once

#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define BYZ_TWO_MEANS_FN __host__ __device__ __forceinline__
#else
#define BYZ_TWO_MEANS_FN inline
#endif

namespace byz {
namespace two_means {

// a column's state between two sweeps over its values
struct Column {
    double c0, c1;        // the centres: min and max at the start, then the clusters' means
    double t;             // the threshold of the next sweep; once the column has stopped: of its last one, the final assignment's
    int32_t m;            // the finite values
    int32_t m1;           // the values above t in the last sweep (-1 before the first)
    int32_t stopped;      // no further sweep changes the column
    int32_t clustered;    // m >= 2 and min < max
    int32_t capped;       // stopped by max_iter with m1 still moving
    int32_t pad;
};

// a value takes part in its column when it is finite (the exponent's bits: no compiler flag changes this test)
BYZ_TWO_MEANS_FN bool takes_part(float x) {
    uint32_t b;
    std::memcpy(&b, &x, sizeof b);
    return (b & 0x7f800000u) != 0x7f800000u;
}

BYZ_TWO_MEANS_FN double threshold(double c0, double c1) { return 0.5 * (c0 + c1); }

// cluster 1: strictly above the threshold (a value equal to it stays in cluster 0; -0 and +0 are one value)
BYZ_TWO_MEANS_FN bool upper(float x, double t) { return static_cast<double>(x) > t; }

// the column before its first sweep: mn and mx are the smallest and largest of its m finite values (anything when m == 0)
BYZ_TWO_MEANS_FN void start(Column& c, int32_t m, float mn, float mx) {
    c.m = m;
    c.m1 = -1;
    c.capped = 0;
    c.pad = 0;
    c.clustered = (m >= 2 && mn < mx) ? 1 : 0;
    c.stopped = c.clustered ? 0 : 1;
    c.c0 = c.clustered ? static_cast<double>(mn) : 0.0;
    c.c1 = c.clustered ? static_cast<double>(mx) : 0.0;
    c.t = threshold(c.c0, c.c1);
}

// Sweep k (1-based) of a column that has not stopped found m1 values above c.t, their sum s1, and the sum s0 of the others.
// min <= t < max throughout, so neither cluster is empty; a count that says otherwise (it cannot) stops the column as it stands.
BYZ_TWO_MEANS_FN void step(Column& c, int k, int max_iter, int32_t m1, double s1, double s0) {
    if (m1 <= 0 || m1 >= c.m) {
        c.stopped = 1;
        return;
    }
    c.c1 = s1 / static_cast<double>(m1);
    c.c0 = s0 / static_cast<double>(c.m - m1);
    const bool settled = k >= 2 && m1 == c.m1;      // an integer: the order of the sums has no say in it
    c.m1 = m1;
    if (settled) {
        c.stopped = 1;
    } else if (k >= max_iter) {
        c.stopped = 1;
        c.capped = 1;
    } else {
        c.t = threshold(c.c0, c.c1);
    }
}

BYZ_TWO_MEANS_FN double gap(const Column& c) { return c.clustered ? c.c1 - c.c0 : 0.0; }

BYZ_TWO_MEANS_FN bool indicative(const Column& c, double alpha) { return c.clustered != 0 && (c.c1 - c.c0) > alpha; }

// the suspicious side of an indicative column: 1 the values above c.t, 0 the others, -1 nobody (not indicative, or equal counts)
BYZ_TWO_MEANS_FN int suspicious_side(const Column& c, double alpha) {
    if (!indicative(c, alpha) || c.m1 < 0) return -1;
    const int32_t m0 = c.m - c.m1;
    if (c.m1 == m0) return -1;
    return c.m1 < m0 ? 1 : 0;
}

// one value's vote in a column whose suspicious side is `side`
BYZ_TWO_MEANS_FN bool votes(float x, double t, int side) { return side >= 0 && takes_part(x) && (upper(x, t) ? 1 : 0) == side; }

}  // namespace two_means
}  // namespace byz

#undef BYZ_TWO_MEANS_FN
