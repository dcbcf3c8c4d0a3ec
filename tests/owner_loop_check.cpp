// Host check of csrc/owner_loop.hpp's ownership and removal key (tests/test_owner_loop.py compiles and runs this; plain C++17, no HIP).
//   ownership     every row below the ceiling: row_of(owner_thread(r), slot_of(r)) == r, thread and slot in range.
//   removal key   (bad, s, row) over bad in 0 .. 16383 (edges and a stride), s over zeros, subnormals, adjacent doubles, huge values
//                 and +inf, rows 0, 1023, 1024, 16383: every pair of packed keys compares as (more bad first, then larger s, then the
//                 LOWER row) does, the unpacking returns bad, the row and the bits of s, and no key is {0, 0}.
//   the fp64 map  ordered_bits_total(double) equals the sign flip FABA used to carry, value_of_total_key gives the bits back, on
//                 every sample that is neither a NaN nor -0.0.
// Exit status 0 when every property holds; the first violations are printed otherwise.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "order_keys.hpp"
#include "owner_loop.hpp"

namespace {

int failures = 0;
void fail(const char* what, long long a, long long b) {
    if (failures < 20) std::printf("FAIL %s: %lld %lld\n", what, a, b);
    ++failures;
}

uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}
// the map faba.hip had of its own: valid for every double but a NaN, -0.0 strictly below +0.0
uint64_t flip(double v) {
    const uint64_t b = bits_of(v);
    return (b >> 63) ? ~b : (b | (uint64_t{1} << 63));
}

struct Row {
    int bad;
    double s;
    int row;
};
// is `a` removed before `b`?  (FABA's rule: more unusable entries, then the larger sum, then the lower row)
bool before(const Row& a, const Row& b) {
    if (a.bad != b.bad) return a.bad > b.bad;
    if (a.s != b.s) return a.s > b.s;
    return a.row < b.row;
}

}  // namespace

int main() {
    using namespace byz;
    for (int r = 0; r < kOwnerMaxRows; ++r) {
        const int t = owner_thread(r), s = slot_of(r);
        if (t < 0 || t >= kOwnerThreads || s < 0 || s >= kOwnerSlots) fail("owner out of range", r, t);
        if (row_of(t, s) != r) fail("row_of(owner_thread, slot_of)", r, row_of(t, s));
    }

    const double inf = std::numeric_limits<double>::infinity(), tiny = std::numeric_limits<double>::denorm_min();
    const double huge = std::numeric_limits<double>::max();
    const std::vector<double> sums = {0.0, tiny, 2 * tiny, std::numeric_limits<double>::min(), 1.0, std::nextafter(1.0, 2.0),
                                      std::nextafter(1.0, 0.0), 3.5e10, 16384.0, std::nextafter(16384.0, inf), 1e300,
                                      std::nextafter(huge, 0.0), huge, inf};
    std::vector<int> bads = {0, 1, 2, 1023, 1024, 8191, 8192, 16382, 16383};
    for (int b = 5; b < 16384; b += 1237) bads.push_back(b);
    const int rows[] = {0, 1023, 1024, 16383};
    std::vector<Row> all;
    for (int b : bads)
        for (double s : sums)
            for (int r : rows) all.push_back({b, s, r});
    std::vector<RemovalKey> keys;
    for (const Row& x : all) {
        const RemovalKey k = removal_key(x.bad, ordered_bits_total(x.s), x.row);
        keys.push_back(k);
        if (k.hi == 0 && k.lo == 0) fail("a row's key is {0, 0}", x.bad, x.row);
        if (removal_bad(k.hi) != x.bad) fail("bad unpacked", removal_bad(k.hi), x.bad);
        if (removal_row(k.lo) != x.row) fail("row unpacked", removal_row(k.lo), x.row);
        if (bits_of(value_of_total_key(removal_s_key(k.hi, k.lo))) != bits_of(x.s)) fail("s unpacked", x.bad, x.row);
    }
    for (size_t i = 0; i < all.size(); ++i)
        for (size_t j = 0; j < all.size(); ++j) {
            const bool want = before(all[i], all[j]);           // i wins the maximum against j
            if (removal_less(keys[j], keys[i]) != want) fail("key order", static_cast<long long>(i), static_cast<long long>(j));
            if (i != j && !removal_less(keys[j], keys[i]) && !removal_less(keys[i], keys[j])) fail("two rows tie", (long long)i, (long long)j);
        }
    // a bad count outside 0 .. 16383 (cannot happen) is clamped, not spilled into the other fields
    if (removal_bad(removal_key(-3, ordered_bits_total(1.0), 7).hi) != 0) fail("negative bad", -3, 0);
    if (removal_bad(removal_key(1 << 20, ordered_bits_total(1.0), 7).hi) != 16383) fail("large bad", 1 << 20, 0);

    std::vector<double> samples = sums;
    for (double s : sums) samples.push_back(-s);
    for (double v : samples) {
        if (v != v || (v == 0.0 && std::signbit(v))) continue;
        if (ordered_bits_total(v) != flip(v)) fail("ordered_bits_total against the flip", (long long)bits_of(v), 0);
        if (bits_of(value_of_total_key(ordered_bits_total(v))) != bits_of(v)) fail("value_of_total_key", (long long)bits_of(v), 0);
    }
    if (failures != 0) {
        std::printf("owner_loop FAILED: %d\n", failures);
        return 1;
    }
    std::printf("owner_loop ok: %d rows, %zu keys\n", static_cast<int>(kOwnerMaxRows), keys.size());
    return 0;
}
