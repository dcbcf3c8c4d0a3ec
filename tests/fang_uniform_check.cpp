// csrc/philox.hpp's philox_uniform on the host: compiled as plain C++17 (no HIP) and run by tests/test_fang.py, once plain and
// once under the host sanitizers.  Checks the draw's own properties (inside [fl32(A), fl32(B)], a degenerate interval gives its
// end, an end that is not finite gives the fallback and no NaN), then prints, for fixed (seed, round, row, column, A, B), the
// word and the value as bit patterns for the test to compare with its numpy restatement.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "philox.hpp"

namespace {

int failures = 0;

void expect(const char* what, bool ok) {
    if (!ok) {
        std::printf("FAIL %s\n", what);
        ++failures;
    }
}

uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

struct Case {
    uint64_t seed, round, row, column;
    double A, B;
};

}  // namespace

int main() {
    using namespace byz;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // the ends of the word range stay inside the interval
    expect("word 0 is at least fl32(A)", philox_uniform(0u, 1.0, 2.0, -7.0f) >= 1.0f);
    expect("word 2^32 - 1 is at most fl32(B)", philox_uniform(0xffffffffu, 1.0, 2.0, -7.0f) <= 2.0f);
    expect("a degenerate interval gives its end", bits(philox_uniform(12345u, -0.375, -0.375, -7.0f)) == bits(-0.375f));
    // an end that is not finite: the fallback, whatever the word
    expect("A = -inf gives the fallback", bits(philox_uniform(1u, -inf, 3.0, -7.0f)) == bits(-7.0f));
    expect("B = +inf gives the fallback", bits(philox_uniform(1u, 3.0, inf, 9.0f)) == bits(9.0f));
    expect("both ends infinite: no inf - inf", bits(philox_uniform(1u, -inf, inf, 2.5f)) == bits(2.5f));
    expect("a NaN end gives the fallback", bits(philox_uniform(1u, nan, 1.0, 4.0f)) == bits(4.0f));
    {
        const float passed_on = philox_uniform(1u, nan, nan, std::numeric_limits<float>::quiet_NaN());
        expect("a NaN fallback is handed on", passed_on != passed_on);
    }
    // fp32 ends widened to fp64 and a factor of 2: the value never leaves [fl32(A), fl32(B)]
    {
        const float lo = 0.1f;
        bool inside = true;
        for (uint32_t w = 0; w < 4096u; ++w) {
            const float v = philox_uniform(w * 1048573u, static_cast<double>(lo) / 2.0, static_cast<double>(lo), lo);
            inside = inside && v >= static_cast<float>(static_cast<double>(lo) / 2.0) && v <= lo;
        }
        expect("4096 words inside [lo / 2, lo]", inside);
    }
    if (failures != 0) return 1;
    std::printf("uniform ok\n");
    const Case cases[] = {
        {0, 0, 0, 0, 0.5, 1.0},
        {12345, 7, 3, 10, -2.0, -1.0},
        {12345, 7, 3, 11, 0.05000000074505806, 0.10000000149011612},
        {12345, 7, 4, 11, 0.05000000074505806, 0.10000000149011612},
        {0x9e3779b97f4a7c15ull, 0xffffffffull, 799, (uint64_t{1} << 34) + 2, -1e30, 1e30},
        {1, 2, 1, 5, 3.0, 3.0},
    };
    for (const Case& c : cases) {
        uint32_t x[4];
        philox_block(c.seed, c.round | (c.row << 32), c.column >> 2, x);
        const uint32_t word = x[c.column & 3];
        std::printf("%08" PRIx32 " %08" PRIx32 "\n", word, bits(philox_uniform(word, c.A, c.B, 0.0f)));
    }
    return 0;
}
