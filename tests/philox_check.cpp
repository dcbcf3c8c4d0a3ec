// csrc/philox.hpp on the host: compiled as plain C++17 (no HIP) and run by tests/test_weak_dp.py.
// Checks Random123's three known answers for philox4x32_10, the counter layout of the stream (block 2^32 increments counter word
// 1, `round` lands in words 2 and 3, the seed's halves are the key), that the third known answer comes back through
// philox_block, and the range of the normals; then prints the normals of eight columns as fp64 bit patterns for the test to
// compare with its numpy restatement.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "philox.hpp"

namespace {

int failures = 0;

void expect_words(const char* what, const uint32_t (&got)[4], uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t want[4] = {a, b, c, d};
    if (std::memcmp(got, want, sizeof(want)) != 0) {
        std::printf("FAIL %s: got %08x %08x %08x %08x, want %08x %08x %08x %08x\n", what, got[0], got[1], got[2], got[3], a, b, c, d);
        ++failures;
    }
}

void expect(const char* what, bool ok) {
    if (!ok) {
        std::printf("FAIL %s\n", what);
        ++failures;
    }
}

}  // namespace

int main() {
    using namespace byz;
    // the known answers
    {
        uint32_t c[4] = {0, 0, 0, 0};
        philox4x32_10(c, 0, 0);
        expect_words("zero counter, zero key", c, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u);
    }
    {
        uint32_t c[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
        philox4x32_10(c, 0xffffffffu, 0xffffffffu);
        expect_words("all ones", c, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu);
    }
    {
        uint32_t c[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u};
        philox4x32_10(c, 0xa4093822u, 0x299f31d0u);
        expect_words("digits of pi", c, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u);
    }
    // the counter layout
    {
        uint32_t c[4];
        philox_counter(uint64_t{1} << 32, 0, c);
        expect("block 2^32 is counter (0, 1, 0, 0)", c[0] == 0 && c[1] == 1 && c[2] == 0 && c[3] == 0);
        philox_counter((uint64_t{1} << 32) - 1, 0, c);
        expect("block 2^32 - 1 is counter (ffffffff, 0, 0, 0)", c[0] == 0xffffffffu && c[1] == 0 && c[2] == 0 && c[3] == 0);
        philox_counter(3, (uint64_t{1} << 32) + 5, c);
        expect("round 2^32 + 5 is counter words (5, 1)", c[0] == 3 && c[1] == 0 && c[2] == 5 && c[3] == 1);
    }
    {
        // the stream of seed 0, round 0 starts with the first known answer; the third one through block, round and seed
        uint32_t x[4];
        philox_block(0, 0, 0, x);
        expect_words("the stream's first block", x, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u);
        philox_block(0x299f31d0a4093822ull, 0x0370734413198a2eull, 0x85a308d3243f6a88ull, x);
        expect_words("digits of pi through the stream", x, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u);
        uint32_t y[4], c[4] = {0, 1, 0, 0};
        philox_block(0, 0, uint64_t{1} << 32, y);
        philox4x32_10(c, 0, 0);
        expect("block 2^32 uses counter word 1", std::memcmp(y, c, sizeof(c)) == 0);
        uint32_t r[4], cr[4] = {0, 0, 7, 0};
        philox_block(0, 7, 0, r);
        philox4x32_10(cr, 0, 0);
        expect("the round is counter word 2", std::memcmp(r, cr, sizeof(cr)) == 0);
    }
    // the normals: the extreme words stay finite and inside sqrt(66 log 2)
    {
        const uint32_t lowest[4] = {0, 0, 0, 0xffffffffu}, highest[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0};
        double z[4];
        philox_normals(lowest, z);
        expect("u1 = 2^-33 gives the largest radius", z[0] > 6.76 && z[0] < 6.77 && z[0] == z[0] && z[1] > 0.0 && z[1] < 1e-8);
        philox_normals(highest, z);
        expect("u1 next to 1 gives the smallest radius", z[0] > 0.0 && z[0] < 2e-5 && z[1] < 0.0 && z[1] > -2e-14);
    }
    if (failures != 0) return 1;
    std::printf("philox ok\n");
    for (uint64_t b = 0; b < 2; ++b) {
        uint32_t x[4];
        double z[4];
        philox_block(12345, 7, b, x);
        philox_normals(x, z);
        for (int i = 0; i < 4; ++i) {
            uint64_t u;
            std::memcpy(&u, &z[i], sizeof(u));
            std::printf("%016" PRIx64 " ", u);
        }
    }
    std::printf("\n");
    return 0;
}
