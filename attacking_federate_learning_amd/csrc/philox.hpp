// The library's random numbers on the device: a counter-based Philox4x32-10 stream (Salmon, Moraes, Dror and Shaw, "Parallel
// Random Numbers: As Easy as 1, 2, 3", SC'11) addressed by GLOBAL COLUMN, and the fp64 Box-Muller transform on top of it.
// Nothing here keeps a state: a word is a function of (seed, round, column), so one call, a misaligned caller and any split of
// the columns over ranks draw the same integers, and the normals differ only where two math libraries' fp64 log, sin and cos do.
//
//   key      (low word of seed, high word of seed)
//   counter  (low word of b, high word of b, low word of round, high word of round),   b = column >> 2
//   word i (0..3) of block b belongs to column 4 b + i
//   normals  one Box-Muller pair per two words, all in fp64: for pair p in {0, 1}
//              u1 = (x[2p] + 0.5) * 2^-32,  u2 = (x[2p+1] + 0.5) * 2^-32         both exact, both inside (0, 1)
//              r  = sqrt(-2 log(u1)),  t = fl64(6.283185307179586 * u2)          the constant's bits: 0x401921FB54442D18
//              z[4b + 2p] = r cos(t),  z[4b + 2p + 1] = r sin(t)                 cos and sin of t itself, not cospi / sinpi of 2 u2
// |z| <= sqrt(2 * 33 * log 2) = 6.77: u1 >= 2^-33, so no normal is infinite or NaN.
// Plain C++ integer arithmetic; compiles for the host with a plain C++17 compiler as well (tests/philox_check.cpp).  The files
// that include it are built with -ffp-contract=off: every product above is rounded before it is used.
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define BYZ_PHILOX_FN __host__ __device__ __forceinline__
#else
#define BYZ_PHILOX_FN inline
#endif

namespace byz {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;     // the round's multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;     // the key's increments (golden ratio, sqrt(3) - 1)

// Philox4x32-10: ten rounds on the counter c under the key k, the key bumped between them; the result replaces c
BYZ_PHILOX_FN void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = static_cast<uint64_t>(kPhiloxM0) * c[0];
        const uint64_t p1 = static_cast<uint64_t>(kPhiloxM1) * c[2];
        const uint32_t y0 = static_cast<uint32_t>(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t y2 = static_cast<uint32_t>(p0 >> 32) ^ c[3] ^ k1;
        c[0] = y0;
        c[1] = static_cast<uint32_t>(p1);
        c[2] = y2;
        c[3] = static_cast<uint32_t>(p0);
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
}

// the counter of block b in round `round`
BYZ_PHILOX_FN void philox_counter(uint64_t b, uint64_t round, uint32_t (&c)[4]) {
    c[0] = static_cast<uint32_t>(b);
    c[1] = static_cast<uint32_t>(b >> 32);
    c[2] = static_cast<uint32_t>(round);
    c[3] = static_cast<uint32_t>(round >> 32);
}

// the four words of block b: those of the global columns 4 b .. 4 b + 3
BYZ_PHILOX_FN void philox_block(uint64_t seed, uint64_t round, uint64_t b, uint32_t (&x)[4]) {
    philox_counter(b, round, x);
    philox4x32_10(x, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
}

// the four standard normals of a block's words
BYZ_PHILOX_FN void philox_normals(const uint32_t (&x)[4], double (&z)[4]) {
    constexpr double kTwoPi = 6.283185307179586;       // 0x401921FB54442D18
    constexpr double kUnit = 1.0 / 4294967296.0;       // 2^-32
    for (int p = 0; p < 2; ++p) {
        const double u1 = (static_cast<double>(x[2 * p]) + 0.5) * kUnit;
        const double u2 = (static_cast<double>(x[2 * p + 1]) + 0.5) * kUnit;
        const double r = sqrt(-2.0 * log(u1));
        const double t = kTwoPi * u2;
        z[2 * p] = r * cos(t);
        z[2 * p + 1] = r * sin(t);
    }
}

// One uniform draw from the interval [A, B] (A <= B, both fp64 formed from fp32 numbers) out of one word:
//     u = (word + 0.5) * 2^-32                 exact, inside (0, 1)
//     value = fl32(A + u * (B - A))            every operation rounded; rounding is monotone, so fl32(A) <= value <= fl32(B)
// An end that is not finite gives `otherwise` (the caller's extreme) and no arithmetic: no inf - inf, never a new NaN.
BYZ_PHILOX_FN float philox_uniform(uint32_t word, double A, double B, float otherwise) {
    constexpr double kUnit = 1.0 / 4294967296.0;       // 2^-32
    if (!(__builtin_isfinite(A) && __builtin_isfinite(B))) return otherwise;
    const double u = (static_cast<double>(word) + 0.5) * kUnit;
    const double w = B - A;
    const double step = u * w;
    return static_cast<float>(A + step);
}

}  // namespace byz

#undef BYZ_PHILOX_FN
