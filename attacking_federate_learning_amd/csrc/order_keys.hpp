// The order-preserving integer keys of floats, the reference's visit order and the flag compaction: what every kernel that sorts,
// ranks or selects builds on, written once.  Where NaN and -0.0 fall in a key order is what the selections' bit-for-bit
// agreement with the reference rests on, so it is decided here and nowhere else.
//
// Two maps, and who needs which:
//   plain   ordered_bits: monotone in the value, -0.0 strictly below +0.0, a NaN wherever its bits fall (positive NaNs above
//           +inf, negative NaNs below -inf), invertible (from_ordered_bits).  For the kernels that read VALUES back off the keys
//           or step through key space and settle NaN on their own: the row sorts (select.hip, large_rows.hip), the radix
//           selects (tall_select.hip, rank_select.hip), the window kernels' min / max and probes (window_lean.hip,
//           median_window.hip) and the small Krum argmin (krum_small.hip, which admits no NaN to its keys).
//           select.hip and large_rows.hip give a NaN distance the key 0xfffffffe, not 0xffffffff: all ones is the SELF entry
//           there, which has to sort behind everything, a NaN included.  rank_select.hip keeps a NaN key of its own likewise.
//   total   ordered_bits_total: every NaN of either sign -> all ones (strictly behind +inf), -0.0 folded onto +0.0, the plain map
//           otherwise.  For the kernels that RANK by key and never read a value back: Multi-Krum's scores (multi_krum.hip), NNM's
//           distances (nnm.hip), DnC's fp64 scores (dnc.hip).  Equal values must tie (and fall to the index in the key's low
//           half) and a NaN must lose to everything, as `<` on the values would have it; not invertible.
//           The fp64 total map is read back (value_of_total_key) by the two that sort doubles by value: FABA's removal key
//           (faba.hip, owner_loop.hpp; its sums are never a NaN and never -0.0, so the map is one to one there) and AFA's median
//           (afa.hip; the zeros' key gives +0.0).
// Everything but block_exclusive_scan also compiles for the host with a plain C++17 compiler (tests/order_keys_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define BYZ_KEY_FN __host__ __device__ __forceinline__
#else
#define BYZ_KEY_FN inline
#endif

namespace byz {

BYZ_KEY_FN uint32_t ordered_bits(float v) {
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
BYZ_KEY_FN float from_ordered_bits(uint32_t o) {
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

BYZ_KEY_FN uint32_t ordered_bits_total(float v) {
    if (v != v) return 0xffffffffu;                    // any NaN: behind +inf (0xff800000)
    return ordered_bits(v == 0.0f ? 0.0f : v);         // -0.0 == +0.0
}
BYZ_KEY_FN uint64_t ordered_bits_total(double v) {      // (no plain fp64 map to build on: FABA and AFA's median use this one)
    constexpr uint64_t kSign = uint64_t{1} << 63;
    if (v != v) return ~uint64_t{0};
    uint64_t b = __builtin_bit_cast(uint64_t, v);
    if (b == kSign) b = 0;
    return (b & kSign) ? ~b : (b | kSign);
}

// the fp64 total map read back: the NaN key gives a NaN, every other key its value (the zeros' key: +0.0)
BYZ_KEY_FN double value_of_total_key(uint64_t key) {
    constexpr uint64_t kSign = uint64_t{1} << 63;
    if (key == ~uint64_t{0}) return __builtin_nan("");
    return __builtin_bit_cast(double, (key & kSign) ? (key & ~kSign) : ~key);
}

// The median of the rows' norms, by key and sort (SignGuard's M, weak DP's adaptive clip).  norm_key: the key of sqrt(q) for a
// squared norm q; a row whose q is not finite gets all ones (kNoNormKey, the padding's key as well) and sorts behind every norm.
// median_of_norm_keys: np.median over the `finite` first keys of the ascending sort -- the middle value, or the mean of the two
// middle values (finite >= 1).
constexpr uint64_t kNoNormKey = ~uint64_t{0};
BYZ_KEY_FN uint64_t norm_key(double q) { return __builtin_isfinite(q) ? ordered_bits_total(sqrt(q)) : kNoNormKey; }
BYZ_KEY_FN double norm_of_key(uint64_t key) {           // ordered_bits_total's inverse on values >= +0.0
    return __builtin_bit_cast(double, key & ~(uint64_t{1} << 63));
}
template <typename Key>                                 // (Key: uint64_t or the device's unsigned long long)
BYZ_KEY_FN double median_of_norm_keys(const Key* sorted_keys, int64_t finite) {
    return (norm_of_key(sorted_keys[(finite - 1) / 2]) + norm_of_key(sorted_keys[finite / 2])) / 2.0;
}

// the exponent is not all ones
BYZ_KEY_FN bool finite_bits(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u; }
// the same, asked of a key of ordered_bits_total (whose only NaN key is all ones)
BYZ_KEY_FN bool ordered_is_finite(uint32_t o) {
    constexpr uint32_t kOrderedPosInf = 0xff800000u;   // ordered bits of +inf: every finite value is below
    constexpr uint32_t kOrderedNegInf = 0x007fffffu;   // ordered bits of -inf: the lowest key of the total map
    return o < kOrderedPosInf && o != kOrderedNegInf;
}

// The reference walks its clients in dict order 1, 0, 2, 3, ...: row u is visited at visit_position(u), and a tie goes to the
// lower position.  The order is an involution, so row_of_visit is the same swap; the two names say which way a call site reads.
BYZ_KEY_FN int visit_position(int u) { return u == 0 ? 1 : (u == 1 ? 0 : u); }
BYZ_KEY_FN int row_of_visit(int position) { return visit_position(position); }

#ifdef __HIPCC__
// Flag compaction's scan over one workgroup of THREADS threads: `mine` is what this thread's rows contribute, the return value
// is the sum over the threads before it -- its first output slot -- and *total (optional) the sum over all.  An inclusive
// Hillis-Steele scan in lds (THREADS ints, free for reuse after the caller's next barrier), log2(THREADS) steps, every thread
// of the workgroup must call.
template <int THREADS>
__device__ __forceinline__ int block_exclusive_scan(int mine, int* lds, int* total) {
    const int tid = threadIdx.x;
    lds[tid] = mine;
    __syncthreads();
    for (int step = 1; step < THREADS; step <<= 1) {
        const int add = tid >= step ? lds[tid - step] : 0;
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    if (total != nullptr) *total = lds[THREADS - 1];
    return lds[tid] - mine;
}
#endif

}  // namespace byz

#undef BYZ_KEY_FN
