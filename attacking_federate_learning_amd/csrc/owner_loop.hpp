// The loops that ONE workgroup runs to the end (Prim in flame.hip, the linkage in linkage.hip, FABA's and AFA's removals): who
// owns which row, the exchange of the waves' results behind one barrier, and FABA's removal key.  DESIGN.md 3.4t states the
// scheme and its three orders; the kernels are compared bit for bit with restatements, so those orders are a contract.
//
//   ownership   kOwnerThreads threads, thread t owns the rows t + kOwnerThreads * s for s < kOwnerSlots, in registers under static
//               indices, and a mask of kOwnerSlots bits says which of them are live.  A row's owner and slot are its low and high bits.
//   lane fold   inside a wave: lanes::lanes_fold<32> (lane_exchange.hpp) for the integer keys, lanes::wave_sum_shfl for AFA's sums.
//   exchange    block_exchange: lane 0 of every wave writes buf[turn & 1][wave], ONE barrier, every lane reads the slot
//               lane & (WAVES - 1), the caller folds the waves' values (lanes_fold<WAVES / 2>, or AFA's 8, 4, 2, 1 sum), ++turn.
//               A call's reads are behind the next call's barrier before the call after that writes the buffer again.
// The ownership and the removal key also compile for the host with a plain C++17 compiler (tests/owner_loop_check.cpp).
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define BYZ_OWNER_FN __host__ __device__ __forceinline__
#else
#define BYZ_OWNER_FN inline
#endif

namespace byz {

// ---- ownership ----------------------------------------------------------------------------------
constexpr int kOwnerThreads = 1024;
constexpr int kOwnerSlots = 16;
constexpr int kOwnerWaves = kOwnerThreads / 64;
constexpr int kOwnerShift = 10;                // a row's slot is what is left above its owner's bits
constexpr int kOwnerIndexBits = 14;            // a row, and a count of rows, is below 2^14
constexpr int64_t kOwnerMaxRows = int64_t{kOwnerThreads} * kOwnerSlots;
static_assert((1 << kOwnerShift) == kOwnerThreads && (int64_t{1} << kOwnerIndexBits) == kOwnerMaxRows && kOwnerMaxRows == 16384 &&
                  kOwnerSlots <= 32 && kOwnerWaves == 16, "every row has one owner, and the owner's mask a bit for it");

BYZ_OWNER_FN int row_of(int thread, int slot) { return thread + kOwnerThreads * slot; }
BYZ_OWNER_FN int owner_thread(int row) { return row & (kOwnerThreads - 1); }
BYZ_OWNER_FN int slot_of(int row) { return row >> kOwnerShift; }

// ---- FABA's removal key -------------------------------------------------------------------------
// Larger is removed first: bad (14 bits), the total key of s (64 bits, order_keys.hpp), the row counted down (14), in 96 bits:
// hi = bad << 50 | key >> 14, lo = (key & 0x3fff) << 14 | (16383 - row).  The key of an s >= +0.0 has its top bit set, so no row's
// key is {0, 0}: that is "nobody".
struct RemovalKey {
    unsigned long long hi;
    uint32_t lo;
};
BYZ_OWNER_FN RemovalKey removal_key(int bad, uint64_t s_key, int row) {
    constexpr int kLast = static_cast<int>(kOwnerMaxRows) - 1;
    const unsigned long long b = static_cast<unsigned long long>(bad < 0 ? 0 : (bad > kLast ? kLast : bad));
    return RemovalKey{(b << 50) | (s_key >> kOwnerIndexBits),
                      (static_cast<uint32_t>(s_key & kLast) << kOwnerIndexBits) | static_cast<uint32_t>(kLast - row)};
}
BYZ_OWNER_FN int removal_bad(unsigned long long hi) { return static_cast<int>(hi >> 50); }
BYZ_OWNER_FN int removal_row(uint32_t lo) { return static_cast<int>(kOwnerMaxRows) - 1 - static_cast<int>(lo & (kOwnerMaxRows - 1)); }
BYZ_OWNER_FN uint64_t removal_s_key(unsigned long long hi, uint32_t lo) {
    return ((hi & ((1ull << 50) - 1)) << kOwnerIndexBits) | (lo >> kOwnerIndexBits);
}
BYZ_OWNER_FN bool removal_less(const RemovalKey& a, const RemovalKey& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

#ifdef __HIPCC__
// the key's fields for lanes::lane_xor and lanes::lanes_fold (lane_exchange.hpp, which the kernel files include themselves)
template <typename X>
__device__ __forceinline__ RemovalKey each_field(const RemovalKey& k, X x) { return {x(k.hi), x(k.lo)}; }

// ---- the block exchange -------------------------------------------------------------------------
// The two buffers (in LDS); `mine` is the wave's value (lane 0's is published); `turn` counts the calls on `buf`, the same in
// every thread.
template <typename T, int WAVES = kOwnerWaves>
struct ExchangeBuf {
    T slot[2][WAVES];
};
template <int WAVES, typename T, typename Fold>
__device__ __forceinline__ T block_exchange(T mine, ExchangeBuf<T, WAVES>& buf, int& turn, int lane, int wave, Fold fold) {
    static_assert(WAVES == 16 || WAVES == 4, "a power of two: the slot a lane reads");
    const int which = turn & 1;
    ++turn;
    if (lane == 0) buf.slot[which][wave] = mine;
    __syncthreads();
    return fold(buf.slot[which][lane & (WAVES - 1)]);
}

#endif

}  // namespace byz

#undef BYZ_OWNER_FN
