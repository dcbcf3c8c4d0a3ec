// Cross-lane exchange primitives (one word, and through it any 4- or 8-byte value or small struct), the fold over the lanes that
// differ in the low bits (the one-workgroup loops' lane fold: owner_loop.hpp), the in-register bitonic network shared by the
// median-window kernels, the wave-wide reductions (sum, min, max) and the Krum / Bulyan ordering with its wave and block argmin.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

namespace byz {
namespace lanes {

// ---- cross-lane exchange ------------------------------------------------------------------------
// value held by lane (lane ^ MASK); MASK is a compile-time constant after unrolling.
__device__ __forceinline__ float lane_xor(float v, int mask, int lane) {
    const int b = __float_as_int(v);
    int r;
    switch (mask) {
        case 1: r = __builtin_amdgcn_update_dpp(0, b, 0xB1, 0xF, 0xF, true); break;   // quad_perm [1,0,3,2]
        case 2: r = __builtin_amdgcn_update_dpp(0, b, 0x4E, 0xF, 0xF, true); break;   // quad_perm [2,3,0,1]
        case 3: r = __builtin_amdgcn_update_dpp(0, b, 0x1B, 0xF, 0xF, true); break;   // quad_perm [3,2,1,0]
        case 7: r = __builtin_amdgcn_update_dpp(0, b, 0x141, 0xF, 0xF, true); break;  // row_half_mirror
        case 8: r = __builtin_amdgcn_update_dpp(0, b, 0x128, 0xF, 0xF, true); break;  // row_ror:8
        case 15: r = __builtin_amdgcn_update_dpp(0, b, 0x140, 0xF, 0xF, true); break; // row_mirror
        case 4:   // xor 4 inside a 16-lane row without the LDS pipe: banks 0, 2 take lane + 4, banks 1, 3 lane - 4
            r = __builtin_amdgcn_update_dpp(0, b, 0x104, 0xF, 0x5, false);             // row_shl:4
            r = __builtin_amdgcn_update_dpp(r, b, 0x114, 0xF, 0xA, false);             // row_shr:4
            break;
        case 16: r = __builtin_amdgcn_ds_swizzle(b, 0x401F); break;                    // xor 16
        case 31: r = __builtin_amdgcn_ds_swizzle(b, 0x7C1F); break;                    // xor 31
        default: r = __builtin_amdgcn_ds_bpermute((lane ^ mask) << 2, b); break;       // 32, 63
    }
    return __int_as_float(r);
}

__device__ __forceinline__ void cmp_swap(float& lo, float& hi) {
    const float a = lo, b = hi;
    lo = __builtin_fminf(a, b);
    hi = __builtin_fmaxf(a, b);
}

// compile-time loops over powers of two (a `k <<= 1` loop is not reliably unrolled, and a register
// array indexed by a runtime value would be demoted to scratch)
template <int K, int KMAX, typename F>
__device__ __forceinline__ void for_pow2_up(F&& f) {
    if constexpr (K <= KMAX) {
        f(std::integral_constant<int, K>{});
        for_pow2_up<K * 2, KMAX>(f);
    }
}
template <int J, typename F>
__device__ __forceinline__ void for_pow2_down(F&& f) {
    if constexpr (J > 0) {
        f(std::integral_constant<int, J>{});
        for_pow2_down<J / 2>(f);
    }
}

// The exchange above for any value: 4 bytes as they are, 8 bytes as two words, a struct field by field through its each_field
// (found by the struct's namespace).  Nothing but moves touches the bits.
template <int MASK, typename T>
__device__ __forceinline__ T lane_xor(T v, int lane) {
    if constexpr (std::is_class_v<T>) {
        return each_field(v, [lane](auto f) { return lane_xor<MASK>(f, lane); });
    } else if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, lane_xor(__builtin_bit_cast(float, v), MASK, lane));
    } else {
        static_assert(sizeof(T) == 8 && std::is_trivially_copyable_v<T>, "words of 4 or 8 bytes");
        const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
        const uint32_t lo = lane_xor<MASK>(static_cast<uint32_t>(b), lane), hi = lane_xor<MASK>(static_cast<uint32_t>(b >> 32), lane);
        return __builtin_bit_cast(T, (static_cast<unsigned long long>(hi) << 32) | lo);
    }
}
// v = op(v, the value of lane ^ m) for m = 1, 2, ..., TOP: the fold over the 2 * TOP lanes that differ in the low bits, and every
// one of them gets the result (op: a minimum or maximum under a total order, or any operator that gives both partners the same)
template <int TOP, typename T, typename Op>
__device__ __forceinline__ T lanes_fold(T v, int lane, Op op) {
    for_pow2_up<1, TOP>([&](auto mc) { v = op(v, lane_xor<decltype(mc)::value>(v, lane)); });
    return v;
}

// Sorts the 64*R values {x[r] of lane l} ascending in index i = r + R*l, for C independent columns.
template <int R, int C>
__device__ __forceinline__ void wave_bitonic_sort(float (&x)[C][R], int lane) {
    const float pinf = __builtin_inff();
    for_pow2_up<2, 64 * R>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        // flip: i <-> i ^ (k-1); the element whose bit (k/2) is clear keeps the minimum
        if constexpr (k <= R) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int p = r ^ (k - 1);
                if (p > r) {
#pragma unroll
                    for (int c = 0; c < C; ++c) cmp_swap(x[c][r], x[c][p]);
                }
            }
        } else {
            constexpr int lane_mask = k / R - 1;
            constexpr int lane_bit = k / (2 * R);
            const float sel = (lane & lane_bit) ? pinf : -pinf;  // upper partner keeps the maximum
#pragma unroll
            for (int r = 0; r < (R + 1) / 2; ++r) {
                const int p = R - 1 - r;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float from_p = lane_xor(x[c][p], lane_mask, lane);
                    if (p != r) {
                        const float from_r = lane_xor(x[c][r], lane_mask, lane);
                        x[c][p] = __builtin_amdgcn_fmed3f(x[c][p], from_r, sel);
                    }
                    x[c][r] = __builtin_amdgcn_fmed3f(x[c][r], from_p, sel);
                }
            }
        }
        // half-cleaners: i <-> i ^ j, j = k/4 ... 1
        for_pow2_down<k / 4>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if constexpr (j < R) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if ((r & j) == 0) {
#pragma unroll
                        for (int c = 0; c < C; ++c) cmp_swap(x[c][r], x[c][r | j]);
                    }
                }
            } else {
                constexpr int s = j / R;
                const float sel = (lane & s) ? pinf : -pinf;
#pragma unroll
                for (int r = 0; r < R; ++r) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float other = lane_xor(x[c][r], s, lane);
                        x[c][r] = __builtin_amdgcn_fmed3f(x[c][r], other, sel);
                    }
                }
            }
        });
    });
}

// Sorts a BITONIC sequence of 64*R values ascending (same index order i = r + R*l): log2(64 R) half-cleaner steps
// instead of the full network.  |x - median| over values sorted by x is such a sequence (it falls, then rises).
template <int R, int C>
__device__ __forceinline__ void wave_bitonic_merge(float (&x)[C][R], int lane) {
    const float pinf = __builtin_inff();
    for_pow2_down<32 * R>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if constexpr (j < R) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if ((r & j) == 0) {
#pragma unroll
                    for (int c = 0; c < C; ++c) cmp_swap(x[c][r], x[c][r | j]);
                }
            }
        } else {
            constexpr int s = j / R;
            const float sel = (lane & s) ? pinf : -pinf;
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float other = lane_xor(x[c][r], s, lane);
                    x[c][r] = __builtin_amdgcn_fmed3f(x[c][r], other, sel);
                }
            }
        }
    });
}

// ---- wave-wide reductions -----------------------------------------------------------------------
// Two exchange kinds, one reduction each, generic over the value (int, uint32_t, float, double, long long: 64-bit values
// travel as two 32-bit halves) and the operator:
//   _dpp   four DPP steps inside every 16-lane row (xor 1, xor 2, half mirror, mirror: each an involution, so every lane ends
//          up with its row's result), then the four rows' results through v_readlane, combined (r0 . r1) . (r2 . r3).  No LDS
//          pipe: a DPP move costs ~8 cycles of dependent latency where a ds_bpermute shuffle costs ~100.  Wave-uniform result.
//   _shfl  the __shfl_xor butterfly, masks 32, 16, ..., 1.  Every lane gets the result.
// Both orders are fixed; kernels whose outputs are compared bit for bit depend on them.
template <int CTRL, typename T>
__device__ __forceinline__ T dpp(T v) {
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
    } else {
        const long long b = __builtin_bit_cast(long long, v);
        const int lo = dpp<CTRL>(static_cast<int>(b)), hi = dpp<CTRL>(static_cast<int>(b >> 32));
        return __builtin_bit_cast(T, (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
    }
}
template <typename T>
__device__ __forceinline__ T readlane(T v, int l) {   // l is wave-uniform
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
    } else {
        const long long b = __builtin_bit_cast(long long, v);
        const int lo = readlane(static_cast<int>(b), l), hi = readlane(static_cast<int>(b >> 32), l);
        return __builtin_bit_cast(T, (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
    }
}

struct Sum {
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
    __device__ __forceinline__ float operator()(float a, float b) const { return __fadd_rn(a, b); }   // never contracted
};
struct Min {   // NaN-free inputs
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
    __device__ __forceinline__ float operator()(float a, float b) const { return __builtin_fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct Max {   // NaN-free inputs
    template <typename T>
    __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
    __device__ __forceinline__ float operator()(float a, float b) const { return __builtin_fmaxf(a, b); }
};

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce_dpp(T v, Op op) {
    v = op(v, dpp<0xB1>(v));    // quad_perm [1,0,3,2]
    v = op(v, dpp<0x4E>(v));    // quad_perm [2,3,0,1]
    v = op(v, dpp<0x141>(v));   // row_half_mirror
    v = op(v, dpp<0x140>(v));   // row_mirror
    return op(op(readlane(v, 0), readlane(v, 16)), op(readlane(v, 32), readlane(v, 48)));
}
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce_shfl(T v, Op op) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = op(v, __shfl_xor(v, m, 64));
    return v;
}
template <typename T> __device__ __forceinline__ T wave_sum_dpp(T v) { return wave_reduce_dpp(v, Sum{}); }
template <typename T> __device__ __forceinline__ T wave_min_dpp(T v) { return wave_reduce_dpp(v, Min{}); }
template <typename T> __device__ __forceinline__ T wave_max_dpp(T v) { return wave_reduce_dpp(v, Max{}); }
template <typename T> __device__ __forceinline__ T wave_sum_shfl(T v) { return wave_reduce_shfl(v, Sum{}); }
template <typename T> __device__ __forceinline__ T wave_min_shfl(T v) { return wave_reduce_shfl(v, Min{}); }
template <typename T> __device__ __forceinline__ T wave_max_shfl(T v) { return wave_reduce_shfl(v, Max{}); }

// ---- the Krum / Bulyan ordering and its argmin --------------------------------------------------
// A candidate is a score, its position in the reference's visit order (INT_MAX = none) and its row.
template <typename S>
struct Scored {
    S score;
    int pos;
    int row;
};
struct Candidate {
    double score;
    int pos;
    int row;
    int cls;   // the row's twin class where the caller needs it (the Bulyan loop), else 0: travels with the winner
};

// strict '<' on the score; an equal score keeps the earlier visitor
template <typename C>
__device__ __forceinline__ bool better(const C& a, const C& b) {
    return a.score < b.score || (a.score == b.score && a.pos < b.pos);
}

// the candidate whose every field went through the exchange x
template <typename S, typename X>
__device__ __forceinline__ Scored<S> each_field(const Scored<S>& c, X x) { return {x(c.score), x(c.pos), x(c.row)}; }
template <typename X>
__device__ __forceinline__ Candidate each_field(const Candidate& c, X x) { return {x(c.score), x(c.pos), x(c.row), x(c.cls)}; }

template <typename C>
__device__ __forceinline__ C wave_best_dpp(C c) {   // wave-uniform result
    const auto step = [&c](auto x) {
        const C o = each_field(c, x);
        if (better(o, c)) c = o;
    };
    step([](auto v) { return dpp<0xB1>(v); });
    step([](auto v) { return dpp<0x4E>(v); });
    step([](auto v) { return dpp<0x141>(v); });
    step([](auto v) { return dpp<0x140>(v); });
    C best = each_field(c, [](auto v) { return readlane(v, 0); });
#pragma unroll
    for (int l = 16; l < 64; l += 16) {
        const C o = each_field(c, [l](auto v) { return readlane(v, l); });
        if (better(o, best)) best = o;
    }
    return best;
}
template <typename C>
__device__ __forceinline__ C wave_best_shfl(C c) {   // every lane gets the result
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const C o = each_field(c, [m](auto v) { return __shfl_xor(v, m, 64); });
        if (better(o, c)) c = o;
    }
    return c;
}

// Block-wide best of the waves' bests, broadcast to every thread.  `slots` holds one candidate per wave: WAVES of them where
// the kernel fixes its workgroup size, blockDim.x / 64 otherwise.
template <int WAVES = 0, typename C>
__device__ __forceinline__ C block_best_of_waves(C c, C* slots) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = WAVES > 0 ? WAVES : blockDim.x >> 6;
    __syncthreads();  // slots may still be read from the previous call
    if (lane == 0) slots[wave] = c;
    __syncthreads();
    C best = slots[0];
    for (int w = 1; w < n_waves; ++w) {
        const C o = slots[w];
        if (better(o, best)) best = o;
    }
    return best;
}
template <int WAVES = 0, typename C>
__device__ __forceinline__ C block_best_dpp(C c, C* slots) { return block_best_of_waves<WAVES>(wave_best_dpp(c), slots); }
template <int WAVES = 0, typename C>
__device__ __forceinline__ C block_best_shfl(C c, C* slots) { return block_best_of_waves<WAVES>(wave_best_shfl(c), slots); }

}  // namespace lanes
}  // namespace byz
