// The streaming row walk that the column kernels share, and the small device helpers around it.
//
// One thread owns VEC consecutive columns and walks down the rows; a wave then reads 64 (or 256, with dwordx4) consecutive
// columns of a row in one coalesced request.  The rows go in runs of kRowRun: a run's loads are issued together, the additions
// follow in row order.  That order (with -ffp-contract=off in the files that include this) is what makes the outputs numpy's
// bits, so it is written once, here: column_sequential_kernel and column_chain_kernel (column_stats.hip) and
// weighted_rows_kernel (geomed.hip: the weighted mean, centered clipping's update and FLTrust's sum) are walk_rows with different `add`s.
#pragma once

#include "common.hpp"
#include "lane_exchange.hpp"

namespace byz {

constexpr int kWalkThreads = 256;       // threads of a workgroup of every kernel built on walk_rows

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// The launch shape of a walk over n_cols columns: 16-byte loads (VEC = 4) when every row starts 16-byte aligned and the
// columns alone fill the chip; one column per thread otherwise (few columns: four times the threads).
struct WalkShape {
    bool vec4;
    int64_t blocks;     // workgroups of kWalkThreads threads
};
inline int walk_shape(byz_ctx* ctx, const float* G, int64_t ld, int64_t n_cols, const char* who, WalkShape* out) {
    out->vec4 = (ld % 4 == 0) && aligned16(G) && n_cols >= static_cast<int64_t>(4) * kWalkThreads * ctx->num_cus * 2;
    out->blocks = ceil_div(n_cols, static_cast<int64_t>(kWalkThreads) * (out->vec4 ? 4 : 1));
    if (out->blocks >= (int64_t{1} << 31)) {
        set_error("%s: %lld columns is beyond one launch", who, (long long)n_cols);
        return BYZ_E_UNSUPPORTED;
    }
    return BYZ_OK;
}

// the VEC columns at p (column c0 of a row of n_cols): dwordx4 when whole (`full`), masked otherwise
template <int VEC>
__device__ __forceinline__ void load_columns(const float* __restrict__ p, bool full, int64_t c0, int64_t n_cols, float (&x)[VEC]) {
    if constexpr (VEC == 4) {
        if (full) {
            const float4u q = *reinterpret_cast<const float4u*>(p);
            x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) x[v] = (c0 + v < n_cols) ? p[v] : 0.0f;
        }
    } else {
        x[0] = p[0];
    }
}

// The walk of the thread that owns columns c0 .. c0 + VEC - 1; p is its address in row 0 (G + c0).  row_of(r): the matrix row
// that step r of the walk reads (r itself, or a row list's entry).  take(r): a weight, a scale, or `true`; a row whose value
// is zero is neither loaded nor added.  Both are the same for every lane and arrive through scalar loads.  add(r, take's
// value, x): the row's columns, called in row order.
// Per run: the run's take values and row numbers first (a row list's eight entries are one s_load_dwordx8), then its loads
// back to back with nothing but address arithmetic between them, then its adds.
template <int VEC, int kRowRun = 8, typename RowOf, typename Take, typename Add>
__device__ __forceinline__ void walk_rows(const float* p, int64_t ld, int64_t n_rows, int64_t c0, int64_t n_cols, RowOf row_of,
                                          Take take, Add add) {
    using T = decltype(take(int64_t{0}));
    const bool full = c0 + VEC <= n_cols;
    int64_t r = 0;
    for (; r + kRowRun <= n_rows; r += kRowRun) {
        T t[kRowRun];
#pragma unroll
        for (int u = 0; u < kRowRun; ++u) t[u] = take(r + u);
        int64_t row[kRowRun];
#pragma unroll
        for (int u = 0; u < kRowRun; ++u) row[u] = row_of(r + u);
        float x[kRowRun][VEC];
#pragma unroll
        for (int u = 0; u < kRowRun; ++u)
            if (t[u] != T{}) load_columns<VEC>(p + row[u] * ld, full, c0, n_cols, x[u]);
#pragma unroll
        for (int u = 0; u < kRowRun; ++u)
            if (t[u] != T{}) {
                // (a copy: handed a reference into x, the compiler keeps the run's kRowRun x VEC values as one register tuple
                // and shuffles it through every branch on t: 54 -> 84 VGPRs in the four-wide weighted mean)
                float xu[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) xu[v] = x[u][v];
                add(r + u, t[u], xu);
            }
    }
    for (; r < n_rows; ++r) {
        const T t = take(r);
        if (t != T{}) {
            float x[VEC];
            load_columns<VEC>(p + row_of(r) * ld, full, c0, n_cols, x);
            add(r, t, x);
        }
    }
}

// run unless *skip_if_set != 0; with run_if_set, only if *run_if_set != 0
__device__ __forceinline__ bool gated_out(const int32_t* skip_if_set, const int32_t* run_if_set) {
    if (skip_if_set != nullptr && __hip_atomic_load(skip_if_set, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return true;
    if (run_if_set != nullptr && __hip_atomic_load(run_if_set, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return true;
    return false;
}

// the column kernels' wave sum is lane_exchange.hpp's fixed butterfly (every lane gets the total), under its own name
using lanes::wave_sum_shfl;

// fixed-order tree over one workgroup of THREADS threads (lds: THREADS values); every thread gets the total
template <typename T, int THREADS>
__device__ T block_sum(T v, T* lds) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int step = THREADS / 2; step >= 1; step >>= 1) {
        if (tid < step) lds[tid] = lds[tid] + lds[tid + step];
        __syncthreads();
    }
    const T total = lds[0];
    __syncthreads();
    return total;
}

}  // namespace byz
