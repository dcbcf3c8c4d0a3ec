// s-bucketing (Karimireddy, He and Jaggi, "Byzantine-Robust Learning on Heterogeneous Datasets via Bucketing", ICLR 2022; beyond
// the reference): a PRE-aggregation.  The clients are shuffled and every s consecutive ones replaced by their mean; the
// B = ceil(n / s) bucket means are what Krum, the median, the geometric median or centered clipping then see.  An HBM-bound
// streaming kernel, like column_stats.hip's.
//
//   Y[b][c] = ( G[perm[b s]][c] + G[perm[b s + 1]][c] + ... ) / float(c_b)        c_b = min(s, n - b s) rows, in list order
//
// The sum is column_sequential_kernel's chain (sequential fp32 from +0.0, then a true division), so Y[b] is
// np.mean(G[perm[b s : (b + 1) s]], axis=0) bit for bit and s = n with the identity is no_defense's vector.
// One thread owns VEC columns and walks the rows of its buckets in list order (walk_rows, row_walk.hpp).  The walk does not
// stop at a bucket's end: the rows of ALL the thread's buckets are one walk, so that a run of eight loads is in flight whatever
// s is (with one walk per bucket, s = 2 -- the paper's choice -- would never fill a run), and the bucket that has ended is
// divided and stored from inside the walk.  Every element of Y is still one chain, whatever the grid.
// This file is compiled with -ffp-contract=off, as column_stats.hip is (the chain has no multiply today; the flag keeps it so).
// Algorithmic traffic: 4*rows*cols bytes read + 4*buckets*cols written.  No LDS, no atomics.
#include "row_walk.hpp"

#include <algorithm>

namespace byz {
namespace {

constexpr int kThreads = kWalkThreads;

// The buckets b_lo .. b_hi - 1 of the thread that owns columns c0 .. c0 + VEC - 1.  LISTED: the rows come from perm, whose
// entries are the same for every lane and arrive through scalar loads (a run's eight in one load, as in
// column_sequential_kernel's MODE 2); an entry outside [0, n_rows) is rejected by `take`, which means that it is never used
// as a row number, and the bucket's divisor stays c_b.
template <int VEC, bool LISTED>
__device__ __forceinline__ void bucket_walk(const float* __restrict__ G, int64_t n_rows, int64_t n_cols, int64_t ld,
                                            const int32_t* __restrict__ perm, int64_t s, float* __restrict__ Y, int64_t ldy,
                                            int64_t c0, int64_t b_lo, int64_t b_hi) {
    const int64_t first = b_lo * s;                                 // the walk's step r reads list entry first + r
    const int64_t steps = (b_hi * s < n_rows ? b_hi * s : n_rows) - first;
    float sum[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) sum[v] = 0.0f;
    int64_t cur = b_lo;         // the bucket the chain is in
    int64_t end = s;            // the step at which it ends
    // bucket `cur` is complete (no row at all, if every entry of it was rejected: +0.0 / c_b): divide, store, start the next
    auto flush = [&]() __attribute__((always_inline)) {
        const int64_t left = n_rows - cur * s;
        const float len_f = static_cast<float>(left < s ? left : s);       // c_b: the last bucket may be short
        float* y = Y + cur * ldy + c0;
        float q[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            q[v] = sum[v] / len_f;
            sum[v] = 0.0f;
        }
        if constexpr (VEC == 4) {
            if (c0 + VEC <= n_cols) {
                *reinterpret_cast<float4u*>(y) = float4u{q[0], q[1], q[2], q[3]};
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (c0 + v < n_cols) y[v] = q[v];
            }
        } else {
            y[0] = q[0];
        }
        ++cur;
        end += s;
    };
    walk_rows<VEC>(
        G + c0, ld, steps, c0, n_cols,
        [&](int64_t r) __attribute__((always_inline)) -> int64_t {
            if constexpr (LISTED) return perm[first + r];
            else return first + r;
        },
        [&](int64_t r) __attribute__((always_inline)) -> bool {
            if constexpr (LISTED) return static_cast<uint32_t>(perm[first + r]) < static_cast<uint32_t>(n_rows);
            else return true;
        },
        [&](int64_t r, bool, const float(&x)[VEC]) __attribute__((always_inline)) {
            while (r >= end) flush();       // (r is the same for every lane: a scalar test)
#pragma unroll
            for (int v = 0; v < VEC; ++v) sum[v] = sum[v] + x[v];       // (a masked column of the last vector reads +0.0)
        });
    while (cur < b_hi) flush();
}

// Y: n_buckets x n_cols, leading dimension ldy.  blockIdx.y takes per_y consecutive buckets (the launcher leaves no y without
// one): where the columns alone do not fill the chip the buckets do.
template <int VEC>
__global__ __launch_bounds__(kThreads) void bucket_means_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols,
                                                                int64_t ld, const int32_t* __restrict__ perm, int64_t s,
                                                                int64_t n_buckets, int64_t per_y, float* __restrict__ Y,
                                                                int64_t ldy) {
    const int64_t c0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * VEC;
    if (c0 >= n_cols) return;
    const int64_t b_lo = static_cast<int64_t>(blockIdx.y) * per_y;
    const int64_t b_hi = b_lo + per_y < n_buckets ? b_lo + per_y : n_buckets;
    if (perm != nullptr) bucket_walk<VEC, true>(G, n_rows, n_cols, ld, perm, s, Y, ldy, c0, b_lo, b_hi);
    else bucket_walk<VEC, false>(G, n_rows, n_cols, ld, nullptr, s, Y, ldy, c0, b_lo, b_hi);
}

}  // namespace

// perm == nullptr: the identity.  1 <= s <= n_rows <= kLargeMaxRows, ldy >= n_cols and Y clear of G are the caller's business.
int launch_bucket_means(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* perm, int64_t s,
                        float* Y, int64_t ldy, hipStream_t stream) {
    BYZ_REQUIRE(G && Y && n_rows > 0 && n_cols > 0 && ld >= n_cols && ldy >= n_cols, "bucket means: bad shape %lld x %lld ld %lld ldy %lld",
                (long long)n_rows, (long long)n_cols, (long long)ld, (long long)ldy);
    BYZ_REQUIRE(s >= 1 && s <= n_rows && n_rows <= kLargeMaxRows, "bucket means: s = %lld outside 1..%lld", (long long)s,
                (long long)n_rows);
    WalkShape shape;
    BYZ_TRY(walk_shape(ctx, G, ld, n_cols, "bucket means", &shape));
    const int64_t n_buckets = ceil_div(n_rows, s);
    // eight workgroups of four waves fill a CU; the y dimension of a grid ends at 65,535
    int64_t want_y = shape.vec4 ? 1 : ceil_div(static_cast<int64_t>(ctx->num_cus) * 8, shape.blocks);
    want_y = std::max<int64_t>(1, std::min<int64_t>({want_y, n_buckets, 65535}));
    const int64_t per_y = ceil_div(n_buckets, want_y);
    const dim3 grid(static_cast<unsigned>(shape.blocks), static_cast<unsigned>(ceil_div(n_buckets, per_y)));
    KernelTimer t(ctx, BYZ_K_COLUMN_STATS, stream);
    if (shape.vec4) bucket_means_kernel<4><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, perm, s, n_buckets, per_y, Y, ldy);
    else bucket_means_kernel<1><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, perm, s, n_buckets, per_y, Y, ldy);
    return check_launch("bucket_means_kernel");
}

}  // namespace byz
