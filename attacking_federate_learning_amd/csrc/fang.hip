// The attacks of Fang, Cao, Jia and Gong, "Local Model Poisoning Attacks to Byzantine-Robust Federated Learning" (USENIX Security
// 2020): the trimmed-mean / median attack of section 4.3 with full and with partial knowledge, and the Krum attack of section 4.2;
// beyond the reference.  G is n x d, rows 0 .. c - 1 are the attacker's, rows c .. n - 1 benign.  The paper works on local MODELS; a
// gradient g moves the model by -lr g, so its "changing direction" s_j = -1 is a column mean above 0 here and its "above the largest
// benign model" is "below the smallest benign gradient".  The rules below are the paper's on G as it lies.
//
// Trimmed mean, full knowledge, per column j (column_extremes_kernel, then fang_fill_kernel<., false>):
//     mean_j = np.mean(G[:, j]) over ALL rows      no_defense's bits: the sequential fp32 chain from +0.0 in row order, / float(n)
//     lo_j, hi_j = np.fmin.reduce, np.fmax.reduce over the BENIGN rows: acc = (acc <= x || isnan(x)) ? acc : x from NaN on (>= for
//                  hi): a NaN is skipped, a column with no benign number gives NaN.  (Of zeros of both signs the first stays;
//                  numpy's vector loops may keep either.)
//     mean_j > 0:  the attackers draw from [lo / b, lo] when lo > 0, else from [b lo, lo]
//     otherwise (<= 0, -0.0, NaN): from [hi, b hi] when hi > 0, else from [hi, hi / b]      (every interval away from the benign values)
//   The ends A <= B are fp64, formed from the fp32 extreme e by one fp64 product or quotient.
// Trimmed mean, partial knowledge (fang_fill_kernel<., true>): mu, sigma = the attacker rows' np.mean and np.var ** 0.5 (the drift
//   attack's statistics, bit for bit); mu > 0: [mu - k_hi sigma, mu - k_lo sigma], otherwise [mu + k_lo sigma, mu + k_hi sigma], the
//   ends (double)mu -+ k * (double)sigma with the product rounded first.  One attacker has sigma = 0: the value is the end itself.
// The draw (philox.hpp: philox_uniform): value = fl32(A + u (B - A)), u = (word + 0.5) 2^-32; an end that is not finite gives the
//   extreme itself (e, or the k_lo end).  The word of (attacker row i, global column j) is word j & 3 of
//   philox_block(seed, round | (uint64_t)i << 32, j >> 2): `round` has 32 bits, the row sits in the counter's top word, key and block
//   layout are the noise's.  Every attacker row draws independently (the paper's "sample c numbers"); one call, a misaligned caller
//   and any split of the columns over ranks draw the same bits.
// Krum, full knowledge: s_j = +1 where mean_j > 0, else -1 (sign_vector_kernel); every attacker row becomes the ONE vector
//   -lambda s -- the paper's other c - 1 rows "within epsilon of the first" are copies of it here, as in every public implementation.
//   With t_i = g_i . s and q_i = |g_i|^2 (row_dots, fp64) the squared distance from benign i to -lambda s is
//   q_i + 2 lambda t_i + lambda^2 d: fang_krum_fill_kernel rewrites the attacker's c rows and columns of the n x n distance matrix
//   for a lambda without touching G, and the benign block is computed once.  fang_krum_bound_kernel gives the two reductions of
//   Theorem 1's upper bound lambda_0 (fang_lambda0 below).
// This file is compiled with -ffp-contract=off: every product above is rounded before it is added.
#include "philox.hpp"
#include "row_walk.hpp"

#include <cmath>

namespace byz {
namespace {

constexpr int kThreads = kWalkThreads;
constexpr int kBlocksPerCu = 8;          // the fill's grid: 32 waves a CU, sized from the chip

typedef float float4a __attribute__((ext_vector_type(4)));       // naturally (16-byte) aligned: the VEC = 4 path proved it

// One walk over all n rows: the sum chain of every row, the extremes of the rows >= first_benign.  The row number is uniform, so
// the two tests on it are scalar branches round the run's adds.
template <int VEC>
__global__ __launch_bounds__(kThreads) void column_extremes_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols,
                                                                   int64_t ld, int64_t first_benign, float* __restrict__ mean_out,
                                                                   float* __restrict__ lo_out, float* __restrict__ hi_out) {
    const int64_t c0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * VEC;
    if (c0 >= n_cols) return;
    float s[VEC], lo[VEC], hi[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        s[v] = 0.0f;
        lo[v] = hi[v] = __builtin_nanf("");
    }
    walk_rows<VEC>(
        G + c0, ld, n_rows, c0, n_cols, [](int64_t r) __attribute__((always_inline)) { return r; },
        [](int64_t) __attribute__((always_inline)) { return true; },
        [&](int64_t r, bool, const float(&x)[VEC]) __attribute__((always_inline)) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) s[v] = s[v] + x[v];
            // (selects, not branches on r: a branch round the run's adds makes the compiler carry the run's values as one
            // register tuple, row_walk.hpp says how that ends; an attacker row offers NaN, which the rule skips)
            const bool benign = r >= first_benign;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float y = benign ? x[v] : __builtin_nanf("");
                const bool skip = y != y;
                lo[v] = (lo[v] <= y || skip) ? lo[v] : y;
                hi[v] = (hi[v] >= y || skip) ? hi[v] : y;
            }
        });
    const float rows_f = static_cast<float>(n_rows);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        if (c0 + v >= n_cols) continue;
        if (mean_out) mean_out[c0 + v] = s[v] / rows_f;
        if (lo_out) lo_out[c0 + v] = lo[v];
        if (hi_out) hi_out[c0 + v] = hi[v];
    }
}

// One thread owns one Philox block of four consecutive GLOBAL columns, cut to the caller's [offset, offset + n_cols), and loops
// the attacker rows: the column vectors are read and the intervals formed once, every row costs one generator call and four
// draws.  A whole block is one 16-byte store when every row's first whole block is 16-byte aligned (VEC = 4); the head and tail
// blocks, and every block of the scalar instantiation, are predicated per column and never touch anything outside the row.
template <int VEC, bool PARTIAL>
__global__ __launch_bounds__(kThreads) void fang_fill_kernel(float* __restrict__ G, int64_t n_attackers, int64_t n_cols, int64_t ld,
                                                             FangDraw a, const float* __restrict__ va, const float* __restrict__ vb,
                                                             const float* __restrict__ vc) {
    const int64_t head = a.offset & 3;                                   // columns of the first block in front of the caller's
    const uint64_t b0 = static_cast<uint64_t>(a.offset) >> 2;
    const int64_t n_blocks = (head + n_cols + 3) >> 2;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; j < n_blocks; j += stride) {
        const int64_t c0 = 4 * j - head;                                 // the caller's column of the block's word 0 (< 0: the head)
        const bool whole = c0 >= 0 && c0 + 4 <= n_cols;
        double A[4], B[4];
        float ext[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = c0 + i >= 0 && c0 + i < n_cols;
            A[i] = B[i] = 0.0;
            ext[i] = 0.0f;
            if (!in) continue;
            if constexpr (PARTIAL) {
                const double mu = static_cast<double>(va[c0 + i]), sigma = static_cast<double>(vb[c0 + i]);
                const double near = a.k_lo * sigma, far = a.k_hi * sigma;
                if (va[c0 + i] > 0.0f) {
                    A[i] = mu - far;
                    B[i] = mu - near;
                    ext[i] = static_cast<float>(B[i]);
                } else {
                    A[i] = mu + near;
                    B[i] = mu + far;
                    ext[i] = static_cast<float>(A[i]);
                }
            } else {
                if (va[c0 + i] > 0.0f) {
                    const float e = vb[c0 + i];
                    ext[i] = e;
                    A[i] = e > 0.0f ? static_cast<double>(e) / a.b : a.b * static_cast<double>(e);
                    B[i] = static_cast<double>(e);
                } else {
                    const float e = vc[c0 + i];
                    ext[i] = e;
                    A[i] = static_cast<double>(e);
                    B[i] = e > 0.0f ? a.b * static_cast<double>(e) : static_cast<double>(e) / a.b;
                }
            }
        }
        for (int64_t r = 0; r < n_attackers; ++r) {
            uint32_t w[4];
            philox_block(a.seed, a.round | (static_cast<uint64_t>(r) << 32), b0 + static_cast<uint64_t>(j), w);
            float y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = philox_uniform(w[i], A[i], B[i], ext[i]);
            float* row = G + r * ld;
            if (VEC == 4 && whole) {
                float4a q;
                q.x = y[0]; q.y = y[1]; q.z = y[2]; q.w = y[3];
                *reinterpret_cast<float4a*>(row + c0) = q;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (c0 + i >= 0 && c0 + i < n_cols) row[c0 + i] = y[i];
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void sign_vector_kernel(const float* __restrict__ mean, int64_t n_cols, float positive,
                                                               float otherwise, float* __restrict__ out) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (j < n_cols) out[j] = mean[j] > 0.0f ? positive : otherwise;
}

// One thread per benign row: the first of the row's largest off-diagonal entries, then the fp64 sum of the others in column order.
// The minimum over the rows and the maximum of q are order-free: non-negative doubles compare as their bit patterns do, a NaN
// (either sign) lies above +inf, so bounds[0] is a number whenever one row's sum is and bounds[1] is not when any q is not.
__global__ __launch_bounds__(kThreads) void fang_krum_bound_kernel(const float* __restrict__ block, const double* __restrict__ q,
                                                                   int64_t m, unsigned long long* __restrict__ bounds) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= m) return;
    const float* row = block + i * m;
    int64_t top = -1;
    float best = 0.0f;
    for (int64_t j = 0; j < m; ++j) {
        if (j == i) continue;
        const float v = row[j];
        if (top < 0 || v > best) {
            top = j;
            best = v;
        }
    }
    double sum = 0.0;
    for (int64_t j = 0; j < m; ++j)
        if (j != i && j != top) sum = sum + static_cast<double>(row[j]);
    atomicMin(bounds, static_cast<unsigned long long>(__double_as_longlong(sum)));
    atomicMax(bounds + 1, static_cast<unsigned long long>(__double_as_longlong(q[i])));
}

// Thread (x: row i of the matrix, y: a share of the attackers): entry (i, a) and its mirror (a, i).  i < c: 0, +inf on the diagonal.
__global__ __launch_bounds__(kThreads) void fang_krum_fill_kernel(float* __restrict__ dist, int64_t n, int64_t c, double cols_f,
                                                                  const double* __restrict__ q, const double* __restrict__ t,
                                                                  double lambda) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    float v = 0.0f;
    if (i >= c) {
        const double twice = 2.0 * lambda, cross = twice * t[i - c];
        const double square = lambda * lambda, shift = square * cols_f;
        const double sq = (q[i - c] + cross) + shift;
        v = static_cast<float>(sqrt(sq > 0.0 ? sq : 0.0));
    }
    for (int64_t a = blockIdx.y; a < c; a += gridDim.y) {
        const float e = i == a ? __builtin_inff() : v;
        dist[i * n + a] = e;
        dist[a * n + i] = e;
    }
}

}  // namespace

int launch_column_extremes(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t first_benign, float* mean,
                           float* lo, float* hi, hipStream_t stream) {
    BYZ_REQUIRE(G && n_rows > 0 && n_cols > 0 && ld >= n_cols && first_benign >= 0 && first_benign <= n_rows,
                "column extremes: bad shape %lld x %lld ld %lld, %lld attacker rows", (long long)n_rows, (long long)n_cols, (long long)ld,
                (long long)first_benign);
    WalkShape shape;
    BYZ_TRY(walk_shape(ctx, G, ld, n_cols, "column extremes", &shape));
    const unsigned blocks = static_cast<unsigned>(shape.blocks);
    KernelTimer timer(ctx, BYZ_K_COLUMN_STATS, stream);
    if (shape.vec4) column_extremes_kernel<4><<<blocks, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, first_benign, mean, lo, hi);
    else column_extremes_kernel<1><<<blocks, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, first_benign, mean, lo, hi);
    return check_launch("column_extremes_kernel");
}

// 1 <= n_attackers, 1 <= n_cols <= ld, 0 <= offset, offset + n_cols <= 2^62, round < 2^32 are the caller's business (api.hip)
int launch_fang_fill(byz_ctx* ctx, float* G, int64_t n_attackers, int64_t n_cols, int64_t ld, const FangDraw& draw, bool partial,
                     const float* a, const float* b, const float* c, hipStream_t stream) {
    const int64_t first_whole = (4 - (draw.offset & 3)) & 3;      // the caller's column at which the first whole block starts
    const bool vec4 = ld % 4 == 0 && aligned16(G + first_whole);
    const int64_t n_blocks = ((draw.offset & 3) + n_cols + 3) >> 2;
    const int64_t want = ceil_div(n_blocks, kThreads), most = static_cast<int64_t>(kBlocksPerCu) * ctx->num_cus;
    const unsigned grid = static_cast<unsigned>(want < most ? want : most);
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    if (partial) {
        if (vec4) fang_fill_kernel<4, true><<<grid, kThreads, 0, stream>>>(G, n_attackers, n_cols, ld, draw, a, b, c);
        else fang_fill_kernel<1, true><<<grid, kThreads, 0, stream>>>(G, n_attackers, n_cols, ld, draw, a, b, c);
    } else {
        if (vec4) fang_fill_kernel<4, false><<<grid, kThreads, 0, stream>>>(G, n_attackers, n_cols, ld, draw, a, b, c);
        else fang_fill_kernel<1, false><<<grid, kThreads, 0, stream>>>(G, n_attackers, n_cols, ld, draw, a, b, c);
    }
    return check_launch("fang_fill_kernel");
}

int launch_sign_vector(byz_ctx* ctx, const float* mean, int64_t n_cols, float positive, float otherwise, float* out, hipStream_t stream) {
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    sign_vector_kernel<<<static_cast<unsigned>(ceil_div(n_cols, kThreads)), kThreads, 0, stream>>>(mean, n_cols, positive, otherwise, out);
    return check_launch("sign_vector_kernel");
}

int launch_fang_krum_bound(byz_ctx* ctx, const float* block, const double* q, int64_t m, unsigned long long* bounds, hipStream_t stream) {
    BYZ_HIP(hipMemsetAsync(bounds, 0xff, sizeof(unsigned long long), stream));
    BYZ_HIP(hipMemsetAsync(bounds + 1, 0, sizeof(unsigned long long), stream));
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    fang_krum_bound_kernel<<<static_cast<unsigned>(ceil_div(m, kThreads)), kThreads, 0, stream>>>(block, q, m, bounds);
    return check_launch("fang_krum_bound_kernel");
}

// Theorem 1 with w_Re the zero gradient: min_i S_i / ((n - 2c - 1) sqrt(d)) + max_i |g_i| / sqrt(d), every operation in fp64
double fang_lambda0(double s_min, double q_max, int64_t n, int64_t c, int64_t n_cols) {
    const double root_d = std::sqrt(static_cast<double>(n_cols));
    const double spread = s_min / (static_cast<double>(n - 2 * c - 1) * root_d);
    const double reach = std::sqrt(q_max) / root_d;
    return spread + reach;
}

int launch_fang_krum_fill(byz_ctx* ctx, float* dist, int64_t n, int64_t c, int64_t n_cols, const double* q, const double* t,
                          double lambda, hipStream_t stream) {
    const unsigned blocks = static_cast<unsigned>(ceil_div(n, kThreads));
    int64_t share = ceil_div(static_cast<int64_t>(ctx->num_cus) * 4, blocks);
    if (share > c) share = c;
    if (share > 65535) share = 65535;
    KernelTimer timer(ctx, BYZ_K_DISTANCES, stream);
    fang_krum_fill_kernel<<<dim3(blocks, static_cast<unsigned>(share)), kThreads, 0, stream>>>(dist, n, c, static_cast<double>(n_cols), q, t,
                                                                                           lambda);
    return check_launch("fang_krum_fill_kernel");
}

}  // namespace byz
