// Multi-Metrics (Huang, Li, Wang, Chen, Zhang and Li, "Multi-metrics adaptively identifies backdoors in Federated Learning",
// ICCV 2023; beyond the reference): every client is described by its summed Manhattan, Euclidean and cosine distance to the
// others, the three features are whitened by their own covariance, and the clients with the smallest squared Mahalanobis norm
// are averaged.  The distance matrices come from manhattan.hip, gram.hip and flame.hip; here are the small kernels behind them
// (DESIGN.md 3.4n).  Everything is fp64 and every sum has a fixed order.
//
//   mm_usable_*_kernel    U, the usable rows: the Gram's g_ii finite and > 0 (the whole call: cosine_distances' notion), or, where
//                         only the matrices are known (byz_multi_metrics_features_dev), row i of the cosine matrix has a finite
//                         off-diagonal entry -- the same set whenever two rows are usable and their dot products finite.
//   mm_features_kernel    one workgroup a row: x_i = (sum m_ij, sum e_ij, sum c_ij) over j in U, j != i.  Thread t adds the entries
//                         j = t, t + 256, ... in ascending j, the 256 sums meet in block_sum's fixed tree.  A row outside U gets
//                         (inf, inf, inf).
//   mm_score_kernel       ONE workgroup.  U' = the rows whose three features are finite, u = |U'|.  The moments are taken about
//                         the first usable row's features y_i = x_i - x_first (the variance does not see the shift; a constant
//                         feature then has s EXACTLY 0): s_k = sqrt(sum (y_ik - mean y_k)^2 / (u - 1)), R_kl = (sum (y_ik - mean
//                         y_k)(y_il - mean y_l) / (u - 1)) / (s_k s_l), R^-1 = adj R / det R in closed form, score_i = z_i^T R^-1
//                         z_i with z_i = x_i / s (uncentred, as in the paper).  Degenerate -- u < 4, an s_k that is zero or not
//                         finite, det R not above 1e-12 -- score_i = x_i0, the Manhattan feature.  A row outside U' scores +inf.
//   mm_rank_kernel        rank_i = the usable rows before i in the order (ordered_bits_total(score) ascending, row ascending: a
//                         NaN is last, equal scores fall to the lower row), counted, not sorted: n^2 comparisons of keys staged
//                         through LDS.  flag_i = i usable and rank_i < min(u, keep).
//   mm_compact_kernel     the flagged rows ascending and their number (what the counted mean reads).
#include "order_keys.hpp"
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kFeatThreads = 256;
constexpr int kScoreThreads = 1024;
constexpr int kRankThreads = 256;
constexpr int kCompactSlots = 16;              // rows a thread of the compaction owns: kScoreThreads * kCompactSlots = kMmMaxRows
constexpr double kMmMinDet = 1e-12;
static_assert(kScoreThreads * kCompactSlots == kMmMaxRows, "every row has an owner");

__global__ __launch_bounds__(256) void mm_usable_from_gram_kernel(const double* __restrict__ gram, int64_t n, int32_t* __restrict__ usable) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const double g = gram[i * n + i];
    usable[i] = (__builtin_isfinite(g) && g > 0.0) ? 1 : 0;
}

__global__ __launch_bounds__(kFeatThreads) void mm_usable_from_cos_kernel(const float* __restrict__ cos, int n, int32_t* __restrict__ usable) {
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ row = cos + static_cast<int64_t>(i) * n;
    int finite = 0;
    for (int j = tid; j < n; j += kFeatThreads)
        if (j != i) finite |= finite_bits(row[j]) ? 1 : 0;
    finite = __syncthreads_or(finite);
    if (tid == 0) usable[i] = finite ? 1 : 0;
}

__global__ __launch_bounds__(kFeatThreads) void mm_features_kernel(const float* __restrict__ man, const float* __restrict__ euc,
                                                                   const float* __restrict__ cos, const int32_t* __restrict__ usable,
                                                                   int n, double* __restrict__ feat) {
    __shared__ double red[kFeatThreads];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int64_t base = static_cast<int64_t>(i) * n;
    double m = 0.0, e = 0.0, c = 0.0;
    for (int j = tid; j < n; j += kFeatThreads) {
        if (j == i || usable[j] == 0) continue;
        m = m + static_cast<double>(man[base + j]);
        e = e + static_cast<double>(euc[base + j]);
        c = c + static_cast<double>(cos[base + j]);
    }
    m = block_sum<double, kFeatThreads>(m, red);
    e = block_sum<double, kFeatThreads>(e, red);
    c = block_sum<double, kFeatThreads>(c, red);
    if (tid == 0) {
        const bool ok = usable[i] != 0;
        const double inf = __builtin_inf();
        feat[3 * static_cast<int64_t>(i) + 0] = ok ? m : inf;
        feat[3 * static_cast<int64_t>(i) + 1] = ok ? e : inf;
        feat[3 * static_cast<int64_t>(i) + 2] = ok ? c : inf;
    }
}

__global__ __launch_bounds__(kScoreThreads) void mm_score_kernel(const double* __restrict__ feat, int n, int keep,
                                                                 double* __restrict__ scores, double* __restrict__ scores_out,
                                                                 int32_t* __restrict__ usable, MmInfo* __restrict__ info) {
    __shared__ double red[kScoreThreads];
    __shared__ int ired[kScoreThreads];
    __shared__ double sh[10];                  // s (3), R^-1 (6: 00 01 02 11 12 22), degenerate
    const int tid = threadIdx.x;
    int count = 0, first = n;
    for (int i = tid; i < n; i += kScoreThreads) {
        const double* x = feat + 3 * static_cast<int64_t>(i);
        const int ok = (__builtin_isfinite(x[0]) && __builtin_isfinite(x[1]) && __builtin_isfinite(x[2])) ? 1 : 0;
        usable[i] = ok;
        count += ok;
        if (ok && i < first) first = i;
    }
    const int u = block_sum<int, kScoreThreads>(count, ired);
    ired[tid] = first;                         // the first usable row: a minimum, any order
    __syncthreads();
    for (int step = kScoreThreads / 2; step >= 1; step >>= 1) {
        if (tid < step) ired[tid] = ired[tid] < ired[tid + step] ? ired[tid] : ired[tid + step];
        __syncthreads();
    }
    first = ired[0];
    __syncthreads();
    double ref[3] = {0.0, 0.0, 0.0};
    if (first < n)
        for (int k = 0; k < 3; ++k) ref[k] = feat[3 * static_cast<int64_t>(first) + k];
    double sum[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += kScoreThreads) {
        if (usable[i] == 0) continue;
        for (int k = 0; k < 3; ++k) sum[k] = sum[k] + (feat[3 * static_cast<int64_t>(i) + k] - ref[k]);
    }
    double mean[3];
    for (int k = 0; k < 3; ++k) mean[k] = block_sum<double, kScoreThreads>(sum[k], red) / static_cast<double>(u > 0 ? u : 1);
    double cm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};        // 00 01 02 11 12 22
    for (int i = tid; i < n; i += kScoreThreads) {
        if (usable[i] == 0) continue;
        double y[3];
        for (int k = 0; k < 3; ++k) y[k] = (feat[3 * static_cast<int64_t>(i) + k] - ref[k]) - mean[k];
        cm[0] = cm[0] + y[0] * y[0];
        cm[1] = cm[1] + y[0] * y[1];
        cm[2] = cm[2] + y[0] * y[2];
        cm[3] = cm[3] + y[1] * y[1];
        cm[4] = cm[4] + y[1] * y[2];
        cm[5] = cm[5] + y[2] * y[2];
    }
    for (int k = 0; k < 6; ++k) cm[k] = block_sum<double, kScoreThreads>(cm[k], red);
    if (tid == 0) {
        bool degenerate = u < 4;
        double s[3] = {1.0, 1.0, 1.0}, det = 0.0, inv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (!degenerate) {
            const double dof = static_cast<double>(u - 1);
            const double c00 = cm[0] / dof, c01 = cm[1] / dof, c02 = cm[2] / dof, c11 = cm[3] / dof, c12 = cm[4] / dof, c22 = cm[5] / dof;
            s[0] = sqrt(c00);
            s[1] = sqrt(c11);
            s[2] = sqrt(c22);
            for (int k = 0; k < 3; ++k)
                if (!(s[k] > 0.0) || !__builtin_isfinite(s[k])) degenerate = true;
            if (!degenerate) {
                const double r00 = c00 / (s[0] * s[0]), r01 = c01 / (s[0] * s[1]), r02 = c02 / (s[0] * s[2]);
                const double r11 = c11 / (s[1] * s[1]), r12 = c12 / (s[1] * s[2]), r22 = c22 / (s[2] * s[2]);
                const double a00 = r11 * r22 - r12 * r12, a01 = r02 * r12 - r01 * r22, a02 = r01 * r12 - r02 * r11;
                const double a11 = r00 * r22 - r02 * r02, a12 = r01 * r02 - r00 * r12, a22 = r00 * r11 - r01 * r01;
                det = r00 * a00 + r01 * a01 + r02 * a02;
                if (!(det > kMmMinDet) || !__builtin_isfinite(det)) degenerate = true;
                inv[0] = a00 / det;
                inv[1] = a01 / det;
                inv[2] = a02 / det;
                inv[3] = a11 / det;
                inv[4] = a12 / det;
                inv[5] = a22 / det;
            }
        }
        for (int k = 0; k < 3; ++k) sh[k] = s[k];
        for (int k = 0; k < 6; ++k) sh[3 + k] = inv[k];
        sh[9] = degenerate ? 1.0 : 0.0;
        info->kept = u < keep ? u : keep;
        info->usable = u;
        info->degenerate = degenerate ? 1 : 0;
        info->pad = 0;
        info->det = __builtin_isfinite(det) ? det : 0.0;
    }
    __syncthreads();
    const bool degenerate = sh[9] != 0.0;
    for (int i = tid; i < n; i += kScoreThreads) {
        double score = __builtin_inf();
        if (usable[i] != 0) {
            const double* x = feat + 3 * static_cast<int64_t>(i);
            if (degenerate) {
                score = x[0];
            } else {
                const double z0 = x[0] / sh[0], z1 = x[1] / sh[1], z2 = x[2] / sh[2];
                score = (sh[3] * z0 * z0 + sh[6] * z1 * z1 + sh[8] * z2 * z2) + 2.0 * (sh[4] * z0 * z1 + sh[5] * z0 * z2 + sh[7] * z1 * z2);
            }
        }
        scores[i] = score;
        if (scores_out != nullptr) scores_out[i] = score;
    }
}

__global__ __launch_bounds__(kRankThreads) void mm_rank_kernel(const double* __restrict__ scores, const int32_t* __restrict__ usable,
                                                               int n, const MmInfo* __restrict__ info, int32_t* __restrict__ flags) {
    __shared__ unsigned long long key[kRankThreads];
    __shared__ int live[kRankThreads];
    const int tid = threadIdx.x, i = blockIdx.x * kRankThreads + tid;
    const unsigned long long mine = i < n ? ordered_bits_total(scores[i]) : 0ull;
    int rank = 0;
    for (int base = 0; base < n; base += kRankThreads) {
        const int j = base + tid;
        key[tid] = j < n ? ordered_bits_total(scores[j]) : 0ull;
        live[tid] = j < n ? usable[j] : 0;
        __syncthreads();
        const int top = n - base < kRankThreads ? n - base : kRankThreads;
        for (int q = 0; q < top; ++q) {
            const unsigned long long k = key[q];
            rank += (live[q] != 0 && (k < mine || (k == mine && base + q < i))) ? 1 : 0;
        }
        __syncthreads();
    }
    if (i < n) flags[i] = (usable[i] != 0 && rank < info->kept) ? 1 : 0;
}

__global__ __launch_bounds__(kScoreThreads) void mm_compact_kernel(const int32_t* __restrict__ flags, int n, int32_t* __restrict__ rows,
                                                                   int32_t* __restrict__ count, int32_t* __restrict__ flags_out) {
    __shared__ int lds[kScoreThreads];
    const int tid = threadIdx.x;
    int mine = 0;
    for (int s = 0; s < kCompactSlots; ++s) {
        const int i = tid * kCompactSlots + s;
        if (i < n) {
            const int f = flags[i];
            mine += f;
            if (flags_out != nullptr) flags_out[i] = f;
        }
    }
    int total = 0;
    int slot = block_exclusive_scan<kScoreThreads>(mine, lds, &total);
    for (int s = 0; s < kCompactSlots; ++s) {
        const int i = tid * kCompactSlots + s;
        if (i < n && flags[i] != 0) rows[slot++] = i;
    }
    if (tid == 0) *count = total;
}

__global__ __launch_bounds__(256) void mm_zero_if_empty_kernel(const int32_t* __restrict__ count, int64_t n_cols, float* __restrict__ out) {
    if (*count != 0) return;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (c < n_cols) out[c] = 0.0f;
}

}  // namespace

int multi_metrics_workspace(byz_ctx* ctx, int64_t n, bool matrices, MmScratch* out) {
    out->info = &device_scalars(ctx)->mm;
    Carve c;
    c.take(&out->man, matrices ? n * n : 0);
    c.take(&out->cos, matrices ? n * n : 0);
    c.take(&out->feat, 3 * n);
    c.take(&out->scores, n);
    c.take(&out->usable, n);
    c.take(&out->flags, n);
    c.take(&out->rows, n);
    c.take(&out->count, 1);
    return c.commit(ctx->multi_metrics);
}

int launch_mm_usable_from_gram(byz_ctx* ctx, const double* gram, int64_t n, int32_t* usable, hipStream_t stream) {
    BYZ_REQUIRE(gram && usable && n > 0, "multi_metrics usable rows: bad arguments");
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    mm_usable_from_gram_kernel<<<static_cast<unsigned>(ceil_div(n, 256)), 256, 0, stream>>>(gram, n, usable);
    return check_launch("mm_usable_from_gram_kernel");
}

int launch_mm_usable_from_cos(byz_ctx* ctx, const float* cos, int64_t n, int32_t* usable, hipStream_t stream) {
    BYZ_REQUIRE(cos && usable && n > 0 && n <= kMmMaxRows, "multi_metrics usable rows: bad arguments");
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    mm_usable_from_cos_kernel<<<static_cast<unsigned>(n), kFeatThreads, 0, stream>>>(cos, static_cast<int>(n), usable);
    return check_launch("mm_usable_from_cos_kernel");
}

int launch_mm_features(byz_ctx* ctx, const float* man, const float* euc, const float* cos, const int32_t* usable, int64_t n,
                       double* feat, hipStream_t stream) {
    BYZ_REQUIRE(man && euc && cos && usable && feat && n > 0 && n <= kMmMaxRows, "multi_metrics features: bad arguments (n = %lld)",
                (long long)n);
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    mm_features_kernel<<<static_cast<unsigned>(n), kFeatThreads, 0, stream>>>(man, euc, cos, usable, static_cast<int>(n), feat);
    return check_launch("mm_features_kernel");
}

int launch_mm_select(byz_ctx* ctx, const MmScratch& t, const double* feat, int64_t n, int64_t keep, int32_t* flags_out,
                     double* scores_out, hipStream_t stream) {
    BYZ_REQUIRE(feat && n > 0 && n <= kMmMaxRows && keep >= 1 && keep <= n, "multi_metrics select: bad arguments (n = %lld, keep = %lld)",
                (long long)n, (long long)keep);
    {
        KernelTimer timer(ctx, BYZ_K_MISC, stream);
        mm_score_kernel<<<1, kScoreThreads, 0, stream>>>(feat, static_cast<int>(n), static_cast<int>(keep), t.scores, scores_out, t.usable,
                                                         t.info);
        BYZ_TRY(check_launch("mm_score_kernel"));
    }
    KernelTimer timer(ctx, BYZ_K_ROW_SORT, stream);
    mm_rank_kernel<<<static_cast<unsigned>(ceil_div(n, kRankThreads)), kRankThreads, 0, stream>>>(t.scores, t.usable, static_cast<int>(n),
                                                                                                  t.info, t.flags);
    BYZ_TRY(check_launch("mm_rank_kernel"));
    mm_compact_kernel<<<1, kScoreThreads, 0, stream>>>(t.flags, static_cast<int>(n), t.rows, t.count, flags_out);
    return check_launch("mm_compact_kernel");
}

int launch_mm_zero_if_empty(byz_ctx* ctx, const int32_t* count_dev, int64_t n_cols, float* out, hipStream_t stream) {
    BYZ_REQUIRE(count_dev && out && n_cols > 0, "multi_metrics: bad arguments");
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    mm_zero_if_empty_kernel<<<static_cast<unsigned>(ceil_div(n_cols, 256)), 256, 0, stream>>>(count_dev, n_cols, out);
    return check_launch("mm_zero_if_empty_kernel");
}

}  // namespace byz
