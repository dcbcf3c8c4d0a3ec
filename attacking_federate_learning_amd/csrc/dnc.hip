// DnC, the spectral defence (Shejwalkar and Houmansadr, NDSS 2021, Algorithm 2): colluding rows line up along the top right
// singular vector of the centred gradient matrix; every row is scored by its squared projection on it and the highest scores
// are removed.  The contract (include/byzagg.h) is written in N-space -- M = C C^T, a power iteration on M -- and this file gets
// the same values without ever forming M: y = M u is two mat-vecs, w = C^T u (a vector over the sampled columns) and y = C w, so
// an iteration reads the n x b fp64 matrix C twice and nothing here is of order n^2 b.  It is also what the columns layout
// needs: w stays on the rank that owns the columns, y's per-row partial sums are all-reduced.
//
//   gather   C[i][j] = (double)G[i][columns[j]], one workgroup per row; bad[i] = 1.0 when a sampled value is not finite
//   prepare  (bad all-reduced) weights 1 / 0 of the active rows, n_a
//   colsum   part[chunk][j] = sum over the chunk's rows, in row order, of wt_i * C[i][j] (a row of weight 0 adds +0.0, it is
//            not multiplied: 0 * inf never reaches a column); finish adds the chunks in chunk order: the column means (/ n_a)
//            and w = C^T u
//   centre   C[i][j] -= mu_j (an inactive row becomes zeros), diag[i] = sum_j C[i][j]^2 = M_ii
//   start    (diag all-reduced) i0 = the active row with the largest M_ii, the lowest index on a tie; u = e_i0
//   rowdot   y[i] = sum_j C[i][j] w[j], one wave per row, lane sums then a fixed butterfly
//   step     (y all-reduced) u = y / |y|, or after the last product lambda = u.y and the scores y_i^2 / lambda
//   rank     keep_i = #{k : (s_k, k) < (s_i, i)} < n - remove_count, by counting: exact on the fp64 scores (every NaN behind
//            +inf, -0.0 as +0.0), n^2 comparisons through LDS tiles; ANDed into the running intersection
//   compact  the kept rows in ascending order and their count (block_exclusive_scan, order_keys.hpp)
// Every sum has a fixed order: two calls give the same bits.  Nothing synchronises with the host; the kept count stays in the
// context's DncReport (device_scalars.hpp) until byz_dnc_info reads it.
#include "order_keys.hpp"
#include "row_walk.hpp"

#include <algorithm>

namespace byz {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kOneThreads = 1024;                   // the single-workgroup kernels
constexpr int kMaxChunks = 64;                      // row chunks of colsum at most
constexpr int kRowRun = 8;                          // colsum: rows whose loads are issued together

// state words (fp64) behind the vectors of the workspace
constexpr int kStateActive = 0;                     // n_a
constexpr int kStateZero = 1;                       // != 0: M_i0i0, a |y| or lambda was 0 (or no row is active): active scores are 0
constexpr int kStateWords = 4;

__global__ __launch_bounds__(kThreads) void dnc_gather_kernel(const float* __restrict__ G, int64_t ld,
                                                              const int64_t* __restrict__ columns, int64_t b,
                                                              double* __restrict__ C, double* __restrict__ bad) {
    const int64_t i = blockIdx.x;
    const float* row = G + i * ld;
    double* out = C + i * b;
    int nonfinite = 0;
    for (int64_t j = threadIdx.x; j < b; j += kThreads) {
        const float x = row[columns[j]];
        if (!__builtin_isfinite(x)) nonfinite = 1;
        out[j] = static_cast<double>(x);
    }
    nonfinite = __syncthreads_or(nonfinite);
    if (threadIdx.x == 0) bad[i] = nonfinite ? 1.0 : 0.0;
}

// wt_i = 1 for an active row (bad_i == 0 after the all-reduce), 0 otherwise; state: n_a, the zero flag cleared
__global__ __launch_bounds__(kOneThreads) void dnc_prepare_kernel(const double* __restrict__ bad, int64_t n, double* __restrict__ wt,
                                                                  double* __restrict__ state) {
    __shared__ double lds[kOneThreads];
    double count = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kOneThreads) {
        const bool active = bad[i] == 0.0;
        wt[i] = active ? 1.0 : 0.0;
        if (active) count = count + 1.0;
    }
    const double n_a = block_sum<double, kOneThreads>(count, lds);
    if (threadIdx.x == 0) {
        state[kStateActive] = n_a;
        state[kStateZero] = n_a == 0.0 ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(kThreads) void dnc_colsum_partial_kernel(const double* __restrict__ C, int64_t n, int64_t b,
                                                                      const double* __restrict__ wt, int64_t chunk_rows,
                                                                      double* __restrict__ part) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (j >= b) return;
    const int64_t r_begin = static_cast<int64_t>(blockIdx.y) * chunk_rows;
    const int64_t r_end = r_begin + chunk_rows < n ? r_begin + chunk_rows : n;
    const double* p = C + j;
    double acc = 0.0;
    int64_t r = r_begin;
    for (; r + kRowRun <= r_end; r += kRowRun) {
        double w[kRowRun], c[kRowRun];
#pragma unroll
        for (int u = 0; u < kRowRun; ++u) w[u] = wt[r + u];            // uniform: scalar loads
#pragma unroll
        for (int u = 0; u < kRowRun; ++u) c[u] = p[(r + u) * b];
#pragma unroll
        for (int u = 0; u < kRowRun; ++u) acc = acc + (w[u] != 0.0 ? w[u] * c[u] : 0.0);
    }
    for (; r < r_end; ++r) {
        const double w = wt[r];
        const double c = p[r * b];
        acc = acc + (w != 0.0 ? w * c : 0.0);
    }
    part[static_cast<int64_t>(blockIdx.y) * b + j] = acc;
}

// out[j] = the chunks of column j added in chunk order; divide_by (optional): / *divide_by (the column means)
__global__ __launch_bounds__(kThreads) void dnc_colsum_finish_kernel(const double* __restrict__ part, int64_t b, int chunks,
                                                                     const double* __restrict__ divide_by,
                                                                     double* __restrict__ out) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (j >= b) return;
    double s = 0.0;
    for (int p = 0; p < chunks; ++p) s = s + part[static_cast<int64_t>(p) * b + j];
    out[j] = divide_by != nullptr ? s / *divide_by : s;
}

__global__ __launch_bounds__(kThreads) void dnc_centre_kernel(double* __restrict__ C, int64_t b, const double* __restrict__ mu,
                                                              const double* __restrict__ bad, double* __restrict__ diag) {
    __shared__ double lds[kThreads];
    const int64_t i = blockIdx.x;
    const bool active = bad[i] == 0.0;
    double* row = C + i * b;
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < b; j += kThreads) {
        const double c = active ? row[j] - mu[j] : 0.0;
        row[j] = c;
        acc = acc + c * c;
    }
    const double total = block_sum<double, kThreads>(acc, lds);
    if (threadIdx.x == 0) diag[i] = total;
}

// u = e_i0, i0 the active row with the largest diag (lowest index on a tie); diag[i0] == 0 raises the zero flag
__global__ __launch_bounds__(kOneThreads) void dnc_start_kernel(const double* __restrict__ diag, const double* __restrict__ bad,
                                                                int64_t n, double* __restrict__ u, double* __restrict__ state) {
    __shared__ double best_v[kOneThreads];
    __shared__ long long best_i[kOneThreads];
    const int tid = threadIdx.x;
    double bv = -1.0;
    long long bi = -1;
    for (int64_t i = tid; i < n; i += kOneThreads) {           // ascending within a thread: '>' keeps the lowest index
        if (bad[i] == 0.0 && (bi < 0 || diag[i] > bv)) {
            bv = diag[i];
            bi = i;
        }
    }
    best_v[tid] = bv;
    best_i[tid] = bi;
    __syncthreads();
    for (int step = kOneThreads / 2; step >= 1; step >>= 1) {
        if (tid < step) {
            const double ov = best_v[tid + step];
            const long long oi = best_i[tid + step];
            const long long mi = best_i[tid];
            if (oi >= 0 && (mi < 0 || ov > best_v[tid] || (ov == best_v[tid] && oi < mi))) {
                best_v[tid] = ov;
                best_i[tid] = oi;
            }
        }
        __syncthreads();
    }
    const long long i0 = best_i[0];
    const double top = best_v[0];
    for (int64_t i = tid; i < n; i += kOneThreads) u[i] = i == i0 ? 1.0 : 0.0;
    if (tid == 0 && (i0 < 0 || top == 0.0)) state[kStateZero] = 1.0;
}

__global__ __launch_bounds__(kThreads) void dnc_rowdot_kernel(const double* __restrict__ C, int64_t n, int64_t b,
                                                              const double* __restrict__ w, double* __restrict__ y) {
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
    if (i >= n) return;
    const double* row = C + i * b;
    double acc = 0.0;
#pragma unroll 4
    for (int64_t j = lane; j < b; j += 64) acc = acc + row[j] * w[j];
    const double s = wave_sum_shfl(acc);
    if (lane == 0) y[i] = s;
}

// not the last product: u = y / |y|.  The last: lambda = u.y, scores_i = y_i^2 / lambda (0 under the zero flag, +inf for an
// inactive row).
__global__ __launch_bounds__(kOneThreads) void dnc_step_kernel(const double* __restrict__ y, const double* __restrict__ bad,
                                                               int64_t n, double* __restrict__ u, double* __restrict__ state,
                                                               int last, double* __restrict__ scores) {
    __shared__ double lds[kOneThreads];
    const int64_t per = (n + kOneThreads - 1) / kOneThreads;
    const int64_t lo = threadIdx.x * per < n ? threadIdx.x * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    double s = 0.0;
    for (int64_t i = lo; i < hi; ++i) s = s + (last ? u[i] * y[i] : y[i] * y[i]);
    const double total = block_sum<double, kOneThreads>(s, lds);
    const bool zero_before = state[kStateZero] != 0.0;
    __syncthreads();                                  // every thread has read the flag
    if (!last) {
        const double norm = sqrt(total);
        if (norm == 0.0) {
            if (threadIdx.x == 0) state[kStateZero] = 1.0;
            return;
        }
        for (int64_t i = lo; i < hi; ++i) u[i] = y[i] / norm;
        return;
    }
    const bool zero = zero_before || total == 0.0;
    if (threadIdx.x == 0 && zero) state[kStateZero] = 1.0;
    for (int64_t i = lo; i < hi; ++i) {
        if (bad[i] != 0.0) scores[i] = __builtin_inf();
        else scores[i] = zero ? 0.0 : (y[i] * y[i]) / total;
    }
}

// keep[i] (&)= rank of (s_i, i) < n_keep
__global__ __launch_bounds__(kThreads) void dnc_rank_kernel(const double* __restrict__ scores, int64_t n, int64_t n_keep, int first,
                                                            int32_t* __restrict__ keep) {
    __shared__ unsigned long long tile[kThreads];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const unsigned long long mine = i < n ? ordered_bits_total(scores[i]) : 0ull;
    int64_t below = 0;
    for (int64_t k0 = 0; k0 < n; k0 += kThreads) {
        const int64_t k = k0 + threadIdx.x;
        tile[threadIdx.x] = k < n ? ordered_bits_total(scores[k]) : ~0ull;
        __syncthreads();
        const int limit = n - k0 < kThreads ? static_cast<int>(n - k0) : kThreads;
        for (int t = 0; t < limit; ++t) {
            const unsigned long long other = tile[t];
            below += (other < mine || (other == mine && k0 + t < i)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (i < n) {
        const int32_t flag = below < n_keep ? 1 : 0;
        keep[i] = first ? flag : (keep[i] & flag);
    }
}

// good: n int32, the kept rows ascending, -1 behind them; the count to the context's report and to count_out (optional);
// report->inactive: the rows the last iteration found inactive
__global__ __launch_bounds__(kOneThreads) void dnc_compact_kernel(const int32_t* __restrict__ keep, const double* __restrict__ bad,
                                                                  int64_t n, int32_t* __restrict__ good,
                                                                  DncReport* __restrict__ report, int32_t* __restrict__ count_out) {
    __shared__ int lds[kOneThreads];
    const int tid = threadIdx.x;
    const int64_t chunk = (n + kOneThreads - 1) / kOneThreads;
    const int64_t lo = tid * chunk < n ? tid * chunk : n;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    int count = 0, ina = 0;
    for (int64_t r = lo; r < hi; ++r) {
        count += keep[r] != 0 ? 1 : 0;
        ina += bad[r] != 0.0 ? 1 : 0;
    }
    const int inactive = block_sum<int, kOneThreads>(ina, lds);
    int total;
    int slot = block_exclusive_scan<kOneThreads>(count, lds, &total);
    for (int64_t r = lo; r < hi; ++r)
        if (keep[r] != 0) good[slot++] = static_cast<int32_t>(r);
    for (int64_t r = total + tid; r < n; r += kOneThreads) good[r] = -1;
    if (tid == 0) {
        report->kept = total;
        report->inactive = inactive;
        if (count_out != nullptr) *count_out = total;
    }
}

__global__ __launch_bounds__(kThreads) void dnc_copy_i32_kernel(const int32_t* __restrict__ src, int64_t n, int32_t* __restrict__ dst) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

int colsum_chunks(byz_ctx* ctx, int64_t n, int64_t b, int64_t* chunk_rows) {
    const int64_t col_blocks = std::max<int64_t>(1, ceil_div(b, kThreads));
    const int64_t target = static_cast<int64_t>(ctx->num_cus) * 8;
    int64_t p = std::max<int64_t>(1, ceil_div(target, col_blocks));
    p = std::min<int64_t>({p, static_cast<int64_t>(kMaxChunks), ceil_div(n, 4 * kRowRun)});
    p = std::max<int64_t>(p, 1);
    *chunk_rows = ceil_div(n, p);
    return static_cast<int>(ceil_div(n, *chunk_rows));
}

}  // namespace

int dnc_workspace(byz_ctx* ctx, int64_t n, int64_t b, DncScratch* out) {
    // C, the colsum partials, w; then the n-vectors bad, wt, diag (also y), u, scores, the state; then keep and good
    Carve c;
    c.take(&out->C, n * b);
    c.take(&out->part, static_cast<int64_t>(kMaxChunks) * b);
    c.take(&out->w, b);
    for (double** per_row : {&out->bad, &out->wt, &out->y, &out->u, &out->scores}) c.take(per_row, n);
    c.take(&out->state, kStateWords);
    c.take(&out->keep, n);
    c.take(&out->good, n);
    return c.commit(ctx->dnc);
}

// w_out = (C^T wt) [/ *divide_by]
static int colsum(byz_ctx* ctx, const DncScratch& t, int64_t n, int64_t b, const double* wt, const double* divide_by, double* w_out,
                  hipStream_t stream) {
    if (b == 0) return BYZ_OK;
    int64_t chunk_rows = 0;
    const int chunks = colsum_chunks(ctx, n, b, &chunk_rows);
    const dim3 grid(static_cast<unsigned>(ceil_div(b, kThreads)), static_cast<unsigned>(chunks));
    dnc_colsum_partial_kernel<<<grid, kThreads, 0, stream>>>(t.C, n, b, wt, chunk_rows, t.part);
    BYZ_TRY(check_launch("dnc_colsum_partial_kernel"));
    dnc_colsum_finish_kernel<<<static_cast<unsigned>(ceil_div(b, kThreads)), kThreads, 0, stream>>>(t.part, b, chunks, divide_by, w_out);
    return check_launch("dnc_colsum_finish_kernel");
}

int launch_dnc_scores(byz_ctx* ctx, const DncScratch& t, const float* G, int64_t n, int64_t ld, const int64_t* columns, int64_t b,
                      int64_t power_iters, byz_allreduce_f64_fn allreduce, void* user, void* stream_arg) {
    hipStream_t stream = as_stream(stream_arg);
    auto reduce = [&](double* buf, const char* what) -> int {
        if (allreduce == nullptr) return BYZ_OK;
        const int rc = allreduce(user, buf, n, stream_arg);
        if (rc != 0) {
            set_error("dnc (%s): the caller's all-reduce returned %d", what, rc);
            return BYZ_E_COLLECTIVE;
        }
        return BYZ_OK;
    };
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    const unsigned row_grid = static_cast<unsigned>(n);
    if (b > 0) {
        dnc_gather_kernel<<<row_grid, kThreads, 0, stream>>>(G, ld, columns, b, t.C, t.bad);
        BYZ_TRY(check_launch("dnc_gather_kernel"));
    } else {
        BYZ_HIP(hipMemsetAsync(t.bad, 0, static_cast<size_t>(n) * sizeof(double), stream));     // a rank with no sampled column
    }
    BYZ_TRY(reduce(t.bad, "activity"));
    dnc_prepare_kernel<<<1, kOneThreads, 0, stream>>>(t.bad, n, t.wt, t.state);
    BYZ_TRY(check_launch("dnc_prepare_kernel"));
    BYZ_TRY(colsum(ctx, t, n, b, t.wt, t.state + kStateActive, t.w, stream));                   // the column means
    if (b > 0) {
        dnc_centre_kernel<<<row_grid, kThreads, 0, stream>>>(t.C, b, t.w, t.bad, t.y);
        BYZ_TRY(check_launch("dnc_centre_kernel"));
    } else {
        BYZ_HIP(hipMemsetAsync(t.y, 0, static_cast<size_t>(n) * sizeof(double), stream));
    }
    BYZ_TRY(reduce(t.y, "diagonal"));
    dnc_start_kernel<<<1, kOneThreads, 0, stream>>>(t.y, t.bad, n, t.u, t.state);
    BYZ_TRY(check_launch("dnc_start_kernel"));
    for (int64_t k = 0; k <= power_iters; ++k) {
        BYZ_TRY(colsum(ctx, t, n, b, t.u, nullptr, t.w, stream));                               // w = C^T u
        if (b > 0) {
            dnc_rowdot_kernel<<<static_cast<unsigned>(ceil_div(n, kWaves)), kThreads, 0, stream>>>(t.C, n, b, t.w, t.y);
            BYZ_TRY(check_launch("dnc_rowdot_kernel"));
        } else {
            BYZ_HIP(hipMemsetAsync(t.y, 0, static_cast<size_t>(n) * sizeof(double), stream));
        }
        BYZ_TRY(reduce(t.y, "product"));
        dnc_step_kernel<<<1, kOneThreads, 0, stream>>>(t.y, t.bad, n, t.u, t.state, k == power_iters ? 1 : 0, t.scores);
        BYZ_TRY(check_launch("dnc_step_kernel"));
    }
    return BYZ_OK;
}

int launch_dnc_rank(byz_ctx* ctx, const DncScratch& t, int64_t n, int64_t n_keep, bool first, hipStream_t stream) {
    KernelTimer timer(ctx, BYZ_K_KRUM_ARGMIN, stream);
    dnc_rank_kernel<<<static_cast<unsigned>(ceil_div(n, kThreads)), kThreads, 0, stream>>>(t.scores, n, n_keep, first ? 1 : 0, t.keep);
    return check_launch("dnc_rank_kernel");
}

int launch_dnc_compact(byz_ctx* ctx, const DncScratch& t, int64_t n, int32_t* good_out, int32_t* count_out, hipStream_t stream) {
    KernelTimer timer(ctx, BYZ_K_KRUM_ARGMIN, stream);
    dnc_compact_kernel<<<1, kOneThreads, 0, stream>>>(t.keep, t.bad, n, t.good, &device_scalars(ctx)->dnc, count_out);
    BYZ_TRY(check_launch("dnc_compact_kernel"));
    if (good_out != nullptr) {
        dnc_copy_i32_kernel<<<static_cast<unsigned>(ceil_div(n, kThreads)), kThreads, 0, stream>>>(t.good, n, good_out);
        BYZ_TRY(check_launch("dnc_copy_i32_kernel"));
    }
    return BYZ_OK;
}

}  // namespace byz
