// The geometric median by smoothed Weiszfeld iterations (RFA: Pillutla, Kakade and Harchaoui, "Robust Aggregation for
// Federated Learning"): two streaming passes over G per iteration, nothing of order N^2.
//
//   rowsq   sq[i] = sum_c ((double)x_ic - (double)z_c)^2 in fp64, on the difference (never |x|^2 - 2 x.z + |z|^2, which
//           cancels when the rows cluster round z).  Workgroups take (block of 32 rows, chunk of columns); each wave owns 8
//           rows and walks its chunk in windows of 1024 columns: a lane keeps its 16 floats of z in registers across the 8
//           rows and loads dwordx4.  Every (row, chunk) partial comes from one wave (lane sums, then a fixed butterfly), so
//           partials[chunk][row] needs no atomics; the finishing kernel adds a row's chunks in chunk order.  At most
//           kMaxChunks chunks: the scratch is O(n_rows) whatever n_cols is.
//   wmean   out[c] = fl32(S_c / W), S_c = sum over rows with w_i != 0 of w_i * (double)x_ic, W = sum w_i, both sequential in
//           row order with no fused multiply-add (this file is compiled with -ffp-contract=off).  One thread walks the rows
//           for VEC columns (walk_rows, row_walk.hpp); the weights are uniform and arrive through scalar loads.  A row of
//           weight 0 is neither loaded nor multiplied, so 0 * inf never reaches a column.
//   update  centered clipping's step (cclip.hip has its scales): out[c] = fl32((double)v[c] + S_c / n), S_c = sum over the
//           rows with s_i != 0 of s_i * ((double)x_ic - (double)v[c]).  The same kernel template as wmean (weighted_rows_kernel,
//           kRowsCentred): the same walk, the same launch shape, another product and another last line.
//   dots    FLTrust's first pass (fltrust.hip has its trust scores): p[i] = sum_c (double)x_ic * (double)r_c and
//           q[i] = sum_c (double)x_ic^2 in one read of G.  rowsq's kernel template with two accumulators a row
//           (rowsq_partial_kernel<VEC4, kRowsqDots>): the same geometry, the same order of additions, partials[2][chunk][row].
//   moments the Min-Max / Min-Sum attacks' pass (minmax.hip): a[i] = sum_c ((double)x_ic - (double)mu_c)^2, rowsq's bits, and
//           b[i] = sum_c (double)p_c * ((double)mu_c - (double)x_ic) in one read of G: the template's third form.
//   scaled  FLTrust's second pass: out[c] = T > 0 ? fl32(S_c / T) : 0, S_c as wmean's, T read from one device double.
//           weighted_rows_kernel's third mode (kRowsScaled).
//   step    one workgroup: d_i = sqrt(sq_i), F = sum of d over the active rows (fixed order), the stop test
//           |F_old - F| <= ftol * F, beta_i = 1 / max(nu, d_i).
// Every launch of the loop is enqueued up front; after the stop the remaining launches read the done word and return at once
// (the redo_gate idiom of column_sequential_kernel).  The state lives in the context's GeomedReport (device_scalars.hpp).
#include "row_walk.hpp"

#include <algorithm>

namespace byz {
namespace {

constexpr int kThreads = kWalkThreads;              // rowsq and weighted_rows workgroups
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerWave = 8;
constexpr int kRowBlock = kWaves * kRowsPerWave;    // rows of one rowsq workgroup
constexpr int kSegs = 4;                            // dwordx4 loads per lane and row in one window
constexpr int kWindow = 64 * 4 * kSegs;             // columns a wave covers at once (1024)
constexpr int kMaxChunks = 64;                      // fp64 partials per row at most
constexpr int kStepThreads = 1024;

// four consecutive floats at column c (of a window that ends at c_end): dwordx4 when whole and aligned, masked otherwise
template <bool VEC4>
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t c, int64_t c_end, float (&x)[4]) {
    if (VEC4 && c + 4 <= c_end) {
        const float4u q = *reinterpret_cast<const float4u*>(p + c);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) x[v] = c + v < c_end ? p[c + v] : 0.0f;
    }
}

// The three forms of one (block of 32 rows, chunk of columns) pass; every form has the same geometry and the same order of
// additions, and the forms with two sums a row write partials[2][chunk][row] (chunks = gridDim.y).
//   kRowsqDist     partials[chunk * n_rows + row] = the row's squared distance to z over the chunk; z == nullptr: to the origin.
//   kRowsqDots     z is FLTrust's root (never null): plane 0 the row's dot product with it, plane 1 the row's own squared norm.
//   kRowsqMoments  z is a centre mu, p a direction (neither null), d = (double)mu - (double)x: plane 0 the sum of d * d -- the
//                  bits of kRowsqDist's sum, the square of a difference does not see its sign -- plane 1 the sum of (double)p * d.
//                  A lane keeps its 16 floats of p beside its 16 doubles of mu across the wave's 8 rows and converts them where
//                  it multiplies: 16 registers instead of 32 (profiles/minmax_timing.md has the counts).
constexpr int kRowsqDist = 0, kRowsqDots = 1, kRowsqMoments = 2;
// the direction of the moments form travels behind the arguments that the three forms share
__device__ __forceinline__ const float* rowsq_direction() { return nullptr; }
__device__ __forceinline__ const float* rowsq_direction(const float* p_vec) { return p_vec; }
template <bool VEC4, int FORM, typename... Direction>
__global__ __launch_bounds__(kThreads) void rowsq_partial_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols,
                                                                 int64_t ld, const float* __restrict__ z, int64_t chunk_cols,
                                                                 double* __restrict__ partials, const int32_t* skip_if_set,
                                                                 const int32_t* run_if_set, Direction... direction) {
    static_assert(sizeof...(Direction) == (FORM == kRowsqMoments ? 1 : 0), "the moments form alone takes a direction");
    constexpr bool TWO = FORM != kRowsqDist;
    if (gated_out(skip_if_set, run_if_set)) return;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kRowBlock + wave * kRowsPerWave;
    if (row0 >= n_rows) return;
    const int64_t c_begin = static_cast<int64_t>(blockIdx.y) * chunk_cols;
    const int64_t c_end = c_begin + chunk_cols < n_cols ? c_begin + chunk_cols : n_cols;
    [[maybe_unused]] const float* p_vec = rowsq_direction(direction...);
    double acc[kRowsPerWave];
    [[maybe_unused]] double acc_q[TWO ? kRowsPerWave : 1];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) acc[r] = 0.0;
    if constexpr (TWO) {
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) acc_q[r] = 0.0;
    }
    for (int64_t w0 = c_begin; w0 < c_end; w0 += kWindow) {
        double zs[kSegs][4];
        [[maybe_unused]] float ps[FORM == kRowsqMoments ? kSegs : 1][4];
#pragma unroll
        for (int k = 0; k < kSegs; ++k) {
            float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (z != nullptr) load4<VEC4>(z, w0 + k * 256 + lane * 4, c_end, t);
#pragma unroll
            for (int v = 0; v < 4; ++v) zs[k][v] = static_cast<double>(t[v]);
            if constexpr (FORM == kRowsqMoments) load4<VEC4>(p_vec, w0 + k * 256 + lane * 4, c_end, ps[k]);
        }
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            if (row0 + r < n_rows) {
                const float* p = G + (row0 + r) * ld;
                float x[kSegs][4];
#pragma unroll
                for (int k = 0; k < kSegs; ++k) load4<VEC4>(p, w0 + k * 256 + lane * 4, c_end, x[k]);
                double s = 0.0;
                [[maybe_unused]] double s_q = 0.0;
#pragma unroll
                for (int k = 0; k < kSegs; ++k)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        if constexpr (FORM == kRowsqDots) {
                            const double xd = static_cast<double>(x[k][v]);
                            s = s + xd * zs[k][v];
                            s_q = s_q + xd * xd;
                        } else if constexpr (FORM == kRowsqMoments) {
                            const double d = zs[k][v] - static_cast<double>(x[k][v]);
                            s = s + d * d;
                            s_q = s_q + static_cast<double>(ps[k][v]) * d;
                        } else {
                            const double d = static_cast<double>(x[k][v]) - zs[k][v];
                            s = s + d * d;
                        }
                    }
                acc[r] = acc[r] + s;
                if constexpr (TWO) acc_q[r] = acc_q[r] + s_q;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        const double s = wave_sum_shfl(acc[r]);
        if (lane == 0 && row0 + r < n_rows) partials[static_cast<int64_t>(blockIdx.y) * n_rows + row0 + r] = s;
        if constexpr (TWO) {
            const double s_q = wave_sum_shfl(acc_q[r]);
            if (lane == 0 && row0 + r < n_rows)
                partials[(static_cast<int64_t>(gridDim.y) + blockIdx.y) * n_rows + row0 + r] = s_q;
        }
    }
}

// blockIdx.y = 1 (the dots pass alone): the second plane of partials into sq2
__global__ __launch_bounds__(256) void rowsq_finish_kernel(const double* __restrict__ partials, int64_t n_rows, int chunks,
                                                           double* __restrict__ sq, double* __restrict__ sq2,
                                                           const int32_t* skip_if_set, const int32_t* run_if_set) {
    if (gated_out(skip_if_set, run_if_set)) return;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const double* plane = partials + static_cast<int64_t>(blockIdx.y) * chunks * n_rows;
    double s = 0.0;
    for (int p = 0; p < chunks; ++p) s = s + plane[p * n_rows + i];
    (blockIdx.y == 0 ? sq : sq2)[i] = s;
}

// kRowsMean, the weighted mean: acc += w * (double)x, W += w, out = fl32(acc / W); v and divisor are not read.
// kRowsCentred, centered clipping's update: acc += s * ((double)x - (double)v), out = fl32((double)v + acc / n_rows); v and out
// may be the same buffer (a thread reads its own columns of v before it writes them).
// kRowsScaled, FLTrust's sum: acc as the mean's, out = T > 0 ? fl32(acc / T) : 0 with T = *divisor (a device double).
constexpr int kRowsMean = 0, kRowsCentred = 1, kRowsScaled = 2;
template <int VEC, int MODE>
__global__ __launch_bounds__(kThreads) void weighted_rows_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols,
                                                                 int64_t ld, const float* v, const double* __restrict__ w,
                                                                 const double* __restrict__ divisor_dev, float* out,
                                                                 const int32_t* skip_if_set, const int32_t* run_if_set) {
    constexpr bool CENTRED = MODE == kRowsCentred;
    if (gated_out(skip_if_set, run_if_set)) return;
    const int64_t c0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * VEC;
    if (c0 >= n_cols) return;
    double vd[VEC], acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        vd[k] = CENTRED && c0 + k < n_cols ? static_cast<double>(v[c0 + k]) : 0.0;
        acc[k] = 0.0;
    }
    double W = 0.0;
    walk_rows<VEC>(
        G + c0, ld, n_rows, c0, n_cols, [](int64_t r) __attribute__((always_inline)) { return r; },
        [&](int64_t r) __attribute__((always_inline)) { return w[r]; },          // uniform: one scalar load for a run
        [&](int64_t, double wr, const float(&x)[VEC]) __attribute__((always_inline)) {
            if constexpr (MODE == kRowsMean) W = W + wr;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                if constexpr (CENTRED) acc[k] = acc[k] + wr * (static_cast<double>(x[k]) - vd[k]);
                else acc[k] = acc[k] + wr * static_cast<double>(x[k]);
            }
        });
    double divisor = W;
    if constexpr (CENTRED) divisor = static_cast<double>(n_rows);
    if constexpr (MODE == kRowsScaled) divisor = *divisor_dev;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        if (c0 + k >= n_cols) continue;
        if constexpr (CENTRED) out[c0 + k] = static_cast<float>(vd[k] + acc[k] / divisor);
        else if constexpr (MODE == kRowsScaled) out[c0 + k] = divisor > 0.0 ? static_cast<float>(acc[k] / divisor) : 0.0f;
        else out[c0 + k] = static_cast<float>(acc[k] / divisor);
    }
}

// ---- the loop's small kernels (state: GeomedReport, device_scalars.hpp) ------------------------------------------------------
__global__ __launch_bounds__(256) void finite_check_kernel(const float* __restrict__ v, int64_t n, GeomedReport* r,
                                                           double* flag_f64) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = v[i];
    if (!__builtin_isfinite(x)) {
        __hip_atomic_store(&r->fallback, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (flag_f64 != nullptr) *flag_f64 = 1.0;
    }
}

// mean0 was not finite: the active rows are those with a finite sq0 (the fp64 squared norm), their weights 1, the others 0
__global__ __launch_bounds__(kStepThreads) void geomed_fallback_kernel(const double* __restrict__ sq0, int64_t n, double* w,
                                                                       GeomedReport* r, const double* global_flag) {
    __shared__ double lds[kStepThreads];
    const bool fallback = global_flag != nullptr ? *global_flag > 0.0
                                                 : __hip_atomic_load(&r->fallback, __ATOMIC_RELAXED,
                                                                     __HIP_MEMORY_SCOPE_AGENT) != 0;
    if (global_flag != nullptr && threadIdx.x == 0) r->fallback = fallback ? 1 : 0;
    if (!fallback) return;
    double excluded = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kStepThreads) {
        const bool active = __builtin_isfinite(sq0[i]);
        w[i] = active ? 1.0 : 0.0;
        if (!active) excluded = excluded + 1.0;
    }
    const double total = block_sum<double, kStepThreads>(excluded, lds);
    if (threadIdx.x == 0) {
        const int64_t ex = static_cast<int64_t>(total);
        r->excluded = static_cast<int32_t>(ex);
        if (ex == n) r->done = 1;          // no row left: the output is wmean's NaN, iterations 0
    }
}

// k = 0: the objective at the starting point; k >= 1: after the k-th update.  Active rows: every row unless the fallback
// flag is set, then those with a non-zero weight (a beta of an active row is never 0).  k < max_iter and no stop: the weights
// of update k + 1.
__global__ __launch_bounds__(kStepThreads) void geomed_step_kernel(const double* __restrict__ sq, int64_t n, double* w,
                                                                   GeomedReport* r, double nu, double ftol, int64_t k,
                                                                   int64_t max_iter) {
    __shared__ double lds[kStepThreads];
    if (__hip_atomic_load(&r->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    const bool fallback = r->fallback != 0;
    const int64_t per = (n + kStepThreads - 1) / kStepThreads;
    const int64_t lo = threadIdx.x * per < n ? threadIdx.x * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    double f = 0.0;
    for (int64_t i = lo; i < hi; ++i)
        if (!fallback || w[i] != 0.0) f = f + sqrt(sq[i]);
    const double F = block_sum<double, kStepThreads>(f, lds);
    const double F_old = r->objective;
    const bool stop = k > 0 && fabs(F_old - F) <= ftol * F;
    __syncthreads();                                  // every thread has read F_old
    if (threadIdx.x == 0) {
        r->objective = F;
        r->iterations = static_cast<int32_t>(k);
        if (stop) r->done = 1;
    }
    if (stop || k >= max_iter) return;
    for (int64_t i = lo; i < hi; ++i) {
        const bool active = !fallback || w[i] != 0.0;
        const double d = sqrt(sq[i]);
        w[i] = active ? 1.0 / (d > nu ? d : nu) : 0.0;
    }
}

// weights_out = beta / sum(beta) of the last update, or uniform over the active rows when there was none
__global__ __launch_bounds__(kStepThreads) void geomed_weights_kernel(const double* __restrict__ w, int64_t n,
                                                                      const GeomedReport* r, double* __restrict__ out) {
    __shared__ double lds[kStepThreads];
    const bool fallback = r->fallback != 0;
    const bool updated = r->iterations > 0;
    const int64_t per = (n + kStepThreads - 1) / kStepThreads;
    const int64_t lo = threadIdx.x * per < n ? threadIdx.x * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    double s = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
        if (updated) s = s + w[i];
        else if (!fallback || w[i] != 0.0) s = s + 1.0;
    }
    const double total = block_sum<double, kStepThreads>(s, lds);
    for (int64_t i = lo; i < hi; ++i) {
        const bool active = !fallback || w[i] != 0.0;
        if (total == 0.0) out[i] = 0.0;
        else if (updated) out[i] = w[i] / total;
        else out[i] = active ? 1.0 / total : 0.0;
    }
}

}  // namespace

int geomed_chunks(byz_ctx* ctx, int64_t n_rows, int64_t n_cols, int64_t* chunk_cols) {
    const int64_t row_blocks = ceil_div(n_rows, kRowBlock);
    const int64_t target = static_cast<int64_t>(ctx->num_cus) * 8;       // workgroups of four waves: 32 waves per CU
    int64_t p = std::max<int64_t>(1, ceil_div(target, row_blocks));
    p = std::min<int64_t>({p, static_cast<int64_t>(kMaxChunks), ceil_div(n_cols, kWindow)});
    const int64_t chunk = ceil_div(ceil_div(n_cols, p), kWindow) * kWindow;
    *chunk_cols = chunk;
    return static_cast<int>(ceil_div(n_cols, chunk));
}

int launch_row_sqdist(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* z, double* partials,
                      double* sq, const int32_t* skip_if_set, const int32_t* run_if_set, hipStream_t stream) {
    BYZ_REQUIRE(G && partials && sq && n_rows > 0 && n_rows <= kLargeMaxRows && n_cols > 0 && ld >= n_cols,
                "row distances: bad arguments");
    int64_t chunk = 0;
    const int chunks = geomed_chunks(ctx, n_rows, n_cols, &chunk);
    const bool vec4 = (ld % 4 == 0) && aligned16(G) && (z == nullptr || aligned16(z));
    const dim3 grid(static_cast<unsigned>(ceil_div(n_rows, kRowBlock)), static_cast<unsigned>(chunks));
    KernelTimer t(ctx, BYZ_K_MISC, stream);
    if (vec4) rowsq_partial_kernel<true, kRowsqDist><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, z, chunk, partials, skip_if_set, run_if_set);
    else rowsq_partial_kernel<false, kRowsqDist><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, z, chunk, partials, skip_if_set, run_if_set);
    BYZ_TRY(check_launch("rowsq_partial_kernel"));
    rowsq_finish_kernel<<<static_cast<unsigned>(ceil_div(n_rows, 256)), 256, 0, stream>>>(partials, n_rows, chunks, sq, nullptr,
                                                                                        skip_if_set, run_if_set);
    return check_launch("rowsq_finish_kernel");
}

// dot[i] = x_i . r and sq[i] = |x_i|^2 in one read of G; partials: 2 * chunks * n_rows (geomed_chunks' chunks)
int launch_row_dots(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* r, double* partials,
                    double* dot, double* sq, hipStream_t stream) {
    BYZ_REQUIRE(G && r && partials && dot && sq && n_rows > 0 && n_rows <= kLargeMaxRows && n_cols > 0 && ld >= n_cols,
                "row dots: bad arguments");
    int64_t chunk = 0;
    const int chunks = geomed_chunks(ctx, n_rows, n_cols, &chunk);
    const bool vec4 = (ld % 4 == 0) && aligned16(G) && aligned16(r);
    const dim3 grid(static_cast<unsigned>(ceil_div(n_rows, kRowBlock)), static_cast<unsigned>(chunks));
    KernelTimer t(ctx, BYZ_K_MISC, stream);
    if (vec4) rowsq_partial_kernel<true, kRowsqDots><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, r, chunk, partials, nullptr, nullptr);
    else rowsq_partial_kernel<false, kRowsqDots><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, r, chunk, partials, nullptr, nullptr);
    BYZ_TRY(check_launch("rowsq_partial_kernel (dots)"));
    rowsq_finish_kernel<<<dim3(static_cast<unsigned>(ceil_div(n_rows, 256)), 2), 256, 0, stream>>>(partials, n_rows, chunks, dot, sq,
                                                                                                 nullptr, nullptr);
    return check_launch("rowsq_finish_kernel (dots)");
}

// a[i] = sum_c ((double)x_ic - (double)mu_c)^2 (launch_row_sqdist's bits) and b[i] = sum_c (double)p_c * ((double)mu_c - (double)x_ic)
// in one read of G; partials: 2 * chunks * n_rows (geomed_chunks' chunks)
int launch_row_moments(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* mu, const float* p,
                       double* partials, double* a, double* b, hipStream_t stream) {
    BYZ_REQUIRE(G && mu && p && partials && a && b && n_rows > 0 && n_rows <= kLargeMaxRows && n_cols > 0 && ld >= n_cols,
                "row moments: bad arguments");
    int64_t chunk = 0;
    const int chunks = geomed_chunks(ctx, n_rows, n_cols, &chunk);
    const bool vec4 = (ld % 4 == 0) && aligned16(G) && aligned16(mu) && aligned16(p);
    const dim3 grid(static_cast<unsigned>(ceil_div(n_rows, kRowBlock)), static_cast<unsigned>(chunks));
    KernelTimer t(ctx, BYZ_K_MISC, stream);
    if (vec4) rowsq_partial_kernel<true, kRowsqMoments><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, mu, chunk, partials, nullptr, nullptr, p);
    else rowsq_partial_kernel<false, kRowsqMoments><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, mu, chunk, partials, nullptr, nullptr, p);
    BYZ_TRY(check_launch("rowsq_partial_kernel (moments)"));
    rowsq_finish_kernel<<<dim3(static_cast<unsigned>(ceil_div(n_rows, 256)), 2), 256, 0, stream>>>(partials, n_rows, chunks, a, b,
                                                                                                 nullptr, nullptr);
    return check_launch("rowsq_finish_kernel (moments)");
}

// wmean (v == nullptr), centered clipping's update (v: the centre) or FLTrust's sum (divisor: one device double); one launch
// shape for the three
static int launch_weighted_rows(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* v,
                                const double* w, const double* divisor, float* out, const int32_t* skip_if_set,
                                const int32_t* run_if_set, const char* who, hipStream_t stream) {
    BYZ_REQUIRE(G && w && out && n_rows > 0 && n_rows <= kLargeMaxRows && n_cols > 0 && ld >= n_cols, "%s: bad arguments", who);
    WalkShape shape;
    BYZ_TRY(walk_shape(ctx, G, ld, n_cols, who, &shape));
    const unsigned blocks = static_cast<unsigned>(shape.blocks);
    KernelTimer t(ctx, BYZ_K_MISC, stream);
#define BYZ_WEIGHTED_ROWS(VEC, MODE) \
    weighted_rows_kernel<VEC, MODE><<<blocks, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, v, w, divisor, out, skip_if_set, run_if_set)
    if (v != nullptr) {
        if (shape.vec4) BYZ_WEIGHTED_ROWS(4, kRowsCentred); else BYZ_WEIGHTED_ROWS(1, kRowsCentred);
    } else if (divisor != nullptr) {
        if (shape.vec4) BYZ_WEIGHTED_ROWS(4, kRowsScaled); else BYZ_WEIGHTED_ROWS(1, kRowsScaled);
    } else {
        if (shape.vec4) BYZ_WEIGHTED_ROWS(4, kRowsMean); else BYZ_WEIGHTED_ROWS(1, kRowsMean);
    }
#undef BYZ_WEIGHTED_ROWS
    return check_launch("weighted_rows_kernel");
}

int launch_weighted_mean(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const double* w, float* out,
                         const int32_t* skip_if_set, const int32_t* run_if_set, hipStream_t stream) {
    return launch_weighted_rows(ctx, G, n_rows, n_cols, ld, nullptr, w, nullptr, out, skip_if_set, run_if_set, "weighted mean",
                                stream);
}

int launch_clip_update(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* v, const double* s,
                       float* out, hipStream_t stream) {
    BYZ_REQUIRE(v, "clip update: bad arguments");
    return launch_weighted_rows(ctx, G, n_rows, n_cols, ld, v, s, nullptr, out, nullptr, nullptr, "clip update", stream);
}

int launch_scaled_rows_sum(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const double* w,
                           const double* divisor, float* out, hipStream_t stream) {
    BYZ_REQUIRE(divisor, "scaled rows sum: bad arguments");
    return launch_weighted_rows(ctx, G, n_rows, n_cols, ld, nullptr, w, divisor, out, nullptr, nullptr, "scaled rows sum", stream);
}

int launch_geomed_finite_check(byz_ctx* ctx, const float* v, int64_t n, double* flag_f64, hipStream_t stream) {
    finite_check_kernel<<<static_cast<unsigned>(ceil_div(n, 256)), 256, 0, stream>>>(v, n, &device_scalars(ctx)->geomed, flag_f64);
    return check_launch("finite_check_kernel");
}

int launch_geomed_fallback(byz_ctx* ctx, const double* sq0, int64_t n, double* w, const double* global_flag, hipStream_t stream) {
    geomed_fallback_kernel<<<1, kStepThreads, 0, stream>>>(sq0, n, w, &device_scalars(ctx)->geomed, global_flag);
    return check_launch("geomed_fallback_kernel");
}

int launch_geomed_step(byz_ctx* ctx, const double* sq, int64_t n, double* w, double nu, double ftol, int64_t k, int64_t max_iter,
                       hipStream_t stream) {
    geomed_step_kernel<<<1, kStepThreads, 0, stream>>>(sq, n, w, &device_scalars(ctx)->geomed, nu, ftol, k, max_iter);
    return check_launch("geomed_step_kernel");
}

int launch_geomed_weights(byz_ctx* ctx, const double* w, int64_t n, double* out, hipStream_t stream) {
    geomed_weights_kernel<<<1, kStepThreads, 0, stream>>>(w, n, &device_scalars(ctx)->geomed, out);
    return check_launch("geomed_weights_kernel");
}

}  // namespace byz
