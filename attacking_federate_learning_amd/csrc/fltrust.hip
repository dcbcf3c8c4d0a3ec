// FLTrust (Cao, Fang, Liu and Gong, "FLTrust: Byzantine-robust Federated Learning via Trust Bootstrapping", NDSS 2021): every
// row is compared with the gradient r the server computed on its own root dataset.  The trust score is the ReLU of the
// cosine, a trusted row is rescaled to the root's norm, and the aggregate is the trust-weighted mean of the rescaled rows.
// Two streaming passes over G, nothing of order N^2.
//
//   dots    p_i = x_i . r and q_i = |x_i|^2 in one read of G: rowsq's kernel template with two accumulators a row
//           (rowsq_partial_kernel<VEC4, kRowsqDots>, geomed.hip, where launch_row_dots lives beside launch_row_sqdist);
//           q0 = |r|^2 is launch_row_sqdist on the 1 x n_cols matrix r.
//   trust   one workgroup, here: c_i = p_i / (sqrt(q_i) * sqrt(q0)), ts_i = max(c_i, 0), w_i = ts_i * (sqrt(q0) / sqrt(q_i)),
//           T = sum ts_i in a fixed order; T and the counts go to the context's report (device_scalars.hpp).
//   sum     out[c] = T > 0 ? fl32(S_c / T) : 0, S_c = sum over the rows with w_i != 0 of w_i * (double)x_ic, sequential in row
//           order, no fused multiply-add; a row of weight 0 is neither loaded nor multiplied.  The weighted mean's kernel
//           template with another last line (weighted_rows_kernel<VEC, kRowsScaled>, geomed.hip: launch_scaled_rows_sum).
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kStepThreads = 1024;

// pq: p (n), q (n), q0 (1).  A thread takes a run of consecutive rows; T is the threads' sums through block_sum's tree.
__global__ __launch_bounds__(kStepThreads) void fltrust_trust_kernel(const double* __restrict__ pq, int64_t n,
                                                                     double* __restrict__ ts, double* __restrict__ w,
                                                                     FltrustReport* r) {
    __shared__ double lds[kStepThreads];
    __shared__ int lds_i[kStepThreads];
    const double q0 = pq[2 * n];
    const bool root_ok = __builtin_isfinite(q0) && q0 > 0.0;
    const double root_norm = sqrt(q0);
    const int64_t per = (n + kStepThreads - 1) / kStepThreads;
    const int64_t lo = threadIdx.x * per < n ? threadIdx.x * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    double t_sum = 0.0;
    int trusted = 0, excluded = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const double p = pq[i], q = pq[n + i];
        const bool finite = __builtin_isfinite(p) && __builtin_isfinite(q);
        const bool usable = finite && q > 0.0;
        const double norm = sqrt(usable ? q : 1.0);
        const double c = p / (norm * root_norm);
        const double t = root_ok && usable && c > 0.0 ? c : 0.0;
        ts[i] = t;
        w[i] = t != 0.0 ? t * (root_norm / norm) : 0.0;
        t_sum = t_sum + t;
        if (t > 0.0) ++trusted;
        if (!finite) ++excluded;
    }
    const double T = block_sum<double, kStepThreads>(t_sum, lds);
    const int n_trusted = block_sum<int, kStepThreads>(trusted, lds_i);
    const int n_excluded = block_sum<int, kStepThreads>(excluded, lds_i);
    if (threadIdx.x == 0) {
        r->trusted = n_trusted;
        r->excluded = n_excluded;
        r->root_ok = root_ok ? 1 : 0;
        r->trust_sum = T;
    }
}

}  // namespace

int launch_fltrust_trust(byz_ctx* ctx, const double* pq, int64_t n, double* ts, double* w, hipStream_t stream) {
    BYZ_REQUIRE(pq && ts && w && n > 0 && n <= kLargeMaxRows, "trust scores: bad arguments");
    fltrust_trust_kernel<<<1, kStepThreads, 0, stream>>>(pq, n, ts, w, &device_scalars(ctx)->fltrust);
    return check_launch("fltrust_trust_kernel");
}

}  // namespace byz
