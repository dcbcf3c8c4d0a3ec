// Centered clipping (Karimireddy, He and Jaggi, "Learning from History for Byzantine Robust Optimization", ICML 2021,
// Algorithm 2): v <- v + (1/n) sum_i (x_i - v) min(1, tau / |x_i - v|).  Streaming passes over G, nothing of order N^2.
//
//   scales  one workgroup: d_i = sqrt(sq_i), s_i = 1 (d_i <= tau), tau / d_i (tau < d_i < inf), 0 (d_i not finite: the row is
//           excluded); the clipped and excluded counts go to the context's report (device_scalars.hpp).
//   update  out[c] = fl32((double)v[c] + S_c / n), S_c = sum over the rows with s_i != 0 of s_i * ((double)x_ic - (double)v[c]),
//           sequential in row order, no fused multiply-add; a row of scale 0 is neither loaded nor multiplied.  It is the
//           weighted mean's kernel template with another product (weighted_rows_kernel<VEC, kRowsCentred>, geomed.hip, where
//           launch_clip_update lives beside launch_weighted_mean).
// One iteration is launch_row_sqdist (geomed.hip, reused as it is), scales, update: two passes over G.
// Weak DP's clipping piece (byz_clip_scales_dev) is the same scales kernel with another clip: fixed, or the np.median of the
// finite rows' norms (FLAME's adaptive bound), found by SignGuard's key-and-sort route (order_keys.hpp: norm_key,
// median_of_norm_keys; segment_sort_u64) and read by the scales' workgroup off the sorted keys.
#include "order_keys.hpp"
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kStepThreads = 1024;

// keys[i] = the norm's order-preserving key; a row whose q is not finite, and the padding: all ones, behind every norm
__global__ __launch_bounds__(256) void clip_norm_keys_kernel(const double* __restrict__ sq, int64_t n, int64_t n_pad,
                                                             unsigned long long* __restrict__ keys) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n_pad) keys[i] = i < n ? norm_key(sq[i]) : kNoNormKey;
}

// sq == nullptr: no iteration ran, every scale is 1 and both counts 0.  sorted_keys != nullptr (n_pad of them): tau is the
// median of the finite norms instead (0 when no row is finite; a clip of 0 leaves every scale 0).  clipped_out, excluded_out:
// the report's counts; clip_word, clip_out (optional): the clip used.
__global__ __launch_bounds__(kStepThreads) void cclip_scales_kernel(const double* __restrict__ sq, int64_t n, double tau,
                                                                    const unsigned long long* __restrict__ sorted_keys,
                                                                    int64_t n_pad, double* __restrict__ s, int32_t* clipped_out,
                                                                    int32_t* excluded_out, double* clip_word, double* clip_out) {
    __shared__ int lds[kStepThreads];
    if (sorted_keys != nullptr) {
        int finite = 0;
        for (int64_t i = threadIdx.x; i < n_pad; i += kStepThreads) finite += sorted_keys[i] != kNoNormKey ? 1 : 0;
        finite = block_sum<int, kStepThreads>(finite, lds);
        tau = finite > 0 ? median_of_norm_keys(sorted_keys, finite) : 0.0;
    }
    int clipped = 0, excluded = 0;
    for (int64_t i = threadIdx.x; i < n; i += kStepThreads) {
        double scale = 1.0;
        if (sq != nullptr) {
            const double d = sqrt(sq[i]);
            if (!__builtin_isfinite(d)) {
                scale = 0.0;
                ++excluded;
            } else if (d > tau) {
                scale = tau / d;
                ++clipped;
            } else if (tau == 0.0) {
                scale = 0.0;
            }
        }
        s[i] = scale;
    }
    const int c = block_sum<int, kStepThreads>(clipped, lds);
    const int e = block_sum<int, kStepThreads>(excluded, lds);
    if (threadIdx.x == 0) {
        *clipped_out = c;
        *excluded_out = e;
        if (clip_word != nullptr) *clip_word = tau;
        if (clip_out != nullptr) *clip_out = tau;
    }
}

}  // namespace

int launch_cclip_scales(byz_ctx* ctx, const double* sq, int64_t n, double tau, double* s, hipStream_t stream) {
    BYZ_REQUIRE(s && n > 0 && n <= kLargeMaxRows, "clip scales: bad arguments");
    CclipReport* r = &device_scalars(ctx)->cclip;
    cclip_scales_kernel<<<1, kStepThreads, 0, stream>>>(sq, n, tau, nullptr, 0, s, &r->clipped, &r->excluded, nullptr, nullptr);
    return check_launch("cclip_scales_kernel");
}

// weak DP's scales: adaptive = false: the clip is `clip` and s has launch_cclip_scales' bits; adaptive = true: the median of the
// finite norms.  The counts and the clip go to the context's weak-DP report, the clip to clip_out as well (optional).
int launch_clip_scales(byz_ctx* ctx, const double* sq, int64_t n, double clip, bool adaptive, double* s, double* clip_out,
                       hipStream_t stream) {
    BYZ_REQUIRE(sq && s && n > 0 && n <= kLargeMaxRows, "clip scales: bad arguments");
    unsigned long long* keys = nullptr;
    const int64_t n_pad = n < 2 ? 2 : next_pow2(n);            // segment_sort_u64 takes two keys at least
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    if (adaptive) {
        Carve c;
        c.take(&keys, n_pad);
        BYZ_TRY(c.commit(ctx->weak_dp));
        clip_norm_keys_kernel<<<static_cast<unsigned>(ceil_div(n_pad, 256)), 256, 0, stream>>>(sq, n, n_pad, keys);
        BYZ_TRY(check_launch("clip_norm_keys_kernel"));
        BYZ_TRY(segment_sort_u64(ctx, keys, 1, n_pad, stream));
    }
    WeakDpReport* r = &device_scalars(ctx)->weak_dp;
    cclip_scales_kernel<<<1, kStepThreads, 0, stream>>>(sq, n, clip, keys, n_pad, s, &r->clipped, &r->excluded, &r->clip, clip_out);
    return check_launch("cclip_scales_kernel");
}

}  // namespace byz
