// Centered clipping (Karimireddy, He and Jaggi, "Learning from History for Byzantine Robust Optimization", ICML 2021,
// Algorithm 2): v <- v + (1/n) sum_i (x_i - v) min(1, tau / |x_i - v|).  Streaming passes over G, nothing of order N^2.
//
//   scales  one workgroup: d_i = sqrt(sq_i), s_i = 1 (d_i <= tau), tau / d_i (tau < d_i < inf), 0 (d_i not finite: the row is
//           excluded); the clipped and excluded counts go to the context's small area (common.hpp).
//   update  out[c] = fl32((double)v[c] + S_c / n), S_c = sum over the rows with s_i != 0 of s_i * ((double)x_ic - (double)v[c]),
//           sequential in row order, no fused multiply-add; a row of scale 0 is neither loaded nor multiplied.  It is the
//           weighted mean's kernel template with another product (weighted_rows_kernel<VEC, kRowsCentred>, geomed.hip, where
//           launch_clip_update lives beside launch_weighted_mean).
// One iteration is launch_row_sqdist (geomed.hip, reused as it is), scales, update: two passes over G.
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kStepThreads = 1024;

// sq == nullptr: no iteration ran, every scale is 1 and both counts 0
__global__ __launch_bounds__(kStepThreads) void cclip_scales_kernel(const double* __restrict__ sq, int64_t n, double tau,
                                                                    double* __restrict__ s, int32_t* words) {
    __shared__ int lds[kStepThreads];
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
            }
        }
        s[i] = scale;
    }
    const int c = block_sum<int, kStepThreads>(clipped, lds);
    const int e = block_sum<int, kStepThreads>(excluded, lds);
    if (threadIdx.x == 0) {
        words[kCclipClipped] = c;
        words[kCclipExcluded] = e;
    }
}

}  // namespace

int launch_cclip_scales(byz_ctx* ctx, const double* sq, int64_t n, double tau, double* s, hipStream_t stream) {
    BYZ_REQUIRE(s && n > 0 && n <= kLargeMaxRows, "clip scales: bad arguments");
    cclip_scales_kernel<<<1, kStepThreads, 0, stream>>>(sq, n, tau, s, geomed_words(ctx));
    return check_launch("cclip_scales_kernel");
}

}  // namespace byz
