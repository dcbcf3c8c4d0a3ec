// Centered clipping (Karimireddy, He and Jaggi, "Learning from History for Byzantine Robust Optimization", ICML 2021,
// Algorithm 2): v <- v + (1/n) sum_i (x_i - v) min(1, tau / |x_i - v|).  Streaming passes over G, nothing of order N^2.
//
//   scales  one workgroup: d_i = sqrt(sq_i), s_i = 1 (d_i <= tau), tau / d_i (tau < d_i < inf), 0 (d_i not finite: the row is
//           excluded); the clipped and excluded counts go to the context's small area (common.hpp).
//   update  out[c] = fl32((double)v[c] + S_c / n), S_c = sum over the rows with s_i != 0 of s_i * ((double)x_ic - (double)v[c]),
//           sequential in row order, no fused multiply-add (this file is compiled with -ffp-contract=off).  One thread walks the
//           rows for VEC columns as wmean_kernel does; the scales are uniform and arrive through scalar loads; a row of scale 0
//           is neither loaded nor multiplied.
// One iteration is launch_row_sqdist (geomed.hip, reused as it is), scales, update: two passes over G.
#include "common.hpp"

namespace byz {
namespace {

constexpr int kThreads = 256;
constexpr int kRowRun = 8;                          // update: rows whose loads are issued together
constexpr int kStepThreads = 1024;

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// fixed-order sum over one workgroup of kStepThreads threads (every thread gets the total)
__device__ int block_sum_i32(int v, int* lds) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int step = kStepThreads / 2; step >= 1; step >>= 1) {
        if (tid < step) lds[tid] = lds[tid] + lds[tid + step];
        __syncthreads();
    }
    const int total = lds[0];
    __syncthreads();
    return total;
}

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
    const int c = block_sum_i32(clipped, lds);
    const int e = block_sum_i32(excluded, lds);
    if (threadIdx.x == 0) {
        words[kCclipClipped] = c;
        words[kCclipExcluded] = e;
    }
}

template <int VEC>
__device__ __forceinline__ void load_cols(const float* __restrict__ p, bool full, int64_t c0, int64_t n_cols, float (&x)[VEC]) {
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

// v and out may be the same buffer: a thread reads its own columns of v before it writes them
template <int VEC>
__global__ __launch_bounds__(kThreads) void clip_update_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols,
                                                               int64_t ld, const float* v, const double* __restrict__ s,
                                                               float* out) {
    const int64_t c0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * VEC;
    if (c0 >= n_cols) return;
    const bool full = c0 + VEC <= n_cols;
    const float* p = G + c0;
    double vd[VEC], acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        vd[k] = c0 + k < n_cols ? static_cast<double>(v[c0 + k]) : 0.0;
        acc[k] = 0.0;
    }
    int64_t r = 0;
    for (; r + kRowRun <= n_rows; r += kRowRun) {
        double sr[kRowRun];
#pragma unroll
        for (int u = 0; u < kRowRun; ++u) sr[u] = s[r + u];          // uniform: one scalar load for the run
        float x[kRowRun][VEC];
#pragma unroll
        for (int u = 0; u < kRowRun; ++u) {
            if (sr[u] != 0.0) load_cols<VEC>(p + (r + u) * ld, full, c0, n_cols, x[u]);
        }
#pragma unroll
        for (int u = 0; u < kRowRun; ++u) {
            if (sr[u] != 0.0) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + sr[u] * (static_cast<double>(x[u][k]) - vd[k]);
            }
        }
    }
    for (; r < n_rows; ++r) {
        const double su = s[r];
        if (su != 0.0) {
            float x[VEC];
            load_cols<VEC>(p + r * ld, full, c0, n_cols, x);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + su * (static_cast<double>(x[k]) - vd[k]);
        }
    }
    const double count = static_cast<double>(n_rows);
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        if (c0 + k < n_cols) out[c0 + k] = static_cast<float>(vd[k] + acc[k] / count);
}

}  // namespace

int launch_cclip_scales(byz_ctx* ctx, const double* sq, int64_t n, double tau, double* s, hipStream_t stream) {
    BYZ_REQUIRE(s && n > 0 && n <= kLargeMaxRows, "clip scales: bad arguments");
    cclip_scales_kernel<<<1, kStepThreads, 0, stream>>>(sq, n, tau, s, geomed_words(ctx));
    return check_launch("cclip_scales_kernel");
}

int launch_clip_update(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* v, const double* s,
                       float* out, hipStream_t stream) {
    BYZ_REQUIRE(G && v && s && out && n_rows > 0 && n_rows <= kLargeMaxRows && n_cols > 0 && ld >= n_cols,
                "clip update: bad arguments");
    // launch_weighted_mean's rule: 16-byte loads when every row starts 16-byte aligned and the columns alone fill the chip
    const bool vec4 = (ld % 4 == 0) && aligned16(G) && n_cols >= static_cast<int64_t>(4) * kThreads * ctx->num_cus * 2;
    const int64_t blocks = ceil_div(n_cols, static_cast<int64_t>(kThreads) * (vec4 ? 4 : 1));
    if (blocks >= (int64_t{1} << 31)) {
        set_error("clip update: %lld columns is beyond one launch", (long long)n_cols);
        return BYZ_E_UNSUPPORTED;
    }
    KernelTimer t(ctx, BYZ_K_MISC, stream);
    if (vec4) clip_update_kernel<4><<<static_cast<unsigned>(blocks), kThreads, 0, stream>>>(G, n_rows, n_cols, ld, v, s, out);
    else clip_update_kernel<1><<<static_cast<unsigned>(blocks), kThreads, 0, stream>>>(G, n_rows, n_cols, ld, v, s, out);
    return check_launch("clip_update_kernel");
}

}  // namespace byz
