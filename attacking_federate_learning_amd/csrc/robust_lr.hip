// The robust learning rate (Ozdayi, Kantarcioglu and Gel, "Defending against Backdoors in Federated Learning with Robust Learning
// Rate", AAAI 2021; beyond the reference): a per-coordinate sign vote over the clients' updates, and the aggregate's sign
// inverted where the vote is weak.  HBM-bound streaming kernels, like column_stats.hip's.
//
//   votes[c] = #{ r : G[r][c] > 0 } - #{ r : G[r][c] < 0 }                                  int32
//   out[c]   = |votes[c]| < theta ? agg[c] with its sign bit inverted : agg[c] verbatim
//
// The vote of a value is decided on its BITS with integer comparisons (sign bit; magnitude in (0, 0x7f800000]): +0.0, -0.0 and
// NaN cast no vote, +-inf and denormals vote by their sign, whatever the denormal mode of the floating-point unit.  The flip is
// an XOR of the sign bit: a zero becomes -0.0, a NaN keeps its payload, nothing is sanitised.
// One thread owns VEC columns and walks the rows (walk_rows, row_walk.hpp) with VEC int32 counters.  FUSED: the same walk also
// runs column_sequential_kernel<VEC, 0>'s chain (sequential fp32 from +0.0 in row order, then / float(n)), so out is
// no_defense's vector with the flips applied and the matrix is read once.
// This file is compiled with -ffp-contract=off, as column_stats.hip is (the chain has no multiply today; the flag keeps it so).
// Algorithmic traffic: 4*rows*cols bytes read + 4*cols (+ 4*cols for the votes) written.
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kThreads = kWalkThreads;
constexpr uint32_t kSignBit = 0x80000000u;
constexpr uint32_t kInfBits = 0x7f800000u;

// +1, -1 or 0: the vote of the value with these bits
__device__ __forceinline__ int32_t vote_of(float x) {
    const uint32_t u = __float_as_uint(x);
    const uint32_t mag = u & ~kSignBit;
    const bool votes = mag - 1u < kInfBits;                 // 0 < mag <= 0x7f800000 (mag = 0 wraps to the top)
    return votes ? (static_cast<int32_t>(u) >> 31) | 1 : 0;
}

__device__ __forceinline__ bool weak(int32_t votes, int32_t theta) { return (votes < 0 ? -votes : votes) < theta; }

__device__ __forceinline__ float flipped(float x) { return __uint_as_float(__float_as_uint(x) ^ kSignBit); }

// the workgroup's flipped columns into the device counter: a fixed tree over the workgroup, one integer atomic per workgroup
// (integer additions commute: the total does not depend on the order of the workgroups)
__device__ __forceinline__ void count_flips(int32_t mine, unsigned long long* __restrict__ counter) {
    __shared__ int32_t lds[kThreads];
    const int32_t total = block_sum<int32_t, kThreads>(mine, lds);
    if (threadIdx.x == 0 && total != 0) atomicAdd(counter, static_cast<unsigned long long>(total));
}

// votes (optional with FUSED): n_cols int32.  out (FUSED only): n_cols fp32.  theta = 0: nothing can flip and nothing is counted.
template <int VEC, bool FUSED>
__global__ __launch_bounds__(kThreads) void sign_votes_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols, int64_t ld,
                                                              int32_t theta, float* __restrict__ out, int32_t* __restrict__ votes,
                                                              unsigned long long* __restrict__ flip_counter) {
    const int64_t c0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * VEC;
    int32_t flips = 0;
    if (c0 < n_cols) {      // (no early return: the whole workgroup meets in count_flips)
        int32_t k[VEC];
        float s[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            k[v] = 0;
            s[v] = 0.0f;
        }
        walk_rows<VEC>(
            G + c0, ld, n_rows, c0, n_cols, [](int64_t r) __attribute__((always_inline)) { return r; },
            [](int64_t) __attribute__((always_inline)) { return true; },
            [&](int64_t, bool, const float(&x)[VEC]) __attribute__((always_inline)) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if constexpr (FUSED) s[v] = s[v] + x[v];
                    k[v] += vote_of(x[v]);      // (a masked column of the last vector reads +0.0: no vote)
                    // one value's vote is counted before the next is begun: left to itself the scheduler interleaves the
                    // integer work of a whole run of rows and holds its temporaries all at once (80 VGPRs and 6 waves per SIMD in the fused four-wide kernel; 66 and 7 with this)
                    asm volatile("" : "+v"(k[v]));
                }
            });
        const float rows_f = static_cast<float>(n_rows);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            if (c0 + v >= n_cols) continue;
            const bool flip = weak(k[v], theta);
            flips += flip ? 1 : 0;
            if constexpr (FUSED) {
                const float mean = s[v] / rows_f;
                out[c0 + v] = flip ? flipped(mean) : mean;
            }
            if (votes != nullptr) votes[c0 + v] = k[v];
        }
    }
    if (theta > 0) count_flips(flips, flip_counter);
}

// out[c] = |votes[c]| < theta ? agg[c] ^ sign bit : agg[c]; out may be agg (no __restrict__ on the two)
__global__ __launch_bounds__(kThreads) void sign_flip_kernel(const float* agg, const int32_t* __restrict__ votes, int64_t n_cols,
                                                             int32_t theta, float* out, unsigned long long* __restrict__ flip_counter) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    int32_t flips = 0;
    if (c < n_cols) {
        const bool flip = weak(votes[c], theta);
        const float a = agg[c];
        out[c] = flip ? flipped(a) : a;
        flips = flip ? 1 : 0;
    }
    if (theta > 0) count_flips(flips, flip_counter);
}

}  // namespace

// out == nullptr: the votes alone (votes required); otherwise the fused call (votes optional).  0 <= theta <= n_rows is the
// caller's business.  The counter is zeroed on the stream in front of the kernel.
int launch_sign_votes(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t theta, float* out,
                      int32_t* votes, hipStream_t stream) {
    BYZ_REQUIRE(G && n_rows > 0 && n_cols > 0 && ld >= n_cols, "sign votes: bad shape %lld x %lld ld %lld", (long long)n_rows,
                (long long)n_cols, (long long)ld);
    BYZ_REQUIRE(out || votes, "sign votes: neither an output vector nor a vote vector");
    BYZ_REQUIRE(theta >= 0 && theta <= n_rows && n_rows <= kLargeMaxRows, "sign votes: theta %lld outside 0..%lld", (long long)theta,
                (long long)n_rows);
    WalkShape shape;
    BYZ_TRY(walk_shape(ctx, G, ld, n_cols, "sign votes", &shape));
    unsigned long long* counter = &device_scalars(ctx)->rlr.flipped;
    BYZ_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), stream));
    const dim3 grid(static_cast<unsigned>(shape.blocks));
    const int32_t th = static_cast<int32_t>(theta);
    KernelTimer t(ctx, BYZ_K_COLUMN_STATS, stream);
    if (out != nullptr) {
        if (shape.vec4) sign_votes_kernel<4, true><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, th, out, votes, counter);
        else sign_votes_kernel<1, true><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, th, out, votes, counter);
    } else {
        if (shape.vec4) sign_votes_kernel<4, false><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, th, nullptr, votes, counter);
        else sign_votes_kernel<1, false><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, th, nullptr, votes, counter);
    }
    return check_launch("sign_votes_kernel");
}

int launch_sign_flip(byz_ctx* ctx, const float* agg, const int32_t* votes, int64_t n_cols, int64_t theta, float* out,
                     hipStream_t stream) {
    BYZ_REQUIRE(agg && votes && out && n_cols > 0, "sign flip: null vector or no columns");
    BYZ_REQUIRE(theta >= 0 && theta <= kLargeMaxRows, "sign flip: theta %lld outside 0..%lld", (long long)theta, (long long)kLargeMaxRows);
    const int64_t blocks = ceil_div(n_cols, kThreads);
    if (blocks >= (int64_t{1} << 31)) {
        set_error("sign flip: %lld columns is beyond one launch", (long long)n_cols);
        return BYZ_E_UNSUPPORTED;
    }
    unsigned long long* counter = &device_scalars(ctx)->rlr.flipped;
    BYZ_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned long long), stream));
    KernelTimer t(ctx, BYZ_K_MISC, stream);
    sign_flip_kernel<<<static_cast<unsigned>(blocks), kThreads, 0, stream>>>(agg, votes, n_cols, static_cast<int32_t>(theta), out, counter);
    return check_launch("sign_flip_kernel");
}

}  // namespace byz
