// Gaussian noise on a vector from the Philox stream (philox.hpp): the noise half of "weak DP" (Sun, Kairouz, Suresh and McMahan,
// "Can You Really Backdoor Federated Learning?", 2019), of FLAME's last stage (Nguyen et al., USENIX Security 2022) and of
// DP-FedAvg's server step; beyond the reference.
//
//   out[c] = fl32((double)x[c] + sigma_eff * z[column_offset + c]),     sigma_eff = sigma * (scale_dev ? *scale_dev : 1.0)
//
// z is addressed by GLOBAL column, so the vector is the same for one call, a misaligned caller and any split of the columns over
// ranks.  One thread owns one Philox block, the four consecutive global columns 4 b .. 4 b + 3, cut to the caller's
// [column_offset, column_offset + n): one generator call and two Box-Muller pairs per four outputs.  A whole block is one dwordx4
// load and store when the first whole block's address is 16-byte aligned in x and in out (VEC = 4); the head and tail blocks,
// and every block of the scalar instantiation, are predicated per column and never touch anything outside [0, n).
// sigma_eff is read on the device: the adaptive mode's clip needs no host synchronisation.  A thread reads its columns before
// it writes them, so out may be x.  A NaN or an infinity in x stays where it is; nothing is sanitised.
// Grid-stride over the blocks, no LDS, no atomics.  gaussian_words_kernel writes the raw words instead (the integer-exact tests).
#include "philox.hpp"
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kThreads = kWalkThreads;
constexpr int kBlocksPerCu = 8;          // 32 waves a CU: the grid is sized from the chip, never from n alone

typedef float float4a __attribute__((ext_vector_type(4)));       // naturally (16-byte) aligned: the VEC = 4 path proved it

struct NoiseStream {
    uint64_t seed, round;
    int64_t offset;       // the global column of the caller's column 0
};

// x and out carry no __restrict__: out may be x
template <int VEC>
__global__ __launch_bounds__(kThreads) void gaussian_noise_kernel(const float* x, int64_t n, NoiseStream a, double sigma,
                                                                  const double* __restrict__ scale_dev, float* out) {
    const double sigma_eff = sigma * (scale_dev != nullptr ? *scale_dev : 1.0);
    const int64_t head = a.offset & 3;                                   // columns of the first block in front of the caller's
    const uint64_t b0 = static_cast<uint64_t>(a.offset) >> 2;
    const int64_t n_blocks = (head + n + 3) >> 2;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; j < n_blocks; j += stride) {
        const int64_t c0 = 4 * j - head;                                 // the caller's column of the block's word 0 (< 0: the head)
        uint32_t w[4];
        philox_block(a.seed, a.round, b0 + static_cast<uint64_t>(j), w);
        double z[4];
        philox_normals(w, z);
        const bool whole = c0 >= 0 && c0 + 4 <= n;
        float v[4];
        if (VEC == 4 && whole) {
            const float4a q = *reinterpret_cast<const float4a*>(x + c0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (c0 + i >= 0 && c0 + i < n) ? x[c0 + i] : 0.0f;
        }
        float y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = static_cast<float>(static_cast<double>(v[i]) + sigma_eff * z[i]);
        if (VEC == 4 && whole) {
            float4a q;
            q.x = y[0]; q.y = y[1]; q.z = y[2]; q.w = y[3];
            *reinterpret_cast<float4a*>(out + c0) = q;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c0 + i >= 0 && c0 + i < n) out[c0 + i] = y[i];
        }
    }
}

// the raw stream: words[c] = the word of global column offset + c
__global__ __launch_bounds__(kThreads) void gaussian_words_kernel(int64_t n, NoiseStream a, uint32_t* __restrict__ words) {
    const int64_t head = a.offset & 3;
    const uint64_t b0 = static_cast<uint64_t>(a.offset) >> 2;
    const int64_t n_blocks = (head + n + 3) >> 2;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; j < n_blocks; j += stride) {
        const int64_t c0 = 4 * j - head;
        uint32_t w[4];
        philox_block(a.seed, a.round, b0 + static_cast<uint64_t>(j), w);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (c0 + i >= 0 && c0 + i < n) words[c0 + i] = w[i];
    }
}

unsigned noise_grid(byz_ctx* ctx, int64_t n, int64_t offset) {
    const int64_t n_blocks = ((offset & 3) + n + 3) >> 2;
    const int64_t want = ceil_div(n_blocks, kThreads), most = static_cast<int64_t>(kBlocksPerCu) * ctx->num_cus;
    return static_cast<unsigned>(want < most ? want : most);
}

}  // namespace

// 1 <= n, 0 <= offset, offset + n <= 2^62, sigma finite and >= 0 and the overlaps are the caller's business (api.hip)
int launch_gaussian_noise(byz_ctx* ctx, const float* x, int64_t n, double sigma, uint64_t seed, uint64_t round, int64_t offset,
                          const double* scale_dev, float* out, hipStream_t stream) {
    const NoiseStream a = {seed, round, offset};
    const int64_t first_whole = (4 - (offset & 3)) & 3;       // the caller's column at which the first whole block starts
    const bool vec4 = aligned16(x + first_whole) && aligned16(out + first_whole);
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    if (vec4) gaussian_noise_kernel<4><<<noise_grid(ctx, n, offset), kThreads, 0, stream>>>(x, n, a, sigma, scale_dev, out);
    else gaussian_noise_kernel<1><<<noise_grid(ctx, n, offset), kThreads, 0, stream>>>(x, n, a, sigma, scale_dev, out);
    return check_launch("gaussian_noise_kernel");
}

int launch_noise_words(byz_ctx* ctx, uint64_t seed, uint64_t round, int64_t offset, int64_t n, uint32_t* words, hipStream_t stream) {
    const NoiseStream a = {seed, round, offset};
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    gaussian_words_kernel<<<noise_grid(ctx, n, offset), kThreads, 0, stream>>>(n, a, words);
    return check_launch("gaussian_words_kernel");
}

}  // namespace byz
