// The AGR-agnostic attacks of Shejwalkar and Houmansadr, "Manipulating the Byzantine: Optimizing Model Poisoning Attacks and
// Defenses for Federated Learning" (NDSS 2021, section IV-C): Min-Max and Min-Sum; beyond the reference.  Every attacker row
// becomes the ONE vector mal = mu + gamma p, with the largest gamma that keeps mal as close to every known row as the known rows
// are to each other (Min-Max: in the largest distance; Min-Sum: in the sum of squared distances).  include/byzagg.h states the
// rule operation for operation; the search of the paper's Algorithm 1 is a closed form here (minmax_solve.hpp):
//     |mal - g_i|^2 = a_i + 2 gamma b_i + gamma^2 c,   a_i = |g_i - mu|^2,  b_i = p . (mu - g_i),  c = |p|^2,
// so one pass over G gives every row's quadratic (rowsq_partial_kernel's moments form, geomed.hip) and gamma is the smallest of r
// roots (Min-Max) or one root (Min-Sum: sum_j |g_i - g_j|^2 = r a_i + sum_j a_j about the rows' mean, no n x n table).
//   perturbation_kernel   p from mu, sigma and |mu|^2 (read from the device): unit, std or sign
//   dist_max_kernel       the largest finite entry of the known block of the distance matrix, diagonal skipped: a workgroup's
//                         maximum a launch, a second launch over the workgroups' values; no atomics, one value
//   minmax_solve_kernel   one workgroup: the rows' roots, their minimum and its lowest row (owner_loop.hpp's block_exchange), or
//                         Min-Sum's max a_i and the two sums in row order; gamma and the report into the typed scalar block
//   minmax_fill_kernel    one thread per four columns forms fl32(mu + gamma p) once and writes it into every attacker row;
//                         it reads gamma and the broken flag from the report: a broken call leaves the rows as they were
// This file is compiled with -ffp-contract=off: gamma * p is rounded before it is added, numpy reproduces the rows as bits.
#include "common.hpp"
#include "lane_exchange.hpp"
#include "minmax_solve.hpp"
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kThreads = kWalkThreads;
constexpr int kBlocksPerCu = 8;          // the fill's grid: 32 waves a CU, sized from the chip
constexpr int kMaxPartials = 1024;       // workgroups of the distance maximum's first launch at most

typedef float float4a __attribute__((ext_vector_type(4)));       // naturally (16-byte) aligned: the VEC = 4 path proved it

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(kThreads) void perturbation_kernel(const float* __restrict__ mu, const float* __restrict__ sigma,
                                                                const double* __restrict__ norm_sq, int kind, int64_t n_cols,
                                                                float* __restrict__ p) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (j >= n_cols) return;
    const float m = mu[j];
    float v;
    if (kind == minmax::kPerturbUnit) {
        const double nrm = sqrt(*norm_sq);
        v = nrm == 0.0 ? 0.0f : static_cast<float>(-static_cast<double>(m) / nrm);
    } else if (kind == minmax::kPerturbStd) {
        v = -sigma[j];
    } else {
        v = m > 0.0f ? -1.0f : (m < 0.0f ? 1.0f : 0.0f);          // +0.0 for a zero of either sign and for a NaN
    }
    p[j] = v;
}

// out[blockIdx.x] = the largest finite entry above 0 of the rows blockIdx.x, blockIdx.x + gridDim.x, ... (0 when there is none);
// DIAG: entry (i, i) is skipped.  A maximum does not depend on the order it is taken in; the order is fixed all the same.
template <bool DIAG>
__global__ __launch_bounds__(kThreads) void dist_max_kernel(const float* __restrict__ m, int64_t rows, int64_t cols, int64_t ld,
                                                            float* __restrict__ out) {
    __shared__ float part[kThreads / 64];
    float best = 0.0f;
    for (int64_t i = blockIdx.x; i < rows; i += gridDim.x) {
        const float* __restrict__ row = m + i * ld;
        for (int64_t j = threadIdx.x; j < cols; j += kThreads) {
            const float v = row[j];
            const bool take = !(DIAG && i == j) && finite_f32(v) && v > best;
            best = take ? v : best;
        }
    }
    best = lanes::wave_max_shfl(best);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        float all = part[0];
        for (int w = 1; w < kThreads / 64; ++w) all = __builtin_fmaxf(all, part[w]);
        out[blockIdx.x] = all;
    }
}

__device__ __forceinline__ unsigned long long min_u64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// One workgroup.  A non-negative double orders as its bits do: the smallest root is the smallest key, the largest a_i the
// smallest complemented key; a second exchange gives the lowest row that holds it.  Rows whose moments are not finite, and every
// row when c is not a positive number, carry no key: the call is broken or degenerate then and no root is read.
__global__ __launch_bounds__(kOwnerThreads) void minmax_solve_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                                     const double* __restrict__ c_dev,
                                                                     const float* __restrict__ dmax_dev, int64_t r, int kind,
                                                                     MinmaxReport* __restrict__ report) {
    __shared__ ExchangeBuf<unsigned long long> slot;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool sum = kind == minmax::kKindMinSum;
    const double c = *c_dev;
    const double dmax = sum ? 0.0 : static_cast<double>(*dmax_dev);
    const double T = dmax * dmax;
    const bool solvable = minmax::is_finite(c) && c > 0.0;
    constexpr unsigned long long kNone = ~0ull;
    unsigned long long bad = 0, best = kNone, best_row = kNone;
    for (int64_t i = t; i < r; i += kOwnerThreads) {
        const double ai = a[i], bi = b[i];
        if (!minmax::is_finite(ai) || !minmax::is_finite(bi)) {
            bad = 1;
            continue;
        }
        if (!solvable) continue;
        const double v = sum ? ai : minmax::row_gamma(ai, bi, c, T);
        unsigned long long key = static_cast<unsigned long long>(__double_as_longlong(v)) & 0x7fffffffffffffffull;   // (-0.0 is 0)
        if (sum) key = ~key;
        if (key < best) {                 // a thread meets its rows in ascending order: the first of equal keys stays
            best = key;
            best_row = static_cast<unsigned long long>(i);
        }
    }
    int turn = 0;
    const auto waves_min = [lane](unsigned long long v) { return lanes::lanes_fold<kOwnerWaves / 2>(v, lane, min_u64); };
    const unsigned long long any_bad = ~block_exchange(lanes::lanes_fold<32>(~bad, lane, min_u64), slot, turn, lane, wave, waves_min);
    const unsigned long long win = block_exchange(lanes::lanes_fold<32>(best, lane, min_u64), slot, turn, lane, wave, waves_min);
    const unsigned long long mine = best == win ? best_row : kNone;
    const unsigned long long win_row = block_exchange(lanes::lanes_fold<32>(mine, lane, min_u64), slot, turn, lane, wave, waves_min);
    if (t != 0) return;
    const double nan = __builtin_nan("");
    MinmaxReport out;
    out.c = c;
    out.r = static_cast<int32_t>(r);
    out.row = -1;
    out.degenerate = 0;
    out.broken = (any_bad != 0 || !minmax::is_finite(c)) ? 1 : 0;
    out.gamma = nan;
    out.bound = sum ? nan : T;
    double A = 0.0, B = 0.0;
    if (sum && !out.broken) {
        for (int64_t i = 0; i < r; ++i) {     // in row order, as stated
            A = A + a[i];
            B = B + b[i];
        }
        if (!minmax::is_finite(A) || !minmax::is_finite(B)) out.broken = 1;
    }
    if (!out.broken) {
        if (c == 0.0 || r == 1) {
            out.degenerate = 1;
            out.gamma = 0.0;
            if (sum) {
                double a_max = 0.0;
                for (int64_t i = 0; i < r; ++i) a_max = a[i] > a_max ? a[i] : a_max;
                out.bound = minmax::sum_bound(a_max, A, static_cast<double>(r));
            }
        } else if (win == kNone) {            // (cannot happen: c > 0 and every row finite gave every row a key)
            out.broken = 1;
        } else {
            const double v = __longlong_as_double(static_cast<long long>(sum ? ~win : win));
            out.row = static_cast<int32_t>(win_row);
            if (sum) {
                out.bound = minmax::sum_bound(v, A, static_cast<double>(r));
                out.gamma = minmax::sum_gamma(v, B, c, static_cast<double>(r));
            } else {
                out.gamma = v;
            }
            if (!minmax::is_finite(out.gamma) || !minmax::is_finite(out.bound)) {      // b^2 or c q beyond fp64: no vector is formed from it
                out.broken = 1;
                out.gamma = nan;
                out.row = -1;
            }
        }
    }
    *report = out;
}

// Thread j owns the four columns 4 j - shift .. 4 j - shift + 3 of the caller's, `shift` chosen so that a whole block starts on a
// 16-byte boundary in every row (VEC = 4: ld is a multiple of 4); the first and last blocks, and every block of the scalar
// instantiation, are predicated per column and never touch anything outside the row.
template <int VEC>
__global__ __launch_bounds__(kThreads) void minmax_fill_kernel(float* __restrict__ G, int64_t n_attackers, int64_t n_cols, int64_t ld,
                                                               int64_t shift, const float* __restrict__ mu,
                                                               const float* __restrict__ p, const MinmaxReport* __restrict__ report) {
    if (report->broken != 0) return;
    const double gamma = report->gamma;
    const bool as_mu = report->degenerate != 0;
    const int64_t n_blocks = (shift + n_cols + 3) >> 2;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; j < n_blocks; j += stride) {
        const int64_t c0 = 4 * j - shift;
        const bool whole = c0 >= 0 && c0 + 4 <= n_cols;
        float y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = c0 + i >= 0 && c0 + i < n_cols;
            y[i] = 0.0f;
            if (!in) continue;
            const float m = mu[c0 + i];
            const double step = gamma * static_cast<double>(p[c0 + i]);
            y[i] = as_mu ? m : static_cast<float>(static_cast<double>(m) + step);
        }
        for (int64_t r = 0; r < n_attackers; ++r) {
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

}  // namespace

int launch_perturbation(byz_ctx* ctx, const float* mu, const float* sigma, const double* norm_sq, int kind, int64_t n_cols, float* p,
                        hipStream_t stream) {
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    perturbation_kernel<<<static_cast<unsigned>(ceil_div(n_cols, kThreads)), kThreads, 0, stream>>>(mu, sigma, norm_sq, kind, n_cols, p);
    return check_launch("perturbation_kernel");
}

// *dmax = the largest finite entry of the leading r x r block of dist (row stride ld) off its diagonal, 0 when there is none;
// partials: kMinmaxMaxPartials floats
int launch_dist_max(byz_ctx* ctx, const float* dist, int64_t r, int64_t ld, float* partials, float* dmax, hipStream_t stream) {
    static_assert(kMaxPartials == kMinmaxMaxPartials, "the workspace holds one value a workgroup");
    const int64_t blocks = r < kMaxPartials ? r : kMaxPartials;
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    dist_max_kernel<true><<<static_cast<unsigned>(blocks), kThreads, 0, stream>>>(dist, r, r, ld, blocks == 1 ? dmax : partials);
    BYZ_TRY(check_launch("dist_max_kernel"));
    if (blocks == 1) return BYZ_OK;
    dist_max_kernel<false><<<1, kThreads, 0, stream>>>(partials, 1, blocks, blocks, dmax);
    return check_launch("dist_max_kernel (workgroups)");
}

int launch_minmax_solve(byz_ctx* ctx, const double* a, const double* b, const double* c, const float* dmax, int64_t r, int kind,
                        hipStream_t stream) {
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    minmax_solve_kernel<<<1, kOwnerThreads, 0, stream>>>(a, b, c, dmax, r, kind, &device_scalars(ctx)->minmax);
    return check_launch("minmax_solve_kernel");
}

// 1 <= n_attackers, 1 <= n_cols <= ld are the caller's business (api.hip)
int launch_minmax_fill(byz_ctx* ctx, float* G, int64_t n_attackers, int64_t n_cols, int64_t ld, const float* mu, const float* p,
                       hipStream_t stream) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(G);
    const bool vec4 = ld % 4 == 0 && at % 4 == 0;
    const int64_t head = vec4 ? static_cast<int64_t>(((16 - at % 16) % 16) / 4) : 0;      // columns in front of the first boundary
    const int64_t shift = (4 - head) & 3;
    const int64_t n_blocks = (shift + n_cols + 3) >> 2;
    const int64_t want = ceil_div(n_blocks, kThreads), most = static_cast<int64_t>(kBlocksPerCu) * ctx->num_cus;
    const unsigned grid = static_cast<unsigned>(want < most ? want : most);
    const MinmaxReport* report = &device_scalars(ctx)->minmax;
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    if (vec4) minmax_fill_kernel<4><<<grid, kThreads, 0, stream>>>(G, n_attackers, n_cols, ld, shift, mu, p, report);
    else minmax_fill_kernel<1><<<grid, kThreads, 0, stream>>>(G, n_attackers, n_cols, ld, 0, mu, p, report);
    return check_launch("minmax_fill_kernel");
}

}  // namespace byz
