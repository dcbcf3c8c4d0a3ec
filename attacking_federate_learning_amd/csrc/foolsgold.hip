// FoolsGold (Fung, Yoon and Beschastnikh, "Mitigating Sybils in Federated Learning Poisoning", arXiv:1808.04866; beyond the
// reference): the clients whose ACCUMULATED updates point the same way get their weight cut.  The decision runs on ONE n x n fp64
// Gram -- of the per-client history, or of this round's gradients -- and never on the gradients (include/byzagg.h states the
// rule (R) operation for operation, csrc/foolsgold_rule.hpp holds what decides).
//
//   rows_add_kernel<VEC>       the history update H[i][c] = fl32(H[i][c] + G[i][col_start + c]): an elementwise read-read-write,
//                              grid-stride over (rows, groups of four columns), no LDS, no atomics.  VEC = 4: both operands
//                              take 16-byte accesses in every row (the launcher has checked bases and leading dimensions).
//                              VEC = 1, the mixed path: every row is cut at H's own 16-byte boundaries -- a predicated head of
//                              up to three floats, 16-byte groups of H, a predicated tail -- and G, whose window starts wherever
//                              the caller's columns start, is read by dwords.
//   foolsgold_norms_kernel     one thread a row: r_i = sqrt(C_ii), -1 for an excluded row.  Written once, read as a vector.
//   foolsgold_rowmax_kernel    one wave a row: m_i, the largest cosine of the row with the others, not below 0.
//   foolsgold_pardon_kernel    one wave a row, behind the kernel boundary that makes every m_j visible: a_i, the largest pardoned
//                              cosine.  Both read the row coalesced, four loads in flight a lane; max is exact, so the order in
//                              which a wave folds is free.
//   foolsgold_weights_kernel   ONE workgroup on owner_loop.hpp's ownership and block exchange: v, top and the counts, then w and
//                              the clipped logit, then T: the usable count, or the weights added by wave 0 in ascending row
//                              order (64 coalesced loads, 64 additions out of lane 0, 1, ..., 63).  Any number of rows.
// No floating-point atomics, no scratch, no host synchronisation.
#include "common.hpp"
#include "foolsgold_rule.hpp"
#include "lane_exchange.hpp"
#include "owner_loop.hpp"

namespace byz {
namespace {

constexpr int kAddThreads = 256;
constexpr int kRowThreads = 256;              // four rows a workgroup, one wave each
constexpr int kRowBatch = 4;                  // row reads a lane keeps in flight

template <int VEC>
__global__ __launch_bounds__(kAddThreads) void rows_add_kernel(float* __restrict__ H, int64_t ld_h, const float* __restrict__ G,
                                                               int64_t ld_g, int64_t n, int64_t w) {
    // group 0 of a row is its head, group g > 0 the four columns from head + 4 (g - 1): 1 + ceil(w / 4) groups cover every head
    const int64_t groups = 1 + (w + 3) / 4;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        float* __restrict__ h = H + i * ld_h;
        const float* __restrict__ g = G + i * ld_g;
        int64_t head = 0;
        if constexpr (VEC == 1) {
            head = static_cast<int64_t>((4u - static_cast<unsigned>((reinterpret_cast<uintptr_t>(h) >> 2) & 3u)) & 3u);
            head = head < w ? head : w;
        }
        for (int64_t q = static_cast<int64_t>(blockIdx.x) * kAddThreads + threadIdx.x; q < groups; q += static_cast<int64_t>(gridDim.x) * kAddThreads) {
            const int64_t c0 = q == 0 ? 0 : head + 4 * (q - 1);
            const int64_t c1 = q == 0 ? head : (c0 + 4 < w ? c0 + 4 : w);
            if (q > 0 && c1 - c0 == 4) {
                float4 a = *reinterpret_cast<const float4*>(h + c0);
                float4 b;
                if constexpr (VEC == 4) {
                    b = *reinterpret_cast<const float4*>(g + c0);
                } else {
                    b.x = g[c0], b.y = g[c0 + 1], b.z = g[c0 + 2], b.w = g[c0 + 3];
                }
                a.x = __fadd_rn(a.x, b.x), a.y = __fadd_rn(a.y, b.y), a.z = __fadd_rn(a.z, b.z), a.w = __fadd_rn(a.w, b.w);
                *reinterpret_cast<float4*>(h + c0) = a;
            } else {
                for (int64_t c = c0; c < c1; ++c) h[c] = __fadd_rn(h[c], g[c]);
            }
        }
    }
}

__global__ void foolsgold_norms_kernel(const double* __restrict__ C, int n, double* __restrict__ r) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) r[i] = foolsgold::norm(C[static_cast<int64_t>(i) * n + i]);
}

// The row's maximum of f(j, C_ij) over the j != i with r_j > 0, from +0.0, in every lane.
template <typename F>
__device__ __forceinline__ double row_max(const double* __restrict__ row, const double* __restrict__ r, int n, int i, int lane, F f) {
    double acc = 0.0;
    for (int j0 = lane; j0 < n; j0 += 64 * kRowBatch) {
        double c[kRowBatch], rj[kRowBatch];
#pragma unroll
        for (int b = 0; b < kRowBatch; ++b) {
            const int j = j0 + 64 * b;
            const bool in = j < n;
            c[b] = in ? row[j] : 0.0;
            rj[b] = in ? r[j] : -1.0;
        }
#pragma unroll
        for (int b = 0; b < kRowBatch; ++b) {
            const int j = j0 + 64 * b;
            if (j != i && rj[b] > 0.0) acc = foolsgold::take_max(acc, f(j, c[b], rj[b]));
        }
    }
    return lanes::wave_reduce_shfl(acc, [](double a, double b) { return foolsgold::take_max(a, b); });
}

__global__ __launch_bounds__(kRowThreads) void foolsgold_rowmax_kernel(const double* __restrict__ C, const double* __restrict__ r,
                                                                       int n, double* __restrict__ m, double* __restrict__ m_out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
    if (i >= n) return;                               // (a whole wave: the kernel has no barrier)
    const double ri = r[i];
    double acc = 0.0;
    if (ri > 0.0)
        acc = row_max(C + static_cast<int64_t>(i) * n, r, n, i, lane,
                      [ri](int, double c, double rj) { return foolsgold::cosine(c, ri, rj); });
    if (lane == 0) {
        m[i] = acc;
        if (m_out != nullptr) m_out[i] = acc;
    }
}

__global__ __launch_bounds__(kRowThreads) void foolsgold_pardon_kernel(const double* __restrict__ C, const double* __restrict__ r,
                                                                       const double* __restrict__ m, int n, double* __restrict__ a,
                                                                       double* __restrict__ a_out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const double ri = r[i], mi = m[i];
    double acc = 0.0;
    if (ri > 0.0)
        acc = row_max(C + static_cast<int64_t>(i) * n, r, n, i, lane, [ri, mi, m](int j, double c, double rj) {
            return foolsgold::pardoned(foolsgold::cosine(c, ri, rj), mi, m[j]);
        });
    if (lane == 0) {
        a[i] = acc;
        if (a_out != nullptr) a_out[i] = acc;
    }
}

struct WeightsLds {
    ExchangeBuf<double> top;
    ExchangeBuf<int> count;
};

__device__ __forceinline__ int block_count(int mine, ExchangeBuf<int>& buf, int& turn) {
    return block_exchange(lanes::wave_sum_shfl(mine), buf, turn, threadIdx.x & 63, threadIdx.x >> 6, [](int v) {
#pragma unroll
        for (int s = kOwnerWaves / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
        return v;
    });
}

__global__ __launch_bounds__(kOwnerThreads) void foolsgold_weights_kernel(const double* __restrict__ r, const double* __restrict__ a,
                                                                         int n, double kappa, int normalise,
                                                                         double* __restrict__ weights, double* __restrict__ weights_out,
                                                                         double* __restrict__ rescaled, int32_t* __restrict__ flags,
                                                                         FoolsgoldReport* __restrict__ info) {
    __shared__ WeightsLds lds;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int turn_top = 0, turn_count = 0;
    // (6), (7): the raw weights' maximum and the usable rows
    double top = 0.0;
    int usable = 0;
    for (int s = 0; row_of(t, s) < n; ++s) {
        const int v = row_of(t, s);
        if (r[v] >= 0.0) {
            ++usable;
            top = foolsgold::take_max(top, foolsgold::raw_weight(a[v]));
        }
    }
    top = block_exchange(lanes::wave_reduce_shfl(top, lanes::Max{}), lds.top, turn_top, lane, wave, [](double v) {
#pragma unroll
        for (int s = kOwnerWaves / 2; s > 0; s >>= 1) {
            const double o = __shfl_xor(v, s, 64);
            v = o > v ? o : v;
        }
        return v;
    });
    usable = block_count(usable, lds.count, turn_count);
    const bool few = usable < 2, degenerate = !few && top == 0.0;
    // (8): the rescaled weight and the clipped logit
    int at_zero = 0, at_one = 0;
    for (int s = 0; row_of(t, s) < n; ++s) {
        const int v = row_of(t, s);
        const bool in = r[v] >= 0.0;
        double w = 0.0, l = 0.0;
        if (in && few) {
            w = 1.0, l = 1.0;
        } else if (in && !degenerate) {
            w = foolsgold::rescaled(foolsgold::raw_weight(a[v]), top);
            l = foolsgold::clipped_logit(w, kappa);
        }
        if (in) at_zero += l == 0.0 ? 1 : 0, at_one += l == 1.0 ? 1 : 0;
        weights[v] = l;
        if (weights_out != nullptr) weights_out[v] = l;
        rescaled[v] = w;
        flags[v] = in ? 1 : 0;
    }
    at_zero = block_count(at_zero, lds.count, turn_count);
    at_one = block_count(at_one, lds.count, turn_count);     // (its barrier also stands between the weights' stores and wave 0's loads)
    // (9): T
    double total = static_cast<double>(usable);
    if (normalise == foolsgold::kNormaliseSum && wave == 0) {
        total = 0.0;
        for (int v0 = 0; v0 < n; v0 += 64) {
            const double mine = v0 + lane < n ? weights[v0 + lane] : 0.0;
            const int len = n - v0 < 64 ? n - v0 : 64;
            for (int k = 0; k < len; ++k) total = total + lanes::readlane(mine, k);
        }
    }
    if (t == 0) {
        info->usable = usable;
        info->excluded = n - usable;
        info->at_zero = at_zero;
        info->at_one = at_one;
        info->degenerate = degenerate ? 1 : 0;
        info->pad = 0;
        info->top = top;
        info->divisor = total;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int foolsgold_workspace(byz_ctx* ctx, int64_t n, FoolsgoldScratch* out) {
    out->info = &device_scalars(ctx)->foolsgold;
    Carve c;
    c.take(&out->r, n);
    c.take(&out->m, n);
    c.take(&out->a, n);
    c.take(&out->w, n);
    c.take(&out->rescaled, n);
    c.take(&out->flags, n);
    return c.commit(ctx->foolsgold);
}

// H (n x w, ld_h) += G's window (n x w from G, which already points at the window's first column, ld_g)
int launch_rows_add(byz_ctx* ctx, float* H, int64_t ld_h, const float* G, int64_t n, int64_t w, int64_t ld_g, hipStream_t stream) {
    BYZ_REQUIRE(H && G && n >= 1 && w >= 1 && ld_h >= w && ld_g >= w, "rows_add: bad arguments (%lld x %lld, ld %lld and %lld)",
                (long long)n, (long long)w, (long long)ld_h, (long long)ld_g);
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    const int64_t groups = 1 + (w + 3) / 4;
    const unsigned gx = static_cast<unsigned>(std::min<int64_t>(ceil_div(groups, kAddThreads), 1024));
    const unsigned gy = static_cast<unsigned>(std::min<int64_t>(n, std::max<int64_t>(1, 8192 / gx)));
    const bool both = aligned16(H) && aligned16(G) && ld_h % 4 == 0 && ld_g % 4 == 0;
    if (both) rows_add_kernel<4><<<dim3(gx, gy), kAddThreads, 0, stream>>>(H, ld_h, G, ld_g, n, w);
    else rows_add_kernel<1><<<dim3(gx, gy), kAddThreads, 0, stream>>>(H, ld_h, G, ld_g, n, w);
    return check_launch("rows_add_kernel");
}

// n >= 1, kappa finite and > 0, normalise 0 or 1: the caller's business (api.hip), checked again before anything runs
int launch_foolsgold_weights(byz_ctx* ctx, const FoolsgoldScratch& t, const double* gram, int64_t n, double kappa, int normalise,
                             double* weights_out, double* maxcs_out, double* alpha_out, hipStream_t stream) {
    BYZ_REQUIRE(gram && n >= 1 && n <= kLargeMaxRows && kappa > 0.0 && (normalise == 0 || normalise == 1),
                "foolsgold weights: bad arguments (n = %lld, kappa = %g, normalise = %d)", (long long)n, kappa, normalise);
    const int rows = static_cast<int>(n);
    const unsigned row_blocks = static_cast<unsigned>(ceil_div(n, kRowThreads / 64));
    {
        KernelTimer timer(ctx, BYZ_K_ROW_SORT, stream);
        foolsgold_norms_kernel<<<static_cast<unsigned>(ceil_div(n, 256)), 256, 0, stream>>>(gram, rows, t.r);
        BYZ_TRY(check_launch("foolsgold_norms_kernel"));
        foolsgold_rowmax_kernel<<<row_blocks, kRowThreads, 0, stream>>>(gram, t.r, rows, t.m, maxcs_out);
        BYZ_TRY(check_launch("foolsgold_rowmax_kernel"));
        foolsgold_pardon_kernel<<<row_blocks, kRowThreads, 0, stream>>>(gram, t.r, t.m, rows, t.a, alpha_out);
        BYZ_TRY(check_launch("foolsgold_pardon_kernel"));
    }
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    foolsgold_weights_kernel<<<1, kOwnerThreads, 0, stream>>>(t.r, t.a, rows, kappa, normalise, t.w, weights_out, t.rescaled, t.flags,
                                                             t.info);
    return check_launch("foolsgold_weights_kernel");
}

}  // namespace byz
