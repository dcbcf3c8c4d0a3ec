// FABA (Xia, Chen, Yu and Ma, "FABA: An Algorithm for Fast Aggregation against Byzantine Attacks in Distributed Neural Networks",
// IJCAI 2019; beyond the reference): drop the gradient farthest from the mean of those still kept, r times, and average the rest.
// For a set S of m rows and a row i of S
//     |g_i - mean(S)|^2 = (1 / m) sum_{j in S} |g_i - g_j|^2 - (1 / (2 m^2)) sum_{j, k in S} |g_j - g_k|^2
// and the second term is the same for every i: the row farthest from the mean is the row with the largest SUM of squared
// distances to the kept rows, and removing row q takes one entry off every other row's sum.  So the rule runs on the n x n
// distance matrix and never reads the gradients (include/byzagg.h states it operation for operation).
//
//   faba_init_kernel   one wave per row: s_i = the fp64 sum of the usable entries' terms of row i, bad_i = the entries that are
//                      not usable.  Lane l adds the columns l, l + 64, ... in ascending order (64 interleaved chains), the
//                      chains fold 32, 16, 8, 4, 2, 1 by lane_exchange.hpp's exchange: an order that no launch geometry changes.
//   faba_loop_kernel   ONE workgroup on owner_loop.hpp's scheme: the owned rows' s and bad in registers (every index static) and
//                      a bit mask of those still kept.  A step is the argmax of (bad, s, lowest row) over the owned rows, the
//                      lane fold of the three-word removal key (six exchanges of three words deep, where a reduction word by
//                      word would be eighteen deep), one block exchange and the waves' fold, one coalesced read of the removed
//                      row and one fp64 subtraction or one decrement a row.  At most n steps.  No atomics, no grid synchronisation.
//                      It ends by writing the flags, the removal order, the fp64 weights, the divisor and the report.
#include "common.hpp"
#include "lane_exchange.hpp"
#include "order_keys.hpp"

namespace byz {
namespace {

constexpr int kFabaInitThreads = 256;          // four rows a workgroup, one wave each

// an off-diagonal entry takes part in the sums when it is finite and >= 0 (-0.0 is: its term is a zero)
__device__ __forceinline__ bool faba_usable(float c) { return __builtin_isfinite(c) && c >= 0.0f; }
// (the square of a float is exact in fp64: a contraction with the addition behind it cannot change a bit)
__device__ __forceinline__ double faba_term(float c, int power) {
    const double d = static_cast<double>(c);
    return power == 2 ? d * d : d;
}

// The step's key is owner_loop.hpp's removal_key on order_keys.hpp's total key of s (s is never a NaN and never -0.0: the sums
// start at +0.0 and x - x is +0.0, so the map is the plain sign flip and value_of_total_key gives the bits back).
__device__ __forceinline__ RemovalKey faba_max(RemovalKey a, RemovalKey b) { return removal_less(a, b) ? b : a; }

__global__ __launch_bounds__(kFabaInitThreads) void faba_init_kernel(const float* __restrict__ dist, int n, int power,
                                                                     double* __restrict__ s, int32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (kFabaInitThreads / 64) + (threadIdx.x >> 6);
    if (i >= n) return;                               // (a whole wave: the kernel has no barrier)
    const float* __restrict__ row = dist + static_cast<int64_t>(i) * n;
    double acc = 0.0;
    int nb = 0;
    for (int j = lane; j < n; j += 64) {
        if (j == i) continue;
        const float c = row[j];
        if (faba_usable(c)) acc += faba_term(c, power);
        else ++nb;
    }
    lanes::for_pow2_down<32>([&](auto mc) {
        constexpr int mask = decltype(mc)::value;
        acc += lanes::lane_xor<mask>(acc, lane);
        nb += lanes::lane_xor<mask>(nb, lane);
    });
    if (lane == 0) {
        s[i] = acc;
        bad[i] = nb;
    }
}

__global__ __launch_bounds__(kOwnerThreads) void faba_loop_kernel(const float* __restrict__ dist, const double* __restrict__ s0,
                                                                 const int32_t* __restrict__ bad0, int n, int r, int power,
                                                                 int32_t* __restrict__ order, int32_t* __restrict__ kept,
                                                                 int32_t* __restrict__ kept_out, double* __restrict__ w,
                                                                 FabaReport* __restrict__ info) {
    __shared__ ExchangeBuf<RemovalKey> slot;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int slots = (n + kOwnerThreads - 1) / kOwnerThreads;     // the slots that hold a row: uniform
    double sv[kOwnerSlots];
    int bad[kOwnerSlots];
    uint32_t live = 0;                                // bit s: row row_of(t, s) is kept
    int any = 0;
#pragma unroll
    for (int s = 0; s < kOwnerSlots; ++s) {
        const int v = row_of(t, s);
        const bool in = v < n;
        sv[s] = in ? s0[v] : 0.0;
        bad[s] = in ? bad0[v] : 0;
        if (in) {
            live |= 1u << s;
            any |= bad[s] < n - 1 ? 1 : 0;
        }
    }
    // no usable entry anywhere: no row can be judged, and the loop does not stop before it has removed them all
    const bool judged = __syncthreads_or(any) != 0;
    int removed = 0, turn = 0;
    unsigned long long last = 0;                      // the ordered bits of the last removed row's s
    for (int step = 0; step < n; ++step) {
        int bb = 0, bi = 0;
        double bs = 0.0;
        bool found = false;
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s) {
            if (s < slots) {
                const bool mine = ((live >> s) & 1u) != 0;
                if (mine && (!found || bad[s] > bb || (bad[s] == bb && sv[s] > bs))) {      // (ascending rows: a tie stays low)
                    found = true;
                    bb = bad[s];
                    bs = sv[s];
                    bi = row_of(t, s);
                }
            }
        }
        RemovalKey k{0ull, 0u};
        __builtin_assume(bs == bs);                   // (never a NaN: the total map's NaN test and its branch fold away)
        if (found) k = removal_key(bb, ordered_bits_total(bs), bi);
        const auto waves_max = [lane](RemovalKey v) { return lanes::lanes_fold<kOwnerWaves / 2>(v, lane, faba_max); };
        const RemovalKey win = block_exchange(lanes::lanes_fold<32>(k, lane, faba_max), slot, turn, lane, wave, waves_max);
        const uint32_t hi_hi = __builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(win.hi >> 32)));
        const uint32_t hi_lo = __builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(win.hi)));
        const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<int>(win.lo));
        const unsigned long long hi = (static_cast<unsigned long long>(hi_hi) << 32) | hi_lo;
        if (hi == 0 && lo == 0) break;                // (cannot happen: a kept row is left at every step below n)
        const int wbad = removal_bad(hi);
        if (step >= r && wbad == 0 && judged) break;
        const int q = removal_row(lo);
        if (q >= n) break;                            // (cannot happen: the key came from a row)
        last = removal_s_key(hi, lo);
        removed = step + 1;
        if (t == 0) order[step] = q;
        if (owner_thread(q) == t) live &= ~(1u << slot_of(q));
        const float* __restrict__ row = dist + static_cast<int64_t>(q) * n;
        float c[kOwnerSlots];
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s) {
            const int v = row_of(t, s);
            c[s] = (s < slots && v < n) ? row[v] : 0.0f;
        }
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s) {
            const int v = row_of(t, s);
            if (s < slots && v < n && v != q) {
                if (faba_usable(c[s])) sv[s] -= faba_term(c[s], power);
                else bad[s] -= 1;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < kOwnerSlots; ++s) {
        const int v = row_of(t, s);
        if (v < n) {
            const int flag = static_cast<int>((live >> s) & 1u);
            kept[v] = flag;
            if (kept_out != nullptr) kept_out[v] = flag;
            w[v] = flag ? 1.0 : 0.0;
        }
    }
    for (int e = removed + t; e < n; e += kOwnerThreads) order[e] = -1;
    if (t == 0) {
        info->removed = removed;
        info->kept = n - removed;
        info->forced = removed > r ? removed - r : 0;
        info->pad = 0;
        info->last_score = removed > 0 ? value_of_total_key(last) : 0.0;
        info->kept_f64 = static_cast<double>(n - removed);
    }
}

}  // namespace

int faba_workspace(byz_ctx* ctx, int64_t n, FabaScratch* out) {
    out->info = &device_scalars(ctx)->faba;
    Carve c;
    c.take(&out->s, n);
    c.take(&out->w, n);
    c.take(&out->bad, n);
    c.take(&out->order, n);
    c.take(&out->kept, n);
    return c.commit(ctx->faba);
}

// 2 <= n <= kFabaMaxRows, 0 <= r <= n - 1, power 1 or 2: the caller's business (api.hip), checked again before anything runs
int launch_faba_select(byz_ctx* ctx, const FabaScratch& t, const float* dist, int64_t n, int64_t r, int power, int32_t* kept_out,
                       int32_t* order_out, hipStream_t stream) {
    BYZ_REQUIRE(dist && n >= 2 && n <= kFabaMaxRows && r >= 0 && r <= n - 1 && (power == 1 || power == 2),
                "faba select: bad arguments (n = %lld, r = %lld, power = %d)", (long long)n, (long long)r, power);
    {
        KernelTimer timer(ctx, BYZ_K_ROW_SORT, stream);
        faba_init_kernel<<<static_cast<unsigned>(ceil_div(n, kFabaInitThreads / 64)), kFabaInitThreads, 0, stream>>>(
            dist, static_cast<int>(n), power, t.s, t.bad);
        BYZ_TRY(check_launch("faba_init_kernel"));
    }
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    faba_loop_kernel<<<1, kOwnerThreads, 0, stream>>>(dist, t.s, t.bad, static_cast<int>(n), static_cast<int>(r), power,
                                                     order_out != nullptr ? order_out : t.order, t.kept, kept_out, t.w, t.info);
    return check_launch("faba_loop_kernel");
}

}  // namespace byz
