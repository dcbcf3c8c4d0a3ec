// AFA, Adaptive Federated Averaging (Munoz-Gonzalez, Co and Lupu, "Byzantine-Robust Federated Machine Learning through Adaptive
// Model Averaging", arXiv:1909.05125, Algorithm 1; beyond the reference): every row's cosine with the weighted aggregate of
// the rows still kept, the rows whose cosine lies more than xi standard deviations from the median removed on the side the
// mean points away from, xi raised, again, until a round removes nobody.  With the kept set S, the weights w and the Gram C
//     g_k . agg  is proportional to  u_k = sum_{j in S} w_j C[k][j],     |agg|^2  to  A = sum_{k in S} w_k u_k,
// and removing row q takes w_q C[q][k] off every u_k: the rule runs on the n x n fp64 Gram and never reads the gradients
// (include/byzagg.h states it operation for operation).
//
//   afa_rows_kernel   one thread a row: the weight a row counts with (0: the row is excluded) and r_k = sqrt(C[k][k]).
//   afa_init_kernel   one wave a row: u_k over the usable columns.  Lane l adds the products of the columns l, l + 64, ... in
//                     ascending order (64 interleaved chains), the chains fold 32, 16, 8, 4, 2, 1.
//   afa_loop_kernel   ONE workgroup on owner_loop.hpp's scheme: the owned rows' u in registers (every index static), a bit mask
//                     of those still kept, their s in LDS (128 KiB).  A round is three sums over the workgroup in one stated
//                     order (afa_block_sum: a block exchange), the exact median of the s by an 8-bit radix walk
//                     over their ordered keys (a 256-bin LDS histogram, integer LDS atomics only, one barrier a digit), the
//                     removals, and the update: the removed rows of a block of 1024 rows are listed in LDS in ascending
//                     order, and every thread then takes them off its u four row reads at a time: the reads of a batch are
//                     independent and in flight together, the subtractions behind them in ascending row order.  The number of
//                     rounds is the only data-dependent trip count.  No scratch, no floating-point atomics, no grid or host
//                     synchronisation.  It ends by writing the flags, the rounds of removal, the scores, the fp64 weights,
//                     their sum and the report.
#include "common.hpp"
#include "lane_exchange.hpp"
#include "order_keys.hpp"

namespace byz {
namespace {

constexpr int kAfaInitThreads = 256;          // four rows a workgroup, one wave each
constexpr int kAfaBatch = 4;                  // row reads a thread keeps in flight in the update (6 and 8 spill scalars)
constexpr int kAfaDigits = 256;               // the radix walk's digit: 8 bits, 8 digits a key

__global__ void afa_rows_kernel(const double* __restrict__ C, const double* __restrict__ w_in, int n, double* __restrict__ w,
                                double* __restrict__ r) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double d = C[static_cast<int64_t>(k) * n + k];
    const double wk = w_in != nullptr ? w_in[k] : 1.0;
    const bool usable = __builtin_isfinite(d) && d > 0.0 && __builtin_isfinite(wk) && wk > 0.0;
    w[k] = usable ? wk : 0.0;
    r[k] = usable ? sqrt(d) : 0.0;
}

__global__ __launch_bounds__(kAfaInitThreads) void afa_init_kernel(const double* __restrict__ C, const double* __restrict__ w, int n,
                                                                   double* __restrict__ u) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (kAfaInitThreads / 64) + (threadIdx.x >> 6);
    if (k >= n) return;                               // (a whole wave: the kernel has no barrier)
    const double* __restrict__ row = C + static_cast<int64_t>(k) * n;
    double acc = 0.0;
    for (int j = lane; j < n; j += 64) {
        const double wj = w[j];
        if (wj > 0.0) acc += wj * row[j];             // (an excluded column is skipped, not added as a zero: its entry may be a NaN)
    }
    acc = lanes::wave_sum_shfl(acc);
    if (lane == 0) u[k] = acc;
}

// The one order of a sum over the workgroup: thread t's chain (the caller's: its rows ascending from +0.0), the 64 chains of a
// wave folded 32, 16, 8, 4, 2, 1, the 16 waves' sums folded 8, 4, 2, 1.  Every thread gets the same bits (an exchange adds
// the same two numbers in both lanes).  One barrier a call: owner_loop.hpp's block exchange.
__device__ __forceinline__ double afa_block_sum(double chain, ExchangeBuf<double>& buf, int& turn) {
    return block_exchange(lanes::wave_sum_shfl(chain), buf, turn, threadIdx.x & 63, threadIdx.x >> 6, [](double v) {
#pragma unroll
        for (int m = kOwnerWaves / 2; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
        return v;
    });
}
__device__ __forceinline__ int afa_block_count(int mine, int* slots) {     // (two barriers: not on a round's critical path twice)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    mine = lanes::wave_sum_shfl(mine);
    __syncthreads();
    if (lane == 0) slots[wave] = mine;
    __syncthreads();
    int v = slots[lane & (kOwnerWaves - 1)];
#pragma unroll
    for (int m = kOwnerWaves / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return __builtin_amdgcn_readfirstlane(v);
}

// A value of the thread again, as one the compiler knows nothing about: what is formed from it is formed where it is used.  (Formed from threadIdx.x they are the same in every round, and sixteen 64-bit addresses an array, hoisted
// out of the round loop for every array, do not fit the 128 registers a thread of 1024 has.)
__device__ __forceinline__ int afa_here(int t) {
    asm volatile("" : "+v"(t));
    return t;
}
// the same for a mask of rows: its sixteen tests are made where they are used, not kept as sixteen scalar pairs
__device__ __forceinline__ uint32_t afa_here(uint32_t mask) {
    asm volatile("" : "+v"(mask));
    return mask;
}

struct AfaLds {
    double s[kAfaMaxRows];                    // every row's last s
    double list_w[kOwnerThreads];               // the removed rows of one block of 1024 rows, ascending: their weights
    int list_q[kOwnerThreads];                  //                                                         and their rows
    unsigned hist[3][kAfaDigits];             // the radix walk's histograms, taken in turn (one barrier a digit)
    ExchangeBuf<double> sum;
    unsigned long long key[kOwnerWaves];
    int count[kOwnerWaves];                     // afa_block_count's alone: written behind its first barrier, read behind its second
    int listed[kOwnerWaves];                    // the update's alone: a block's counts, written before the block's first barrier, read
                                              // behind it, and the block's last barrier stands before the next block's (and the next
                                              // round's) write.  Were they one array, a wave still reading a round's removed count
                                              // could meet the first block's list counts.
};

// The order statistics lo = (m - 1) / 2 and hi = m / 2 of the kept rows' s, by value: np.median's two middle ones.  The keys are
// order_keys.hpp's total map (-0.0 is +0.0, a NaN sorts behind +inf).  Eight digits from the top: the kept keys that share the
// prefix found so far are counted by digit, every wave scans the 256 counts (four a lane) to the digit that holds the rank.
// The last digit's count is the number of keys EQUAL to the lower statistic: the upper one is the same key when that count
// covers rank + 1, and the smallest key above it otherwise.
__device__ __forceinline__ double afa_median(AfaLds& lds, uint32_t live, int m) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < kAfaDigits) lds.hist[0][t] = 0;
    __syncthreads();
    unsigned long long prefix = 0, known = 0;         // the digits found so far, and the mask of their bits
    int rank = (m - 1) / 2, equal = 0;
#pragma unroll 1
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        unsigned* hist = lds.hist[pass % 3];
        if (t < kAfaDigits) lds.hist[(pass + 1) % 3][t] = 0;
        int run_digit = -1, run = 0;                  // equal digits of a thread's rows are counted before they are added
        const uint32_t mask = afa_here(live);
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s) {
            if ((mask >> s) & 1u) {
                const unsigned long long key = ordered_bits_total(lds.s[row_of(t, s)]);
                if ((key & known) == prefix) {
                    const int digit = static_cast<int>((key >> shift) & 0xffu);
                    if (digit != run_digit) {
                        if (run > 0) atomicAdd(&hist[run_digit], static_cast<unsigned>(run));
                        run_digit = digit;
                        run = 0;
                    }
                    ++run;
                }
            }
        }
        if (run > 0) atomicAdd(&hist[run_digit], static_cast<unsigned>(run));
        __syncthreads();
        const int c0 = static_cast<int>(hist[4 * lane]), c1 = static_cast<int>(hist[4 * lane + 1]),
                  c2 = static_cast<int>(hist[4 * lane + 2]), c3 = static_cast<int>(hist[4 * lane + 3]);
        const int mine = c0 + c1 + c2 + c3;
        int upto = mine;                              // the counts of the lanes up to and including this one
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int other = __shfl_up(upto, d, 64);
            if (lane >= d) upto += other;
        }
        const int before = upto - mine;
        const bool holds = before <= rank && rank < upto;       // one lane: the counts add up to more than the rank
        const unsigned long long who = __ballot(holds);
        int digit = 0, left = 0, count = 0;
        if (holds) {
            left = rank - before;
            digit = 4 * lane;
            count = c0;
            if (left >= count) { left -= count; ++digit; count = c1;
                if (left >= count) { left -= count; ++digit; count = c2;
                    if (left >= count) { left -= count; ++digit; count = c3; } } }
        }
        const int src = who != 0 ? static_cast<int>(__builtin_ctzll(who)) : 0;     // (who == 0 cannot happen: rank < the kept)
        digit = __builtin_amdgcn_readlane(digit, src);
        rank = __builtin_amdgcn_readlane(left, src);
        equal = __builtin_amdgcn_readlane(count, src);
        prefix |= static_cast<unsigned long long>(digit) << shift;
        known |= 0xffull << shift;
    }
    const double lo = value_of_total_key(prefix);
    if ((m & 1) != 0) return lo;
    if (rank + 1 < equal) return (lo + lo) / 2.0;
    unsigned long long above = ~0ull;                 // the smallest kept key above the lower statistic
    const uint32_t mask = afa_here(live);
#pragma unroll
    for (int s = 0; s < kOwnerSlots; ++s) {
        if ((mask >> s) & 1u) {
            const unsigned long long key = ordered_bits_total(lds.s[row_of(t, s)]);
            if (key > prefix && key < above) above = key;
        }
    }
    above = lanes::wave_min_shfl(above);
    if (lane == 0) lds.key[wave] = above;
    __syncthreads();
    above = lds.key[lane & (kOwnerWaves - 1)];
#pragma unroll
    for (int d = kOwnerWaves / 2; d > 0; d >>= 1) {
        const unsigned long long other = __shfl_xor(above, d, 64);
        above = other < above ? other : above;
    }
    return (lo + value_of_total_key(above)) / 2.0;
}

__global__ __launch_bounds__(kOwnerThreads) void afa_loop_kernel(const double* __restrict__ C, const double* __restrict__ u0,
                                                               const double* __restrict__ r0, double* __restrict__ w, int n,
                                                               double xi, double delta_xi, int max_rounds,
                                                               int32_t* __restrict__ kept, int32_t* __restrict__ kept_out,
                                                               int32_t* __restrict__ round_of, double* __restrict__ score,
                                                               AfaReport* __restrict__ info) {
    __shared__ AfaLds lds;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int slots = (n + kOwnerThreads - 1) / kOwnerThreads;       // the slots that hold a row: uniform
    double u[kOwnerSlots];                              // (r is read again where a round needs it: once)
    uint32_t live = 0;                                // bit s: row row_of(t, s) is kept
#pragma unroll
    for (int s = 0; s < kOwnerSlots; ++s) {
        const int v = row_of(t, s);
        const bool in = v < n;
        u[s] = in ? u0[v] : 0.0;
        if (in) {
            lds.s[v] = 0.0;
            if (r0[v] > 0.0) live |= 1u << s;         // (an excluded row has r = 0)
        }
    }
    int turn = 0;
    const int usable = afa_block_count(__builtin_popcount(live), lds.count);
    int m = usable, rounds = 0, branch = 0, degenerate = 0;
    double mean = 0.0, med = 0.0, sd = 0.0, thr = 0.0;
    for (int round = 1; m > 0 && round <= n; ++round) {
        rounds = round;
        double chain = 0.0;
        int h = afa_here(t);
        uint32_t mask = afa_here(live);
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s)
            if ((mask >> s) & 1u) chain += w[row_of(h, s)] * u[s];
        const double A = afa_block_sum(chain, lds.sum, turn);
        if (!(__builtin_isfinite(A) && A > 0.0)) {
            degenerate = 1;
            break;
        }
        const double root = sqrt(A);
        chain = 0.0;
        h = afa_here(t);
        mask = afa_here(live);
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s) {
            if ((mask >> s) & 1u) {
                const double sk = u[s] / (r0[row_of(h, s)] * root);
                lds.s[row_of(t, s)] = sk;
                chain += sk;
            }
        }
        const double md = static_cast<double>(m);
        mean = afa_block_sum(chain, lds.sum, turn) / md;
        chain = 0.0;
        mask = afa_here(live);
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s) {
            if ((mask >> s) & 1u) {
                const double d = lds.s[row_of(t, s)] - mean;
                chain += d * d;
            }
        }
        sd = sqrt(afa_block_sum(chain, lds.sum, turn) / md);
        med = afa_median(lds, live, m);
        const bool lower = mean < med;
        thr = lower ? med - xi * sd : med + xi * sd;
        uint32_t gone = 0;                            // bit s: row row_of(t, s) is removed in this round
        h = afa_here(t);
        mask = afa_here(live);
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s) {
            if ((mask >> s) & 1u) {
                const double sk = lds.s[row_of(t, s)];
                if (lower ? sk < thr : sk > thr) {
                    gone |= 1u << s;
                    round_of[row_of(h, s)] = round;
                }
            }
        }
        const int removed = afa_block_count(__builtin_popcount(gone), lds.count);
        if (removed == 0) break;
        branch = lower ? -1 : 1;
        live &= ~gone;
        m -= removed;
        if (max_rounds > 0 && round >= max_rounds) break;
        // the update, one block of 1024 rows after the other: its removed rows listed in ascending order, then taken off every kept row's u
        for (int g = 0; g < slots; ++g) {
            const bool mine = ((gone >> g) & 1u) != 0;
            const unsigned long long votes = __ballot(mine);
            if (lane == 0) lds.listed[wave] = __builtin_popcountll(votes);
            __syncthreads();
            int first = 0, listed = 0;
#pragma unroll
            for (int v = 0; v < kOwnerWaves; ++v) {
                const int c = lds.listed[v];
                first += v < wave ? c : 0;
                listed += c;
            }
            listed = __builtin_amdgcn_readfirstlane(listed);
            if (listed > 0) {
                if (mine) {
                    const int at = first + __builtin_popcountll(votes & ((1ull << lane) - 1ull));
                    const int q = row_of(afa_here(t), g);
                    lds.list_q[at] = q;
                    lds.list_w[at] = w[q];
                }
                __syncthreads();
                h = afa_here(t);
                mask = afa_here(live);                // (the rows still kept: nobody reads a removed or excluded row's u again)
#pragma unroll
                for (int s = 0; s < kOwnerSlots; ++s) {
                    const int v = row_of(h, s);
                    if ((mask >> s) & 1u) {
                        double acc = u[s];
                        for (int b0 = 0; b0 < listed; b0 += kAfaBatch) {
                            double c[kAfaBatch];
#pragma unroll
                            for (int b = 0; b < kAfaBatch; ++b) {      // (the row is uniform: its start is a scalar)
                                const int q = __builtin_amdgcn_readfirstlane(lds.list_q[b0 + b < listed ? b0 + b : b0]);
                                c[b] = b0 + b < listed ? (C + static_cast<int64_t>(q) * n)[v] : 0.0;
                            }
#pragma unroll
                            for (int b = 0; b < kAfaBatch; ++b)
                                if (b0 + b < listed) acc = acc - lds.list_w[b0 + b] * c[b];
                        }
                        u[s] = acc;
                    }
                }
            }
            __syncthreads();                          // (the list and its counts are the next block's)
        }
        xi = xi + delta_xi;
    }
    double chain = 0.0;
    const int h = afa_here(t);
#pragma unroll
    for (int s = 0; s < kOwnerSlots; ++s) {
        const int v = row_of(h, s);
        if (v < n) {
            const int flag = static_cast<int>((live >> s) & 1u);
            kept[v] = flag;
            if (kept_out != nullptr) kept_out[v] = flag;
            if (flag) round_of[v] = -1;
            else if (!(r0[v] > 0.0)) round_of[v] = 0;
            if (score != nullptr) score[v] = lds.s[v];
            if (flag) chain += w[v];
            else w[v] = 0.0;
        }
    }
    const double divisor = afa_block_sum(chain, lds.sum, turn);
    if (t == 0) {
        info->rounds = rounds;
        info->kept = m;
        info->removed = usable - m;
        info->excluded = n - usable;
        info->branch = branch;
        info->degenerate = degenerate;
        info->mean = mean;
        info->med = med;
        info->sd = sd;
        info->thr = thr;
        info->divisor = divisor;
    }
}

// owner_loop.hpp's pieces on one workgroup (tests/test_gpu_parity.py restates every row): row r holds thread t's word at
// out[r * 1024 + t]; a 64-bit value takes two rows (low, high), a RemovalKey three (hi's low, hi's high, lo).
__global__ __launch_bounds__(kOwnerThreads) void owner_loop_selftest_kernel(int32_t* __restrict__ out) {
    __shared__ ExchangeBuf<unsigned long long> keys;
    __shared__ ExchangeBuf<double> sums;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int row = 0;
    const auto word = [&](uint32_t w) { out[row++ * kOwnerThreads + t] = static_cast<int32_t>(w); };
    const auto put = [&](auto v) {                    // 8 bytes: the low word, the high word
        word(static_cast<uint32_t>(__builtin_bit_cast(unsigned long long, v)));
        word(static_cast<uint32_t>(__builtin_bit_cast(unsigned long long, v) >> 32));
    };
    const auto put_key = [&](RemovalKey k) { put(k.hi), word(k.lo); };
    const auto key_max = [](RemovalKey a, RemovalKey b) { return removal_less(a, b) ? b : a; };
    const auto key_min = [](unsigned long long a, unsigned long long b) { return a < b ? a : b; };
    // (a) the exchange of a 64-bit value and of a three-word struct
    const unsigned long long wide = static_cast<unsigned long long>(t) * 0x0001000300050007ull + 0x1234ull;
    const RemovalKey three{wide ^ 0xffffull, static_cast<uint32_t>(t) * 40503u + 7u};
    lanes::for_pow2_up<1, 32>([&](auto mc) {
        put(lanes::lane_xor<decltype(mc)::value>(wide, lane));
        put_key(lanes::lane_xor<decltype(mc)::value>(three, lane));
    });
    // (b) the lane fold: eight-way ties on the high word, the low word decides
    const RemovalKey tied{static_cast<unsigned long long>((37 * lane + 11 + wave) % 8), static_cast<uint32_t>(t) * 2654435761u};
    put_key(lanes::lanes_fold<32>(tied, lane, key_max));
    put_key(lanes::lanes_fold<8>(tied, lane, key_max));
    // (c) two block exchanges with no barrier of the kernel's between them: the winner sits in wave 5, then in wave 11
    int turn = 0;
    const auto waves_min = [&](unsigned long long v) { return lanes::lanes_fold<kOwnerWaves / 2>(v, lane, key_min); };
    const unsigned long long first = (static_cast<unsigned long long>(t ^ (5 * 64 + 17)) << 32) | static_cast<uint32_t>(t);
    const unsigned long long second = (static_cast<unsigned long long>(t ^ (11 * 64 + 3)) << 32) | static_cast<uint32_t>(t);
    const unsigned long long won = block_exchange(lanes::lanes_fold<32>(first, lane, key_min), keys, turn, lane, wave, waves_min);
    const unsigned long long won_next = block_exchange(lanes::lanes_fold<32>(second, lane, key_min), keys, turn, lane, wave, waves_min);
    put(won), put(won_next);
    // (d) the block sum on inputs whose additions round, twice in a row
    int sum_turn = 0;
    const double x = (1.0 + static_cast<double>(lane) / 3.0) * static_cast<double>(1 << (wave % 5));
    const double total = afa_block_sum(x, sums, sum_turn), total_next = afa_block_sum(x / 7.0, sums, sum_turn);
    put(total), put(total_next);
}
constexpr int kOwnerSelftestRows = 6 * (2 + 3) + 3 + 3 + 2 + 2 + 2 + 2;
static_assert(kOwnerSelftestRows <= 64, "byzagg.h promises the caller at most 64 rows");

}  // namespace

int launch_owner_loop_selftest(byz_ctx* ctx, int32_t* out, int32_t* n_rows, hipStream_t stream) {
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    owner_loop_selftest_kernel<<<1, kOwnerThreads, 0, stream>>>(out);
    *n_rows = kOwnerSelftestRows;
    return check_launch("owner_loop_selftest_kernel");
}

int afa_workspace(byz_ctx* ctx, int64_t n, AfaScratch* out) {
    out->info = &device_scalars(ctx)->afa;
    Carve c;
    c.take(&out->u, n);
    c.take(&out->r, n);
    c.take(&out->w, n);
    c.take(&out->kept, n);
    c.take(&out->round_of, n);
    return c.commit(ctx->afa);
}

// 2 <= n <= kAfaMaxRows and the parameters: the caller's business (api.hip), checked again before anything runs
int launch_afa_select(byz_ctx* ctx, const AfaScratch& t, const double* gram, int64_t n, const double* weights, double xi0,
                      double delta_xi, int64_t max_rounds, int32_t* kept_out, int32_t* round_of_out, double* score_out,
                      hipStream_t stream) {
    BYZ_REQUIRE(gram && n >= 2 && n <= kAfaMaxRows && xi0 >= 0.0 && delta_xi >= 0.0 && max_rounds >= 0,
                "afa select: bad arguments (n = %lld, xi0 = %g, delta_xi = %g, max_rounds = %lld)", (long long)n, xi0, delta_xi,
                (long long)max_rounds);
    {
        KernelTimer timer(ctx, BYZ_K_ROW_SORT, stream);
        afa_rows_kernel<<<static_cast<unsigned>(ceil_div(n, 256)), 256, 0, stream>>>(gram, weights, static_cast<int>(n), t.w, t.r);
        BYZ_TRY(check_launch("afa_rows_kernel"));
        afa_init_kernel<<<static_cast<unsigned>(ceil_div(n, kAfaInitThreads / 64)), kAfaInitThreads, 0, stream>>>(
            gram, t.w, static_cast<int>(n), t.u);
        BYZ_TRY(check_launch("afa_init_kernel"));
    }
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    const int rounds = static_cast<int>(max_rounds > n ? n : max_rounds);
    afa_loop_kernel<<<1, kOwnerThreads, 0, stream>>>(gram, t.u, t.r, t.w, static_cast<int>(n), xi0, delta_xi, rounds, t.kept, kept_out,
                                                   round_of_out != nullptr ? round_of_out : t.round_of, score_out, t.info);
    return check_launch("afa_loop_kernel");
}

}  // namespace byz
