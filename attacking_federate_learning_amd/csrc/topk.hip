// Global top-k along ONE vector, with the error-feedback addition fused in: SparseFed's sparsification step (Panda, Mahloujifar,
// Bhagoji, Chakraborty and Mittal, "SparseFed: Mitigating Model Poisoning Attacks in Federated Learning with Sparsification",
// AISTATS 2022; beyond the reference), and what top-k gradient compression needs.  Every other radix select of the library
// (tall_select.hip, rank_select.hip) walks down the rows of a column tile; this one selects along the columns.
//
//   w[c]        = add ? fl32(x[c] + add[c]) : x[c]                     one fp32 addition
//   key[c]      = bits(w[c]) & 0x7fffffff                              31 bits, compared as integers whatever the denormal mode
//   selected    = the k columns first in the order (key descending, column ascending)
//   out[c]      = selected ? w[c] : +0.0        residual[c] = selected ? +0.0 : w[c]           w's bits verbatim
//
// +0.0 and -0.0 tie at key 0, denormals rank by their bits, both infinities rank above every finite value and a NaN of either
// sign above the infinities, where its bits fall.  NOTHING IS SANITISED (bucketing's and the robust learning rate's convention):
// a NaN in the memory is selected first and shows in the step instead of being parked in the memory for ever.
// With T the k-th largest key: every column with key > T is selected (`above` of them) and of the `ties` columns with key == T
// the first k - above in index order.  The order is total, so two runs, an aligned and a misaligned caller and the ranks of the
// columns layout select the same set.
//
// The passes, all enqueued up front, nothing read by the host:
//   3 x (histogram, find)   a most-significant-digit-first radix select over the key, 11 + 10 + 10 bits.  A workgroup counts the
//                           digits of its chunk's keys that carry the prefix found so far in an LDS histogram (integer LDS
//                           atomics; a thread first combines the equal digits among its own four values, so that a vector whose
//                           keys share one digit costs a quarter of the same-address atomics) and flushes its non-zero bins to
//                           the pass's global histogram (64-bit integer atomics).  One workgroup then walks the bins from the top
//                           and records the digit, the prefix and the count left.  After the third: T, ties, the quota k - above.
//   tie count, tie scan     only when 0 < quota < ties (read from the device; they return at once otherwise): the ties of every
//                           chunk, then their exclusive scan by one workgroup.
//   apply                   recomputes w, writes out and residual.  When the ties are rationed a tie's global rank is its chunk's
//                           base plus block_exclusive_scan (order_keys.hpp) over the chunk's tiles in index order.
// Only integer atomics anywhere: they commute, so no bit depends on the scheduling.  x and add are only read until the apply pass,
// and there every thread reads its own columns before it writes them: residual may be x and out may be add.
// A chunk is a contiguous run of whole tiles (kThreads * VEC columns); the grid is min(tiles, kChunksPerCu * CUs) chunks, sized
// from the CU count and never from n alone.  dwordx4 accesses (VEC = 4) when all four vectors are 16-byte aligned and n fills
// the chip, with a masked last vector; one column per thread otherwise.
// Algorithmic traffic: (3 + 1) reads of 4 or 8 bytes per element (+ 1 when the ties are rationed) and 4 or 8 bytes written.
// The columns layout: the same kernels on a rank's slice, each pass's bins all-reduced as doubles in front of the find (a count
// is exact as a double), and the ranks' ties at T gathered by summation, from which a rank takes its share of the quota after
// the ranks before it.
#include "order_keys.hpp"
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kThreads = kWalkThreads;
constexpr int kChunksPerCu = 8;
constexpr int kMaxBins = 2048;                       // 2^11: the first pass's digit
constexpr uint32_t kKeyMask = 0x7fffffffu;
constexpr uint32_t kNoKey = 0xffffffffu;             // the threshold of k = 0: above every key

// digit p of the key: bits [shift, shift + bits); the prefix above it: key >> (shift + bits)
__host__ __device__ constexpr int pass_shift(int p) { return p == 0 ? 20 : (p == 1 ? 10 : 0); }
__host__ __device__ constexpr int pass_bits(int p) { return p == 0 ? 11 : 10; }

// what the find kernels leave for the passes behind them (one 16-byte aligned block of the workspace, zeroed per call)
struct TopkState {
    unsigned long long left;        // keys still to take among those that carry the prefix
    unsigned long long ties;        // keys == T (this rank's, once the shares are dealt)
    unsigned long long quota;       // of them the first `quota` in index order are selected (this rank's likewise)
    unsigned long long before;      // ties on the ranks before this one (columns layout)
    uint32_t prefix;                // the digits found so far; after the last pass T itself
    uint32_t pad;
};

__device__ __forceinline__ uint32_t key_of(float w) { return __float_as_uint(w) & kKeyMask; }

// the VEC values w at c0 (a masked column reads +0.0; the callers tell it apart by c0 + v < n)
template <int VEC, bool ADD>
__device__ __forceinline__ void load_w(const float* x, const float* add, int64_t c0, int64_t n, float (&w)[VEC]) {
    const bool full = c0 + VEC <= n;
    load_columns<VEC>(x + c0, full, c0, n, w);
    if constexpr (ADD) {
        float a[VEC];
        load_columns<VEC>(add + c0, full, c0, n, a);
#pragma unroll
        for (int v = 0; v < VEC; ++v) w[v] = w[v] + a[v];
    }
}

// ---- histogram of digit `pass` over the keys that carry the prefix -------------------------------------------------------------
// (PASS is a template parameter: the shifts are immediates, and a kernel trace tells the three passes apart)
template <int VEC, bool ADD, int PASS>
__global__ __launch_bounds__(kThreads) void topk_hist_kernel(const float* __restrict__ x, const float* __restrict__ add, int64_t n,
                                                             int64_t chunk_len, const TopkState* __restrict__ state,
                                                             unsigned long long* __restrict__ hist) {
    constexpr int shift = pass_shift(PASS), bits = pass_bits(PASS), n_bins = 1 << bits;
    // (four privatised copies of this histogram, a lane adding to copy lane % 4, were measured and taken out again: the first
    // pass went from 50.0 to 48.9 us at n = 1e7, profiles/sparsefed_timing.md)
    __shared__ uint32_t bins[n_bins];
    for (int b = threadIdx.x; b < n_bins; b += kThreads) bins[b] = 0;
    const uint32_t prefix = PASS == 0 ? 0u : state->prefix;
    __syncthreads();
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * chunk_len;
    const int64_t end = begin + chunk_len < n ? begin + chunk_len : n;
    const uint32_t digit_mask = static_cast<uint32_t>(n_bins - 1);
    for (int64_t c0 = begin + static_cast<int64_t>(threadIdx.x) * VEC; c0 < end; c0 += static_cast<int64_t>(kThreads) * VEC) {
        float w[VEC];
        load_w<VEC, ADD>(x, add, c0, n, w);
        uint32_t digit[VEC];
        uint32_t count[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const uint32_t key = key_of(w[v]);
            digit[v] = (key >> shift) & digit_mask;
            count[v] = (c0 + v < n && (key >> (shift + bits)) == prefix) ? 1u : 0u;
        }
        // a run of equal digits among the thread's own values becomes one atomic: the count moves to the run's last value
#pragma unroll
        for (int v = 0; v + 1 < VEC; ++v) {
            if (digit[v] == digit[v + 1]) {
                count[v + 1] += count[v];
                count[v] = 0;
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            if (count[v] != 0) atomicAdd(&bins[digit[v]], count[v]);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_bins; b += kThreads) {
        const uint32_t h = bins[b];
        if (h != 0) atomicAdd(&hist[b], static_cast<unsigned long long>(h));
    }
}

// the bins as doubles, for the caller's all-reduce (a count below 2^53 is exact)
__global__ __launch_bounds__(kThreads) void topk_bins_f64_kernel(const unsigned long long* __restrict__ hist, int n_bins,
                                                                 double* __restrict__ out) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b < n_bins) out[b] = static_cast<double>(hist[b]);
}

// ---- one workgroup: the bins walked from the top ------------------------------------------------------------------------------
// hist_f64 != nullptr: the all-reduced bins of every rank (then hist is this rank's own, read for its ties after the last pass
// and written as a double into gather[rank_index]).  info: the four values byz_topk_info reports, written after the last pass.
__global__ __launch_bounds__(kThreads) void topk_find_kernel(const unsigned long long* __restrict__ hist, const double* __restrict__ hist_f64,
                                                             int pass, unsigned long long k, TopkState* __restrict__ state,
                                                             double* __restrict__ gather, int rank_index,
                                                             TopkReport* __restrict__ info) {
    __shared__ unsigned long long scan[kThreads];
    const int bits = pass_bits(pass), n_bins = 1 << bits, per = n_bins / kThreads;   // 8 or 4 bins a thread
    const int tid = threadIdx.x;
    const unsigned long long left = pass == 0 ? k : state->left;
    const uint32_t prefix = pass == 0 ? 0u : state->prefix;
    // thread t owns the bins [top - per + 1, top] with top = n_bins - 1 - t * per: thread 0 the highest digits
    const int top = n_bins - 1 - tid * per;
    unsigned long long h[kMaxBins / kThreads];
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < kMaxBins / kThreads; ++j) {
        h[j] = 0;
        if (j < per) h[j] = hist_f64 != nullptr ? static_cast<unsigned long long>(hist_f64[top - j]) : hist[top - j];
        mine += h[j];
    }
    scan[tid] = mine;
    __syncthreads();
    for (int step = 1; step < kThreads; step <<= 1) {
        const unsigned long long a = tid >= step ? scan[tid - step] : 0;
        __syncthreads();
        scan[tid] += a;
        __syncthreads();
    }
    unsigned long long above = scan[tid] - mine;      // keys in the bins above this thread's
    const bool last = pass == 2;
    // exactly one thread holds the bin in which the count left runs out (1 <= left <= the keys that carry the prefix)
#pragma unroll
    for (int j = 0; j < kMaxBins / kThreads; ++j) {
        if (j < per) {
            if (above < left && left <= above + h[j]) {
                const uint32_t digit = static_cast<uint32_t>(top - j);
                const uint32_t found = (prefix << bits) | digit;
                const unsigned long long quota = left - above;
                state->prefix = found;
                state->left = quota;
                if (last) {
                    state->ties = h[j];
                    state->quota = quota;
                    info->selected = k;
                    info->ties = h[j];
                    info->taken = quota;
                    info->key = found;
                    if (gather != nullptr) gather[rank_index] = static_cast<double>(hist[top - j]);
                }
            }
            above += h[j];
        }
    }
    if (left == 0 && tid == 0) {      // k = 0: nothing is taken; the prefix stays above every key
        state->prefix = last ? kNoKey : ((prefix << bits) | static_cast<uint32_t>(n_bins - 1));
        state->left = 0;
        if (last) {
            state->ties = 0;
            state->quota = 0;
            info->selected = 0;
            info->ties = 0;
            info->taken = 0;
            info->key = kNoKey;
        }
    }
}

// columns layout: this rank's share of the quota, after the ranks before it (gather: every rank's ties at T)
__global__ void topk_share_kernel(const double* __restrict__ gather, int rank_index, TopkState* __restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long before = 0;
    for (int r = 0; r < rank_index; ++r) before += static_cast<unsigned long long>(gather[r]);
    const unsigned long long own = static_cast<unsigned long long>(gather[rank_index]);
    const unsigned long long quota = state->quota;
    unsigned long long share = quota > before ? quota - before : 0;
    if (share > own) share = own;
    state->before = before;
    state->ties = own;
    state->quota = share;
}

// the ties are rationed: neither all of them nor none is taken
__device__ __forceinline__ bool rationed(const TopkState* state) { return state->quota != 0 && state->quota != state->ties; }

// ---- the threshold ties of every chunk ----------------------------------------------------------------------------------------
template <int VEC, bool ADD>
__global__ __launch_bounds__(kThreads) void topk_tie_count_kernel(const float* __restrict__ x, const float* __restrict__ add, int64_t n,
                                                                  int64_t chunk_len, const TopkState* __restrict__ state,
                                                                  uint32_t* __restrict__ chunk_ties) {
    if (!rationed(state)) return;
    __shared__ int lds[kThreads];
    const uint32_t T = state->prefix;
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * chunk_len;
    const int64_t end = begin + chunk_len < n ? begin + chunk_len : n;
    int mine = 0;
    for (int64_t c0 = begin + static_cast<int64_t>(threadIdx.x) * VEC; c0 < end; c0 += static_cast<int64_t>(kThreads) * VEC) {
        float w[VEC];
        load_w<VEC, ADD>(x, add, c0, n, w);
#pragma unroll
        for (int v = 0; v < VEC; ++v) mine += (c0 + v < n && key_of(w[v]) == T) ? 1 : 0;
    }
    const int total = block_sum<int, kThreads>(mine, lds);
    if (threadIdx.x == 0) chunk_ties[blockIdx.x] = static_cast<uint32_t>(total);
}

// one workgroup: chunk_base[b] = the ties in the chunks before b
__global__ __launch_bounds__(kThreads) void topk_tie_scan_kernel(const uint32_t* __restrict__ chunk_ties, int n_chunks,
                                                                 const TopkState* __restrict__ state,
                                                                 unsigned long long* __restrict__ chunk_base) {
    if (!rationed(state)) return;
    __shared__ unsigned long long scan[kThreads];
    const int tid = threadIdx.x;
    unsigned long long carry = 0;
    for (int b0 = 0; b0 < n_chunks; b0 += kThreads) {
        const unsigned long long mine = b0 + tid < n_chunks ? chunk_ties[b0 + tid] : 0;
        scan[tid] = mine;
        __syncthreads();
        for (int step = 1; step < kThreads; step <<= 1) {
            const unsigned long long a = tid >= step ? scan[tid - step] : 0;
            __syncthreads();
            scan[tid] += a;
            __syncthreads();
        }
        if (b0 + tid < n_chunks) chunk_base[b0 + tid] = carry + scan[tid] - mine;
        carry += scan[kThreads - 1];
        __syncthreads();
    }
}

// ---- apply: out and residual ------------------------------------------------------------------------------------------------
template <int VEC>
__device__ __forceinline__ void store_columns(float* p, int64_t c0, int64_t n, const float (&y)[VEC]) {
    if constexpr (VEC == 4) {
        if (c0 + VEC <= n) {
            float4u q;
            q.x = y[0]; q.y = y[1]; q.z = y[2]; q.w = y[3];
            *reinterpret_cast<float4u*>(p + c0) = q;
            return;
        }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        if (c0 + v < n) p[c0 + v] = y[v];
}

// x, add, out and residual carry no __restrict__: residual may be x and out may be add (a thread reads its columns, then writes them)
template <int VEC, bool ADD>
__global__ __launch_bounds__(kThreads) void topk_apply_kernel(const float* x, const float* add, int64_t n, int64_t chunk_len,
                                                              const TopkState* __restrict__ state,
                                                              const unsigned long long* __restrict__ chunk_base, float* out,
                                                              float* residual) {
    __shared__ int lds[kThreads];
    const uint32_t T = state->prefix;
    const unsigned long long quota = state->quota;
    const bool ration = rationed(state);                                  // the same for the whole grid
    const bool take_ties = quota != 0;                                    // (not rationed: all of them or none)
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * chunk_len;
    const int64_t end = begin + chunk_len < n ? begin + chunk_len : n;
    unsigned long long rank_base = ration ? chunk_base[blockIdx.x] : 0;   // ties in front of the tile being written
    // whole tiles: every thread of the workgroup meets in the scan
    for (int64_t t0 = begin; t0 < end; t0 += static_cast<int64_t>(kThreads) * VEC) {
        const int64_t c0 = t0 + static_cast<int64_t>(threadIdx.x) * VEC;
        float w[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) w[v] = 0.0f;
        if (c0 < end) load_w<VEC, ADD>(x, add, c0, n, w);
        bool tie[VEC];
        bool sel[VEC];
        int mine = 0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const uint32_t key = key_of(w[v]);
            tie[v] = c0 + v < n && key == T;
            sel[v] = key > T || (tie[v] && take_ties);
            mine += tie[v] ? 1 : 0;
        }
        if (ration) {
            int tile_total = 0;
            const int before = block_exclusive_scan<kThreads>(mine, lds, &tile_total);
            __syncthreads();                                              // lds is free for the next tile
            unsigned long long r = rank_base + static_cast<unsigned long long>(before);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (tie[v]) {
                    sel[v] = r < quota;
                    ++r;
                }
            }
            rank_base += static_cast<unsigned long long>(tile_total);
        }
        if (c0 < end) {
            float y[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) y[v] = sel[v] ? w[v] : 0.0f;
            store_columns<VEC>(out, c0, n, y);
            if (residual != nullptr) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) y[v] = sel[v] ? 0.0f : w[v];
                store_columns<VEC>(residual, c0, n, y);
            }
        }
    }
}

// the workspace of one call over n columns on a context (ctx->topk): the zeroed block (three histograms, the state), the chunk
// arrays, the doubles of the columns layout, and `agg_cols` floats for SparseFed's aggregate (last: the arrays before it lie
// where a call without it puts them)
struct TopkScratch {
    unsigned long long* zeroed;
    unsigned long long* chunk_base;
    uint32_t* chunk_ties;
    double* f64;
    float* agg;
    bool vec4;
    int64_t chunk_len;
    int n_chunks;
};
constexpr int64_t kStateWords = static_cast<int64_t>(sizeof(TopkState) / sizeof(unsigned long long));
static_assert(sizeof(TopkState) % sizeof(unsigned long long) == 0, "the state is zeroed as 64-bit words");

int topk_scratch(byz_ctx* ctx, int64_t n, int rank_count, int64_t agg_cols, bool aligned, TopkScratch* t) {
    const int64_t max_chunks = static_cast<int64_t>(kChunksPerCu) * ctx->num_cus;
    t->vec4 = aligned && n >= static_cast<int64_t>(4) * kThreads * ctx->num_cus;
    const int64_t tile = static_cast<int64_t>(kThreads) * (t->vec4 ? 4 : 1);
    const int64_t tiles = n > 0 ? ceil_div(n, tile) : 1;
    const int64_t chunks = tiles < max_chunks ? tiles : max_chunks;
    t->chunk_len = ceil_div(tiles, chunks) * tile;
    t->n_chunks = static_cast<int>(n > 0 ? ceil_div(n, t->chunk_len) : 0);
    if (t->chunk_len >= (int64_t{1} << 31)) {     // a chunk's counts are 32-bit
        set_error("topk: %lld columns is beyond one call", (long long)n);
        return BYZ_E_UNSUPPORTED;
    }
    Carve c;
    c.take(&t->zeroed, 3 * kMaxBins + kStateWords);
    c.take(&t->chunk_base, max_chunks);
    c.take(&t->chunk_ties, max_chunks);
    c.take(&t->f64, kMaxBins + rank_count);
    c.take(&t->agg, agg_cols);
    return c.commit(ctx->topk);
}

// one select pass: the histogram, the all-reduce of its bins (columns layout), the find
template <int VEC, bool ADD, int PASS>
int topk_pass(byz_ctx* ctx, const TopkScratch& t, const float* x, const float* add, int64_t n, int64_t k, int rank_index,
              byz_allreduce_f64_fn allreduce, void* user, TopkState* state, double* gather, void* stream) {
    hipStream_t s = as_stream(stream);
    unsigned long long* hist = t.zeroed + PASS * kMaxBins;
    constexpr int n_bins = 1 << pass_bits(PASS);
    if (t.n_chunks > 0) {
        KernelTimer timer(ctx, BYZ_K_COLUMN_STATS, s);
        topk_hist_kernel<VEC, ADD, PASS><<<static_cast<unsigned>(t.n_chunks), kThreads, 0, s>>>(x, add, n, t.chunk_len, state, hist);
        BYZ_TRY(check_launch("topk_hist_kernel"));
    }
    if (allreduce != nullptr) {
        topk_bins_f64_kernel<<<n_bins / kThreads, kThreads, 0, s>>>(hist, n_bins, t.f64);
        BYZ_TRY(check_launch("topk_bins_f64_kernel"));
        const int rc = allreduce(user, t.f64, n_bins, stream);
        if (rc != 0) {
            set_error("sharded top-k (bins of pass %d): the caller's all-reduce returned %d", PASS, rc);
            return BYZ_E_COLLECTIVE;
        }
    }
    KernelTimer timer(ctx, BYZ_K_MISC, s);
    topk_find_kernel<<<1, kThreads, 0, s>>>(hist, allreduce != nullptr ? t.f64 : nullptr, PASS, static_cast<unsigned long long>(k),
                                            state, allreduce != nullptr ? gather : nullptr, rank_index, &device_scalars(ctx)->topk);
    return check_launch("topk_find_kernel");
}

template <int VEC, bool ADD>
int topk_launches(byz_ctx* ctx, const TopkScratch& t, const float* x, const float* add, int64_t n, int64_t k, int rank_index,
                  int rank_count, byz_allreduce_f64_fn allreduce, void* user, float* out, float* residual, void* stream) {
    hipStream_t s = as_stream(stream);
    TopkState* state = reinterpret_cast<TopkState*>(t.zeroed + 3 * kMaxBins);
    double* gather = t.f64 + kMaxBins;
    BYZ_HIP(hipMemsetAsync(t.zeroed, 0, static_cast<size_t>(3 * kMaxBins + kStateWords) * sizeof(unsigned long long), s));
    if (allreduce != nullptr) BYZ_HIP(hipMemsetAsync(gather, 0, static_cast<size_t>(rank_count) * sizeof(double), s));
    const unsigned grid = static_cast<unsigned>(t.n_chunks);
    BYZ_TRY((topk_pass<VEC, ADD, 0>(ctx, t, x, add, n, k, rank_index, allreduce, user, state, gather, stream)));
    BYZ_TRY((topk_pass<VEC, ADD, 1>(ctx, t, x, add, n, k, rank_index, allreduce, user, state, gather, stream)));
    BYZ_TRY((topk_pass<VEC, ADD, 2>(ctx, t, x, add, n, k, rank_index, allreduce, user, state, gather, stream)));
    if (allreduce != nullptr) {
        const int rc = allreduce(user, gather, rank_count, stream);
        if (rc != 0) {
            set_error("sharded top-k (ties of the ranks): the caller's all-reduce returned %d", rc);
            return BYZ_E_COLLECTIVE;
        }
        topk_share_kernel<<<1, 64, 0, s>>>(gather, rank_index, state);
        BYZ_TRY(check_launch("topk_share_kernel"));
    }
    if (grid == 0) return BYZ_OK;
    {
        KernelTimer timer(ctx, BYZ_K_MISC, s);
        topk_tie_count_kernel<VEC, ADD><<<grid, kThreads, 0, s>>>(x, add, n, t.chunk_len, state, t.chunk_ties);
        BYZ_TRY(check_launch("topk_tie_count_kernel"));
        topk_tie_scan_kernel<<<1, kThreads, 0, s>>>(t.chunk_ties, t.n_chunks, state, t.chunk_base);
        BYZ_TRY(check_launch("topk_tie_scan_kernel"));
    }
    KernelTimer timer(ctx, BYZ_K_COLUMN_STATS, s);
    topk_apply_kernel<VEC, ADD><<<grid, kThreads, 0, s>>>(x, add, n, t.chunk_len, state, t.chunk_base, out, residual);
    return check_launch("topk_apply_kernel");
}

}  // namespace

float* topk_aggregate_workspace(byz_ctx* ctx, int64_t n_cols) {
    TopkScratch t;
    if (topk_scratch(ctx, n_cols, 1, n_cols, true, &t) != BYZ_OK) return nullptr;
    return t.agg;
}

// allreduce == nullptr: this GPU holds the whole vector (rank 0 of 1).  0 <= k <= the global length and the overlaps are the
// caller's business (api.hip).  n may be 0 on a rank of the columns layout that holds no column.
int launch_topk_sparsify(byz_ctx* ctx, const float* x, const float* add, int64_t n, int64_t k, int rank_index, int rank_count,
                         byz_allreduce_f64_fn allreduce, void* user, float* out, float* residual, int64_t keep_agg_cols, void* stream) {
    const bool aligned = aligned16(x) && aligned16(out) && (add == nullptr || aligned16(add)) && (residual == nullptr || aligned16(residual));
    TopkScratch t;
    BYZ_TRY(topk_scratch(ctx, n, rank_count, keep_agg_cols, aligned, &t));
    if (add != nullptr) {
        if (t.vec4) return topk_launches<4, true>(ctx, t, x, add, n, k, rank_index, rank_count, allreduce, user, out, residual, stream);
        return topk_launches<1, true>(ctx, t, x, add, n, k, rank_index, rank_count, allreduce, user, out, residual, stream);
    }
    if (t.vec4) return topk_launches<4, false>(ctx, t, x, add, n, k, rank_index, rank_count, allreduce, user, out, residual, stream);
    return topk_launches<1, false>(ctx, t, x, add, n, k, rank_index, rank_count, allreduce, user, out, residual, stream);
}

}  // namespace byz
