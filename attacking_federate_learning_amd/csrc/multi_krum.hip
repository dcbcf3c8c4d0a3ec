// Multi-Krum's ranking (Blanchard et al. 2017, section 4): every row's Krum score -- ctx->scores, the reference's
// defences.py:33-34 as krum_select forms it -- ordered, the first m rows taken.
//
//   key    (canonical order-preserving score bits) << 32 | visit position (1, 0, 2, 3, ...: the reference's dict order), so
//          the ascending key order is the ranking: by value, a tie by visit position, every NaN behind +inf whatever its sign
//          bit, -0.0 folded onto +0.0.  Keys are distinct (visit positions are), the ranking is total; its first key with a
//          score below 1e20 is what krum_argmin picks.
//   sort   segment_sort_u64 (large_rows.hip): ONE segment of n_pad keys, n_pad a power of two, the tail padded with ~0ull
//          (above every row's key: a NaN row's key is 0xffffffff << 32 | visit position < 2^20)
//   take   one workgroup: selection[k] = row of key k (ranking order) and a flag per row, then the flags compacted into the
//          selected rows in ASCENDING order -- the list the row-list mean walks (numpy's np.mean(G[np.sort(sel)], axis=0)).
// Nothing here reads the distance matrix.  Work: O(n log^2 n) compare-exchanges in the sort, O(n) elsewhere.
#include "common.hpp"
#include "order_keys.hpp"

namespace byz {
namespace {

constexpr int kTakeThreads = 1024;

__global__ __launch_bounds__(256) void multi_krum_keys_kernel(const float* __restrict__ scores, int n, int64_t n_pad,
                                                              unsigned long long* __restrict__ keys) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_pad) return;
    unsigned long long key = ~0ull;
    if (i < n)
        key = (static_cast<unsigned long long>(ordered_bits_total(scores[i])) << 32) |
              static_cast<unsigned>(visit_position(static_cast<int>(i)));
    keys[i] = key;
}

// flags: n int32, zero on entry (the launcher clears them); rows_asc: m int32
__global__ __launch_bounds__(kTakeThreads) void multi_krum_take_kernel(const unsigned long long* __restrict__ keys, int n, int m,
                                                                       int32_t* __restrict__ selection, int32_t* __restrict__ flags,
                                                                       int32_t* __restrict__ rows_asc) {
    __shared__ int offsets[kTakeThreads];
    const int tid = threadIdx.x;
    for (int k = tid; k < m; k += kTakeThreads) {
        const int row = row_of_visit(static_cast<int>(keys[k] & 0xffffffffull));
        if (selection != nullptr) selection[k] = row;
        flags[row] = 1;
    }
    __syncthreads();                                       // (workgroup scope: the flags are visible to every thread below)
    // compaction: thread t owns rows [t chunk, (t + 1) chunk); an exclusive scan of the counts gives its first slot
    const int chunk = (n + kTakeThreads - 1) / kTakeThreads;
    const int lo = tid * chunk < n ? tid * chunk : n;
    const int hi = lo + chunk < n ? lo + chunk : n;
    int count = 0;
    for (int r = lo; r < hi; ++r) count += flags[r];
    int slot = block_exclusive_scan<kTakeThreads>(count, offsets, nullptr);
    for (int r = lo; r < hi; ++r)
        if (flags[r] != 0 && slot < m) rows_asc[slot++] = r;
}

}  // namespace

int launch_multi_krum_rank(byz_ctx* ctx, int64_t n, int64_t m, int32_t* selection_dev, int32_t* rows_asc_dev, hipStream_t stream) {
    BYZ_REQUIRE(n >= 1 && n <= kLargeMaxRows && m >= 1 && m <= n && rows_asc_dev, "multi-krum ranking: bad arguments (n %lld, m %lld)",
                (long long)n, (long long)m);
    BYZ_REQUIRE(ctx->scores.bytes >= static_cast<size_t>(n) * sizeof(float), "multi-krum ranking: no scores (run krum_select first)");
    const int64_t n_pad = next_pow2(n < 2 ? 2 : n);
    unsigned long long* keys = nullptr;
    int32_t* flags = nullptr;
    Carve c;
    c.take(&keys, n_pad);
    c.take(&flags, n);
    BYZ_TRY(c.commit(ctx->multi_krum));
    KernelTimer t(ctx, BYZ_K_KRUM_ARGMIN, stream);
    BYZ_HIP(hipMemsetAsync(flags, 0, static_cast<size_t>(n) * sizeof(int32_t), stream));
    multi_krum_keys_kernel<<<static_cast<unsigned>(ceil_div(n_pad, 256)), 256, 0, stream>>>(ctx->scores.as<float>(), (int)n, n_pad, keys);
    BYZ_TRY(check_launch("multi_krum_keys_kernel"));
    BYZ_TRY(segment_sort_u64(ctx, keys, 1, n_pad, stream));
    multi_krum_take_kernel<<<1, kTakeThreads, 0, stream>>>(keys, (int)n, (int)m, selection_dev, flags, rows_asc_dev);
    return check_launch("multi_krum_take_kernel");
}

}  // namespace byz
