// Nearest-neighbour mixing (Allouah, Farhadkhani, Guerraoui, Gupta, Pinot and Stephan, "Fixing by Mixing", AISTATS 2023): every
// row is replaced by the mean of its k = n - f nearest rows, itself included; the mixed matrix then goes to Krum, a trimmed
// mean, a median.  A pre-aggregation: n x D in, n x D out.
//
//   keys    key[i][j] = (order-preserving distance bits) << 32 | j for j != i, ~0 for the diagonal and the padding: ascending
//           key order is (distance, j), -0.0 folded onto +0.0, every NaN behind +inf.  Keys of one row are distinct, so the
//           order is total and ties (the attack's f identical rows) fall the same way on every run.
//   sort    segment_sort_u64 (large_rows.hip): n segments of next_pow2(n) keys
//   take    one workgroup a row: the first k - 1 keys whose distance is finite, and i itself, flagged in an LDS bitmap; the
//           bitmap compacted to the ASCENDING list (block_exclusive_scan, on words of 32 rows); the tail -1
//   mask    A^T as fp32 zeros and ones, [j][i], scattered from the lists: the mix takes ANY lists, so this is the one way in
//   mix     Y = diag(1 / k_i) A G on v_mfma_f32_32x32x2_f32, which is bit for bit a k-ordered fmaf chain: with a multiplier of
//           exactly 1 or 0, fma(1, x, c) = fl32(c + x) and fma(0, x, c) = c for finite x, so ONE accumulator chain over
//           j = 0 .. n - 1 in ascending order is the sequential fp32 sum of the listed rows from +0.0 -- numpy's
//           np.mean(G[list], axis=0) once divided by (float)k_i.  No split-K, no partial sums, no reordering of K blocks: every
//           output element lives in one accumulator register from the first K block to the last.  G is staged through
//           isfinite(x) ? x : 0, so that a zero multiplier never meets an inf or a NaN; a row that is in anyone's list has only
//           finite values, so no value that is used changes.  A row with k_i == 1 is its own G row, copied verbatim.
//
// The mix kernel: a 128 (rows of Y) x 128 (columns) tile a workgroup, 4 waves of 2 x 2 blocks of 32 x 32, K blocks of 16 rows
// of G.  Both operands are read along their contiguous dimension (A^T[j][i] along i, G[j][c] along c) and land in LDS as
// [k][x]; a lane's MFMA operand is one float: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][c = lane & 31].  The next K
// block's global loads are issued before the current block's MFMAs.  Workgroups are numbered so that the row tiles of one
// column panel run next to each other on ONE XCD: the panel is read from HBM once and then served by that XCD's L2.
#include "common.hpp"
#include "lane_exchange.hpp"
#include "order_keys.hpp"

namespace byz {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kKeyThreads = 256;
constexpr int kTakeThreads = 256;
constexpr int kMaxRows = static_cast<int>(kNnmMaxRows);   // 16,384: the keys and the mask are n x n
constexpr int kBitmapWords = kMaxRows / 32;           // 512
constexpr int kWordsPerThread = kBitmapWords / kTakeThreads;   // 2

// grid (n_pad / 256, n): keys[i * n_pad + r]
__global__ __launch_bounds__(kKeyThreads) void nnm_keys_kernel(const float* __restrict__ dist, int n, int64_t n_pad,
                                                               unsigned long long* __restrict__ keys) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kKeyThreads + threadIdx.x;
    const int i = blockIdx.y;
    if (r >= n_pad) return;
    unsigned long long key = ~0ull;
    if (r < n && r != i)
        key = (static_cast<unsigned long long>(ordered_bits_total(dist[static_cast<int64_t>(i) * n + r])) << 32) |
              static_cast<unsigned long long>(r);
    keys[static_cast<int64_t>(i) * n_pad + r] = key;
}

// one workgroup a row.  nbr: n x k int32 (ascending, then -1); counts (optional): n; report: the context's, zeroed before
__global__ __launch_bounds__(kTakeThreads) void nnm_take_kernel(const unsigned long long* __restrict__ keys, int n, int64_t n_pad,
                                                                int k, int32_t* __restrict__ nbr, int32_t* __restrict__ counts,
                                                                NnmReport* __restrict__ report) {
    __shared__ uint32_t bitmap[kBitmapWords];
    __shared__ int offsets[kTakeThreads];
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    for (int w = tid; w < kBitmapWords; w += kTakeThreads) bitmap[w] = 0u;
    __syncthreads();
    const unsigned long long* row_keys = keys + static_cast<int64_t>(i) * n_pad;
    // the first k - 1 candidates (k - 1 <= n - 1 real keys: none of them the diagonal or the padding)
    for (int r = tid; r < k - 1; r += kTakeThreads) {
        const unsigned long long key = row_keys[r];
        const int j = static_cast<int>(key & 0xffffffffull);
        if (ordered_is_finite(static_cast<uint32_t>(key >> 32)) && j >= 0 && j < n) atomicOr(&bitmap[j >> 5], 1u << (j & 31));
    }
    if (tid == 0) atomicOr(&bitmap[i >> 5], 1u << (i & 31));
    __syncthreads();
    // compaction: thread t owns words [2t, 2t + 2); an exclusive scan of the population counts gives its first slot
    int count = 0;
#pragma unroll
    for (int w = 0; w < kWordsPerThread; ++w) count += __popc(bitmap[tid * kWordsPerThread + w]);
    int k_i;
    int slot = block_exclusive_scan<kTakeThreads>(count, offsets, &k_i);
    int32_t* list = nbr + static_cast<int64_t>(i) * k;
#pragma unroll
    for (int w = 0; w < kWordsPerThread; ++w) {
        uint32_t bits = bitmap[tid * kWordsPerThread + w];
        while (bits != 0u) {
            const int b = __ffs(static_cast<int>(bits)) - 1;
            bits &= bits - 1u;
            if (slot < k) list[slot] = (tid * kWordsPerThread + w) * 32 + b;
            ++slot;
        }
    }
    for (int t = k_i + tid; t < k; t += kTakeThreads) list[t] = -1;
    if (tid == 0) {
        if (counts != nullptr) counts[i] = k_i;
        if (k_i < k) atomicAdd(&report->short_rows, 1);
        if (k_i == 1 && k > 1) atomicAdd(&report->solo, 1);
    }
}

// The lists as the mix reads them: mask_t[j * m_pad + i] = 1 for every j in list_i (mask_t zeroed before), k_i into row_count.
// One wave a row.  counts (optional): the caller's lengths; without them a list ends at its first negative entry.  An entry
// outside [0, n) is not written (and not counted).
__global__ __launch_bounds__(64) void nnm_mask_kernel(const int32_t* __restrict__ nbr, const int32_t* __restrict__ counts, int n,
                                                      int k, int64_t m_pad, float* __restrict__ mask_t,
                                                      int32_t* __restrict__ row_count) {
    const int i = blockIdx.x;
    const int lane = threadIdx.x;
    const int32_t* list = nbr + static_cast<int64_t>(i) * k;
    int limit = k;
    if (counts != nullptr) {
        limit = counts[i];
        limit = limit < 0 ? 0 : (limit > k ? k : limit);
    }
    int mine = 0;
    bool open = true;                        // (no counts: entries behind the first negative one are not read)
    for (int t0 = 0; t0 < limit && open; t0 += 64) {
        const int t = t0 + lane;
        const int j = t < limit ? list[t] : -1;
        const unsigned long long negative = __ballot(t < limit && j < 0);
        const bool before = negative == 0ull || lane < __ffsll(static_cast<long long>(negative)) - 1;
        if ((counts != nullptr || before) && j >= 0 && j < n) {
            mask_t[static_cast<int64_t>(j) * m_pad + i] = 1.0f;
            ++mine;
        }
        if (counts == nullptr && negative != 0ull) open = false;
    }
    mine = lanes::wave_sum_shfl(mine);
    if (lane == 0) row_count[i] = mine;
}

// ---- the mix ------------------------------------------------------------------------------------------------------------
constexpr int MIX_THREADS = 256;
constexpr int BM = 128;                  // rows of Y a workgroup
constexpr int BN = 128;                  // columns a workgroup
constexpr int BK = 16;                   // rows of G a K block
constexpr int LDS_LD = BM + 32;          // row k + 1 starts 32 banks behind row k: a wave's two half-reads do not collide

__device__ __forceinline__ float finite_or_zero(float x) { return __builtin_isfinite(x) ? x : 0.0f; }

// VEC: G's base and rows are 16-byte aligned (16-byte loads where a whole chunk of 4 columns exists); otherwise every value is
// loaded on its own.  mask_t: k_pad x m_pad with k_pad a multiple of BK and m_pad a multiple of BM, zero outside n x n, so the
// A operand needs no bounds at all.
template <bool VEC>
__global__ __launch_bounds__(MIX_THREADS, 2) void nnm_mix_kernel(const float* __restrict__ G, int n, int64_t n_cols, int64_t ld,
                                                                 const float* __restrict__ mask_t, int64_t m_pad,
                                                                 const int32_t* __restrict__ row_count, float* __restrict__ Y,
                                                                 int64_t ldy, int tiles_m, int64_t n_tiles) {
    __shared__ __attribute__((aligned(16))) float lds_a[BK * LDS_LD];
    __shared__ __attribute__((aligned(16))) float lds_b[BK * LDS_LD];

    // Workgroups are dealt to the 8 XCDs round-robin (only speed depends on it): XCD x walks its own contiguous share of the
    // tile list, row tile fastest, so the row tiles of a column panel follow each other on one XCD.
    const int64_t per_xcd = (n_tiles + 7) / 8;
    const int64_t tile = static_cast<int64_t>(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if ((blockIdx.x >> 3) >= per_xcd || tile >= n_tiles) return;
    const int tm = static_cast<int>(tile % tiles_m);
    const int64_t tn = tile / tiles_m;
    const int i0 = tm * BM;
    const int64_t c0 = tn * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;

    // staging: 32 threads cover one 128-float row, 8 rows a pass, 2 passes an operand
    const int ld_chunk = tid & 31;
    const int ld_row = tid >> 5;
    const int64_t col = c0 + 4 * ld_chunk;
    const int n_blocks = (n + BK - 1) / BK;

    f32x4 ra[2], rb[2];
    auto fetch = [&](int kb) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int j = kb * BK + ld_row + 8 * p;
            ra[p] = *reinterpret_cast<const f32x4*>(mask_t + static_cast<int64_t>(j) * m_pad + i0 + 4 * ld_chunk);
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (j < n) {
                const float* src = G + static_cast<int64_t>(j) * ld + col;
                if (VEC && col + 3 < n_cols) {
                    v = *reinterpret_cast<const f32x4*>(src);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e < n_cols) v[e] = src[e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = finite_or_zero(v[e]);
            rb[p] = v;
        }
    };
    auto stash = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            *reinterpret_cast<f32x4*>(lds_a + (ld_row + 8 * p) * LDS_LD + 4 * ld_chunk) = ra[p];
            *reinterpret_cast<f32x4*>(lds_b + (ld_row + 8 * p) * LDS_LD + 4 * ld_chunk) = rb[p];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][q][e] = 0.0f;

    const int frag_x = lane & 31;
    const int frag_k = lane >> 5;

    fetch(0);
    for (int kb = 0; kb < n_blocks; ++kb) {
        __syncthreads();                       // the previous block's reads are done
        stash();
        __syncthreads();
        if (kb + 1 < n_blocks) fetch(kb + 1);  // in flight under this block's MFMAs
        // ascending k: block kb holds rows 16 kb .. 16 kb + 15 of G, one MFMA takes k = 2 kk, 2 kk + 1 in that order
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) a[m] = lds_a[(2 * kk + frag_k) * LDS_LD + wr * 64 + m * 32 + frag_x];
#pragma unroll
            for (int q = 0; q < 2; ++q) b[q] = lds_b[(2 * kk + frag_k) * LDS_LD + wc * 64 + q * 32 + frag_x];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[q], acc[m][q], 0, 0, 0);
        }
    }

    // epilogue: element e of a lane is row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31 of its 32 x 32 block
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = i0 + wr * 64 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            if (i >= n) continue;
            const int k_i = row_count[i];
            const float divisor = static_cast<float>(k_i);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int64_t c = c0 + wc * 64 + q * 32 + (lane & 31);
                if (c >= n_cols) continue;
                // a list of one row is that row, verbatim (NaN, inf and -0.0 included)
                Y[static_cast<int64_t>(i) * ldy + c] = k_i == 1 ? G[static_cast<int64_t>(i) * ld + c] : acc[m][q][e] / divisor;
            }
        }
    }
}

}  // namespace

int launch_nnm_neighbours(byz_ctx* ctx, const float* dist, int64_t n, int64_t k, int32_t* nbr, int32_t* counts, hipStream_t stream) {
    BYZ_REQUIRE(dist && nbr && n >= 1 && n <= kMaxRows && k >= 1 && k <= n, "nnm neighbours: bad arguments (n %lld, k %lld)",
                (long long)n, (long long)k);
    const int64_t n_pad = next_pow2(n < 2 ? 2 : n);
    BYZ_TRY(ctx->nnm_keys.ensure(static_cast<size_t>(n) * n_pad * 8));
    unsigned long long* keys = ctx->nnm_keys.as<unsigned long long>();
    KernelTimer t(ctx, BYZ_K_ROW_SORT, stream);
    NnmReport* report = &device_scalars(ctx)->nnm;
    BYZ_HIP(hipMemsetAsync(report, 0, sizeof *report, stream));
    nnm_keys_kernel<<<dim3(static_cast<unsigned>(ceil_div(n_pad, kKeyThreads)), static_cast<unsigned>(n)), kKeyThreads, 0, stream>>>(
        dist, (int)n, n_pad, keys);
    BYZ_TRY(check_launch("nnm_keys_kernel"));
    if (k > 1) BYZ_TRY(segment_sort_u64(ctx, keys, n, n_pad, stream));     // (k == 1 takes no candidate)
    nnm_take_kernel<<<static_cast<unsigned>(n), kTakeThreads, 0, stream>>>(keys, (int)n, n_pad, (int)k, nbr, counts, report);
    return check_launch("nnm_take_kernel");
}

int launch_nnm_mix(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, const int32_t* nbr, const int32_t* counts,
                   int64_t k, float* Y, int64_t ldy, hipStream_t stream) {
    BYZ_REQUIRE(G && nbr && Y && n >= 1 && n <= kMaxRows && k >= 1 && k <= n && n_cols >= 1 && ld >= n_cols && ldy >= n_cols,
                "nnm mix: bad arguments (n %lld, k %lld)", (long long)n, (long long)k);
    const int64_t m_pad = ceil_div(n, BM) * BM;
    const int64_t k_pad = ceil_div(n, BK) * BK;
    const size_t mask_bytes = static_cast<size_t>(k_pad) * m_pad * sizeof(float);
    float* mask_t = nullptr;
    int32_t* row_count = nullptr;
    Carve c;
    c.take(&mask_t, k_pad * m_pad);
    c.take(&row_count, n);
    BYZ_TRY(c.commit(ctx->nnm_mask));
    const int tiles_m = static_cast<int>(m_pad / BM);
    const int64_t n_tiles = static_cast<int64_t>(tiles_m) * ceil_div(n_cols, BN);
    const int64_t grid = ceil_div(n_tiles, 8) * 8;
    BYZ_REQUIRE(grid <= 0x7fffffff, "nnm mix: %lld tiles are too many for one launch (walk the columns in panels)", (long long)n_tiles);
    KernelTimer t(ctx, BYZ_K_MISC, stream);
    BYZ_HIP(hipMemsetAsync(mask_t, 0, mask_bytes, stream));
    nnm_mask_kernel<<<static_cast<unsigned>(n), 64, 0, stream>>>(nbr, counts, (int)n, (int)k, m_pad, mask_t, row_count);
    BYZ_TRY(check_launch("nnm_mask_kernel"));
    const bool vec = (reinterpret_cast<uintptr_t>(G) & 15) == 0 && (ld & 3) == 0;
    if (vec)
        nnm_mix_kernel<true><<<static_cast<unsigned>(grid), MIX_THREADS, 0, stream>>>(G, (int)n, n_cols, ld, mask_t, m_pad, row_count, Y,
                                                                                      ldy, tiles_m, n_tiles);
    else
        nnm_mix_kernel<false><<<static_cast<unsigned>(grid), MIX_THREADS, 0, stream>>>(G, (int)n, n_cols, ld, mask_t, m_pad, row_count, Y,
                                                                                       ldy, tiles_m, n_tiles);
    return check_launch("nnm_mix_kernel");
}

}  // namespace byz
