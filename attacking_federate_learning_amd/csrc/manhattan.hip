// Pairwise Manhattan (L1) distances, m_ij = sum_c |g_ic - g_jc|: the one distance of this library that no Gram gives.  An
// n x n x d reduction on the VECTOR pipe (a subtraction and an addition with |.| as the source modifier: 2 instructions per
// pair-element), what Multi-Metrics (multi_metrics.hip) adds to the Euclidean and cosine matrices.
//
//   manhattan_tile_kernel     one workgroup of 512 threads (two waves per SIMD, which is what the vector pipe needs to issue every
//                             2 cycles) owns a 128 x 128 tile of pairs (ti <= tj only: the other triangle is the mirror) and one
//                             CHUNK of columns.  Thread (ty, tx) of 16 x 32 holds the 8 x 4 block of rows i = 8 ty .. + 7 against
//                             rows j = 4 tx .. + 3.  The columns pass through LDS 64 at a time, stored [column][row] so that a
//                             thread's 8 + 4 operands of a column are three 16-byte reads; a wave loads 64 consecutive columns
//                             of one row (one coalesced 256-byte request, dword loads: no alignment asked of G or ld).  The next
//                             stage's global loads are issued before the current stage is computed.
//   manhattan_reduce_kernel   sums[i][j] = the chunks' partials of (min(i, j), max(i, j)) added in ascending chunk order, in fp64,
//                             both triangles written.  No floating-point atomics anywhere.
//   manhattan_finish_kernel   dist[i][j] = fl32(sums[max(i, j)][min(i, j)]), one rounding; the diagonal and every pair whose sum
//                             or whose rounded value is not finite are +inf.  Reading ONE triangle makes the matrix symmetric
//                             as bits whatever an all-reduce did to the two triangles of the sums.
//
// ACCURACY.  Every accumulator is an fp32 chain of at most kChain = 128 terms, c = fl(c + |fl(a - b)|), then folded into an
// fp64 accumulator and restarted from +0.  Per pair: one rounding of a - b per term (relative 2^-24 of a non-negative term),
// at most kChain - 1 roundings in a chain of non-negative terms, one rounding to fp32 at the end; the fp64 folds add
// (d / kChain + chunks) * 2^-53, below 2^-24 for every d < 2^36.  Worst case, relative to the exact sum:
//
//       |m_ij - exact| <= (kChain + 2) * 2^-24 * exact = 130 * 2^-24 = 7.75e-6        (kManhattanRelBound, <= 1e-5)
//
// REPRODUCIBILITY.  Chains are assigned by COLUMN INDEX: the chain of columns [128 q, 128 q + 128) of a pair is added in
// ascending column order by one thread, whatever the pointer, the leading dimension or the chunk the columns fall in (a
// chunk is a multiple of 128 columns, and its length depends on n, d and the CU count alone).  So the same matrix seen
// through ld > d, or through a base pointer moved by one float, gives the same bits, as does a second run.  Columns beyond
// d and rows beyond n enter as 0 - 0, which changes no chain (x + 0 = x for every x >= +0 and for NaN).
// Compiled with -ffp-contract=off (nothing here could fuse, but the chain is a stated order of operations).
#include "common.hpp"

namespace byz {
namespace {

constexpr int kTile = 128;            // rows of a tile, both ways
constexpr int kThreads = 512;         // 16 (ty) x 32 (tx)
constexpr int kBlockI = 8, kBlockJ = 4;
constexpr int kStage = 64;            // columns in LDS at a time: one per lane of the loading wave
constexpr int kChain = BYZ_MANHATTAN_CHAIN;   // fp32 terms before the fold into fp64: 128
constexpr int kPitch = kTile + 4;     // floats between two columns in LDS: 16-byte aligned rows of operands, writes 4-way conflicted
constexpr int kRowsPerWave = 2 * kTile / (kThreads / 64);      // rows of A and B one wave loads per stage: 32
static_assert(kChain == 2 * kStage, "a chain is two stages");
static_assert((kChain + 2) * 5.9604644775390625e-8 <= 1e-5, "the header's bound stays within the project's distance tolerance");

typedef float float4a __attribute__((ext_vector_type(4)));
typedef float float2a __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(kThreads) void manhattan_tile_kernel(const float* __restrict__ G, int n, int64_t d, int64_t ld, int tiles,
                                                                  int64_t chunk_cols, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float lds_a[kStage * kPitch];
    __shared__ __attribute__((aligned(16))) float lds_b[kStage * kPitch];
    // the tile pair of this workgroup: row ti of the upper triangle holds tiles - ti pairs
    int p = blockIdx.x, ti = 0;
    while (p >= tiles - ti) {
        p -= tiles - ti;
        ++ti;
    }
    const int tj = ti + p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tid >> 5, tx = tid & 31;
    const int64_t c_begin = static_cast<int64_t>(blockIdx.y) * chunk_cols;
    const int64_t c_end = c_begin + chunk_cols < d ? c_begin + chunk_cols : d;
    const int stages = static_cast<int>((c_end - c_begin + kStage - 1) / kStage);

    // the rows this wave loads: slot q < 16 is row wave + 8 q of tile ti, slot q >= 16 the same of tile tj
    float stage_regs[kRowsPerWave];
    auto load_stage = [&](int st) __attribute__((always_inline)) {
        const int64_t col = c_begin + static_cast<int64_t>(st) * kStage + lane;
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) {
            const int local = wave + 8 * (q & 15);
            const int row = (q < 16 ? ti : tj) * kTile + local;
            stage_regs[q] = (row < n && col < c_end) ? G[static_cast<int64_t>(row) * ld + col] : 0.0f;
        }
    };
    auto store_stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) {
            const int local = wave + 8 * (q & 15);
            (q < 16 ? lds_a : lds_b)[lane * kPitch + local] = stage_regs[q];
        }
    };

    float acc[kBlockI][kBlockJ];
    double total[kBlockI][kBlockJ];
#pragma unroll
    for (int a = 0; a < kBlockI; ++a)
#pragma unroll
        for (int b = 0; b < kBlockJ; ++b) {
            acc[a][b] = 0.0f;
            total[a][b] = 0.0;
        }

    if (stages > 0) load_stage(0);
    for (int st = 0; st < stages; ++st) {
        store_stage();
        __syncthreads();
        if (st + 1 < stages) load_stage(st + 1);
#pragma unroll 4
        for (int k = 0; k < kStage; ++k) {
            const float4a a0 = *reinterpret_cast<const float4a*>(&lds_a[k * kPitch + ty * kBlockI]);
            const float4a a1 = *reinterpret_cast<const float4a*>(&lds_a[k * kPitch + ty * kBlockI + 4]);
            const float4a b0 = *reinterpret_cast<const float4a*>(&lds_b[k * kPitch + tx * kBlockJ]);
            const float av[kBlockI] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float2a bv[kBlockJ / 2] = {{b0.x, b0.y}, {b0.z, b0.w}};
            // two differences per packed subtraction; the additions stay single, where |.| is a source modifier (a packed
            // addition has none and would cost two more instructions per pair of terms): 1.5 instructions per pair-element
#pragma unroll
            for (int a = 0; a < kBlockI; ++a)
#pragma unroll
                for (int b = 0; b < kBlockJ / 2; ++b) {
                    const float2a diff = float2a{av[a], av[a]} - bv[b];
                    acc[a][2 * b] = acc[a][2 * b] + __builtin_fabsf(diff.x);
                    acc[a][2 * b + 1] = acc[a][2 * b + 1] + __builtin_fabsf(diff.y);
                }
        }
        if ((st & 1) == 1 || st + 1 == stages) {        // (a chunk starts at a multiple of kChain: odd stages end a chain)
#pragma unroll
            for (int a = 0; a < kBlockI; ++a)
#pragma unroll
                for (int b = 0; b < kBlockJ; ++b) {
                    total[a][b] = total[a][b] + static_cast<double>(acc[a][b]);
                    acc[a][b] = 0.0f;
                }
        }
        __syncthreads();
    }

    double* __restrict__ out = partial + static_cast<int64_t>(blockIdx.y) * n * n;
#pragma unroll
    for (int a = 0; a < kBlockI; ++a) {
        const int i = ti * kTile + ty * kBlockI + a;
#pragma unroll
        for (int b = 0; b < kBlockJ; ++b) {
            const int j = tj * kTile + tx * kBlockJ + b;
            if (i < n && j < n) out[static_cast<int64_t>(i) * n + j] = total[a][b];
        }
    }
}

__global__ __launch_bounds__(256) void manhattan_reduce_kernel(const double* __restrict__ partial, int64_t n, int chunks,
                                                               double* __restrict__ sums) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * 64 + (threadIdx.x & 63);
    const int64_t i = static_cast<int64_t>(blockIdx.y) * 4 + (threadIdx.x >> 6);
    if (i >= n || j >= n) return;
    const int64_t lo = i < j ? i : j, hi = i < j ? j : i;          // tile(lo) <= tile(hi): the pair a workgroup computed
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s = s + partial[static_cast<int64_t>(c) * n * n + lo * n + hi];
    sums[i * n + j] = s;
}

__global__ __launch_bounds__(256) void manhattan_finish_kernel(const double* __restrict__ sums, int64_t n, float* __restrict__ dist) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * 64 + (threadIdx.x & 63);
    const int64_t i = static_cast<int64_t>(blockIdx.y) * 4 + (threadIdx.x >> 6);
    if (i >= n || j >= n) return;
    float m = __builtin_inff();
    if (i != j) {
        const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
        const double s = sums[hi * n + lo];
        const float r = static_cast<float>(s);
        if (__builtin_isfinite(s) && __builtin_isfinite(r)) m = r;
    }
    dist[i * n + j] = m;
}

}  // namespace

// the column chunks of the tile kernel for this shape: enough workgroups for four rounds over the CUs, a multiple of kChain
// columns each, the partials within kManhattanPartialBytes
int64_t manhattan_chunks(byz_ctx* ctx, int64_t n, int64_t d, int64_t* chunk_cols) {
    const int64_t tiles = ceil_div(n, kTile), pairs = tiles * (tiles + 1) / 2;
    int64_t want = ceil_div(static_cast<int64_t>(4) * ctx->num_cus, pairs);
    const int64_t fit = kManhattanPartialBytes / (n * n * static_cast<int64_t>(sizeof(double)));
    if (want > fit) want = fit;
    if (want < 1) want = 1;
    const int64_t cols = ceil_div(ceil_div(d, want), kChain) * kChain;
    *chunk_cols = cols;
    return ceil_div(d, cols);
}

int manhattan_workspace(byz_ctx* ctx, int64_t n, int64_t d, double** partial, double** sums) {
    int64_t chunk_cols = 0;
    const int64_t chunks = manhattan_chunks(ctx, n, d, &chunk_cols);
    Carve c;
    c.take(partial, chunks * n * n);
    c.take(sums, n * n);
    return c.commit(ctx->manhattan);
}

int launch_manhattan_sums(byz_ctx* ctx, const float* G, int64_t n, int64_t d, int64_t ld, double* partial, double* sums,
                          hipStream_t stream) {
    BYZ_REQUIRE(G && partial && sums && n > 0 && n <= kManhattanMaxRows && d > 0 && ld >= d, "manhattan sums: bad arguments (%lld x %lld, ld %lld)",
                (long long)n, (long long)d, (long long)ld);
    int64_t chunk_cols = 0;
    const int64_t chunks = manhattan_chunks(ctx, n, d, &chunk_cols);
    const int64_t tiles = ceil_div(n, kTile);
    BYZ_REQUIRE(chunks < 65536, "manhattan sums: %lld column chunks are beyond one launch", (long long)chunks);
    KernelTimer timer(ctx, BYZ_K_DISTANCES, stream);
    const dim3 grid(static_cast<unsigned>(tiles * (tiles + 1) / 2), static_cast<unsigned>(chunks));
    manhattan_tile_kernel<<<grid, kThreads, 0, stream>>>(G, static_cast<int>(n), d, ld, static_cast<int>(tiles), chunk_cols, partial);
    BYZ_TRY(check_launch("manhattan_tile_kernel"));
    const dim3 flat(static_cast<unsigned>(ceil_div(n, 64)), static_cast<unsigned>(ceil_div(n, 4)));
    manhattan_reduce_kernel<<<flat, 256, 0, stream>>>(partial, n, static_cast<int>(chunks), sums);
    return check_launch("manhattan_reduce_kernel");
}

int launch_manhattan_from_sums(byz_ctx* ctx, const double* sums, int64_t n, float* dist, hipStream_t stream) {
    BYZ_REQUIRE(sums && dist && n > 0 && n <= kManhattanMaxRows, "manhattan distances: bad arguments (n = %lld)", (long long)n);
    KernelTimer timer(ctx, BYZ_K_DISTANCES, stream);
    const dim3 flat(static_cast<unsigned>(ceil_div(n, 64)), static_cast<unsigned>(ceil_div(n, 4)));
    manhattan_finish_kernel<<<flat, 256, 0, stream>>>(sums, n, dist);
    return check_launch("manhattan_finish_kernel");
}

}  // namespace byz
