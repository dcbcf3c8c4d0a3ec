// The mean of the values nearest a GIVEN centre (Phocas' second stage, Xie, Koyejo and Gupta 2018; MeaMed), DESIGN.md 3.3c.
//
//   d      = fl32(col - c)                       one fp32 subtraction (never an FMA: -ffp-contract=off, and __fsub_rn)
//   a      = |d|
//   order  = np.argsort(a, kind='stable')        ties in |d| by logical row order; every NaN behind +inf, in row order
//   kept   = order[:keep]                        1 <= keep <= n
//   radius = a[order[keep - 1]]
//   out    = fl32(sum of col[kept] in fp64 / keep)
//
// ONE order statistic of the keys bits(a) -- a >= 0, so its bits order as unsigned integers as they are -- found by column_select.hpp's
// radix select, 8 bits per pass, with one 32-bit counter per (digit, column): a single rank needs no second half of the word, so
// the same histogram serves every height up to 2^20.  |d| does not invert to x: the resident tile holds the VALUES and forms the
// key again in every pass (a subtract, a mask, a min).  With T the key of rank keep - 1, `run` the keys equal to T and
// `need` of them inside the rank:
//     S = sum{x : key < T} + the ties' share                                   (fp64, a fixed order)
//   need == run             every tie is kept: they are summed with the rest;
//   the ties are one value  (the per-column min and max of their ordered bits agree): need copies of it, need >= 1: never 0 * inf;
//   otherwise               (c + t against c - t, or two values whose differences round alike) one thread walks the column in
//                           logical row order and adds the first `need` ties -- the one place where row order matters.
// A kept NaN, or +inf and -inf both kept, make S NaN by themselves; a non-finite centre needs no case of its own (every key is
// +inf's or the NaNs').  Nothing but the column's own rows, its centre and the height-picked geometry enters a result: the same
// bits for every ld, base alignment, grid and column split.
//
// Two shapes of one kernel template, picked by height alone from column_select.hpp's table:
//   streamed   RPT == 0: 64 columns per workgroup, sixteen waves split the rows, eight loads in flight per thread; the four select
//              passes and the sums: FIVE passes over HBM;
//   resident   RPT  > 0: the workgroup's COLS x n tile is loaded ONCE into registers (thread (tx, ty) holds rows ty, ty + RG, ...).
// The header also has the walk to the rank's digit, the tile and its grid, the row loader, the streamed loop, the fixed-order total
// and the launch.  This file's own: the tile held as values, `fresh`, where the scheduling barriers stand, and the ties.
#include "column_select.hpp"
#include "common.hpp"
#include "order_keys.hpp"

namespace byz {
namespace {

constexpr uint32_t kInfKey = 0x7f800000u;      // bits(+inf): the largest key of a number
constexpr uint32_t kNanKey = 0x7f800001u;      // every NaN difference: one key above +inf's
constexpr uint32_t kPadKey = 0x7f800002u;      // the streamed sums' rows beyond the height: above every threshold
constexpr int kResidentBatch = 4;
// keys formed at a time: the scheduler does not gather more of a tile's keys first (89 VGPRs at 64 rows a thread; 109 without the
// barriers, no spill either way)
constexpr int kResidentGroup = 4;
constexpr int kWalkUnroll = 8;
using colsel::kSegments;

__device__ __forceinline__ uint32_t window_key(float x, float c) {
    const uint32_t a = __float_as_uint(__fsub_rn(x, c)) & 0x7fffffffu;
    return a > kInfKey ? kNanKey : a;
}

constexpr int lds_words(int cols) { return 256 * cols + (kSegments + 5) * cols; }

// One workgroup: COLS columns x RG row groups.  INDEXED: row r is G[row_index[r]] -- decided at compile time, so that a batch of
// loads is straight-line code and stays in flight together (a test of the pointer in front of every load ends that).
template <int COLS, int RG, int RPT, bool INDEXED>
__global__ __launch_bounds__(COLS * RG) void centre_window_kernel(const float* __restrict__ G, int n_rows, int64_t n_cols, int64_t ld,
                                                                  const int32_t* __restrict__ row_index,
                                                                  const float* __restrict__ centre, int keep, int64_t tiles,
                                                                  float* __restrict__ out, float* __restrict__ radius) {
    static_assert(RG >= kSegments && RG <= 128, "sixteen row groups sum the segments; the fp64 partials fit the dead histogram");
    constexpr int kThreads = COLS * RG;
    constexpr int kHist = 256 * COLS;
    extern __shared__ uint32_t lds[];
    uint32_t* const hist = lds;                                      // [256][COLS]
    uint32_t* const seg = lds + kHist;                               // [kSegments][COLS]
    uint32_t* const found = seg + kSegments * COLS;                  // [COLS]: the digits found so far
    int* const left = reinterpret_cast<int*>(found + COLS);          // [COLS]: the rank left inside them
    uint32_t* const run = reinterpret_cast<uint32_t*>(left + COLS);  // [COLS]: keys equal to the answer
    uint32_t* const tie_min = run + COLS;                            // [COLS]: ordered bits of the smallest tied value
    uint32_t* const tie_max = tie_min + COLS;                        // [COLS]: of the largest
    const int tid = threadIdx.x;
    const colsel::ColumnTile tile = colsel::column_tile<COLS>(tiles, n_cols);
    if (tile.none) return;
    const int tx = tile.tx, ty = tile.ty;
    const colsel::ColumnRows rows{G, ld, row_index, tile.col, n_rows - 1};
    auto load = [&](int r) -> float { return rows.at<INDEXED>(r); };
    const float c = centre[tile.col];

    // ---- the resident tile: kept as values.  A row beyond the height holds a NaN: its key is the NaNs', and behind every real
    // row IN ROW ORDER is exactly where the restatement would put a NaN appended to the column -- no rank asked for reaches it,
    // and no pass needs a predicate.  (A tie group it joins is never `all`, and its one-value test or its walk, which reads the
    // real rows only, gives what the real ties give: a NaN wherever a real NaN is kept.)
    float vals[RPT > 0 ? RPT : 1];
    const int mine = n_rows > ty ? (n_rows - ty + RG - 1) / RG : 0;      // row ty + j * RG is inside the column for j < mine
    if constexpr (RPT > 0) {
        static_assert(RPT % kResidentBatch == 0, "the tile is loaded in whole batches");
#pragma unroll
        for (int j0 = 0; j0 < RPT; j0 += kResidentBatch) {      // (a batch of loads in flight per thread; the waves cover the rest)
            float v[kResidentBatch];
#pragma unroll
            for (int j = 0; j < kResidentBatch; ++j) v[j] = load(ty + (j0 + j) * RG);
#pragma unroll
            for (int j = 0; j < kResidentBatch; ++j)
                vals[j0 + j] = j0 + j < mine ? v[j] : __uint_as_float(0x7fc00000u);
            __builtin_amdgcn_sched_barrier(0);      // (one batch's addresses live at a time)
        }
    }
    // The keys are the same in every pass, and a compiler that sees it keeps them beside the values: twice the registers.  Each
    // pass therefore reads the centre through `fresh`, an empty asm the compiler cannot see through, and forms its keys anew.
    float c_pass = c;
    auto fresh = [&] { asm volatile("" : "+v"(c_pass)); };
    auto resident_key = [&](int j) -> uint32_t { return window_key(vals[j], c_pass); };

    if (ty == 0) {
        found[tx] = 0u;
        left[tx] = keep - 1;
        tie_min[tx] = 0xffffffffu;
        tie_max[tx] = 0u;
    }

#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < kHist; i += kThreads) lds[i] = 0u;
        __syncthreads();
        const uint32_t prefix = found[tx];
        fresh();
        auto count = [&](uint32_t key, bool valid) {
            const uint32_t above = pass == 0 ? 0u : key >> ((shift + 8) & 31);
            if (valid && above == prefix) atomicAdd(&hist[((key >> shift) & 255u) * COLS + tx], 1u);
        };
        if constexpr (RPT > 0) {
#pragma unroll
            for (int j = 0; j < RPT; ++j) {
                count(resident_key(j), true);      // (the padding is counted: behind every real row)
                if (j % kResidentGroup == kResidentGroup - 1) __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            colsel::stream_rows<RG>(ty, n_rows, load, [&](float v, int, bool valid) { count(window_key(v, c), valid); });
        }
        __syncthreads();
        auto counter = [hist](int slot) { return hist[slot]; };
        if (ty < kSegments) seg[ty * COLS + tx] = colsel::segment_sum<COLS>(ty, tx, counter);
        __syncthreads();
        if (ty == 0) {      // one thread per column
            const colsel::DigitRank at = colsel::walk_to_digit<COLS>(left[tx], seg, tx, counter);
            found[tx] = (prefix << 8) | static_cast<uint32_t>(at.digit);
            left[tx] = at.left;
            run[tx] = at.run;
        }
        __syncthreads();
    }

    // ---- the sums: everything nearer than the threshold, the ties with it when they all fit; else the ties' extremes
    const uint32_t T = found[tx];
    const int need = left[tx] + 1;                 // ties inside the rank: 1 .. run
    const bool all = need == static_cast<int>(run[tx]);
    double sum = 0.0;
    uint32_t lo = 0xffffffffu, hi = 0u;
    fresh();
    auto fold = [&](float v, uint32_t key) {
        if (key < T || (all && key == T)) {
            sum += static_cast<double>(v);
        } else if (key == T) {
            const uint32_t o = ordered_bits(v);
            lo = o < lo ? o : lo;
            hi = o > hi ? o : hi;
        }
    };
    if constexpr (RPT > 0) {
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            fold(vals[j], resident_key(j));
            if (j % kResidentGroup == kResidentGroup - 1) __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        colsel::stream_rows<RG>(ty, n_rows, load, [&](float v, int, bool valid) { fold(v, valid ? window_key(v, c) : kPadKey); });
    }
    if (lo <= hi) {
        atomicMin(&tie_min[tx], lo);
        atomicMax(&tie_max[tx], hi);
    }
    double* const part = reinterpret_cast<double*>(hist);      // [RG][COLS], over the dead histogram
    part[ty * COLS + tx] = sum;
    __syncthreads();
    if (ty != 0 || !tile.real) return;
    double total = colsel::fixed_order_total<COLS, RG>(part, tx);
    if (!all) {
        const uint32_t t_lo = tie_min[tx], t_hi = tie_max[tx];
        if (t_lo == t_hi) {
            total += static_cast<double>(need) * static_cast<double>(from_ordered_bits(t_lo));
        } else {
            // ties of differing values that do not all fit: the first `need` of them in logical row order
            int open = need;
            for (int r0 = 0; r0 < n_rows && open > 0; r0 += kWalkUnroll) {
                float v[kWalkUnroll];
#pragma unroll
                for (int j = 0; j < kWalkUnroll; ++j) v[j] = load(r0 + j);
#pragma unroll
                for (int j = 0; j < kWalkUnroll; ++j) {
                    if (r0 + j < n_rows && open > 0 && window_key(v[j], c) == T) {
                        total += static_cast<double>(v[j]);
                        --open;
                    }
                }
            }
        }
    }
    out[tile.col] = static_cast<float>(total / static_cast<double>(keep));
    if (radius != nullptr) radius[tile.col] = __uint_as_float(T);      // (kNanKey's bits are a NaN's)
}

}  // namespace

int check_centre_window(const char* who, int64_t n_rows, int64_t keep) {
    if (n_rows > kLargeMaxRows) {
        set_error("%s supports at most %lld rows, got %lld", who, (long long)kLargeMaxRows, (long long)n_rows);
        return BYZ_E_UNSUPPORTED;
    }
    BYZ_REQUIRE(keep >= 1 && keep <= n_rows, "%s: keep %lld outside 1..%lld (the row count)", who, (long long)keep, (long long)n_rows);
    return BYZ_OK;
}

int launch_centre_window(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                         const float* centre, int64_t keep, float* out, float* radius, hipStream_t stream) {
    BYZ_REQUIRE(G && centre && out && n_rows > 0 && n_cols > 0 && ld >= n_cols, "window_mean: bad arguments (%lld x %lld, ld %lld)",
                (long long)n_rows, (long long)n_cols, (long long)ld);
    BYZ_TRY(check_centre_window("window_mean", n_rows, keep));
    const int n = static_cast<int>(n_rows), k = static_cast<int>(keep);
    KernelTimer t(ctx, BYZ_K_TRIMMED_MEAN, stream);
    return colsel::for_height(n, [&](auto geometry) {
        using Geo = decltype(geometry);
        const colsel::TileGrid t = colsel::tile_grid<Geo::COLS>(n_cols);
        auto* kernel = row_index != nullptr ? &centre_window_kernel<Geo::COLS, Geo::RG, Geo::RPT, true>
                                            : &centre_window_kernel<Geo::COLS, Geo::RG, Geo::RPT, false>;
        return colsel::launch_column_tiles(ctx, kernel, "centre_window_kernel", "window mean", t, Geo::COLS * Geo::RG,
                                           lds_words(Geo::COLS) * 4, stream, G, n, n_cols, ld, row_index, centre, k, t.tiles, out, radius);
    });
}

}  // namespace byz
