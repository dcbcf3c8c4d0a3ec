// The coordinate-wise median and the rank-trimmed mean (Yin et al. 2018; not in the reference), DESIGN.md 3.3b.
//
//   median        out[c] = np.median(col)                      fp32; even count -> fl(fl(a + b) * 0.5f); a NaN anywhere -> NaN
//   rank-trimmed  kept = np.sort(col)[b : n - b]               NaN of either sign sorts behind +inf, as np.sort has it
//                 out[c] = fl32(sum of kept in fp64 / (n - 2 b))
//
// Both are TWO order statistics of the SAME keys: ranks (n - 1) / 2 and n / 2, or ranks b and n - 1 - b.  One radix select finds
// them together, 8 bits per pass: the keys are tall_select.hip's order-preserving bits with every NaN mapped to one key behind +inf's; while the
// two ranks' prefixes agree a key is counted once for both, and once they part each rank counts the keys that match its own prefix.
// Heights up to 65,535 keep both counts in ONE word of hist[digit][column] (16 bits each, one LDS atomic per key whatever it
// matches); beyond that each rank has a histogram of 32-bit counters.  Nothing depends on row order: tied keys at a rank's edge are
// equal values, so with lo / hi the two order statistics the kept multiset is {lo < x < hi} plus c_lo copies of lo and c_hi of hi,
//     S = sum{x : lo < x < hi} + c_lo * lo + c_hi * hi        (fp64, a fixed order; c_lo, c_hi >= 1: never 0 * inf)
// and lo == hi (every kept value equal) returns that value as it is.
//
// Two shapes of one kernel template:
//   streamed   RPT == 0: 64 columns per workgroup, sixteen waves split the rows, the column read from HBM once per pass: four
//              select passes and the sums, FIVE passes (the median: four, its values are read off the keys);
//   resident   RPT  > 0: the workgroup's COLS x n tile is loaded ONCE into registers as keys (thread (tx, ty) holds rows ty,
//              ty + RG, ...), the four passes and the sums run over the registers: 4 n D + 4 D bytes of traffic.
// The geometry comes by height alone from column_select.hpp's table, and with it the select's common parts: the walk to a rank's
// digit, the tile and its grid, the row loader, the streamed loop, the fixed-order total and the launch.  This file's own: the two
// ranks counted together, the counters' width (wide beyond 65,535 rows), kNanKey / kPadKey, and the sums.
#include <type_traits>

#include "column_select.hpp"
#include "common.hpp"
#include "order_keys.hpp"

namespace byz {
namespace {

// Every NaN takes one key above +inf's; a resident tile's rows beyond the column's height take the key above that one, so that
// they sit behind every rank asked for and need no predicate.  (Both are bit patterns of NaNs: no other float maps onto them.)
constexpr uint32_t kNanKey = 0xfffffffeu;
constexpr uint32_t kPadKey = 0xffffffffu;
constexpr int kResidentBatch = 4;
using colsel::kSegments;

__device__ __forceinline__ uint32_t rank_key(float v) {
    if ((__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u) return kNanKey;
    return ordered_bits(v);
}
__device__ __forceinline__ float key_value(uint32_t k) { return from_ordered_bits(k); }   // (kNanKey -> 0x7ffffffe, a NaN)

constexpr int lds_words(int cols, bool wide) { return 256 * cols * (wide ? 2 : 1) + (2 * kSegments + 7) * cols; }

// One workgroup: COLS columns x RG row groups.  WIDE: 32-bit counters, a histogram per rank (more than 65,535 rows).
template <int COLS, int RG, int RPT, bool WIDE, bool MEDIAN>
__global__ __launch_bounds__(COLS * RG) void rank_select_kernel(const float* __restrict__ G, int n_rows, int64_t n_cols, int64_t ld,
                                                                const int32_t* __restrict__ row_index, int rank_lo, int rank_hi,
                                                                int64_t tiles, float* __restrict__ out) {
    static_assert(RG >= kSegments && RG <= 128, "sixteen row groups sum the segments; the fp64 partials fit the dead histogram");
    static_assert(!WIDE || RPT == 0, "a resident tile never needs the wide counters");
    constexpr int kThreads = COLS * RG;
    constexpr int kHist = 256 * COLS;
    extern __shared__ uint32_t lds[];
    uint32_t* const hist = lds;                                      // [256][COLS]; WIDE: the low rank's
    uint32_t* const hist_hi = lds + (WIDE ? kHist : 0);              // WIDE: the high rank's, once the prefixes have parted
    uint32_t* const seg = lds + kHist * (WIDE ? 2 : 1);              // [2][kSegments][COLS]
    uint32_t* const found = seg + 2 * kSegments * COLS;              // [2][COLS]: the digits found so far
    int* const left = reinterpret_cast<int*>(found + 2 * COLS);      // [2][COLS]: the rank left inside them
    uint32_t* const run = reinterpret_cast<uint32_t*>(left + 2 * COLS);   // [2][COLS]: keys equal to the answer
    uint32_t* const nan_seen = run + 2 * COLS;                       // [COLS]
    const int tid = threadIdx.x;
    const colsel::ColumnTile tile = colsel::column_tile<COLS>(tiles, n_cols);
    if (tile.none) return;
    const int tx = tile.tx, ty = tile.ty;
    const colsel::ColumnRows rows{G, ld, row_index, tile.col, n_rows - 1};
    auto load = [&](int r) -> float { return rows.at(r); };

    // ---- the resident tile: kept as keys
    uint32_t keys[RPT > 0 ? RPT : 1];
    if constexpr (RPT > 0) {
        static_assert(RPT % kResidentBatch == 0, "the tile is loaded in whole batches");
#pragma unroll
        for (int j0 = 0; j0 < RPT; j0 += kResidentBatch) {      // (a batch of loads in flight per thread; the waves cover the rest)
            float v[kResidentBatch];
#pragma unroll
            for (int j = 0; j < kResidentBatch; ++j) v[j] = load(ty + (j0 + j) * RG);
#pragma unroll
            for (int j = 0; j < kResidentBatch; ++j) keys[j0 + j] = ty + (j0 + j) * RG < n_rows ? rank_key(v[j]) : kPadKey;
        }
    }

    if (ty == 0) {
        found[tx] = 0u;
        found[COLS + tx] = 0u;
        left[tx] = rank_lo;
        left[COLS + tx] = rank_hi;
        nan_seen[tx] = 0u;
    }

#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < kHist * (WIDE ? 2 : 1); i += kThreads) lds[i] = 0u;
        __syncthreads();
        const uint32_t prefix_lo = found[tx], prefix_hi = found[COLS + tx];
        const bool shared = prefix_lo == prefix_hi;      // (the first pass: both empty)
        uint32_t nan = 0u;
        auto count = [&](uint32_t key, bool valid) {
            const uint32_t above = pass == 0 ? 0u : key >> ((shift + 8) & 31);
            const bool m_lo = valid && above == prefix_lo, m_hi = valid && above == prefix_hi;
            const uint32_t slot = ((key >> shift) & 255u) * COLS + tx;
            if constexpr (WIDE) {
                if (m_lo) atomicAdd(&hist[slot], 1u);
                if (m_hi && !shared) atomicAdd(&hist_hi[slot], 1u);
            } else {
                const uint32_t add = (m_lo ? 1u : 0u) | (m_hi ? 0x10000u : 0u);
                if (add != 0u) atomicAdd(&hist[slot], add);
            }
            if (MEDIAN && pass == 0) nan |= valid && key == kNanKey ? 1u : 0u;
        };
        if constexpr (RPT > 0) {
#pragma unroll
            for (int j = 0; j < RPT; ++j) count(keys[j], true);      // (the padding is counted: behind every rank)
        } else {
            colsel::stream_rows<RG>(ty, n_rows, load, [&](float v, int, bool valid) { count(rank_key(v), valid); });
        }
        if (MEDIAN && pass == 0 && nan != 0u) atomicOr(&nan_seen[tx], 1u);
        __syncthreads();
        // the counters of rank `which` (0: low, 1: high)
        auto counter = [&](int which, int slot) -> uint32_t {
            if constexpr (WIDE) return (which != 0 && !shared ? hist_hi : hist)[slot];
            else return which != 0 ? hist[slot] >> 16 : hist[slot] & 0xffffu;
        };
        if (ty < kSegments) {
            const uint2 s = colsel::segment_sum<COLS>(ty, tx, [&](int slot) { return make_uint2(counter(0, slot), counter(1, slot)); });
            seg[ty * COLS + tx] = s.x;
            seg[(kSegments + ty) * COLS + tx] = s.y;
        }
        __syncthreads();
        if (ty < 2) {      // one thread per column and rank
            const int which = ty;
            const colsel::DigitRank at = colsel::walk_to_digit<COLS>(left[which * COLS + tx], seg + which * kSegments * COLS, tx,
                                                                     [&](int slot) { return counter(which, slot); });
            found[which * COLS + tx] = ((which ? prefix_hi : prefix_lo) << 8) | static_cast<uint32_t>(at.digit);
            left[which * COLS + tx] = at.left;
            run[which * COLS + tx] = at.run;
        }
        __syncthreads();
    }

    const uint32_t key_lo = found[tx], key_hi = found[COLS + tx];
    if constexpr (MEDIAN) {
        if (ty != 0 || !tile.real) return;
        const float lo = key_value(key_lo), hi = key_value(key_hi);
        float med = rank_lo == rank_hi ? lo : __fmul_rn(__fadd_rn(lo, hi), 0.5f);
        if (nan_seen[tx] != 0u) med = __uint_as_float(0x7fc00000u);
        out[tile.col] = med;
    } else {
        // ---- the sums: everything strictly between the two order statistics
        double sum = 0.0;
        if constexpr (RPT > 0) {
#pragma unroll
            for (int j = 0; j < RPT; ++j) {
                const bool in = keys[j] > key_lo && keys[j] < key_hi;
                if (in) sum += static_cast<double>(key_value(keys[j]));
            }
        } else {
            colsel::stream_rows<RG>(ty, n_rows, load, [&](float v, int, bool valid) {
                const uint32_t key = rank_key(v);
                const bool in = valid && key > key_lo && key < key_hi;
                if (in) sum += static_cast<double>(v);
            });
        }
        double* const part = reinterpret_cast<double*>(hist);      // [RG][COLS], over the dead histogram
        part[ty * COLS + tx] = sum;
        __syncthreads();
        if (ty != 0 || !tile.real) return;
        const float lo = key_value(key_lo), hi = key_value(key_hi);
        float result = lo;                     // every kept value equal (a NaN key: NaN)
        if (key_lo != key_hi) {
            double total = colsel::fixed_order_total<COLS, RG>(part, tx);
            // kept copies of lo: from its rank to the end of its run; of hi: from the start of its run to its rank
            const double c_lo = static_cast<double>(static_cast<int>(run[tx]) - left[tx]);
            const double c_hi = static_cast<double>(left[COLS + tx] + 1);
            total += c_lo * static_cast<double>(lo);
            total += c_hi * static_cast<double>(hi);
            result = static_cast<float>(total / static_cast<double>(rank_hi - rank_lo + 1));
        }
        out[tile.col] = result;
    }
}

// Heights up to 65,535 keep both ranks' counts in one word; a streamed column beyond that takes the wide counters.
template <bool MEDIAN>
int launch_picked(byz_ctx* ctx, const float* G, int n, int64_t n_cols, int64_t ld, const int32_t* row_index, int rank_lo, int rank_hi,
                  float* out, hipStream_t stream) {
    auto launch = [&](auto geometry, auto wide) {
        using Geo = decltype(geometry);
        constexpr bool WIDE = decltype(wide)::value;
        const colsel::TileGrid t = colsel::tile_grid<Geo::COLS>(n_cols);
        return colsel::launch_column_tiles(ctx, &rank_select_kernel<Geo::COLS, Geo::RG, Geo::RPT, WIDE, MEDIAN>, "rank_select_kernel",
                                           "rank select", t, Geo::COLS * Geo::RG, lds_words(Geo::COLS, WIDE) * 4, stream, G, n, n_cols,
                                           ld, row_index, rank_lo, rank_hi, t.tiles, out);
    };
    return colsel::for_height(n, [&](auto geometry) {
        if constexpr (decltype(geometry)::RPT == 0) {
            if (n > 65535) return launch(geometry, std::true_type{});
        }
        return launch(geometry, std::false_type{});
    });
}

}  // namespace

int launch_rank_select(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                       int64_t trim_count, bool median, float* out, hipStream_t stream) {
    const char* who = median ? "coordinate_median" : "rank_trimmed_mean";
    BYZ_REQUIRE(G && out && n_rows > 0 && n_cols > 0 && ld >= n_cols, "%s: bad arguments (%lld x %lld, ld %lld)", who,
                (long long)n_rows, (long long)n_cols, (long long)ld);
    if (n_rows > kLargeMaxRows) {
        set_error("%s supports at most %lld rows, got %lld", who, (long long)kLargeMaxRows, (long long)n_rows);
        return BYZ_E_UNSUPPORTED;
    }
    const int n = static_cast<int>(n_rows);
    KernelTimer t(ctx, BYZ_K_TRIMMED_MEAN, stream);
    if (median) return launch_picked<true>(ctx, G, n, n_cols, ld, row_index, (n - 1) / 2, n / 2, out, stream);
    BYZ_REQUIRE(trim_count >= 0 && 2 * trim_count < n_rows, "rank_trimmed_mean: trim_count %lld must satisfy 0 <= 2 b < %lld rows",
                (long long)trim_count, (long long)n_rows);
    const int b = static_cast<int>(trim_count);
    return launch_picked<false>(ctx, G, n, n_cols, ld, row_index, b, n - 1 - b, out, stream);
}

}  // namespace byz
