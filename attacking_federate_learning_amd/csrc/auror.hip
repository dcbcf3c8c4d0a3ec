// Auror (Shen, Tople and Saxena, "AUROR: Defending Against Poisoning Attacks in Collaborative Deep Learning Systems", ACSAC 2016;
// beyond the reference): every column's n values are split into two clusters by Lloyd's 2-means from the start (min, max), a
// column whose centres end more than alpha apart is indicative, the smaller cluster of an indicative column is suspicious, and a
// row that is suspicious in more than tau of the indicative columns is removed (include/byzagg.h states the rule operation for
// operation; two_means.hpp holds what decides).
//
//   two_means_votes_kernel   one workgroup a COLS-column tile at a time (column_select.hpp's geometries by height), several tiles a
//                            workgroup: the grid is sized to the CUs.  Up to 4096 rows the tile is resident in registers as values,
//                            read once; beyond, every sweep streams the column.  A sweep gives each thread (m1, S1, S0) of its rows
//                            in ascending order; they go to LDS as [row group][column], and behind one barrier the first row
//                            group's thread of a column adds the row groups' in ascending order from +0.0 and steps the column.
//                            The loop's second barrier is __syncthreads_or of "a column has not stopped": the flag is the same in
//                            every thread, so every thread meets every barrier and the workgroup leaves when its last column stops.
//                            Votes: a row of a tile belongs to one row group, so its counter in LDS (int32 a row) has one writer,
//                            the thread of the row group's first column, which adds the popcount of the wave's ballot over the
//                            row's lanes: no atomic at all inside a workgroup.  A non-finite value sets the row's byte.  At the
//                            end the workgroup adds its non-zero counters to the global int64 votes, one integer atomic a row at
//                            most, raises the bad flags by an integer max, and adds its three column counts.
//   auror_select_kernel      ONE workgroup: votes, bad flags, the indicative count and tau into the kept flags, the 0 / 1 weights
//                            and the report.
// No floating-point atomics, no scratch.
#include "column_select.hpp"
#include "common.hpp"
#include "lane_exchange.hpp"
#include "two_means.hpp"

namespace byz {
namespace {

constexpr int kAurorBatch = 4;               // loads a thread keeps in flight while the resident tile is filled
constexpr int kAurorSelectThreads = 1024;

// what a workgroup keeps in LDS beside its rows' counters
template <int COLS, int RG>
struct alignas(16) AurorLds {
    double s1[RG * COLS], s0[RG * COLS];     // [row group][column]: a sweep's sums
    float mn[RG * COLS], mx[RG * COLS];      // the first pass: the row groups' extremes
    int32_t m1[RG * COLS];                   // a sweep's count above the threshold; the first pass: the finite values
    two_means::Column col[COLS];
    int32_t counts[4];                       // the workgroup's indicative, clustered and capped columns
};

template <int COLS, int RG>
constexpr size_t auror_lds_bytes(int64_t n_rows) {
    return sizeof(AurorLds<COLS, RG>) + static_cast<size_t>(n_rows) * sizeof(int32_t) + (static_cast<size_t>(n_rows) + 15) / 16 * 16;
}

template <int COLS, int RG, int RPT>
__global__ __launch_bounds__(COLS * RG) void two_means_votes_kernel(const float* __restrict__ G, int n_rows, int64_t n_cols, int64_t ld,
                                                                    double alpha, int max_iter, int64_t tiles, int64_t places,
                                                                    unsigned long long* __restrict__ votes, int32_t* __restrict__ bad,
                                                                    unsigned long long* __restrict__ counts, double* __restrict__ gap) {
    static_assert(64 % COLS == 0, "a row's lanes are COLS neighbours of one wave");
    constexpr int kThreads = COLS * RG;
    using Lds = AurorLds<COLS, RG>;
    extern __shared__ __align__(16) unsigned char auror_lds[];
    Lds& L = *reinterpret_cast<Lds*>(auror_lds);
    int32_t* const row_votes = reinterpret_cast<int32_t*>(auror_lds + sizeof(Lds));            // [n_rows]
    unsigned char* const row_bad = reinterpret_cast<unsigned char*>(row_votes + n_rows);       // [n_rows]
    const int tid = threadIdx.x, lane = tid & 63;
    for (int r = tid; r < n_rows; r += kThreads) {
        row_votes[r] = 0;
        row_bad[r] = 0;
    }
    if (tid < 4) L.counts[tid] = 0;
    __syncthreads();

    // the votes of the lanes that hold this thread's row: COLS neighbours of the wave
    const int shift = COLS < 64 ? COLS * (lane / COLS) : 0;
    constexpr unsigned long long kRowLanes = COLS < 64 ? (1ull << (COLS & 63)) - 1ull : ~0ull;
    auto row_count = [&](bool flag) -> int {
        return __builtin_popcountll((static_cast<unsigned long long>(__ballot(flag)) >> shift) & kRowLanes);
    };
    const float kAbstain = __uint_as_float(0x7fc00000u);      // a row beyond the column: it takes no part anywhere

    for (int64_t place = blockIdx.x; place < places; place += gridDim.x) {      // (uniform: every thread meets every barrier)
        const colsel::ColumnTile tile = colsel::column_tile<COLS>(place, tiles, n_cols);
        if (tile.none) continue;
        // the row group again, as a value the compiler knows nothing about: the rows' 64-bit offsets are formed in the tile that
        // loads them, not kept across the tiles (RPT pairs of registers, which spill)
        int ty = tile.ty;
        asm volatile("" : "+v"(ty));
        const int tx = tile.tx, at = ty * COLS + tx;
        const colsel::ColumnRows rows{G, ld, nullptr, tile.col, n_rows - 1};
        auto load = [&](int r) -> float { return rows.at<false>(r); };

        // ---- the first pass: the values (resident: into registers), their extremes and count, the rows with a non-finite value
        float vals[RPT > 0 ? RPT : 1];
        float mn = __uint_as_float(0x7f800000u), mx = __uint_as_float(0xff800000u);
        int m = 0;
        auto first = [&](float x, int r, bool in) {
            const bool fin = two_means::takes_part(x);
            if (in && fin) {
                mn = x < mn ? x : mn;
                mx = x > mx ? x : mx;
                ++m;
            }
            if (in && !fin && tile.real) row_bad[r] = 1;      // (every writer stores the same byte)
        };
        if constexpr (RPT > 0) {
            static_assert(RPT % kAurorBatch == 0, "the tile is loaded in whole batches");
#pragma unroll
            for (int j0 = 0; j0 < RPT; j0 += kAurorBatch) {
                float v[kAurorBatch];
#pragma unroll
                for (int j = 0; j < kAurorBatch; ++j) v[j] = load(ty + (j0 + j) * RG);
#pragma unroll
                for (int j = 0; j < kAurorBatch; ++j) {
                    const int r = ty + (j0 + j) * RG;
                    const bool in = r < n_rows;
                    vals[j0 + j] = in ? v[j] : kAbstain;
                    first(v[j], r, in);
                }
            }
        } else {
            colsel::stream_rows<RG>(ty, n_rows, load, first);
        }
        // every value of the thread's column and rows again, in row order: body(x, row), x = kAbstain beyond the column
        auto sweep = [&](auto body) {
            if constexpr (RPT > 0) {
#pragma unroll
                for (int j = 0; j < RPT; ++j) {
                    // the value again, as one the compiler knows nothing about: what a sweep forms from it (its double, its
                    // finiteness) is formed where it is used, not kept for every value across the iterations (that spills)
                    asm volatile("" : "+v"(vals[j]));
                    body(vals[j], ty + j * RG);
                }
            } else {
                colsel::stream_rows<RG>(ty, n_rows, load, [&](float v, int r, bool in) { body(in ? v : kAbstain, r); });
            }
        };
        L.mn[at] = mn;
        L.mx[at] = mx;
        L.m1[at] = m;
        __syncthreads();
        int live = 0;
        if (ty == 0) {
            for (int g = 1; g < RG; ++g) {
                const float a = L.mn[g * COLS + tx], b = L.mx[g * COLS + tx];
                mn = a < mn ? a : mn;
                mx = b > mx ? b : mx;
                m += L.m1[g * COLS + tx];
            }
            two_means::start(L.col[tx], m, mn, mx);
            live = L.col[tx].stopped ? 0 : 1;
        }
        // ---- Lloyd's iterations: a sweep, the row groups' sums in one order, the step
        if (__syncthreads_or(live)) {
            for (int k = 1;; ++k) {                           // (step() stops every column at k == max_iter)
                const double t = L.col[tx].t;
                int m1 = 0;
                double s1 = 0.0, s0 = 0.0;
                sweep([&](float x, int) {
                    const bool fin = two_means::takes_part(x);
                    const bool up = fin && two_means::upper(x, t);
                    const double xd = static_cast<double>(x);
                    m1 += up ? 1 : 0;
                    s1 += up ? xd : 0.0;                      // (+0.0 changes no sum that began at +0.0)
                    s0 += (fin && !up) ? xd : 0.0;
                });
                L.m1[at] = m1;
                L.s1[at] = s1;
                L.s0[at] = s0;
                __syncthreads();
                live = 0;
                if (ty == 0) {
                    two_means::Column& c = L.col[tx];
                    if (!c.stopped) {
                        int total = 0;
                        double sum1 = 0.0, sum0 = 0.0;
                        for (int g = 0; g < RG; ++g) {
                            total += L.m1[g * COLS + tx];
                            sum1 += L.s1[g * COLS + tx];
                            sum0 += L.s0[g * COLS + tx];
                        }
                        two_means::step(c, k, max_iter, total, sum1, sum0);
                    }
                    live = c.stopped ? 0 : 1;
                }
                if (!__syncthreads_or(live)) break;
            }
        }
        // ---- the votes of the final assignment
        const two_means::Column c = L.col[tx];
        const int side = tile.real ? two_means::suspicious_side(c, alpha) : -1;
        if (ty == 0 && tile.real) {
            if (gap != nullptr) gap[tile.col] = two_means::gap(c);
            if (two_means::indicative(c, alpha)) atomicAdd(&L.counts[0], 1);
            if (c.clustered) atomicAdd(&L.counts[1], 1);
            if (c.capped) atomicAdd(&L.counts[2], 1);
        }
        if (__syncthreads_or(side >= 0 ? 1 : 0)) {            // (a tile without a suspicious side: no sweep)
            sweep([&](float x, int r) {
                const int n = row_count(two_means::votes(x, c.t, side));
                if (tx == 0 && n > 0) row_votes[r] += n;      // (the row's one writer; n > 0: r is a row of the matrix)
            });
        }
    }

    __syncthreads();
    for (int r = tid; r < n_rows; r += kThreads) {
        const int32_t v = row_votes[r];
        if (v > 0) atomicAdd(&votes[r], static_cast<unsigned long long>(v));
        if (row_bad[r] != 0) atomicMax(&bad[r], 1);
    }
    if (tid < 3 && L.counts[tid] > 0) atomicAdd(&counts[tid], static_cast<unsigned long long>(L.counts[tid]));
}

__global__ __launch_bounds__(kAurorSelectThreads) void auror_select_kernel(const long long* __restrict__ votes,
                                                                           const int32_t* __restrict__ bad,
                                                                           const long long* __restrict__ counts, int n, double tau,
                                                                           int32_t* __restrict__ kept_out, double* __restrict__ w,
                                                                           AurorReport* __restrict__ info) {
    __shared__ int part[2][kAurorSelectThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long indicative = counts[0];
    const double limit = tau * static_cast<double>(indicative);
    int kept = 0, broken = 0;
    for (int i = t; i < n; i += kAurorSelectThreads) {
        const bool is_bad = bad[i] != 0;
        const bool voted_out = indicative > 0 && static_cast<double>(votes[i]) > limit;
        const int keep = (is_bad || voted_out) ? 0 : 1;
        if (kept_out != nullptr) kept_out[i] = keep;
        w[i] = keep ? 1.0 : 0.0;
        kept += keep;
        broken += is_bad ? 1 : 0;
    }
    kept = lanes::wave_sum_shfl(kept);
    broken = lanes::wave_sum_shfl(broken);
    if (lane == 0) {
        part[0][wave] = kept;
        part[1][wave] = broken;
    }
    __syncthreads();
    if (t == 0) {
        kept = broken = 0;
        for (int v = 0; v < kAurorSelectThreads / 64; ++v) {
            kept += part[0][v];
            broken += part[1][v];
        }
        info->indicative = indicative;
        info->clustered = counts[1];
        info->capped = counts[2];
        info->removed = n - kept;
        info->kept = kept;
        info->bad_rows = broken;
        info->pad = 0;
        info->kept_f64 = static_cast<double>(kept);
    }
}

}  // namespace

int auror_workspace(byz_ctx* ctx, int64_t n, AurorScratch* out) {
    out->info = &device_scalars(ctx)->auror;
    Carve c;
    c.take(&out->w, n);
    c.take(&out->votes, n);
    c.take(&out->counts, 4);
    c.take(&out->bad, n);
    return c.commit(ctx->auror);
}

// 1 <= n_rows <= kAurorMaxRows and the parameters: the caller's business (api.hip), checked again before anything runs
int launch_auror_votes(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, double alpha, int64_t max_iter,
                       bool accumulate, long long* votes, int32_t* bad, long long* counts, double* gap, hipStream_t stream) {
    BYZ_REQUIRE(G && votes && bad && counts && n_rows >= 1 && n_rows <= kAurorMaxRows && n_cols >= 1 && ld >= n_cols && alpha >= 0.0 &&
                    max_iter >= 1,
                "auror votes: bad arguments (%lld x %lld, ld %lld, alpha = %g, max_iter = %lld)", (long long)n_rows, (long long)n_cols,
                (long long)ld, alpha, (long long)max_iter);
    if (!accumulate) {
        BYZ_HIP(hipMemsetAsync(votes, 0, static_cast<size_t>(n_rows) * sizeof(long long), stream));
        BYZ_HIP(hipMemsetAsync(bad, 0, static_cast<size_t>(n_rows) * sizeof(int32_t), stream));
        BYZ_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(long long), stream));
    }
    const int n = static_cast<int>(n_rows);
    const int sweeps = static_cast<int>(max_iter > 0x7fffffff ? 0x7fffffff : max_iter);
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    return colsel::for_height(n_rows, [&](auto geometry) -> int {
        using Geo = decltype(geometry);
        constexpr int kThreads = Geo::COLS * Geo::RG;
        const colsel::TileGrid t = colsel::tile_grid<Geo::COLS>(n_cols);
        BYZ_REQUIRE(t.grid <= 0x7fffffff, "auror votes: too many columns");
        const int lds = static_cast<int>(auror_lds_bytes<Geo::COLS, Geo::RG>(n_rows));
        // one workgroup a CU (by registers none of the geometries fits twice: DESIGN.md 3.4s), in whole groups of eight
        // (column_tile's XCD label)
        int64_t grid = static_cast<int64_t>(ctx->num_cus) / 8 * 8;
        if (grid < 8) grid = 8;
        if (grid > t.grid) grid = t.grid;
        auto kernel = &two_means_votes_kernel<Geo::COLS, Geo::RG, Geo::RPT>;
        BYZ_HIP(allow_dynamic_lds(ctx, reinterpret_cast<const void*>(kernel), lds));
        kernel<<<static_cast<unsigned>(grid), kThreads, lds, stream>>>(G, n, n_cols, ld, alpha, sweeps, t.tiles, t.grid,
                                                                       reinterpret_cast<unsigned long long*>(votes), bad,
                                                                       reinterpret_cast<unsigned long long*>(counts), gap);
        return check_launch("two_means_votes_kernel");
    });
}

int launch_auror_select(byz_ctx* ctx, const AurorScratch& t, const long long* votes, const int32_t* bad, const long long* counts,
                        int64_t n, double tau, int32_t* kept_out, hipStream_t stream) {
    BYZ_REQUIRE(votes && bad && counts && n >= 1 && n <= kAurorMaxRows && tau >= 0.0 && tau <= 1.0,
                "auror select: bad arguments (n = %lld, tau = %g)", (long long)n, tau);
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    auror_select_kernel<<<1, kAurorSelectThreads, 0, stream>>>(votes, bad, counts, static_cast<int>(n), tau, kept_out, t.w, t.info);
    return check_launch("auror_select_kernel");
}

}  // namespace byz
