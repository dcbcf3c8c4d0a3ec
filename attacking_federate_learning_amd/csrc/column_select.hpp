// The column radix select, 8 bits per pass, that rank_select.hip (the median, the rank-trimmed mean), centre_window.hip (Phocas,
// window_mean) and tall_select.hip (the trimmed mean of tall columns) share: what is the same in all three, written once.
//
// A workgroup owns COLS consecutive columns and RG row groups: thread (tx, ty) takes rows ty, ty + RG, ... of column tx.  A pass
// counts the keys that match the digits found so far into hist[digit][COLS] (LDS; one bank per column, no conflicts whatever the
// data), sixteen threads per column sum its sixteen 16-digit segments, and one thread walks 16 + 16 counters to the digit that
// holds the rank.  What a key is, how many ranks are sought, what a counter word holds and what is summed afterwards is the
// kernel's own; the rest is here, a section each.  The walk compiles as plain C++17 too (tests/column_select_check.cpp).
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include "common.hpp"
#define BYZ_SELECT_FN __host__ __device__ __forceinline__
#else
#define BYZ_SELECT_FN inline
#endif

namespace byz {
namespace colsel {

constexpr int kSegments = 16;       // the walk to a rank's digit: sixteen 16-digit segment sums, then 16 + 16 steps
constexpr int kStreamUnroll = 8;    // loads a thread of a streamed pass keeps in flight

// ---- the walk -------------------------------------------------------------------------------------------------------------------
// count(slot): the counter of slot = digit * COLS + tx as the rank in question sees it -- a whole word, one half of a packed
// word, or one of two histograms.

// the sum of segment `segment` (digits 16 * segment ... + 15) of column tx: threads ty < kSegments, one segment each.  What
// count returns is what is summed: a counter, or two ranks' counters side by side (rank_select.hip: one read of a packed word)
template <int COLS, typename Count>
BYZ_SELECT_FN auto segment_sum(int segment, int tx, Count count) {
    auto s = count(16 * segment * COLS + tx);
#pragma unroll
    for (int b = 1; b < 16; ++b) s += count((16 * segment + b) * COLS + tx);
    return s;
}

struct DigitRank {
    int digit;         // the digit that holds the rank
    int left;          // the rank inside that digit's keys: 0 <= left < run
    uint32_t run;      // the keys with that digit
};

// The digit that holds rank `want` (0-based) of column tx's keys; seg: the column's segment sums, [kSegments][COLS].  A rank
// beyond the keys counted (none is ever asked for) ends on the last digit of the last segment with what is left of it.
template <int COLS, typename Count>
BYZ_SELECT_FN DigitRank walk_to_digit(int want, const uint32_t* seg, int tx, Count count) {
    int s16 = kSegments - 1;
    for (int g = 0; g < kSegments; ++g) {
        const int cnt = static_cast<int>(seg[g * COLS + tx]);
        if (want < cnt) {
            s16 = g;
            break;
        }
        want -= cnt;
    }
    int digit = 16 * s16 + 15;
    uint32_t cnt = 0u;
    for (int b = 16 * s16; b < 16 * s16 + 16; ++b) {
        cnt = count(b * COLS + tx);
        if (want < static_cast<int>(cnt)) {
            digit = b;
            break;
        }
        want -= static_cast<int>(cnt);
    }
    return {digit, want, cnt};
}

// ---- the heights ----------------------------------------------------------------------------------------------------------------
// RPT > 0: the workgroup's COLS x n tile is resident in registers, RPT rows a thread (RG * RPT rows at most); RPT == 0: streamed,
// 64 columns per workgroup, sixteen waves split the rows.  (DESIGN.md 3.3b has the timings behind the edges.)
template <int COLS_, int RG_, int RPT_>
struct Geometry {
    static constexpr int COLS = COLS_, RG = RG_, RPT = RPT_;
};
using Streamed = Geometry<64, 16, 0>;

// f(Geometry<...>{}) for the geometry that takes columns of n_rows rows
template <typename F>
inline auto for_height(int64_t n_rows, F&& f) {
    if (n_rows <= 256) return f(Geometry<64, 16, 16>{});
    if (n_rows <= 1024) return f(Geometry<16, 32, 32>{});
    if (n_rows <= 2304) return f(Geometry<16, 64, 36>{});
    if (n_rows <= 4096) return f(Geometry<16, 64, 64>{});
    return f(Streamed{});
}

#ifdef __HIPCC__
// ---- the tile -------------------------------------------------------------------------------------------------------------------
struct TileGrid {
    int64_t tiles, grid;      // column tiles; workgroups launched (narrow tiles: rounded up to whole groups of eight)
};
template <int COLS>
inline TileGrid tile_grid(int64_t n_cols) {
    const int64_t tiles = ceil_div(n_cols, COLS);
    return {tiles, COLS < 64 ? ceil_div(tiles, 8) * 8 : tiles};
}

struct ColumnTile {
    int tx, ty;
    bool none;        // a workgroup beyond the last tile of a narrow grid: it returns at once, all of it
    bool real;        // the thread's column exists;
    int64_t col;      // it is clamped into the matrix otherwise, so that every thread loads and meets every barrier
};
// `tiles` is read by tiles narrower than 64 columns only.  block: the workgroup's place in tile_grid's grid -- blockIdx.x, or the
// places blockIdx.x, blockIdx.x + gridDim.x, ... of a workgroup that walks several tiles (auror.hip; a grid that is a multiple of
// eight keeps block % 8, the XCD's label, the same at every step)
template <int COLS>
__device__ __forceinline__ ColumnTile column_tile(int64_t block, int64_t tiles, int64_t n_cols) {
    const int tid = threadIdx.x;
    ColumnTile t;
    t.tx = tid % COLS;
    t.ty = tid / COLS;
    int64_t tile = block;
    t.none = false;
    if constexpr (COLS < 64) {
        // a row segment of a narrow tile is a part of a 128-byte line: workgroups b and b + 8 (one XCD, dispatched together) take
        // neighbouring tiles so that the parts of a line meet in one L2
        const int64_t per = (tiles + 7) / 8;
        tile = (block % 8) * per + block / 8;
        t.none = tile >= tiles;
    }
    const int64_t col_raw = tile * COLS + t.tx;
    t.real = col_raw < n_cols;
    t.col = t.real ? col_raw : n_cols - 1;
    return t;
}
template <int COLS>
__device__ __forceinline__ ColumnTile column_tile(int64_t tiles, int64_t n_cols) {
    return column_tile<COLS>(static_cast<int64_t>(blockIdx.x), tiles, n_cols);
}

// ---- the rows -------------------------------------------------------------------------------------------------------------------
// Logical row r of the thread's column, a row beyond the last one clamped onto it (a repeated real value: the callers mask it).
struct ColumnRows {
    const float* G;
    int64_t ld;
    const int32_t* row_index;      // row r is G[row_index[r]]; nullptr: G[r]
    int64_t col;
    int last_row;
    // decided at compile time: a batch of loads is straight-line code then (centre_window.hip says what that is worth)
    template <bool INDEXED>
    __device__ __forceinline__ float at(int r) const {
        const int rr = r < last_row ? r : last_row;
        int64_t src = rr;
        if constexpr (INDEXED) src = row_index[rr];
        return G[src * ld + col];
    }
    // the index test at run time (a select of the row number in front of ONE load, not a branch around two)
    __device__ __forceinline__ float at(int r) const {
        const int rr = r < last_row ? r : last_row;
        const int64_t src = row_index ? row_index[rr] : rr;
        return G[src * ld + col];
    }
};

// One streamed pass of thread row group ty over the column: rows ty, ty + RG, ... in batches of UNROLL loads in flight, then
// body(value, row, valid) for each in row order; valid: row < n_rows (the value of a row beyond is load's business).
template <int RG, int UNROLL = kStreamUnroll, typename Load, typename Body>
__device__ __forceinline__ void stream_rows(int ty, int n_rows, Load load, Body body) {
    for (int r0 = ty; r0 < n_rows; r0 += RG * UNROLL) {
        float v[UNROLL];
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) v[j] = load(r0 + j * RG);
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) body(v[j], r0 + j * RG, r0 + j * RG < n_rows);
    }
}

// ---- the total ------------------------------------------------------------------------------------------------------------------
// The row groups' fp64 partial sums, [RG][COLS], lie over the histogram once the selects are done with it (RG <= 128).  Thread
// (tx, ty) stores at [ty * COLS + tx]; behind a barrier one thread per column adds them in a fixed order: the same bits every run.
// (tall_select.hip gathers three counts per row group beside its sum and keeps that one loop over the four arrays.)
template <int COLS, int RG>
__device__ __forceinline__ double fixed_order_total(const double* part, int tx) {
    double total = 0.0;
    for (int w = 0; w < RG; ++w) total += part[w * COLS + tx];
    return total;
}

// ---- the launch -----------------------------------------------------------------------------------------------------------------
// kernel<<<grid of COLS-column tiles, threads, lds_bytes of dynamic LDS, stream>>>(args...); `name` is the kernel's, for a launch
// that fails, `who` the caller's, for a matrix too wide for one grid.  args holds t.tiles where the kernel wants it.
template <typename Kernel, typename... Args>
int launch_column_tiles(byz_ctx* ctx, Kernel kernel, const char* name, const char* who, const TileGrid& t, int threads, int lds_bytes,
                        hipStream_t stream, Args... args) {
    BYZ_REQUIRE(t.grid <= 0x7fffffff, "%s: too many columns", who);
    BYZ_HIP(allow_dynamic_lds(ctx, reinterpret_cast<const void*>(kernel), lds_bytes));
    kernel<<<static_cast<unsigned>(t.grid), threads, lds_bytes, stream>>>(args...);
    return check_launch(name);
}
#endif

}  // namespace colsel
}  // namespace byz

#undef BYZ_SELECT_FN
