// Host check of csrc/column_select.hpp's walk (tests/test_column_select.py compiles and runs this; plain C++17, no HIP).
// segment_sum and walk_to_digit on hist[256][COLS], for COLS 16 and 64 and every column of the tile, against a brute-force
// prefix sum over the column's 256 counters: the digit that holds a rank, the rank left inside it and the digit's count, with
// 0 <= left < run for every rank below the column's key count.  The histograms: all keys in digit 0, all in digit 255, one key per
// digit, empty leading and trailing segments, and random ones of up to 65,535 keys read through a plain accessor and through the
// halves of a packed word (two ranks' counts in one word, as rank_select.hip keeps them), the segment sums of both halves at once.
// Exit status 0 when every property holds; the first violations are printed otherwise.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "column_select.hpp"

namespace {

using byz::colsel::DigitRank;
using byz::colsel::kSegments;

int failures = 0;

// two ranks' counters side by side, as rank_select.hip sums them from one read of a packed word
struct Two {
    uint32_t x, y;
    Two& operator+=(const Two& o) { x += o.x; y += o.y; return *this; }
};

void fail(const char* what, int cols, int tx, int rank, const DigitRank& got, const DigitRank& want) {
    if (failures < 20)
        std::printf("FAIL %s: COLS %d column %d rank %d: digit %d left %d run %u, expected digit %d left %d run %u\n", what, cols, tx,
                    rank, got.digit, got.left, got.run, want.digit, want.left, want.run);
    ++failures;
}

// the prefix sum, counter by counter
DigitRank brute_force(const std::vector<uint32_t>& counts, int rank) {
    int64_t before = 0;
    for (int d = 0; d < 256; ++d) {
        if (rank < before + static_cast<int64_t>(counts[d])) return {d, static_cast<int>(rank - before), counts[d]};
        before += counts[d];
    }
    return {-1, -1, 0u};
}

// Column tx of a [256][COLS] histogram holds `counts` behind count(slot) -- the other columns hold something else -- and every
// rank of `ranks` is walked to.  fill(slot, value) writes a counter in the accessor's own format.
template <int COLS, typename Fill, typename Count>
void check_column(const char* what, const std::vector<uint32_t>& counts, const std::vector<int>& ranks, int tx, Fill fill, Count count) {
    for (int d = 0; d < 256; ++d)
        for (int c = 0; c < COLS; ++c) fill(d * COLS + c, c == tx ? counts[d] : (counts[255 - d] + 7u * c + d) & 0xffffu);
    std::vector<uint32_t> seg(kSegments * COLS, 0xdeadbeefu);
    for (int ty = 0; ty < kSegments; ++ty) seg[ty * COLS + tx] = byz::colsel::segment_sum<COLS>(ty, tx, count);
    for (int g = 0; g < kSegments; ++g) {
        uint32_t s = 0u;
        for (int b = 0; b < 16; ++b) s += counts[16 * g + b];
        if (seg[g * COLS + tx] != s) fail("segment sum", COLS, tx, g, {g, 0, seg[g * COLS + tx]}, {g, 0, s});
    }
    for (int rank : ranks) {
        const DigitRank want = brute_force(counts, rank);
        const DigitRank got = byz::colsel::walk_to_digit<COLS>(rank, seg.data(), tx, count);
        if (got.digit != want.digit || got.left != want.left || got.run != want.run) fail(what, COLS, tx, rank, got, want);
        if (!(0 <= got.left && static_cast<uint32_t>(got.left) < got.run)) fail("0 <= left < run", COLS, tx, rank, got, want);
    }
}

std::vector<int> every_rank(const std::vector<uint32_t>& counts) {
    int64_t n = 0;
    for (uint32_t c : counts) n += c;
    std::vector<int> ranks(n);
    for (int64_t r = 0; r < n; ++r) ranks[r] = static_cast<int>(r);
    return ranks;
}

// first, last, both sides of every occupied digit's edge, and a stride through the rest
std::vector<int> edge_ranks(const std::vector<uint32_t>& counts) {
    std::vector<int> ranks;
    int64_t before = 0;
    for (int d = 0; d < 256; ++d) {
        if (counts[d] != 0u) {
            ranks.push_back(static_cast<int>(before));
            ranks.push_back(static_cast<int>(before + counts[d] - 1));
            ranks.push_back(static_cast<int>(before + counts[d] / 2));
        }
        before += counts[d];
    }
    for (int64_t r = 0; r < before; r += before / 97 + 1) ranks.push_back(static_cast<int>(r));
    return ranks;
}

template <int COLS>
void check_tile() {
    std::vector<uint32_t> plain(256 * COLS), packed(256 * COLS);
    auto fill_plain = [&](int slot, uint32_t v) { plain[slot] = v; };
    auto count_plain = [&](int slot) { return plain[slot]; };
    // the rank in question in one half of the word, something else in the other
    auto fill_low = [&](int slot, uint32_t v) { packed[slot] = v | ((~v & 0xffffu) << 16); };
    auto count_low = [&](int slot) { return packed[slot] & 0xffffu; };
    auto fill_high = [&](int slot, uint32_t v) { packed[slot] = (v << 16) | ((v * 3u + 1u) & 0xffffu); };
    auto count_high = [&](int slot) { return packed[slot] >> 16; };
    auto check = [&](const char* what, const std::vector<uint32_t>& counts, const std::vector<int>& ranks, int tx) {
        check_column<COLS>(what, counts, ranks, tx, fill_plain, count_plain);
        check_column<COLS>(what, counts, ranks, tx, fill_low, count_low);
        check_column<COLS>(what, counts, ranks, tx, fill_high, count_high);
    };
    const std::vector<uint32_t> none(256, 0u);
    for (int tx = 0; tx < COLS; ++tx) {
        std::vector<uint32_t> counts = none;
        counts[0] = 1000u;                                   // all mass in digit 0
        check("all in digit 0", counts, every_rank(counts), tx);
        counts = none;
        counts[255] = 1000u;                                 // all mass in digit 255: the last step of both walks
        check("all in digit 255", counts, every_rank(counts), tx);
        counts.assign(256, 1u);                              // one key per digit; rank 255 is the last key
        check("one key per digit", counts, every_rank(counts), tx);
        counts = none;                                       // empty leading and trailing segments, and empty digits between
        counts[83] = 5u; counts[95] = 1u; counts[96] = 2u; counts[170] = 9u;
        check("empty segments around", counts, every_rank(counts), tx);
        counts = none;                                       // the last key of a column is the last counter's last key
        counts[16] = 3u; counts[254] = 2u; counts[255] = 1u;
        check("the last key", counts, every_rank(counts), tx);
    }
    std::mt19937 rng(20260 + COLS);
    for (int round = 0; round < 200; ++round) {
        // up to 65,535 keys over a random share of the digits: a packed half never overflows
        const int total = round == 0 ? 65535 : 1 + static_cast<int>(rng() % 65535u);
        const int occupied = 1 + static_cast<int>(rng() % 256u);
        std::vector<uint32_t> counts = none;
        if (round % 3 == 0) {                                // spread key by key
            for (int k = 0; k < total; ++k) counts[(static_cast<int>(rng() % static_cast<uint32_t>(occupied)) * 37 + round) & 255] += 1u;
        } else {                                             // in lumps
            for (int left = total; left > 0;) {
                const int lump = 1 + static_cast<int>(rng() % static_cast<uint32_t>(left));
                counts[(static_cast<int>(rng() % static_cast<uint32_t>(occupied)) * 37 + round) & 255] += static_cast<uint32_t>(lump);
                left -= lump;
            }
        }
        std::vector<int> ranks = edge_ranks(counts);
        ranks.push_back(total - 1);                          // the last key: the walk ends inside the counters, not behind them
        const int tx = static_cast<int>(rng() % static_cast<uint32_t>(COLS));
        check("random", counts, ranks, tx);
        // `packed` holds fill_high's words now: both halves of every word summed in one pass over the segment
        for (int g = 0; g < kSegments; ++g) {
            const Two s = byz::colsel::segment_sum<COLS>(g, tx, [&](int slot) { return Two{packed[slot] & 0xffffu, packed[slot] >> 16}; });
            Two want{0u, 0u};
            for (int b = 0; b < 16; ++b) want += Two{(counts[16 * g + b] * 3u + 1u) & 0xffffu, counts[16 * g + b]};
            if (s.x != want.x || s.y != want.y) fail("segment sums of both halves", COLS, tx, g, {g, 0, s.y}, {g, 0, want.y});
        }
    }
}

}  // namespace

int main() {
    check_tile<16>();
    check_tile<64>();
    if (failures != 0) {
        std::printf("column_select: %d failures\n", failures);
        return 1;
    }
    std::printf("column_select ok\n");
    return 0;
}
