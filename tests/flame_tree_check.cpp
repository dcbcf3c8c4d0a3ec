// Stand-alone host check of csrc/flame_tree.hpp: the union-find walk over ascending edges against a brute-force threshold search.
// Seeded edge lists: random spanning trees with weights from a small set (so many tie, also at w*), +inf, NaN and -inf edges,
// n = 2, 3, a spread of small sizes and 16,384; m from n / 2 + 1 up to n.
//   c++ -std=c++17 -I attacking_federate_learning_amd/csrc tests/flame_tree_check.cpp -o flame_tree_check && ./flame_tree_check
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "flame_tree.hpp"

namespace {

struct Edge {
    float w;
    int a, b;
};

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32() {      // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 32);
}

// the threshold search, restated without a union-find: for every finite weight in ascending order, the components of the
// graph of the edges at or below it by breadth-first search; the first weight with a component of m vertices decides
void brute_force(const std::vector<Edge>& edges, int n, int m, std::vector<int>& admitted, float& w_star) {
    std::vector<float> levels;
    for (const Edge& e : edges)
        if (std::isfinite(e.w)) levels.push_back(e.w == 0.0f ? 0.0f : e.w);
    std::sort(levels.begin(), levels.end());
    levels.erase(std::unique(levels.begin(), levels.end()), levels.end());
    admitted.assign(n, 0);
    w_star = std::numeric_limits<float>::infinity();
    std::vector<std::vector<int>> adj(n);
    std::vector<int> comp(n), queue;
    for (float level : levels) {
        for (auto& a : adj) a.clear();
        for (const Edge& e : edges)
            if (std::isfinite(e.w) && e.w <= level) {
                adj[e.a].push_back(e.b);
                adj[e.b].push_back(e.a);
            }
        std::fill(comp.begin(), comp.end(), -1);
        for (int s = 0; s < n; ++s) {
            if (comp[s] >= 0) continue;
            queue.assign(1, s);
            comp[s] = s;
            for (size_t h = 0; h < queue.size(); ++h)
                for (int v : adj[queue[h]])
                    if (comp[v] < 0) {
                        comp[v] = s;
                        queue.push_back(v);
                    }
            if (static_cast<int>(queue.size()) >= m) {
                for (int v : queue) admitted[v] = 1;
                w_star = level;
                return;
            }
        }
    }
}

int run_case(int n, int m, int n_levels, int inf_every, bool extra_edges, int case_id) {
    std::vector<Edge> edges;
    const float levels[8] = {0.0f, 0.25f, 0.25f, 0.5f, 0.75f, 1.0f, 1.5f, 2.0f};
    for (int v = 1; v < n; ++v) {
        Edge e;
        e.a = static_cast<int>(next_u32() % static_cast<uint32_t>(v));
        e.b = v;
        e.w = levels[next_u32() % static_cast<uint32_t>(n_levels)];
        if (e.w == 0.0f && (next_u32() & 1)) e.w = -0.0f;      // ties with +0.0
        if (inf_every > 0 && next_u32() % static_cast<uint32_t>(inf_every) == 0) {
            const uint32_t kind = next_u32() % 4;
            e.w = kind == 0 ? std::numeric_limits<float>::quiet_NaN()
                            : (kind == 1 ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::infinity());
        }
        edges.push_back(e);
    }
    if (extra_edges)       // a list that is no tree: the walk must not care
        for (int k = 0; k < n / 2; ++k) {
            const int a = static_cast<int>(next_u32() % static_cast<uint32_t>(n)), b = static_cast<int>(next_u32() % static_cast<uint32_t>(n));
            if (a != b) edges.push_back({levels[next_u32() % static_cast<uint32_t>(n_levels)], a, b});
        }
    // ascending by (total key, slot), as the device sorts them
    std::vector<uint64_t> keys(edges.size());
    for (size_t i = 0; i < edges.size(); ++i) keys[i] = (static_cast<uint64_t>(byz::ordered_bits_total(edges[i].w)) << 32) | i;
    std::sort(keys.begin(), keys.end());
    std::vector<int32_t> parent(n), size(n, 1);
    for (int v = 0; v < n; ++v) parent[v] = v;
    byz::TreeWalk w = byz::tree_walk_start();
    for (uint64_t k : keys) {
        const Edge& e = edges[static_cast<uint32_t>(k)];
        byz::tree_walk_edge(w, parent.data(), size.data(), n, m, static_cast<uint32_t>(k >> 32), e.a, e.b);
    }
    std::vector<int> want;
    float want_w;
    brute_force(edges, n, m, want, want_w);
    const float got_w = byz::tree_w_star(w);
    int bad = 0;
    if (!(got_w == want_w)) ++bad;
    for (int v = 0; v < n; ++v)
        if ((byz::tree_admitted(w, parent.data(), size.data(), n, m, v) ? 1 : 0) != want[v]) ++bad;
    if (bad) std::printf("case %d (n = %d, m = %d): %d mismatches, w* %g against %g\n", case_id, n, m, bad, got_w, want_w);
    return bad;
}

}  // namespace

int main() {
    int cases = 0, bad = 0;
    const int sizes[] = {2, 3, 4, 5, 7, 16, 33, 64, 65, 200, 1025};
    for (int n : sizes)
        for (int rep = 0; rep < 12; ++rep) {
            const int lo = n / 2 + 1 < 2 ? 2 : n / 2 + 1;
            const int m = lo + static_cast<int>(next_u32() % static_cast<uint32_t>(n - lo + 1));
            bad += run_case(n, m, 1 + rep % 8, rep % 3 == 0 ? 0 : 2 + rep, rep % 4 == 3, cases);
            ++cases;
        }
    // every edge infinite: nobody; every edge one weight: everybody at once
    bad += run_case(9, 5, 1, 1, false, cases++);
    bad += run_case(9, 9, 1, 0, false, cases++);
    for (int rep = 0; rep < 3; ++rep) {
        bad += run_case(16384, 8193 + rep * 4000, 3 + 2 * rep, rep == 1 ? 50 : 0, rep == 2, cases);
        ++cases;
    }
    // a find on a corrupted parent array (a cycle) returns after n steps
    {
        std::vector<int32_t> parent = {1, 2, 0, 3};
        (void)byz::tree_find(parent.data(), 0, 4);
        (void)byz::tree_root(parent.data(), 0, 4);
        ++cases;
    }
    if (bad) {
        std::printf("flame_tree FAILED: %d mismatches in %d cases\n", bad, cases);
        return 1;
    }
    std::printf("flame_tree ok %d cases\n", cases);
    return 0;
}
