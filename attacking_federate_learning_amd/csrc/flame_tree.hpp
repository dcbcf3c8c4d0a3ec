// FLAME's admission rule on a minimum spanning tree: HDBSCAN with 2 * min_cluster_size > n, where two clusters cannot coexist
// and the condensed tree and its stabilities reduce to one threshold.
//
//   w*        the smallest weight at which the graph {R_ij <= w*} has a connected component of at least m vertices
//   admitted  that component, tied edges at w* included; nobody when no finite weight gives one (w* = +inf)
//
// The components of a threshold graph are those of ANY minimum spanning tree cut at the same threshold, so the n - 1 edges of
// one MST in ascending weight order are all the walk needs, and which MST it is does not matter.
//
//   TreeWalk w = tree_walk_start();  the caller fills parent[v] = v, size[v] = 1
//   for every edge (weight key, a, b) in ascending key order:  tree_walk_edge(w, parent, size, n, m, key, a, b)
//   for every vertex v:                                        tree_admitted(w, parent, size, n, m, v)
//
// The union-find is union by size with path halving; every find is capped at n steps, so a corrupted edge list cannot make the
// walk spin.  Weights are the total keys of order_keys.hpp (ordered_bits_total): -0.0 ties with +0.0, every NaN is all ones.
// A weight that is not finite (+inf, NaN, -inf) never merges anything.
// Plain C++17; compiles for the host with a plain compiler as well (tests/flame_tree_check.cpp).
#pragma once

#include <cstdint>

#include "order_keys.hpp"

#ifdef __HIPCC__
#define BYZ_TREE_FN __host__ __device__ __forceinline__
#else
#define BYZ_TREE_FN inline
#endif

namespace byz {

constexpr int kTreeSearching = 0;   // no component has reached m yet
constexpr int kTreeFound = 1;       // w* is known; edges of the same weight still merge
constexpr int kTreeClosed = 2;      // an edge above w* was seen: nothing merges any more

struct TreeWalk {                   // (plain: it lives in LDS on the device)
    int state;
    uint32_t w_star_key;            // (kTreeFound, kTreeClosed) the key of w*
};
BYZ_TREE_FN TreeWalk tree_walk_start() { return TreeWalk{kTreeSearching, 0u}; }

// the root of x, halving the path on the way; at most n steps
template <typename Index>
BYZ_TREE_FN int tree_find(Index* parent, int x, int n) {
    for (int step = 0; step < n; ++step) {
        const int p = static_cast<int>(parent[x]);
        if (p == x) break;
        const int gp = static_cast<int>(parent[p]);
        parent[x] = static_cast<Index>(gp);
        x = gp;
    }
    return x;
}

// the same without writing: what the parallel labelling uses
template <typename Index>
BYZ_TREE_FN int tree_root(const Index* parent, int x, int n) {
    for (int step = 0; step < n; ++step) {
        const int p = static_cast<int>(parent[x]);
        if (p == x) break;
        x = p;
    }
    return x;
}

// one edge of the ascending list
template <typename Index>
BYZ_TREE_FN void tree_walk_edge(TreeWalk& w, Index* parent, Index* size, int n, int m, uint32_t key, int a, int b) {
    if (w.state == kTreeClosed) return;
    if (!ordered_is_finite(key)) return;
    if (w.state == kTreeFound && key != w.w_star_key) {
        w.state = kTreeClosed;
        return;
    }
    if (a < 0 || b < 0 || a >= n || b >= n) return;
    int ra = tree_find(parent, a, n), rb = tree_find(parent, b, n);
    if (ra == rb) return;
    if (static_cast<int>(size[ra]) < static_cast<int>(size[rb])) {
        const int t = ra;
        ra = rb;
        rb = t;
    }
    parent[rb] = static_cast<Index>(ra);
    const int merged = static_cast<int>(size[ra]) + static_cast<int>(size[rb]);
    size[ra] = static_cast<Index>(merged);
    if (w.state == kTreeSearching && merged >= m) {
        w.state = kTreeFound;
        w.w_star_key = key;
    }
}

// 2 m > n: at most one component holds m vertices
template <typename Index>
BYZ_TREE_FN bool tree_admitted(const TreeWalk& w, const Index* parent, const Index* size, int n, int m, int v) {
    if (w.state == kTreeSearching) return false;
    return static_cast<int>(size[tree_root(parent, v, n)]) >= m;
}

// w* as a float: +inf when nobody is admitted
BYZ_TREE_FN float tree_w_star(const TreeWalk& w) {
    return w.state == kTreeSearching ? __builtin_inff() : from_ordered_bits(w.w_star_key);
}

}  // namespace byz

#undef BYZ_TREE_FN
