// FLAME's first stage (Nguyen et al., "FLAME: Taming Backdoors in Federated Learning", USENIX Security 2022; beyond the
// reference): pairwise cosine distances, HDBSCAN with min_cluster_size > n / 2 (Campello, Moulavi and Sander 2013) and the
// rejection of everything outside the one majority cluster.  With 2 m > n two clusters cannot coexist and HDBSCAN's condensed
// tree reduces to one threshold on a minimum spanning tree of the mutual reachability graph (flame_tree.hpp).
//
//   cosine_from_gram_kernel   c_ij = fl32(max(0, 1 - g_ij / (sqrt(g_ii) * sqrt(g_jj)))) from the fp64 Gram, in fp64 in this order
//                             of operations; the diagonal, a row with g_ii not finite or <= 0 (row and column) and a non-finite
//                             g_ij are +inf.  Entry (i, j) reads the lower triangle's g_max(i,j),min(i,j): symmetric as bits.
//   core_distance_kernel      core_i = the ms-th smallest off-diagonal entry of row i in the key order (ordered_bits_total of
//                             the distance, then the column): ms rounds of "smallest key above the previous one", each a
//                             fixed number of trips over the row; ms = 1 is one round, the row minimum; ms = 0: core = 0.
//                             A distance of -inf counts as +inf here and in Prim (weight_key).
//                             isolated_i = row i has no finite off-diagonal entry.
//   mst_prim_kernel           Prim on R_ij = max(C_ij, core_i, core_j), never stored: ONE workgroup on owner_loop.hpp's scheme,
//                             the owned vertices' keys and parents in registers (every index static).
//                             A step is one coalesced read of the new tree vertex's row, the update of the owned keys and the
//                             workgroup's argmin of (key << 32 | vertex): the lane fold, one block exchange, the waves' fold.
//                             Exactly n - 1 steps.  No atomics, no grid synchronisation,
//                             no loop whose length depends on the data.  A vertex in the tree is marked by a bit of its
//                             owner's mask and competes with the all-ones pack, which no (key, vertex) pair equals.
//   flame_admit_kernel        one workgroup: the ascending edges (segment_sort_u64 on (weight key << 32 | slot)) pass through
//                             LDS 2048 at a time, thread 0 walks them with flame_tree.hpp's union-find (parent and size in
//                             LDS: 128 KiB at n = 16,384), then every vertex is labelled in parallel.
//   flame_weights_kernel      w_i = admitted_i ? s_i : 0.
#include "flame_tree.hpp"
#include "lane_exchange.hpp"
#include "order_keys.hpp"
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kCoreThreads = 256;
constexpr int kAdmitThreads = 1024;
constexpr int kAdmitChunk = 2048;              // edges staged in LDS at a time
constexpr unsigned long long kNoPack = ~0ull;  // no (key, vertex) pair: a vertex is below 2^14

// the key a distance competes with: order_keys.hpp's total key, with -inf taken for +inf -- a weight that is not finite merges
// nothing, and only while all of them sort LAST are the tree's finite edges a spanning forest of the finite graph
__device__ __forceinline__ uint32_t weight_key(float v) {
    const uint32_t k = ordered_bits_total(v);
    return k == 0x007fffffu ? 0xff800000u : k;
}

__device__ __forceinline__ unsigned long long min_u64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

__global__ __launch_bounds__(256) void cosine_from_gram_kernel(const double* __restrict__ gram, int64_t n, float* __restrict__ dist) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * 64 + (threadIdx.x & 63);
    const int64_t i = static_cast<int64_t>(blockIdx.y) * 4 + (threadIdx.x >> 6);
    if (i >= n || j >= n) return;
    const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
    float c = __builtin_inff();
    if (i != j) {
        const double g_hh = gram[hi * n + hi], g_ll = gram[lo * n + lo], g_hl = gram[hi * n + lo];
        const bool ok = __builtin_isfinite(g_hh) && g_hh > 0.0 && __builtin_isfinite(g_ll) && g_ll > 0.0 && __builtin_isfinite(g_hl);
        if (ok) {
            const double v = 1.0 - g_hl / (sqrt(g_hh) * sqrt(g_ll));
            if (__builtin_isfinite(v)) c = static_cast<float>(v > 0.0 ? v : 0.0);
        }
    }
    dist[i * n + j] = c;
}

__global__ __launch_bounds__(kCoreThreads) void core_distance_kernel(const float* __restrict__ dist, int n, int ms,
                                                                     float* __restrict__ core, int32_t* __restrict__ isolated) {
    __shared__ unsigned long long part[kCoreThreads / 64];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ row = dist + static_cast<int64_t>(i) * n;
    const int trips = (n + kCoreThreads - 1) / kCoreThreads;
    int finite = 0;
    for (int k = 0; k < trips; ++k) {
        const int j = k * kCoreThreads + tid;
        if (j < n && j != i) finite |= finite_bits(row[j]) ? 1 : 0;
    }
    finite = __syncthreads_or(finite);
    unsigned long long prev = 0;
    for (int r = 0; r < ms; ++r) {                    // (round 0 takes every key: the row minimum)
        unsigned long long best = kNoPack;
        for (int k = 0; k < trips; ++k) {
            const int j = k * kCoreThreads + tid;
            if (j < n && j != i) {
                const unsigned long long key = (static_cast<unsigned long long>(weight_key(row[j])) << 32) | static_cast<uint32_t>(j);
                if ((r == 0 || key > prev) && key < best) best = key;
            }
        }
        best = lanes::lanes_fold<32>(best, lane, min_u64);
        if (lane == 0) part[wave] = best;
        __syncthreads();
        prev = min_u64(min_u64(part[0], part[1]), min_u64(part[2], part[3]));
        __syncthreads();
    }
    if (tid == 0) {
        core[i] = ms == 0 ? 0.0f : from_ordered_bits(static_cast<uint32_t>(prev >> 32));
        isolated[i] = finite ? 0 : 1;
    }
}

__global__ __launch_bounds__(kOwnerThreads) void mst_prim_kernel(const float* __restrict__ dist, const float* __restrict__ core, int n,
                                                                int n_pad, unsigned long long* __restrict__ ekeys,
                                                                int32_t* __restrict__ eab) {
    __shared__ ExchangeBuf<unsigned long long> slot;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t key[kOwnerSlots], ckey[kOwnerSlots];
    int parent[kOwnerSlots];
    uint32_t done = 0;                                // bit s: vertex row_of(t, s) is in the tree, or beyond n
#pragma unroll
    for (int s = 0; s < kOwnerSlots; ++s) {
        const int v = row_of(t, s);
        key[s] = 0xffffffffu;
        parent[s] = 0;
        ckey[s] = v < n ? weight_key(core[v]) : 0xffffffffu;
        if (v >= n) done |= 1u << s;
    }
    if (t == 0) done |= 1u;                           // the tree starts at vertex 0
    for (int e = n - 1 + t; e < n_pad; e += kOwnerThreads) ekeys[e] = kNoPack;      // the sort's padding
    int u = 0, turn = 0;
    for (int step = 0; step < n - 1; ++step) {
        const float* __restrict__ row = dist + static_cast<int64_t>(u) * n;
        const uint32_t cu = weight_key(core[u]);
        float c[kOwnerSlots];
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s) {
            const int v = row_of(t, s);
            c[s] = v < n ? row[v] : __builtin_inff();
        }
        unsigned long long best = kNoPack;
#pragma unroll
        for (int s = 0; s < kOwnerSlots; ++s) {
            const int v = row_of(t, s);
            const bool live = ((done >> s) & 1u) == 0;
            uint32_t r = weight_key(c[s]);
            r = r > cu ? r : cu;
            r = r > ckey[s] ? r : ckey[s];
            if (live && r < key[s]) {
                key[s] = r;
                parent[s] = u;
            }
            const unsigned long long pack = (static_cast<unsigned long long>(key[s]) << 32) | static_cast<uint32_t>(v);
            best = min_u64(best, live ? pack : kNoPack);
        }
        const auto waves_min = [lane](unsigned long long v) { return lanes::lanes_fold<kOwnerWaves / 2>(v, lane, min_u64); };
        const unsigned long long win = block_exchange(lanes::lanes_fold<32>(best, lane, min_u64), slot, turn, lane, wave, waves_min);
        int nu = __builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(win)));
        const uint32_t wkey = __builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(win >> 32)));
        if (nu < 0 || nu >= n) nu = 0;                // (cannot happen: a live vertex is left at every step)
        if (owner_thread(nu) == t) {
            const int su = slot_of(nu);
            int p = 0;
#pragma unroll
            for (int s = 0; s < kOwnerSlots; ++s) p = s == su ? parent[s] : p;
            done |= 1u << su;
            ekeys[step] = (static_cast<unsigned long long>(wkey) << 32) | static_cast<uint32_t>(step);
            eab[2 * step] = p;
            eab[2 * step + 1] = nu;
        }
        u = nu;
    }
}

__global__ __launch_bounds__(kAdmitThreads) void flame_admit_kernel(const unsigned long long* __restrict__ sorted_keys,
                                                                    const int32_t* __restrict__ eab,
                                                                    const int32_t* __restrict__ isolated, int n, int m,
                                                                    int32_t* __restrict__ admitted, int32_t* __restrict__ admitted_out,
                                                                    FlameInfo* __restrict__ info) {
    extern __shared__ int32_t lds[];
    __shared__ TreeWalk walk;
    int32_t* parent = lds;
    int32_t* size = lds + n;
    uint32_t* ckey = reinterpret_cast<uint32_t*>(lds + 2 * static_cast<int64_t>(n));
    uint32_t* cab = ckey + kAdmitChunk;
    int* red = reinterpret_cast<int*>(cab + kAdmitChunk);
    const int tid = threadIdx.x;
    for (int v = tid; v < n; v += kAdmitThreads) {
        parent[v] = v;
        size[v] = 1;
    }
    if (tid == 0) walk = tree_walk_start();
    const int n_edges = n - 1;
    const int chunks = (n_edges + kAdmitChunk - 1) / kAdmitChunk;
    for (int c = 0; c < chunks; ++c) {
        __syncthreads();
        for (int e = tid; e < kAdmitChunk; e += kAdmitThreads) {
            const int g = c * kAdmitChunk + e;
            if (g < n_edges) {
                const unsigned long long k = sorted_keys[g];
                const uint32_t from = static_cast<uint32_t>(k);
                const bool ok = from < static_cast<uint32_t>(n_edges);
                ckey[e] = ok ? static_cast<uint32_t>(k >> 32) : 0xffffffffu;
                cab[e] = ok ? (static_cast<uint32_t>(eab[2 * from]) & 0xffffu) | (static_cast<uint32_t>(eab[2 * from + 1]) << 16) : 0u;
            }
        }
        __syncthreads();
        if (tid == 0) {
            TreeWalk w = walk;
            const int count = n_edges - c * kAdmitChunk < kAdmitChunk ? n_edges - c * kAdmitChunk : kAdmitChunk;
            for (int e = 0; e < count && w.state != kTreeClosed; ++e)
                tree_walk_edge(w, parent, size, n, m, ckey[e], static_cast<int>(cab[e] & 0xffffu), static_cast<int>(cab[e] >> 16));
            walk = w;
        }
    }
    __syncthreads();
    const TreeWalk w = walk;
    int count = 0, broken = 0;
    for (int v = tid; v < n; v += kAdmitThreads) {
        const int a = tree_admitted(w, parent, size, n, m, v) ? 1 : 0;
        admitted[v] = a;
        if (admitted_out != nullptr) admitted_out[v] = a;
        count += a;
        broken += isolated[v];
    }
    const int total = block_sum<int, kAdmitThreads>(count, red);
    const int total_broken = block_sum<int, kAdmitThreads>(broken, red);
    if (tid == 0) {
        info->admitted = total;
        info->broken_rows = total_broken;
        info->w_star = tree_w_star(w);
        info->admitted_f64 = static_cast<double>(total);
    }
}

__global__ __launch_bounds__(256) void flame_weights_kernel(const int32_t* __restrict__ admitted, const double* __restrict__ scales,
                                                            int64_t n, double* __restrict__ w) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) w[i] = admitted[i] != 0 ? scales[i] : 0.0;
}

}  // namespace

int flame_workspace(byz_ctx* ctx, int64_t n, FlameScratch* out) {
    out->n_pad = next_pow2(n - 1 < 2 ? 2 : n - 1);
    out->info = &device_scalars(ctx)->flame;
    Carve c;
    c.take(&out->core, n);
    c.take(&out->isolated, n);
    c.take(&out->ekeys, out->n_pad);
    c.take(&out->eab, 2 * n);
    c.take(&out->admitted, n);
    c.take(&out->w, n);
    return c.commit(ctx->flame);
}

int launch_cosine_from_gram(byz_ctx* ctx, const double* gram, int64_t n, float* dist, hipStream_t stream) {
    BYZ_REQUIRE(gram && dist && n > 0 && n <= kFlameMaxRows, "cosine distances: bad arguments (n = %lld)", (long long)n);
    KernelTimer timer(ctx, BYZ_K_DISTANCES, stream);
    const dim3 grid(static_cast<unsigned>(ceil_div(n, 64)), static_cast<unsigned>(ceil_div(n, 4)));
    cosine_from_gram_kernel<<<grid, 256, 0, stream>>>(gram, n, dist);
    return check_launch("cosine_from_gram_kernel");
}

// core[i] = the ms-th smallest off-diagonal entry of row i (ms = 0: 0); isolated[i] = the row has no finite one
int launch_flame_core(byz_ctx* ctx, const float* dist, int64_t n, int64_t ms, float* core, int32_t* isolated, hipStream_t stream) {
    BYZ_REQUIRE(dist && core && isolated && n >= 1 && n <= kFlameMaxRows && ms >= 0 && ms <= kFlameMaxSamples && ms <= n - 1,
                "flame core distances: bad arguments (n = %lld, ms = %lld)", (long long)n, (long long)ms);
    KernelTimer timer(ctx, BYZ_K_ROW_SORT, stream);
    core_distance_kernel<<<static_cast<unsigned>(n), kCoreThreads, 0, stream>>>(dist, static_cast<int>(n), static_cast<int>(ms), core,
                                                                               isolated);
    return check_launch("core_distance_kernel");
}

// 2 <= n <= kFlameMaxRows, 2 <= m <= n < 2 m, 0 <= ms <= min(32, n - 1): the caller's business (api.hip)
int launch_flame_select(byz_ctx* ctx, const FlameScratch& t, const float* dist, int64_t n, int64_t m, int64_t ms,
                        int32_t* admitted_out, hipStream_t stream) {
    BYZ_REQUIRE(dist && n >= 2 && n <= kFlameMaxRows && ms >= 0 && ms <= kFlameMaxSamples && ms <= n - 1 && m >= 2 && m <= n &&
                    2 * m > n, "flame select: bad arguments (n = %lld, m = %lld, ms = %lld)", (long long)n, (long long)m, (long long)ms);
    BYZ_TRY(launch_flame_core(ctx, dist, n, ms, t.core, t.isolated, stream));
    {
        KernelTimer timer(ctx, BYZ_K_MISC, stream);
        mst_prim_kernel<<<1, kOwnerThreads, 0, stream>>>(dist, t.core, static_cast<int>(n), static_cast<int>(t.n_pad), t.ekeys, t.eab);
        BYZ_TRY(check_launch("mst_prim_kernel"));
    }
    KernelTimer timer(ctx, BYZ_K_ROW_SORT, stream);
    BYZ_TRY(segment_sort_u64(ctx, t.ekeys, 1, t.n_pad, stream));
    const int lds_bytes = static_cast<int>((2 * n + 2 * kAdmitChunk + kAdmitThreads) * sizeof(int32_t));
    BYZ_HIP(allow_dynamic_lds(ctx, reinterpret_cast<const void*>(flame_admit_kernel), lds_bytes));
    flame_admit_kernel<<<1, kAdmitThreads, lds_bytes, stream>>>(t.ekeys, t.eab, t.isolated, static_cast<int>(n), static_cast<int>(m),
                                                               t.admitted, admitted_out, t.info);
    return check_launch("flame_admit_kernel");
}

int launch_flame_weights(byz_ctx* ctx, const int32_t* flags, const double* scales, int64_t n, double* w, hipStream_t stream) {
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    flame_weights_kernel<<<static_cast<unsigned>(ceil_div(n, 256)), 256, 0, stream>>>(flags, scales, n, w);
    return check_launch("flame_weights_kernel");
}

}  // namespace byz
