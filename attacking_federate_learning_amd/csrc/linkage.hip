// Agglomerative clustering (average, complete and single linkage) on a distance matrix, and ClippedClustering's selection on top
// of it (Li, Ngai and Voigt, "An Experimental Study of Byzantine-Robust Aggregation Schemes in Federated Learning", IEEE Trans.
// Big Data 2023; beyond the reference).  The rule is include/byzagg.h's; the algorithm is the nearest-partner cache of the
// "generic" algorithm in Muellner, "Modern hierarchical, agglomerative clustering algorithms" (2011), DESIGN.md 3.4o.
//
//   linkage_prepare_kernel    grid-wide, 64 x 64 tiles of the LOWER triangle through LDS: the fp32 matrix becomes the fp64 working
//                             matrix W, both triangles from the one entry (symmetric by construction); an entry that is not
//                             finite or is negative becomes `fill`, -0.0 becomes +0.0, the diagonal 0.  usable[i] = row i has a
//                             finite off-diagonal entry (an integer OR into a zeroed flag: no floating-point atomic anywhere).
//   linkage_nearest_kernel    grid-wide, a workgroup per row: the first nearest-partner cache, (W[i][k], k) smallest over the usable
//                             k != i.  A nonnegative double orders as its integer bits.
//   linkage_kernel<SLOTS, M>  ONE workgroup on owner_loop.hpp's scheme with SLOTS <= 16 slots a thread: their activity bits and
//                             cached distances in registers (every index static), the sizes and the cached partners in LDS.
//                             A step: the workgroup's argmin of (cached distance, slot) (block_argmin) -- the winner is
//                             the pair (a, b) smallest in (W[a][b], a, b), a < b, because the lowest slot holding the smallest
//                             distance has every partner at that distance above it, and its cache names the lowest of them;
//                             rows a and b of W read coalesced; the Lance-Williams update of the owned columns k; row a written
//                             coalesced and column a as scattered 8-byte stores, so that W stays consistent for a rescan; b retires;
//                             slot k's cache is repaired in registers by the thread that computed W[a][k], or, when its partner
//                             was a or b and the new distance does not win, queued in LDS; slot a's cache is the argmin of the new
//                             values, from registers; every queued slot is rescanned by ONE wave (a coalesced row read, the
//                             wave's argmin by DPP), 16 slots at a time and one barrier a round.  Exactly u - 1 steps for u usable rows.  No atomics on floats, no grid or host
//                             synchronisation.  The queue is the ONE loop whose length depends on the data: at most n a step.
//   linkage_cut_kernel        one workgroup: the first u - c merges set parent[b] = a (every b retires once: in parallel), 14 rounds
//                             of pointer jumping in LDS, flame_tree.hpp's tree_root for the label; a cluster's slot is its lowest
//                             row, so the clusters are numbered by a scan over the roots; the sizes by integer atomics.
//   linkage_pick_kernel       ClippedClustering: the larger of two clusters, label 0 (the lowest usable row's) on a tie.
#include "flame_tree.hpp"
#include "lane_exchange.hpp"
#include "order_keys.hpp"
#include "row_walk.hpp"

namespace byz {
namespace {

constexpr int kLinkBatch = 4;                  // slots whose two row entries are in flight at once (16 registers)
constexpr int kScanBatch = 8;                  // row entries a lane of a rescanning wave has in flight
constexpr int kPrepTile = 64;
constexpr int kNearThreads = 256;
constexpr int kJumpRounds = 14;                // 2^14 = kFlameMaxRows: a chain of parents is shorter
static_assert((int64_t{1} << kJumpRounds) >= kFlameMaxRows && kJumpRounds % 2 == 0, "the jumps end in the first buffer");

// a candidate of the argmin: the distance's bits and the slot it is cached for (or the column, in a rescan)
struct Cand {
    unsigned long long d;
    uint32_t idx;
};
__device__ __forceinline__ Cand no_cand() { return Cand{~0ull, ~0u}; }
__device__ __forceinline__ bool cand_less(const Cand& a, const Cand& b) { return a.d < b.d || (a.d == b.d && a.idx < b.idx); }
__device__ __forceinline__ Cand cand_min(const Cand& a, const Cand& b) { return cand_less(b, a) ? b : a; }
__device__ __forceinline__ unsigned long long dist_bits(double v) { return __builtin_bit_cast(unsigned long long, v); }

template <typename X>
__device__ __forceinline__ Cand each_field(const Cand& c, X x) { return {x(c.d), x(c.idx)}; }
// the minimum over the 2 * TOP lanes that differ in the low bits: every one of them gets it
template <int TOP>
__device__ __forceinline__ Cand lanes_argmin(Cand c, int lane) {
    return lanes::lanes_fold<TOP>(c, lane, [](const Cand& a, const Cand& b) { return cand_min(a, b); });
}
// the workgroup's minimum, in every thread: the lane fold, one block exchange (one barrier), the waves' fold
template <int WAVES>
__device__ __forceinline__ Cand block_argmin(Cand c, ExchangeBuf<Cand, WAVES>& xchg, int& turn, int lane, int wave) {
    return block_exchange(lanes_argmin<32>(c, lane), xchg, turn, lane, wave, [lane](Cand r) { return lanes_argmin<WAVES / 2>(r, lane); });
}

__global__ __launch_bounds__(256) void linkage_prepare_kernel(const float* __restrict__ dist, int64_t n, double fill,
                                                              double* __restrict__ W, int32_t* usable) {
    __shared__ float tile[kPrepTile][kPrepTile + 1];
    __shared__ int row_finite[kPrepTile], col_finite[kPrepTile];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti) return;
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    if (threadIdx.x < kPrepTile) {
        row_finite[threadIdx.x] = 0;
        col_finite[threadIdx.x] = 0;
    }
    __syncthreads();
    const int64_t i0 = static_cast<int64_t>(ti) * kPrepTile, j0 = static_cast<int64_t>(tj) * kPrepTile;
    for (int r = r0; r < kPrepTile; r += 4) {
        const int64_t i = i0 + r, j = j0 + c;
        float v = __builtin_nanf("");
        if (i < n && j < n && i > j) {
            v = dist[i * n + j];
            if (finite_bits(v)) {                     // (every writer stores the same 1)
                row_finite[r] = 1;
                col_finite[c] = 1;
            }
        }
        tile[r][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < kPrepTile) {
        const int64_t i = i0 + threadIdx.x, j = j0 + threadIdx.x;
        if (i < n && row_finite[threadIdx.x] != 0 && usable[i] == 0) atomicOr(&usable[i], 1);
        if (j < n && col_finite[threadIdx.x] != 0 && usable[j] == 0) atomicOr(&usable[j], 1);
    }
    auto clean = [fill](float v) { return (!finite_bits(v) || v < 0.0f) ? fill : (v == 0.0f ? 0.0 : static_cast<double>(v)); };
    for (int r = r0; r < kPrepTile; r += 4) {
        const int64_t i = i0 + r, j = j0 + c;         // the tile itself: below the diagonal, or the diagonal tile's both halves
        if (i < n && j < n) W[i * n + j] = i == j ? 0.0 : clean(i > j ? tile[r][c] : tile[c][r]);
        if (ti != tj) {                               // its mirror image
            const int64_t mi = j0 + r, mj = i0 + c;
            if (mi < n && mj < n) W[mi * n + mj] = clean(tile[c][r]);
        }
    }
}

__global__ __launch_bounds__(kNearThreads) void linkage_nearest_kernel(const double* __restrict__ W, const int32_t* __restrict__ usable,
                                                                       int n, unsigned long long* __restrict__ near_d,
                                                                       int32_t* __restrict__ near_p) {
    __shared__ ExchangeBuf<Cand, kNearThreads / 64> xchg;
    const int i = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ row = W + static_cast<int64_t>(i) * n;
    Cand best = no_cand();
    if (usable[i] != 0)
        for (int k = tid; k < n; k += kNearThreads)
            if (k != i && usable[k] != 0) best = cand_min(best, Cand{dist_bits(row[k]), static_cast<uint32_t>(k)});
    int turn = 0;
    best = block_argmin(best, xchg, turn, tid & 63, tid >> 6);
    if (tid == 0) {
        near_d[i] = best.d;
        near_p[i] = static_cast<int32_t>(best.idx);
    }
}

template <int METHOD>
__device__ __forceinline__ double lance_williams(double x, double y, double sa, double sb) {
    if constexpr (METHOD == BYZ_LINKAGE_AVERAGE) return (sa * x + sb * y) / (sa + sb);      // (-ffp-contract=off: four roundings)
    else if constexpr (METHOD == BYZ_LINKAGE_COMPLETE) return x > y ? x : y;
    else return x < y ? x : y;
}

template <int SLOTS, int METHOD>
__global__ __launch_bounds__(kOwnerThreads) void linkage_kernel(double* W, const int32_t* __restrict__ usable,
                                                               const unsigned long long* __restrict__ near_d,
                                                               const int32_t* __restrict__ near_p, int n, int32_t* __restrict__ pair,
                                                               double* __restrict__ height, int32_t* __restrict__ size_out,
                                                               LinkageInfo* __restrict__ info) {
    __shared__ ExchangeBuf<Cand> xchg;
    __shared__ int32_t sizes[SLOTS * kOwnerThreads];
    __shared__ unsigned short queue[SLOTS * kOwnerThreads];
    __shared__ unsigned short partner[SLOTS * kOwnerThreads];     // the cached partner of every slot (written by the slot's owner)
    __shared__ unsigned char alive[SLOTS * kOwnerThreads];        // the slot is a cluster: what a scanning wave reads of `active`
    __shared__ Cand found[2][kOwnerWaves];                  // a round of rescans: every wave's result (the buffers alternate)
    __shared__ int qcount[2], ucount;
    constexpr int kBatch = SLOTS < kLinkBatch ? SLOTS : (SLOTS == kOwnerSlots ? kLinkBatch / 2 : kLinkBatch);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long cd[SLOTS];
    uint32_t active = 0;                              // bit s: slot row_of(t, s) is a cluster
    if (t == 0) {
        qcount[0] = 0;
        qcount[1] = 0;
        ucount = 0;
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int k = row_of(t, s);
        cd[s] = ~0ull;
        sizes[k] = 1;
        partner[k] = 0;
        alive[k] = 0;
        if (k < n && usable[k] != 0) {
            active |= 1u << s;
            alive[k] = 1;
            cd[s] = near_d[k];
            partner[k] = static_cast<unsigned short>(near_p[k]);
        }
    }
    __syncthreads();
    if (active != 0) atomicAdd(&ucount, __builtin_popcount(active));
    __syncthreads();
    const int u = ucount;
    const int steps = u > 1 ? u - 1 : 0;
    for (int e = steps + t; e < n - 1; e += kOwnerThreads) {      // behind the merges
        pair[2 * e] = -1;
        pair[2 * e + 1] = -1;
        height[e] = __builtin_inf();
        size_out[e] = 0;
    }
    int turn = 0, rescans = 0, max_rescans = 0;
    for (int step = 0; step < steps; ++step) {
        Cand best = no_cand();
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
            if ((active >> s) & 1u) best = cand_min(best, Cand{cd[s], static_cast<uint32_t>(row_of(t, s))});
        const Cand win = block_argmin(best, xchg, turn, lane, wave);
        int a = __builtin_amdgcn_readfirstlane(static_cast<int>(win.idx));
        if (a < 0 || a >= n) a = 0;                   // (cannot happen: two clusters are left at every step)
        int b = partner[a];
        if (b >= n) b = a;                            // (cannot happen)
        const int qb = step & 1;
        int ld = n;                                   // opaque to the optimiser: the 16 products k * n of the scattered stores are
        asm volatile("" : "+s"(ld));                  // formed where they are used, not kept in 32 registers across the steps
        int tt = t;                                   // (the same for the 16 slot numbers and their byte offsets)
        asm volatile("" : "+v"(tt));
        const int na = sizes[a], nb = sizes[b];
        const double sa = static_cast<double>(na), sb = static_cast<double>(nb);
        if (t == 0) {
            pair[2 * step] = a;
            pair[2 * step + 1] = b;
            height[step] = __builtin_bit_cast(double, win.d);
            size_out[step] = na + nb;
            qcount[qb ^ 1] = 0;                       // the next step's queue: nobody reads it before that step's barrier
        }
        double* row_a = W + static_cast<int64_t>(a) * ld;
        const double* row_b = W + static_cast<int64_t>(b) * ld;
        Cand self = no_cand();                        // slot a's new cache
#pragma unroll
        for (int s0 = 0; s0 < SLOTS; s0 += kBatch) {
            double x[kBatch], y[kBatch];
#pragma unroll
            for (int q = 0; q < kBatch; ++q) {
                const int k = row_of(tt, s0 + q);
                const bool live = ((active >> (s0 + q)) & 1u) != 0 && k != a && k != b;
                x[q] = live ? row_a[k] : 0.0;
                y[q] = live ? row_b[k] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < kBatch; ++q) {
                const int s = s0 + q;
                const int k = row_of(tt, s);
                const bool live = ((active >> s) & 1u) != 0 && k != a && k != b;
                if (live) {
                    const double nv = lance_williams<METHOD>(x[q], y[q], sa, sb);
                    row_a[k] = nv;
                    W[static_cast<int64_t>(k) * ld + a] = nv;
                    const unsigned long long nd = dist_bits(nv);
                    self = cand_min(self, Cand{nd, static_cast<uint32_t>(k)});
                    const int p = partner[k];
                    if (nd < cd[s] || (nd == cd[s] && a <= p)) {
                        cd[s] = nd;
                        partner[k] = static_cast<unsigned short>(a);
                    } else if (p == a || p == b) {
                        queue[atomicAdd(&qcount[qb], 1)] = static_cast<unsigned short>(k);     // (k once a step: below n entries)
                    }
                }
            }
            if constexpr (SLOTS > kBatch) __builtin_amdgcn_sched_barrier(0);
        }
        if (owner_thread(b) == t) {
            active &= ~(1u << slot_of(b));
            alive[b] = 0;
        }
        const Cand mine = block_argmin(self, xchg, turn, lane, wave);      // (its barrier publishes W and the queue)
        if (owner_thread(a) == t) {
            const int sa_slot = slot_of(a);
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
                if (s == sa_slot) cd[s] = mine.d;
            partner[a] = static_cast<unsigned short>(mine.idx);
        }
        if (t == 0) sizes[a] = na + nb;               // (read again behind the next step's first barrier)
        int pending = qcount[qb];
        if (pending > n) pending = n;                 // (cannot happen)
        rescans += pending;
        max_rescans = pending > max_rescans ? pending : max_rescans;
        // the one loop whose length depends on the data: the queued slots, a wave each, 16 at a time
        for (int base = 0; base < pending; base += kOwnerWaves) {
            const int round = (base / (kOwnerWaves)) & 1;
            if (base + wave < pending) {
                int k = __builtin_amdgcn_readfirstlane(static_cast<int>(queue[base + wave]));
                if (k >= n) k = 0;                    // (cannot happen)
                const double* row = W + static_cast<int64_t>(k) * ld;
                Cand near = no_cand();
                for (int j0 = 0; j0 < n; j0 += 64 * kScanBatch) {
                    unsigned long long v[kScanBatch];
#pragma unroll
                    for (int q = 0; q < kScanBatch; ++q) {
                        const int j = j0 + 64 * q + lane;
                        const bool ok = j < n && j != k && alive[j < n ? j : 0] != 0;
                        v[q] = ok ? dist_bits(row[j]) : ~0ull;
                    }
#pragma unroll
                    for (int q = 0; q < kScanBatch; ++q)
                        near = cand_min(near, Cand{v[q], v[q] == ~0ull ? ~0u : static_cast<uint32_t>(j0 + 64 * q + lane)});
                }
                near = lanes_argmin<32>(near, lane);
                if (lane == 0) found[round][wave] = near;
            }
            __syncthreads();
            const int count = pending - base < kOwnerWaves ? pending - base : kOwnerWaves;
            for (int q = 0; q < count; ++q) {
                const int k = queue[base + q];
                if (owner_thread(k) == t) {
                    const Cand got = found[round][q];
                    const int sk = slot_of(k);
#pragma unroll
                    for (int s = 0; s < SLOTS; ++s)
                        if (s == sk) cd[s] = got.d;
                    partner[k < n ? k : 0] = static_cast<unsigned short>(got.idx);
                }
            }
        }
    }
    if (t == 0 && info != nullptr) {
        info->steps = steps;
        info->rescans = rescans;
        info->max_rescans = max_rescans;
    }
}

__global__ __launch_bounds__(kOwnerThreads) void linkage_cut_kernel(const int32_t* __restrict__ pair, const int32_t* __restrict__ usable,
                                                                   int n, int n_clusters, int32_t* __restrict__ labels,
                                                                   int32_t* cluster_sizes) {
    extern __shared__ int32_t lds[];
    __shared__ int ucount;
    int32_t* parent = lds;
    int32_t* other = lds + n;                         // the jumps' second buffer, then the clusters' numbers by root
    int* scan = reinterpret_cast<int*>(lds + 2 * static_cast<int64_t>(n));
    const int t = threadIdx.x;
    if (t == 0) ucount = 0;
    __syncthreads();
    int mine = 0;
    for (int v = t; v < n; v += kOwnerThreads) {
        parent[v] = v;
        mine += usable[v] != 0 ? 1 : 0;
    }
    for (int c = t; c < n_clusters; c += kOwnerThreads) cluster_sizes[c] = 0;
    if (mine != 0) atomicAdd(&ucount, mine);
    __syncthreads();
    const int merges = ucount > n_clusters ? ucount - n_clusters : 0;
    for (int m = t; m < merges; m += kOwnerThreads) {
        const int a = pair[2 * m], b = pair[2 * m + 1];
        if (a >= 0 && a < b && b < n) parent[b] = a;  // (every b retires once: no two writers)
    }
    __syncthreads();
    for (int round = 0; round < kJumpRounds; ++round) {
        for (int v = t; v < n; v += kOwnerThreads) other[v] = parent[parent[v]];
        __syncthreads();
        int32_t* swap = parent;
        parent = other;
        other = swap;
    }
    // a cluster's root is its lowest row: the clusters in ascending order of their lowest row are the roots in ascending order
    const int per = (n + kOwnerThreads - 1) / kOwnerThreads;
    const int lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int roots = 0;
    for (int v = lo; v < hi; ++v) roots += (usable[v] != 0 && parent[v] == v) ? 1 : 0;
    int number = block_exclusive_scan<kOwnerThreads>(roots, scan, nullptr);
    for (int v = lo; v < hi; ++v) other[v] = (usable[v] != 0 && parent[v] == v) ? number++ : -1;
    __syncthreads();
    for (int v = t; v < n; v += kOwnerThreads) {
        int label = -1;
        if (usable[v] != 0) label = other[tree_root(parent, v, n)];
        labels[v] = label;
        if (label >= 0 && label < n_clusters) atomicAdd(&cluster_sizes[label], 1);
    }
}

__global__ __launch_bounds__(kOwnerThreads) void linkage_pick_kernel(const int32_t* __restrict__ labels,
                                                                    const int32_t* __restrict__ cluster_sizes,
                                                                    const double* __restrict__ height, int n,
                                                                    int32_t* __restrict__ admitted, int32_t* __restrict__ admitted_out,
                                                                    LinkageInfo* __restrict__ info) {
    __shared__ int red[kOwnerThreads];
    const int t = threadIdx.x;
    const int n0 = cluster_sizes[0], n1 = cluster_sizes[1];
    const int winner = n1 > n0 ? 1 : 0;               // a tie: label 0, the cluster of the lowest usable row
    int count = 0;
    for (int v = t; v < n; v += kOwnerThreads) {
        const int a = labels[v] == winner ? 1 : 0;
        admitted[v] = a;
        if (admitted_out != nullptr) admitted_out[v] = a;
        count += a;
    }
    const int total = block_sum<int, kOwnerThreads>(count, red);
    if (t == 0) {
        const int u = n0 + n1;
        info->admitted = total;
        info->usable = u;
        info->top_height = u >= 2 ? height[u - 2] : 0.0;
        info->second_height = u >= 3 ? height[u - 3] : 0.0;
        info->admitted_f64 = static_cast<double>(total);
    }
}

template <int SLOTS>
int launch_linkage_slots(const LinkageScratch& t, int n, int method, int32_t* pair, double* height, int32_t* size, LinkageInfo* info,
                         hipStream_t stream) {
    if (method == BYZ_LINKAGE_AVERAGE)
        linkage_kernel<SLOTS, BYZ_LINKAGE_AVERAGE><<<1, kOwnerThreads, 0, stream>>>(t.W, t.usable, t.near_d, t.near_p, n, pair, height, size,
                                                                                   info);
    else if (method == BYZ_LINKAGE_COMPLETE)
        linkage_kernel<SLOTS, BYZ_LINKAGE_COMPLETE><<<1, kOwnerThreads, 0, stream>>>(t.W, t.usable, t.near_d, t.near_p, n, pair, height,
                                                                                    size, info);
    else
        linkage_kernel<SLOTS, BYZ_LINKAGE_SINGLE><<<1, kOwnerThreads, 0, stream>>>(t.W, t.usable, t.near_d, t.near_p, n, pair, height, size,
                                                                                  info);
    return check_launch("linkage_kernel");
}

}  // namespace

int linkage_workspace(byz_ctx* ctx, int64_t n, LinkageScratch* out) {
    out->info = &device_scalars(ctx)->linkage;
    Carve c;
    c.take(&out->W, n * n);
    c.take(&out->near_d, n);
    c.take(&out->near_p, n);
    c.take(&out->usable, n);
    c.take(&out->pair, 2 * n);
    c.take(&out->height, n);
    c.take(&out->size, n);
    c.take(&out->labels, n);
    c.take(&out->cluster_sizes, 2);
    c.take(&out->admitted, n);
    c.take(&out->w, n);
    return c.commit(ctx->linkage);
}

// 2 <= n <= kFlameMaxRows, a method of the three, fill finite and >= 0: the caller's business (api.hip)
int launch_linkage(byz_ctx* ctx, const LinkageScratch& t, const float* dist, int64_t n, int method, double fill, int32_t* pair,
                   double* height, int32_t* size, int32_t* usable_out, hipStream_t stream) {
    BYZ_REQUIRE(dist && pair && height && size && n >= 2 && n <= kFlameMaxRows && method >= 0 && method <= 2 && fill >= 0.0 &&
                    __builtin_isfinite(fill), "linkage: bad arguments (n = %lld, method = %d, fill = %g)", (long long)n, method, fill);
    {
        KernelTimer timer(ctx, BYZ_K_ROW_SORT, stream);
        BYZ_HIP(hipMemsetAsync(t.usable, 0, static_cast<size_t>(n) * sizeof(int32_t), stream));
        const unsigned tiles = static_cast<unsigned>(ceil_div(n, kPrepTile));
        linkage_prepare_kernel<<<dim3(tiles, tiles), 256, 0, stream>>>(dist, n, fill, t.W, t.usable);
        BYZ_TRY(check_launch("linkage_prepare_kernel"));
        linkage_nearest_kernel<<<static_cast<unsigned>(n), kNearThreads, 0, stream>>>(t.W, t.usable, static_cast<int>(n), t.near_d,
                                                                                      t.near_p);
        BYZ_TRY(check_launch("linkage_nearest_kernel"));
        if (usable_out != nullptr)
            BYZ_HIP(hipMemcpyAsync(usable_out, t.usable, static_cast<size_t>(n) * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    }
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    const int per = static_cast<int>(ceil_div(n, kOwnerThreads));
    const int ni = static_cast<int>(n);
    if (per <= 1) return launch_linkage_slots<1>(t, ni, method, pair, height, size, t.info, stream);
    if (per <= 2) return launch_linkage_slots<2>(t, ni, method, pair, height, size, t.info, stream);
    if (per <= 4) return launch_linkage_slots<4>(t, ni, method, pair, height, size, t.info, stream);
    if (per <= 8) return launch_linkage_slots<8>(t, ni, method, pair, height, size, t.info, stream);
    return launch_linkage_slots<16>(t, ni, method, pair, height, size, t.info, stream);
}

// labels (n) and cluster_sizes (n_clusters) of the cut into n_clusters; 1 <= n_clusters <= n
int launch_linkage_cut(byz_ctx* ctx, const int32_t* pair, int64_t n, const int32_t* usable, int64_t n_clusters, int32_t* labels,
                       int32_t* cluster_sizes, hipStream_t stream) {
    BYZ_REQUIRE(pair && usable && labels && cluster_sizes && n >= 2 && n <= kFlameMaxRows && n_clusters >= 1 && n_clusters <= n,
                "linkage cut: bad arguments (n = %lld, clusters = %lld)", (long long)n, (long long)n_clusters);
    KernelTimer timer(ctx, BYZ_K_ROW_SORT, stream);
    const int lds_bytes = static_cast<int>((2 * n + kOwnerThreads) * sizeof(int32_t));
    BYZ_HIP(allow_dynamic_lds(ctx, reinterpret_cast<const void*>(linkage_cut_kernel), lds_bytes));
    linkage_cut_kernel<<<1, kOwnerThreads, lds_bytes, stream>>>(pair, usable, static_cast<int>(n), static_cast<int>(n_clusters), labels,
                                                              cluster_sizes);
    return check_launch("linkage_cut_kernel");
}

// ClippedClustering's selection: the linkage, the cut into two, the larger cluster into t.admitted (and admitted_out, optional)
int launch_clipped_clustering_select(byz_ctx* ctx, const LinkageScratch& t, const float* dist, int64_t n, int method, double fill,
                                     int32_t* admitted_out, hipStream_t stream) {
    BYZ_TRY(launch_linkage(ctx, t, dist, n, method, fill, t.pair, t.height, t.size, nullptr, stream));
    BYZ_TRY(launch_linkage_cut(ctx, t.pair, n, t.usable, 2, t.labels, t.cluster_sizes, stream));
    KernelTimer timer(ctx, BYZ_K_ROW_SORT, stream);
    linkage_pick_kernel<<<1, kOwnerThreads, 0, stream>>>(t.labels, t.cluster_sizes, t.height, static_cast<int>(n), t.admitted,
                                                       admitted_out, t.info);
    return check_launch("linkage_pick_kernel");
}

}  // namespace byz
