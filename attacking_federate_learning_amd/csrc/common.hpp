// Shared host-side plumbing of libbyzagg: the context, error reporting, workspace growth and the
// per-kernel event timing used by bench.py.  gfx950 only; no other target is considered.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/byzagg.h"
#include "carve.hpp"
#include "device_scalars.hpp"
#include "owner_loop.hpp"

namespace byz {

void set_error(const char* fmt, ...);

#define BYZ_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            ::byz::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                             __LINE__);                                                     \
            return BYZ_E_HIP;                                                               \
        }                                                                                   \
    } while (0)

#define BYZ_TRY(expr)            \
    do {                         \
        int rc_ = (expr);        \
        if (rc_ != BYZ_OK) return rc_; \
    } while (0)

#define BYZ_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            ::byz::set_error(__VA_ARGS__); \
            return BYZ_E_INVALID;       \
        }                               \
    } while (0)

// A device buffer that only ever grows; growth happens between kernels, never inside the hot loop
// once byz_ctx_reserve has been called with the largest shape.  It frees its memory with the context
// (byz_ctx_destroy: `delete ctx`, on the context's device, after the device has gone idle).
struct Buffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    ~Buffer() {
        if (ptr) (void)hipFree(ptr);
    }
    int ensure(size_t need) {
        if (need <= bytes) return BYZ_OK;
        if (ptr) BYZ_HIP(hipFree(ptr));
        ptr = nullptr;
        bytes = 0;
        BYZ_HIP(hipMalloc(&ptr, need));
        bytes = need;
        return BYZ_OK;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(ptr); }
};

struct PinnedBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() {
        if (ptr) (void)hipHostFree(ptr);
    }
    int ensure(size_t need) {
        if (need <= bytes) return BYZ_OK;
        if (ptr) BYZ_HIP(hipHostFree(ptr));
        ptr = nullptr;
        bytes = 0;
        BYZ_HIP(hipHostMalloc(&ptr, need, hipHostMallocDefault));
        bytes = need;
        return BYZ_OK;
    }
};

struct TimingSlot {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0.0;
    int64_t launches = 0;
};

}  // namespace byz

struct byz_ctx {
    int device = 0;
    int num_cus = 256;
    // workspaces
    byz::Buffer gram_partials;   // split-K slabs of the Gram kernel
    byz::Buffer gram;            // n x n fp64 Gram
    byz::Buffer tile_order;      // (ti, tj) of every lower-triangle tile, in XCD-friendly order
    byz::Buffer dup_rep;         // representative row of every group of identical rows (+ one flag word)
    byz::Buffer gram_tickets;    // chunked Gram schedule: next chunk allowed to update a tile's slab
    byz::Buffer gram_planes;     // pre-split Gram: the bf16 planes of one super-chunk of columns, in MFMA fragment order
    byz::Buffer gram_chunk_sums; // pre-split Gram, f16x2: the fp32 level-1 sums of every (chunk, tile) of a launch (deferred slab update)
    byz::Buffer plane_unscale;   // pre-split Gram, f16x2: 2^-shift of every (chunk, row) of the super-chunk (fp64)
    byz::Buffer plane_order;     // pre-split Gram: (256-row block, 128-row block) of every workgroup tile
    byz::Buffer spec_owner;      // speculative Bulyan loop: the row every (workgroup, thread) slot owns
    byz::Buffer split_redo;      // pre-split Gram: (chunk, row block) pairs whose sampled scale did not hold (count first)
    std::vector<int32_t> plane_order_host;   // bf16x3: (bi, tj) pairs; f16x2: the unit table, then (ti, tj) of every sum slot
    int64_t plane_order_T = -1;
    int64_t plane_order_share = 1 * 65536 + 0;
    int64_t plane_order_blocks = -2;         // f16x2: the live 32-row blocks the table's masks were made for
    int64_t plane_units = 0, plane_sum_slots = 0;
    byz::Buffer row_signature;   // dedup: 64-bit signature of every row
    byz::Buffer unique_rows;     // dedup: the unique rows, ascending
    byz::Buffer row_map;         // dedup: position of every row's representative among the unique rows (+ scratch)
    byz::Buffer gram_compact;    // dedup: Gram of the unique rows
    std::vector<int32_t> tile_order_host;
    int64_t tile_order_T = -1;
    int64_t tile_order_share = 1 * 65536 + 0;   // share_count * 65536 + share_index the list was built for
    byz::Buffer tile_owned;      // one byte per lower-triangle tile: 1 = in this launch's share
    int64_t row_map_rows = 0;    // dedup: row count the row_map currently describes (0: none)
    byz::Buffer gram_rep;        // first row with bitwise equal Gram entries (candidate identical row), per row
    byz::Buffer near_pairs;      // near-duplicate pairs (int2) whose distance is re-evaluated on the difference
    byz::Buffer near_sq;         // their squared distances (fp64)
    byz::Buffer near_rows;       // listed pairs per row (counts, then offsets): what makes the list's order canonical
    byz::Buffer near_partial;    // per (pair, column chunk) partial sums
    int64_t near_pair_capacity = 0;
    byz::Buffer dist;            // n x n fp32 distances (when the caller does not pass one)
    byz::Buffer sorted_idx;      // n x n uint16: column index at every ascending rank
    byz::Buffer sorted_val;      // n x n fp32: every row's distances in ascending order (the reference-arithmetic re-score)
    byz::Buffer rank_t;          // n x n uint16: rank_t[w][u] = rank of column w in row u
    byz::Buffer rank_rows;       // n x n uint16: the same table as the row sort writes it, rank_rows[u][w] (transposed into rank_t)
    byz::Buffer row_total;       // n fp64: sum of a row's finite distances
    byz::Buffer row_top;         // n fp64: sum of a row's largest `drop` finite distances; then n counts of non-finite ones
    byz::Buffer scores;          // n fp32 Krum scores
    byz::Buffer multi_krum;      // Multi-Krum's ranking, carved (carve.hpp): n_pad sort keys; n row flags
    byz::Buffer multi_krum_rows; // Multi-Krum's selected rows in ascending order (the list the row-list mean walks)
    byz::Buffer rows;            // the row-distance loops (geometric median, centered clipping, FLTrust), carved into RowScratch's
                                 // four arrays (api.hip: row_scratch): rowsq's (chunk, row) fp64 partials (at most 64 per row, FLTrust:
                                 // twice that); sq (n + 1; FLTrust: p, q, q0); the weights or scales (n; FLTrust: ts and w); FLTrust's
                                 // root partials
    byz::Buffer dnc;             // DnC, carved into DncScratch's arrays (dnc_workspace): the centred sample (n x sub_dim fp64), the
                                 // column partials, the n-vectors, the state, keep and good (int32, an array each)
    byz::Buffer nnm_keys;        // nearest-neighbour mixing: n segments of next_pow2(n) sort keys
    byz::Buffer nnm_mask;        // carved: its 0/1 fp32 mask, transposed ([j][i], padded to the mix kernel's tiles); the n list lengths
    byz::Buffer nnm_lists;       // its neighbour lists (n x k int32) and their lengths (n) when the caller passes no buffer
    byz::Buffer signguard;       // SignGuard, carved into SgScratch's arrays (signguard_workspace): the census partials, then the selection's
    byz::Buffer topk;            // top-k along a vector, carved (topk.hip: TopkScratch): the three histograms and the state, the chunk
                                 // arrays, the doubles of the columns layout, SparseFed's aggregate
    byz::Buffer weak_dp;         // weak DP's adaptive clip, carved (cclip.hip: launch_clip_scales): the sort keys of the rows' norms
    byz::Buffer flame;           // FLAME, carved into FlameScratch's arrays (flame.hip: flame_workspace): the core distances, the
                                 // tree's edges and their sort keys, the admitted flags, the weights
    byz::Buffer manhattan;       // the Manhattan distances, carved (manhattan.hip: manhattan_workspace): the tile kernel's fp64
                                 // partials (chunks x n x n), then the n x n sums
    byz::Buffer multi_metrics;   // Multi-Metrics, carved into MmScratch's arrays (multi_metrics.hip: multi_metrics_workspace)
    byz::Buffer linkage;         // agglomerative clustering, carved into LinkageScratch's arrays (linkage.hip: linkage_workspace): the fp64
                                 // working matrix (n x n), the first nearest partners, the merges, the labels, the flags, the weights
    byz::Buffer faba;            // FABA, carved into FabaScratch's arrays (faba.hip: faba_workspace): the rows' sums and bad counts, the
                                 // removal order, the kept flags, the weights
    byz::Buffer afa;             // AFA, carved into AfaScratch's arrays (afa.hip: afa_workspace): the rows' u, r and weights, the kept
                                 // flags, the rounds of removal
    byz::Buffer auror;           // Auror, carved into AurorScratch's arrays (auror.hip: auror_workspace): the weights, and the votes,
                                 // bad flags and counts of a call that carries no history
    byz::Buffer foolsgold;       // FoolsGold, carved into FoolsgoldScratch's arrays (foolsgold.hip: foolsgold_workspace): the rows' r, m,
                                 // a, weights and rescaled weights, the usable flags
    int64_t foolsgold_rows = 0;  // the rows of the last weights stage: what byz_foolsgold_trace_dev may copy
    byz::Buffer fang;            // the Fang attacks, carved (api.hip: fang_workspace): the column vectors (mean, lo or std, hi, the
                                 // direction or the attack vector), the Krum attack's t and q, its benign distance block and bounds
    // the last Krum attack's values (byz_fang_krum_info reports them; last[kReportFangKrum] says whether there was one)
    double fang_lambda0 = 0.0, fang_lambda = 0.0;
    int64_t fang_steps = 0, fang_chosen = -1;
    int32_t fang_succeeded = 0;
    byz::Buffer minmax;          // the Min-Max / Min-Sum attacks, carved (api.hip: minmax_workspace): mu, sigma and p, the moments a, b
                                 // and c in one all-reduce's worth, |mu|^2, the distance maximum and its workgroups' values
    byz::Buffer phocas;          // Phocas, carved (api.hip: byz_phocas_dev): the rank-trimmed mean the window is taken around, when the
                                 // caller does not ask for it
    // large_rows.hip: more than 16,384 rows
    byz::Buffer large_keys;    // sort keys of one batch of rows
    byz::Buffer large_idx;       // n x n uint32: column index at every ascending rank
    byz::Buffer large_rank;      // n x n uint32: rank of column w in row u, [u][w]
    byz::Buffer large_rank_t;    // n x n uint32: the same transposed, [w][u]: a pick reads the winner's row of it
    byz::Buffer large_dist_t;    // n x n fp32: the distance matrix transposed, [w][u] = d(u, w) (a caller's matrix need not be symmetric)
    byz::Buffer large_state;     // the Bulyan loop's per-row state
    byz::Buffer large_grid;      // its deciding kernel on many workgroups: every workgroup's best score, the list's counter
    bool redo_valid = false;     // the last trimmed mean went through the ring selection (redo_tiles[0] is its count)
    byz::Buffer redo_tiles;      // trimmed mean: tiles the ring selection handed to the general kernel (count first)
    byz::Buffer twin_class;      // 2n int32: twin class of every row (scratch, then final)
    byz::Buffer xchg;            // Bulyan grid loop: tagged 8-byte granules the workgroups exchange
    int64_t bulyan_rescored = 0; // rows the last Bulyan loop re-scored in the reference's fp32 arithmetic
    byz::Buffer selection;       // theta int32
    byz::Buffer scalars;         // one DeviceScalars (device_scalars.hpp): the winner, the status words, every info call's report
    byz::LastCall last[byz::kReportCount];   // per report: the last call that wrote it (its info call syncs that stream)
    bool small_configured = false;   // krum_small.hip: dynamic-LDS attributes set for this context's device
    // kernels whose hipFuncAttributeMaxDynamicSharedMemorySize has been raised for this context's device, and to what: the
    // attribute belongs to the (function, device) pair and setting it is a runtime call per launch otherwise (round 6)
    std::unordered_map<const void*, int> dynamic_lds;
    byz::Buffer assemble_table;  // byz_assemble_rows_dev: segment starts + every client's tensor pointers
    std::vector<int64_t> assemble_host;   // its host image: owned by the context, because an async copy out of pageable memory
    hipEvent_t assemble_copied = nullptr; // may still be reading it when the call returns; recorded behind that copy
    int64_t assemble_clients = 0, assemble_segments = 0, assemble_longest = 0, assemble_total = 0;   // what the device table holds
    byz::Buffer stage_in;        // device copy of a host matrix
    byz::Buffer stage_out;       // device result before download
    byz::PinnedBuffer pinned;    // host bounce buffer for small results
    // timing
    bool timing = false;
    byz::TimingSlot slots[BYZ_K_COUNT];
};

namespace byz {

inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, context) and size, not once per launch
inline hipError_t allow_dynamic_lds(byz_ctx* ctx, const void* kernel, int bytes) {
    auto it = ctx->dynamic_lds.find(kernel);
    if (it != ctx->dynamic_lds.end() && it->second >= bytes) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) ctx->dynamic_lds[kernel] = bytes;
    return e;
}

inline DeviceScalars* device_scalars(byz_ctx* ctx) { return ctx->scalars.as<DeviceScalars>(); }
inline int32_t* device_status_word(byz_ctx* ctx) { return &device_scalars(ctx)->core.status; }
inline int32_t* attack_redo_word(byz_ctx* ctx) { return &device_scalars(ctx)->core.attack_redo; }
inline int32_t* near_pair_count_word(byz_ctx* ctx) { return &device_scalars(ctx)->core.near_pairs; }
inline int32_t* krum_winner_word(byz_ctx* ctx) { return &device_scalars(ctx)->core.krum_winner; }
// a call that writes the report `kind` on `stream`: what the report's info call synchronises
inline void mark(byz_ctx* ctx, ReportKind kind, hipStream_t stream) { ctx->last[kind] = {stream, true}; }

// Brackets one kernel launch with events when timing is on (bench.py's roofline leg).
struct KernelTimer {
    byz_ctx* ctx;
    int kernel;
    hipStream_t stream;
    hipEvent_t start = nullptr, stop = nullptr;
    KernelTimer(byz_ctx* c, int k, hipStream_t s) : ctx(c), kernel(k), stream(s) {
        if (ctx->timing) {
            (void)hipEventCreate(&start);
            (void)hipEventCreate(&stop);
            (void)hipEventRecord(start, stream);
        }
    }
    ~KernelTimer() {
        if (ctx->timing && start) {
            (void)hipEventRecord(stop, stream);
            ctx->slots[kernel].pending.emplace_back(start, stop);
        }
    }
};

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("launch of %s failed: %s", what, hipGetErrorString(e));
        return BYZ_E_HIP;
    }
    return BYZ_OK;
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t next_pow2(int64_t v) {
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// an integer environment switch: `fallback` when the variable is unset
inline int env_int(const char* name, int fallback) {
    const char* v = std::getenv(name);
    return v ? std::atoi(v) : fallback;
}

// ---- kernel launchers (one per .hip file) -------------------------------------------------------
int launch_column_mean(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                       float* out, hipStream_t stream);
int launch_column_drift(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                        float num_std, float* drift, float* mean, float* stdev, hipStream_t stream);
int launch_column_chain(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* carry,
                        const float* mean, float* out, hipStream_t stream);
int launch_column_finish(byz_ctx* ctx, const float* sum, const float* sumsq, int64_t total_rows, float num_std, int64_t n_cols,
                         float* mean, float* stdev, float* drift, hipStream_t stream);
int launch_broadcast_rows(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                          const float* vec, hipStream_t stream);
int launch_drift_axpy(byz_ctx* ctx, float* mean, const float* stdev, int64_t n, float num_std,
                      hipStream_t stream);
int launch_server_update(byz_ctx* ctx, float* w, float* v, const float* agg, int64_t n, float momentum,
                         float lr, hipStream_t stream);
int launch_copy_row(byz_ctx* ctx, const float* G, int64_t ld, int64_t n_rows, int64_t n_cols,
                    const int32_t* index_dev, float* out, hipStream_t stream);
// out[c] = mean over the rows G[row_list[0]], G[row_list[1]], ... in list order, no_defense's arithmetic
int launch_column_mean_rows(byz_ctx* ctx, const float* G, const int32_t* row_list, int64_t count, int64_t n_cols, int64_t ld,
                            float* out, hipStream_t stream);

// round_edges.hip: the steps either side of the path
constexpr int kMaxSegments = 32;   // tensors one assemble launch can place (more take further launches)
int launch_backdoor_initial(byz_ctx* ctx, const float* params, const float* mean, int64_t n, float lr, float* out,
                            hipStream_t stream);
int launch_backdoor_clip(byz_ctx* ctx, const float* mean, const float* stdev, const float* params, const float* mal,
                         int64_t n, float lr, float z, float* out, hipStream_t stream);
int launch_assemble_row(byz_ctx* ctx, float* row, int64_t n_cols, int64_t n_segments, const float* const* segments,
                        const int64_t* lengths, hipStream_t stream);
int launch_assemble_columns(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_segments,
                            const float* const* segments, const int64_t* lengths, hipStream_t stream);
int launch_assemble_rows_again(byz_ctx* ctx, float* G, int64_t n_cols, int64_t ld, int64_t n_clients, int64_t n_segments,
                               hipStream_t stream);
int launch_assemble_rows(byz_ctx* ctx, float* G, int64_t n_cols, int64_t ld, int64_t n_clients, int64_t n_segments,
                         const float* const* segments, const int64_t* lengths, hipStream_t stream);

int launch_gram(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, double* gram,
                hipStream_t stream);
// gram_planes.hip: the long-K Gram on operands split once into bf16 planes
bool gram_planes_enabled();
int launch_gram_planes(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                       double* slabs, int share_count, int share_index, uint8_t* owned_host, bool f16, hipStream_t stream);
// One workgroup's work on one 8192-column chunk in the f16x2 tile kernel.  rb: the global 32-row block behind each of the
// twelve row-block slots of an LDS stage.  Per wave: `where` = LDS slot of its first A row block | slot of its first B row
// block << 8 | live 32 x 32 blocks of its 64 x 64 sub-tile (bit m32 * 2 + n32) << 16 | (row / 64) << 24 | (column / 64) << 25
// of the sub-tile inside its slab; sum_slot: where the slab's level-1 sums of a chunk go; slab = ti | tj << 16.
struct GramUnitWave {
    uint32_t where;
    int32_t sum_slot, slab;
};
struct GramUnit {
    int32_t rb[12];
    GramUnitWave wave[8];
};
constexpr int kGramUnitWords = static_cast<int>(sizeof(GramUnit) / sizeof(int32_t));
// The unit table for t128 slabs per side of which n_blocks32 32-row blocks hold rows (negative: every block of a live slab
// is multiplied), in launch order, and (ti, tj) of every sum slot (ti < 0: nobody writes it).  diagonal_units: the D1 / D2
// units and one sum slot per lower-triangle slab; otherwise the (bi, tj) list, this share's part of it, two slots per tile.
void build_gram_units(int64_t t128, int64_t n_blocks32, bool diagonal_units, int share_count, int share_index,
                      std::vector<GramUnit>& units, std::vector<int32_t>& slot_slab);
int launch_gram_share(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                      int share_count, int share_index, double* gram, hipStream_t stream, bool accumulate = false);
// dedup.hip: identical rows found before the Gram
int find_unique_rows(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, hipStream_t stream,
                     int64_t* n_unique_host);
int launch_gram_expand(byz_ctx* ctx, const double* compact, int64_t n_unique, int64_t n_rows, double* gram,
                       hipStream_t stream);
int launch_distances_from_gram(byz_ctx* ctx, const double* gram, int64_t n, float* dist, hipStream_t stream,
                               const float* G, int64_t n_cols, int64_t ld);
int launch_near_pair_sqdist(byz_ctx* ctx, const float* G, int64_t n_cols, int64_t ld, const int32_t* row_index,
                            double* sq_dev, hipStream_t stream);
int launch_near_pair_apply(byz_ctx* ctx, const double* sq_dev, int64_t n, float* dist, hipStream_t stream);

int launch_row_sort(byz_ctx* ctx, const float* dist, int64_t n, int64_t prefix_len, int64_t drop_count,
                    bool want_tables, hipStream_t stream);
int launch_krum_argmin(byz_ctx* ctx, int64_t n, int32_t* winner_dev, hipStream_t stream);
int launch_bulyan_loop(byz_ctx* ctx, const float* dist, int64_t n, int64_t theta, int64_t drop_count,
                       int64_t users_count, int64_t corrupted, int32_t* selection_dev, BulyanStatus* status_dev,
                       hipStream_t stream);

// large_rows.hip: beyond the LDS-resident kernels' 16,384 rows (BYZ_SELECT_LARGE=1 takes these paths at any size)
constexpr int64_t kLargeMaxRows = int64_t{1} << 20;
bool select_large_applies(int64_t n);
int segment_sort_u64(byz_ctx* ctx, unsigned long long* keys, int64_t n_segments, int64_t n_pad, hipStream_t stream);
int launch_row_sort_large(byz_ctx* ctx, const float* dist, int64_t n, int64_t prefix_len, int64_t drop_count, bool want_tables,
                          hipStream_t stream);
// multi_krum.hip: ctx->scores ranked (score, visit position), the first m rows in ranking order (selection_dev, optional)
// and in ascending order (rows_asc_dev)
int launch_multi_krum_rank(byz_ctx* ctx, int64_t n, int64_t m, int32_t* selection_dev, int32_t* rows_asc_dev, hipStream_t stream);
// the same with the count read from device memory (*count_dev rows of row_list; 0 rows: every column NaN)
int launch_column_mean_rows_counted(byz_ctx* ctx, const float* G, const int32_t* row_list, const int32_t* count_dev, int64_t n_cols,
                                    int64_t ld, float* out, hipStream_t stream);
// dnc.hip: the spectral defence's pieces.  The workspace for n rows and b sampled columns (ctx->dnc):
struct DncScratch {
    double *C, *part, *w, *bad, *wt, *y, *u, *scores, *state;
    int32_t *keep, *good;
};
int dnc_workspace(byz_ctx* ctx, int64_t n, int64_t b, DncScratch* out);
// one iteration's scores into t.scores (allreduce == nullptr: this GPU holds every sampled column; otherwise 3 + power_iters
// all-reduces of n doubles); b may be 0 on a rank that owns none of the sampled columns
int launch_dnc_scores(byz_ctx* ctx, const DncScratch& t, const float* G, int64_t n, int64_t ld, const int64_t* columns, int64_t b,
                      int64_t power_iters, byz_allreduce_f64_fn allreduce, void* user, void* stream);
// t.keep (&)= the n_keep lowest (score, row); then the kept rows ascending into t.good (and good_out), their count into the
// context's DnC report (and count_out)
int launch_dnc_rank(byz_ctx* ctx, const DncScratch& t, int64_t n, int64_t n_keep, bool first, hipStream_t stream);
int launch_dnc_compact(byz_ctx* ctx, const DncScratch& t, int64_t n, int32_t* good_out, int32_t* count_out, hipStream_t stream);
// geomed.hip: the geometric median's passes (row distances to a vector, weighted row mean) and its small loop kernels.
// skip_if_set / run_if_set (optional device words): the launch returns at once if *skip_if_set != 0, or if *run_if_set == 0.
// the column chunks of rowsq for this shape (at most 64: the partials are chunks x n_rows fp64)
int geomed_chunks(byz_ctx* ctx, int64_t n_rows, int64_t n_cols, int64_t* chunk_cols);
int launch_row_sqdist(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* z, double* partials,
                      double* sq, const int32_t* skip_if_set, const int32_t* run_if_set, hipStream_t stream);
int launch_weighted_mean(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const double* w, float* out,
                         const int32_t* skip_if_set, const int32_t* run_if_set, hipStream_t stream);
int launch_geomed_finite_check(byz_ctx* ctx, const float* v, int64_t n, double* flag_f64, hipStream_t stream);
int launch_geomed_fallback(byz_ctx* ctx, const double* sq0, int64_t n, double* w, const double* global_flag, hipStream_t stream);
int launch_geomed_step(byz_ctx* ctx, const double* sq, int64_t n, double* w, double nu, double ftol, int64_t k, int64_t max_iter,
                       hipStream_t stream);
int launch_geomed_weights(byz_ctx* ctx, const double* w, int64_t n, double* out, hipStream_t stream);
// cclip.hip: centered clipping's scales: s from sq (sq == nullptr: all 1), the counts into the context's report
int launch_cclip_scales(byz_ctx* ctx, const double* sq, int64_t n, double tau, double* s, hipStream_t stream);
// weak DP's scales from sq: the clip is `clip`, or (adaptive) the np.median of the finite rows' norms; s has launch_cclip_scales'
// bits in the fixed mode; the counts and the clip into the context's weak-DP report, the clip into clip_out (optional) as well
int launch_clip_scales(byz_ctx* ctx, const double* sq, int64_t n, double clip, bool adaptive, double* s, double* clip_out,
                       hipStream_t stream);
// noise.hip: out[c] = fl32((double)x[c] + sigma * (scale_dev ? *scale_dev : 1) * z[offset + c]), z the Philox normals of the
// global columns (philox.hpp); out may be x.  launch_noise_words: the stream's raw words of the same columns.
int launch_gaussian_noise(byz_ctx* ctx, const float* x, int64_t n, double sigma, uint64_t seed, uint64_t round, int64_t offset,
                          const double* scale_dev, float* out, hipStream_t stream);
int launch_noise_words(byz_ctx* ctx, uint64_t seed, uint64_t round, int64_t offset, int64_t n, uint32_t* words, hipStream_t stream);
// fang.hip: the Fang et al. attacks on the trimmed mean / median and on Krum.
// mean[j] = no_defense's mean over ALL n_rows rows, lo[j] / hi[j] = np.fmin.reduce / np.fmax.reduce over the rows >= first_benign,
// one read of G (any of the three may be null)
int launch_column_extremes(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t first_benign, float* mean,
                           float* lo, float* hi, hipStream_t stream);
struct FangDraw {
    double b, k_lo, k_hi;
    uint64_t seed, round;
    int64_t offset;       // the global column of the caller's column 0
};
// the n_attackers first rows of G drawn from the columns' intervals; partial: a = mu, b = sigma (c unused), else a = mean, b = lo, c = hi
int launch_fang_fill(byz_ctx* ctx, float* G, int64_t n_attackers, int64_t n_cols, int64_t ld, const FangDraw& draw, bool partial,
                     const float* a, const float* b, const float* c, hipStream_t stream);
// out[j] = mean[j] > 0 ? positive : otherwise
int launch_sign_vector(byz_ctx* ctx, const float* mean, int64_t n_cols, float positive, float otherwise, float* out, hipStream_t stream);
// bounds[0] = the bits of min_i S_i, S_i = the fp64 sum in column order of row i of the m x m benign block without its diagonal and
// without the first of its largest entries; bounds[1] = the bits of max_i q_i.  Non-negative doubles order as their bits do.
int launch_fang_krum_bound(byz_ctx* ctx, const float* block, const double* q, int64_t m, unsigned long long* bounds, hipStream_t stream);
// Theorem 1's bound from the two values above
double fang_lambda0(double s_min, double q_max, int64_t n, int64_t c, int64_t n_cols);
// the c attacker rows and columns of dist (n x n): fl32(sqrt(max(q_i + (2 lambda) t_i + (lambda lambda) d, 0))) against benign i,
// 0 between attackers, +inf on their diagonal
int launch_fang_krum_fill(byz_ctx* ctx, float* dist, int64_t n, int64_t c, int64_t n_cols, const double* q, const double* t,
                          double lambda, hipStream_t stream);
// geomed.hip, rowsq's kernel template in its third form: a[i] = sum_c ((double)x_ic - (double)mu_c)^2 (launch_row_sqdist's bits)
// and b[i] = sum_c (double)p_c ((double)mu_c - (double)x_ic) in one read of G (partials: 2 * chunks * n_rows)
int launch_row_moments(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* mu, const float* p,
                       double* partials, double* a, double* b, hipStream_t stream);
// minmax.hip: the Min-Max / Min-Sum attacks of Shejwalkar & Houmansadr.  The scalars of a call: DeviceScalars::minmax.
constexpr int kMinmaxMaxPartials = 1024;     // workgroups of the distance maximum's first launch at most
// p from mu, sigma and *norm_sq = |mu|^2 (minmax_solve.hpp: kPerturbUnit, kPerturbStd, kPerturbSign)
int launch_perturbation(byz_ctx* ctx, const float* mu, const float* sigma, const double* norm_sq, int kind, int64_t n_cols, float* p,
                        hipStream_t stream);
// *dmax = the largest finite entry off the diagonal of the leading r x r block of dist (row stride ld); 0 when there is none
int launch_dist_max(byz_ctx* ctx, const float* dist, int64_t r, int64_t ld, float* partials, float* dmax, hipStream_t stream);
// gamma and the report from the r rows' moments, c and (Min-Max) *dmax
int launch_minmax_solve(byz_ctx* ctx, const double* a, const double* b, const double* c, const float* dmax, int64_t r, int kind,
                        hipStream_t stream);
// rows 0 .. n_attackers - 1 = fl32(mu + gamma p) with the report's gamma; nothing when the report says broken
int launch_minmax_fill(byz_ctx* ctx, float* G, int64_t n_attackers, int64_t n_cols, int64_t ld, const float* mu, const float* p,
                       hipStream_t stream);
// flame.hip: FLAME's clustering stage.  The scalars of a call: DeviceScalars::flame.
constexpr int64_t kFlameMaxRows = kOwnerMaxRows;     // Prim's one workgroup owns 1024 x 16 vertices; the union-find fills the LDS
constexpr int64_t kFlameMaxSamples = 32;     // rounds of the core distance's selection at most
struct FlameScratch {
    FlameInfo* info;
    float* core;                     // n: the core distances
    int32_t *isolated, *eab, *admitted;      // n flags; the tree's edges (a, b) by slot (2 n); n flags
    unsigned long long* ekeys;       // n_pad: weight key << 32 | slot, all ones behind the n - 1 edges
    double* w;                       // n: the sum's weights
    int64_t n_pad;
};
int flame_workspace(byz_ctx* ctx, int64_t n, FlameScratch* out);
// dist = the cosine distances of the rows behind an fp64 Gram (diagonal and broken rows +inf)
int launch_cosine_from_gram(byz_ctx* ctx, const double* gram, int64_t n, float* dist, hipStream_t stream);
// core[i] = the ms-th smallest off-diagonal entry of row i in the key order (ms = 0: 0); isolated[i]: no finite entry
int launch_flame_core(byz_ctx* ctx, const float* dist, int64_t n, int64_t ms, float* core, int32_t* isolated, hipStream_t stream);
// core distances, Prim, the edge sort, the admission: t.admitted (and admitted_out, optional), the scalars into t.info
int launch_flame_select(byz_ctx* ctx, const FlameScratch& t, const float* dist, int64_t n, int64_t m, int64_t ms,
                        int32_t* admitted_out, hipStream_t stream);
// w[i] = flags[i] ? scales[i] : 0
int launch_flame_weights(byz_ctx* ctx, const int32_t* flags, const double* scales, int64_t n, double* w, hipStream_t stream);
// manhattan.hip: the pairwise L1 distances.  sums (n x n fp64, both triangles) = sum_c |g_ic - g_jc| over the columns given,
// additive over column shards; dist = the sums of the lower triangle rounded once to fp32, the diagonal and every pair whose sum
// is not finite +inf.  partial: the tile kernel's per-chunk sums (manhattan_workspace carves both).
constexpr int64_t kManhattanMaxRows = 16384;                      // the `Distances` limit FLAME has
constexpr int64_t kManhattanPartialBytes = int64_t{512} << 20;    // the column split stops where its partials would pass this
int manhattan_workspace(byz_ctx* ctx, int64_t n, int64_t d, double** partial, double** sums);
int launch_manhattan_sums(byz_ctx* ctx, const float* G, int64_t n, int64_t d, int64_t ld, double* partial, double* sums,
                          hipStream_t stream);
int launch_manhattan_from_sums(byz_ctx* ctx, const double* sums, int64_t n, float* dist, hipStream_t stream);
// multi_metrics.hip: Multi-Metrics' features, scores and selection.  The scalars of a call: DeviceScalars::mm.
constexpr int64_t kMmMaxRows = kOwnerMaxRows;        // the selection's one workgroup owns 1024 x 16 rows
struct MmScratch {
    MmInfo* info;
    float *man, *cos;                        // n x n each: the whole call's Manhattan and cosine matrices
    double *feat, *scores;                   // n x 3; n
    int32_t *usable, *flags, *rows, *count;  // n each; the chosen rows ascending; their number (what the mean reads)
};
int multi_metrics_workspace(byz_ctx* ctx, int64_t n, bool matrices, MmScratch* out);
// usable[i] = the Gram's g_ii is finite and > 0 (cosine_distances' notion), or: row i of cos has a finite off-diagonal entry
int launch_mm_usable_from_gram(byz_ctx* ctx, const double* gram, int64_t n, int32_t* usable, hipStream_t stream);
int launch_mm_usable_from_cos(byz_ctx* ctx, const float* cos, int64_t n, int32_t* usable, hipStream_t stream);
// feat[i] = (sum man_ij, sum euc_ij, sum cos_ij) over the usable j != i, in fp64; (inf, inf, inf) for a row that is not usable
int launch_mm_features(byz_ctx* ctx, const float* man, const float* euc, const float* cos, const int32_t* usable, int64_t n,
                       double* feat, hipStream_t stream);
// scores, the min(usable, keep) lowest (score, row) as 0 / 1 flags (t.flags and flags_out, optional), ascending in t.rows, their
// number in t.count, the scalars into t.info; scores_out optional
int launch_mm_select(byz_ctx* ctx, const MmScratch& t, const double* feat, int64_t n, int64_t keep, int32_t* flags_out,
                     double* scores_out, hipStream_t stream);
// out[c] = 0 for every column when *count_dev == 0 (the counted mean of no rows is 0 / 0)
int launch_mm_zero_if_empty(byz_ctx* ctx, const int32_t* count_dev, int64_t n_cols, float* out, hipStream_t stream);
// linkage.hip: agglomerative clustering and ClippedClustering's selection.  The scalars of a call: DeviceScalars::linkage.
struct LinkageScratch {
    LinkageInfo* info;
    double* W;                       // n x n: the working matrix
    unsigned long long* near_d;      // n: the bits of every row's smallest distance before the first merge
    int32_t *near_p, *usable, *pair, *size, *labels, *cluster_sizes, *admitted;   // its column; n flags; the merges (2 n; n); the
                                     // 2-cut's labels (n) and sizes (2); n flags
    double *height, *w;              // n: the merges' heights; the sum's weights
};
int linkage_workspace(byz_ctx* ctx, int64_t n, LinkageScratch* out);
// the u - 1 merges of the usable rows into pair (2 (n - 1)), height and size (n - 1 each; -1, +inf and 0 behind the merges);
// t.usable (and usable_out, optional): the n flags; the step and rescan counts into t.info
int launch_linkage(byz_ctx* ctx, const LinkageScratch& t, const float* dist, int64_t n, int method, double fill, int32_t* pair,
                   double* height, int32_t* size, int32_t* usable_out, hipStream_t stream);
// the first u - n_clusters merges replayed: labels (n; -1: not usable) numbered by lowest row, cluster_sizes (n_clusters)
int launch_linkage_cut(byz_ctx* ctx, const int32_t* pair, int64_t n, const int32_t* usable, int64_t n_clusters, int32_t* labels,
                       int32_t* cluster_sizes, hipStream_t stream);
// linkage, 2-cut, the larger cluster: t.admitted (and admitted_out, optional), the scalars into t.info
int launch_clipped_clustering_select(byz_ctx* ctx, const LinkageScratch& t, const float* dist, int64_t n, int method, double fill,
                                     int32_t* admitted_out, hipStream_t stream);
// faba.hip: FABA's selection on a distance matrix.  The scalars of a call: DeviceScalars::faba.
constexpr int64_t kFabaMaxRows = kOwnerMaxRows;      // the loop's one workgroup owns 1024 x 16 rows
struct FabaScratch {
    FabaReport* info;
    double *s, *w;                   // n: every row's initial sum; the aggregate's 0 / 1 weights
    int32_t *bad, *order, *kept;     // n: every row's initial bad count; the removal order (-1 behind it); the 0 / 1 flags
};
int faba_workspace(byz_ctx* ctx, int64_t n, FabaScratch* out);
// the initial sums, the removal loop: t.kept and t.w (kept_out optional), the order into order_out (or t.order), the scalars into
// t.info
int launch_faba_select(byz_ctx* ctx, const FabaScratch& t, const float* dist, int64_t n, int64_t r, int power, int32_t* kept_out,
                       int32_t* order_out, hipStream_t stream);
// afa.hip: AFA's selection on an fp64 Gram.  The scalars of a call: DeviceScalars::afa.
constexpr int64_t kAfaMaxRows = kOwnerMaxRows;       // the loop's one workgroup owns 1024 x 16 rows
struct AfaScratch {
    AfaReport* info;
    double *u, *r, *w;               // n: every row's initial u; sqrt of its diagonal (0: excluded); its weight, 0 when not kept
    int32_t *kept, *round_of;        // n: the 0 / 1 flags; the round of removal (0: excluded, -1: kept)
};
int afa_workspace(byz_ctx* ctx, int64_t n, AfaScratch* out);
// the usable rows, the initial u, the rounds: t.kept and t.w (kept_out, round_of_out and score_out optional), the weights' sum and
// the other scalars into t.info
int launch_afa_select(byz_ctx* ctx, const AfaScratch& t, const double* gram, int64_t n, const double* weights, double xi0,
                      double delta_xi, int64_t max_rounds, int32_t* kept_out, int32_t* round_of_out, double* score_out,
                      hipStream_t stream);
// auror.hip: Auror's per-column 2-means, its votes and the selection on them.  The scalars of a call: DeviceScalars::auror.
constexpr int64_t kAurorMaxRows = 16384;     // a workgroup's vote counters: one int32 and one byte a row in LDS
struct AurorScratch {
    AurorReport* info;
    double* w;                       // n: the aggregate's 0 / 1 weights
    long long *votes, *counts;       // n and 4: byz_auror_dev's own when the caller carries no history
    int32_t* bad;                    // n
};
int auror_workspace(byz_ctx* ctx, int64_t n, AurorScratch* out);
// every column clustered, votes (n), bad (n) and counts (4) overwritten or (accumulate) added to, gap (n_cols, optional) written
int launch_auror_votes(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, double alpha, int64_t max_iter,
                       bool accumulate, long long* votes, int32_t* bad, long long* counts, double* gap, hipStream_t stream);
// the flags into kept_out (optional) and t.w, the counts into t.info
int launch_auror_select(byz_ctx* ctx, const AurorScratch& t, const long long* votes, const int32_t* bad, const long long* counts,
                        int64_t n, double tau, int32_t* kept_out, hipStream_t stream);
// foolsgold.hip: FoolsGold's history update and its weights on an fp64 Gram.  The scalars of a call: DeviceScalars::foolsgold.
struct FoolsgoldScratch {
    FoolsgoldReport* info;
    double *r, *m, *a;               // n: sqrt of the diagonal (-1: excluded); the row maximum; the pardoned row maximum
    double *w, *rescaled;            // n: the weights l (0 for an excluded row); v / top with 1 read as 0.99
    int32_t* flags;                  // n: 1 usable, 0 excluded
};
int foolsgold_workspace(byz_ctx* ctx, int64_t n, FoolsgoldScratch* out);
// H (n x w, ld_h) += the n x w window that starts at G (ld_g), numpy's float32 += bits; any base alignment, any ld
int launch_rows_add(byz_ctx* ctx, float* H, int64_t ld_h, const float* G, int64_t n, int64_t w, int64_t ld_g, hipStream_t stream);
// the norms, the row maxima, the pardoned maxima, the weights: t.w, t.rescaled and t.flags (weights_out, maxcs_out and alpha_out
// optional), T and the other scalars into t.info
int launch_foolsgold_weights(byz_ctx* ctx, const FoolsgoldScratch& t, const double* gram, int64_t n, double kappa, int normalise,
                             double* weights_out, double* maxcs_out, double* alpha_out, hipStream_t stream);
// geomed.hip, the weighted mean's kernel template: out = v + sum_i s_i (x_i - v) / n (v and out may be one buffer)
int launch_clip_update(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* v, const double* s,
                       float* out, hipStream_t stream);
// geomed.hip, rowsq's kernel template with two sums a row: dot[i] = x_i . r, sq[i] = |x_i|^2 (partials: 2 * chunks * n_rows)
int launch_row_dots(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* r, double* partials,
                    double* dot, double* sq, hipStream_t stream);
// geomed.hip, the weighted mean's kernel template: out = *divisor > 0 ? sum_i w_i x_i / *divisor : 0
int launch_scaled_rows_sum(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const double* w,
                           const double* divisor, float* out, hipStream_t stream);
// fltrust.hip: FLTrust's trust scores ts and weights w from pq = p (n), q (n), q0 (1); T and the counts into the context's report
int launch_fltrust_trust(byz_ctx* ctx, const double* pq, int64_t n, double* ts, double* w, hipStream_t stream);
// signguard.hip: SignGuard's census and selection.  The workspace for n rows (ctx->signguard):
constexpr int kSgMaxSamples = BYZ_SIGNGUARD_MAX_SAMPLES;   // rows the bandwidth is estimated from at most
constexpr int kSgMaxShifts = 300;                          // mean-shift updates of one seed at most
constexpr double kSgMinBandwidth = 1.0 / (1 << 20);        // below it the bins no longer pack into 21 bits a coordinate
struct SgScratch {
    double *q_part, *pznq, *feat, *centres, *final_centres, *kth, *w;
    long long* cnt_part;
    unsigned long long *keys, *seeds;
    char* state;
    int32_t *norm_ok, *members, *order, *standing, *label_rows, *keep, *labels, *sample;
};
int signguard_workspace(byz_ctx* ctx, int64_t n, int64_t n_cols, SgScratch* out);
// q[i] = |x_i|^2 (launch_row_dots' sq, bit for bit) and the counts of positive, zero and negative values over the columns
// [win_start, win_start + win_len) in one read of G.  counts (3n int64), q (n) and pznq (4n fp64: pos, zero, neg, q) are optional.
int launch_row_signs(byz_ctx* ctx, const SgScratch& t, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t win_start,
                     int64_t win_len, long long* counts, double* q, double* pznq, hipStream_t stream);
int launch_signguard_counts_f64(byz_ctx* ctx, const long long* counts, const double* q, int64_t n, double* pznq, hipStream_t stream);
int launch_signguard_select(byz_ctx* ctx, const SgScratch& t, const double* pznq, int64_t n, int64_t window_len, double lower,
                            double upper, double bandwidth, const int32_t* sample, int64_t n_sample, int32_t* keep, double* w,
                            int32_t* labels, double* mk_out, hipStream_t stream);
// nnm.hip: nearest-neighbour mixing.  Lists: row i's k - 1 nearest rows at a finite distance and i itself, ascending, -1 behind
// them (nbr: n x k int32; counts optional: n); the mix: Y[i] = mean of the listed rows of G, one MFMA accumulator chain in row order
constexpr int64_t kNnmMaxRows = 16384;
int launch_nnm_neighbours(byz_ctx* ctx, const float* dist, int64_t n, int64_t k, int32_t* nbr, int32_t* counts, hipStream_t stream);
int launch_nnm_mix(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, const int32_t* nbr, const int32_t* counts,
                   int64_t k, float* Y, int64_t ldy, hipStream_t stream);
// robust_lr.hip: the robust learning rate's sign vote (votes[c] = #positive - #negative, decided on the bits) and the flip of an
// aggregate's sign bit where |votes[c]| < theta.  out == nullptr: the votes alone; otherwise out = no_defense's vector with the
// flips applied, in the same walk (votes optional).  Both count the flipped columns into the context's report.
int launch_sign_votes(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t theta, float* out,
                      int32_t* votes, hipStream_t stream);
int launch_sign_flip(byz_ctx* ctx, const float* agg, const int32_t* votes, int64_t n_cols, int64_t theta, float* out,
                     hipStream_t stream);
// bucketing.hip: s-bucketing's means.  Y[b] = the mean of the rows perm[b s .. min((b + 1) s, n)) of G in list order, no_defense's
// arithmetic (perm == nullptr: the identity); an entry of perm outside [0, n) is skipped, the divisor stays the bucket's length
int launch_bucket_means(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* perm, int64_t s,
                        float* Y, int64_t ldy, hipStream_t stream);
// topk.hip: the k columns of w = x (+ add) first in the order (key = bits & 0x7fffffff descending, column ascending) into out, the
// rest into residual (optional); residual may be x and out may be add.  allreduce == nullptr: one GPU holds the vector (rank 0
// of 1); otherwise this rank's slice of a vector of which k is the global count (four all-reduces: 2048, 1024, 1024 and
// rank_count doubles).  keep_agg_cols: the floats of topk_aggregate_workspace that must survive the call (0: none).
int launch_topk_sparsify(byz_ctx* ctx, const float* x, const float* add, int64_t n, int64_t k, int rank_index, int rank_count,
                         byz_allreduce_f64_fn allreduce, void* user, float* out, float* residual, int64_t keep_agg_cols, void* stream);
// n_cols floats of the top-k workspace for SparseFed's aggregate (nullptr: the allocation failed, the error text is set)
float* topk_aggregate_workspace(byz_ctx* ctx, int64_t n_cols);
int launch_bulyan_loop_large(byz_ctx* ctx, const float* dist, int64_t n, int64_t theta, int64_t drop_count, int64_t users_count,
                             int64_t corrupted, const int32_t* twin_class, int32_t* selection_dev, BulyanStatus* status_dev,
                             hipStream_t stream);

int launch_trimmed_mean(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                        const int32_t* row_index, int64_t keep, float* out, hipStream_t stream);
// tall_select.hip: more rows than the register kernels hold (5,632): order statistics by radix select, the column streamed from HBM
int64_t trimmed_mean_max_rows();
int launch_trimmed_mean_tall(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                             int64_t keep, float* out, hipStream_t stream);
// rank_select.hip: the coordinate-wise median (median = true; trim_count ignored) and the rank-trimmed mean: two order statistics by one
// radix select (column_select.hpp), the column tile resident in registers up to 4,096 rows, streamed from HBM beyond
int launch_rank_select(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                       int64_t trim_count, bool median, float* out, hipStream_t stream);
// centre_window.hip: per column the mean of the `keep` values nearest a GIVEN centre (ties in row order), optionally the radius
// |x - c| of the last one kept: one order statistic by the same radix select and in the same two geometries.
// check_centre_window: the row ceiling (BYZ_E_UNSUPPORTED) and 1 <= keep <= n_rows (BYZ_E_INVALID), as the launcher applies them
int check_centre_window(const char* who, int64_t n_rows, int64_t keep);
int launch_centre_window(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                         const float* centre, int64_t keep, float* out, float* radius, hipStream_t stream);
// window_lean.hip: the row-split ring selection, first stage of the trimmed mean (round 3)
int launch_window_lean(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                       int64_t keep, float* out, int32_t* redo, hipStream_t stream);
int64_t select_max_rows();

// median_window.hip: lane_exchange.hpp's exchanges over the lane ids
int launch_lane_selftest(byz_ctx* ctx, int32_t* out, int32_t* n_patterns, hipStream_t stream);
// afa.hip: owner_loop.hpp's exchange, folds and block exchange on one workgroup of 1024 threads (rows of 1024 words)
int launch_owner_loop_selftest(byz_ctx* ctx, int32_t* out, int32_t* n_rows, hipStream_t stream);

// krum_small.hip: the whole of Krum for N <= 128 in five launches
bool krum_small_applies(int64_t n_rows, int64_t n_cols);
int reserve_small_workspaces(byz_ctx* ctx);
int launch_small_distances(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, float* dist,
                           hipStream_t stream);
int launch_small_krum(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, float* dist, int64_t prefix_len,
                      int32_t* winner_dev, float* out_row, hipStream_t stream);
int launch_small_select(byz_ctx* ctx, const float* dist, int64_t n_rows, int64_t prefix_len, const float* G, int64_t n_cols,
                        int64_t ld, int32_t* winner_dev, float* out_row, hipStream_t stream);
}  // namespace byz
