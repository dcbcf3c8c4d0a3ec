// extern "C" surface of libbyzagg (include/byzagg.h): argument checks mirroring the reference's asserts,
// workspace management, and the composition of the kernels into the reference's functions.
#include "common.hpp"

#include <cmath>
#include <cstring>

namespace byz {

static thread_local char g_error[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

namespace {

// number of items `some_list[:stop]` keeps for a list of `length` items (Python slice semantics, which
// the reference relies on in defences.py:34 and :50)
int64_t python_prefix_len(int64_t length, int64_t stop) {
    if (stop >= 0) return stop < length ? stop : length;
    return length + stop > 0 ? length + stop : 0;
}

int enter(byz_ctx* ctx) {
    if (!ctx) {
        set_error("null context");
        return BYZ_E_INVALID;
    }
    BYZ_HIP(hipSetDevice(ctx->device));
    return BYZ_OK;
}

int read_i32(byz_ctx* ctx, const int32_t* dev, int32_t* host, int64_t count, hipStream_t stream) {
    BYZ_TRY(ctx->pinned.ensure(static_cast<size_t>(count) * sizeof(int32_t)));
    BYZ_HIP(hipMemcpyAsync(ctx->pinned.ptr, dev, static_cast<size_t>(count) * sizeof(int32_t),
                           hipMemcpyDeviceToHost, stream));
    BYZ_HIP(hipStreamSynchronize(stream));
    std::memcpy(host, ctx->pinned.ptr, static_cast<size_t>(count) * sizeof(int32_t));
    return BYZ_OK;
}

// The first `bytes` of the device scalars (device_scalars.hpp: `host` is a CoreScalars or the whole DeviceScalars, which begins
// with one) in one read-back; the sticky status word is checked and cleared here, so that every entry point that synchronises
// anyway also reports what a kernel could only flag.
int read_scalars(byz_ctx* ctx, void* host, size_t bytes, hipStream_t stream) {
    BYZ_TRY(read_i32(ctx, ctx->scalars.as<int32_t>(), static_cast<int32_t*>(host), static_cast<int64_t>(bytes / sizeof(int32_t)), stream));
    const CoreScalars& core = *static_cast<const CoreScalars*>(host);
    const int32_t sticky = core.status;
    if (sticky != 0) {
        BYZ_HIP(hipMemsetAsync(device_status_word(ctx), 0, sizeof(int32_t), stream));
        if (sticky & kStatusLostTicket) {
            set_error("gram: a K chunk never received its tile's ticket (workgroups dispatched out of order or the GPU is "
                      "shared); the distance matrix of this call is invalid");
            return BYZ_E_HIP;
        }
        if (sticky & kStatusSmallTimeout) {
            set_error("krum (N <= 128): not every row's workgroup reported its score in time (GPU shared with another "
                      "process?); the result of this call is invalid");
            return BYZ_E_HIP;
        }
        if (sticky & kStatusNoTurn) {
            set_error("column statistics: a wave of the register-resident kernel never got its turn; the statistics of this "
                      "call are invalid (please report the shape)");
            return BYZ_E_HIP;
        }
        if (sticky & kStatusFalseTwin) {
            set_error("distances: two rows have bitwise equal Gram entries but differ; their near-duplicate pairs were not "
                      "re-evaluated (please report the input)");
            return BYZ_E_UNSUPPORTED;
        }
        set_error("distances: %d near-duplicate pairs exceed the list capacity (BYZ_NEAR_PAIR_CAPACITY); their distances "
                  "were not re-evaluated", core.near_pairs);
        return BYZ_E_UNSUPPORTED;
    }
    return BYZ_OK;
}

// what a hot path reads: the core alone
int read_core(byz_ctx* ctx, CoreScalars* core, hipStream_t stream) { return read_scalars(ctx, core, sizeof *core, stream); }

// read_core where nothing but the flagged failures is of interest: synchronises; a kernel that flagged one makes the call fail
int check_core(byz_ctx* ctx, hipStream_t stream) {
    CoreScalars core;
    return read_core(ctx, &core, stream);
}

// What every byz_*_info call does before it copies its fields out: the whole block in one read-back on the stream of the last
// call that wrote the report (which synchronises it), the sticky status with it.  refusal (optional): the error of a report
// that is refused before a first call; the others report the zeroed block.
int read_report(byz_ctx* ctx, ReportKind kind, const char* refusal, DeviceScalars* all) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(refusal == nullptr || ctx->last[kind].ran, "%s", refusal);
    return read_scalars(ctx, all, sizeof *all, ctx->last[kind].stream);
}

// the Krum winner's index to the host, when the caller asked for it (one synchronisation, the status word with it)
int read_winner(byz_ctx* ctx, int32_t* index_host, hipStream_t stream) {
    if (!index_host) return BYZ_OK;
    CoreScalars core;
    BYZ_TRY(read_core(ctx, &core, stream));
    *index_host = core.krum_winner;
    return BYZ_OK;
}

// the near-duplicate pairs the last distance kernel listed, refused when the list could not hold them
int near_pair_count(byz_ctx* ctx, int64_t* count, hipStream_t stream) {
    CoreScalars core;
    BYZ_TRY(read_core(ctx, &core, stream));
    *count = core.near_pairs;
    if (*count > ctx->near_pair_capacity) {
        set_error("distances: %lld near-duplicate pairs exceed the list capacity %lld (BYZ_NEAR_PAIR_CAPACITY)", (long long)*count,
                  (long long)ctx->near_pair_capacity);
        return BYZ_E_UNSUPPORTED;
    }
    return BYZ_OK;
}

int ensure_distance_workspaces(byz_ctx* ctx, int64_t n) {
    BYZ_TRY(ctx->gram.ensure(static_cast<size_t>(n) * n * sizeof(double)));
    BYZ_TRY(ctx->dist.ensure(static_cast<size_t>(n) * n * sizeof(float)));
    return BYZ_OK;
}

int check_matrix(const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const char* who) {
    if (!G || n_rows <= 0 || n_cols <= 0 || ld < n_cols) {
        set_error("%s: bad matrix (ptr %p, %lld x %lld, ld %lld)", who, (const void*)G, (long long)n_rows,
                  (long long)n_cols, (long long)ld);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

int check_krum_assert(int check_assert, int64_t users_count, int64_t corrupted_count) {
    if (check_assert && !(users_count >= 2 * corrupted_count + 1)) {  // defences.py:25
        set_error("('users_count>=2*corrupted_count + 3', %lld, %lld)", (long long)users_count, (long long)corrupted_count);
        return BYZ_E_PRECONDITION;
    }
    return BYZ_OK;
}

int check_bulyan_precondition(int64_t users_count, int64_t corrupted_count) {
    if (!(users_count >= 4 * corrupted_count + 3)) {  // defences.py:56
        set_error("bulyan: users_count >= 4*corrupted_count + 3 violated (%lld, %lld)", (long long)users_count,
                  (long long)corrupted_count);
        return BYZ_E_PRECONDITION;
    }
    return BYZ_OK;
}

// the row-count ceiling of the geometric median's family
int check_row_ceiling(const char* who, int64_t n_rows) {
    if (n_rows > kLargeMaxRows) {
        set_error("%s: at most %lld rows, got %lld", who, (long long)kLargeMaxRows, (long long)n_rows);
        return BYZ_E_UNSUPPORTED;
    }
    return BYZ_OK;
}

// What a *_host entry point does around its _dev call, on the null stream: the host matrix goes to ctx->stage_in, the vectors
// and lists the call reads or writes are carved out of ctx->stage_out (Carve: the first one at its base, each 16-byte aligned).
// Declare the arrays, stage(), run the _dev call on G() and stream(), end with finish() or finish_sync().  Nothing is allocated
// or copied before stage(), so every argument check of the wrapper runs first.
class HostStage {
  public:
    explicit HostStage(byz_ctx* ctx) : ctx_(ctx) {}
    // an optional output: carved, and copied to `host` by the ending, when host != nullptr; *dev = nullptr otherwise
    template <typename T>
    void out(T** dev, T* host, int64_t count) {
        if (host != nullptr) inout<T>(dev, nullptr, host, count);
        else *dev = nullptr;
    }
    // an optional input: carved, and uploaded by stage(), when host != nullptr; *dev = nullptr otherwise
    template <typename T>
    void in(T** dev, const T* host, int64_t count) {
        if (host != nullptr) inout<T>(dev, host, nullptr, count);
        else *dev = nullptr;
    }
    // always carved; uploaded from `from` and downloaded to `to` where they are not null: a start vector the call runs in place
    // on, an output the device call writes whether or not the caller asked for it
    template <typename T>
    void inout(T** dev, const T* from, T* to, int64_t count) {
        const int slot = carve_.slots();
        carve_.take(dev, count);
        if (carve_.slots() > slot) copies_[slot] = {from, to, static_cast<size_t>(count) * sizeof(T)};   // (a refused take fails stage())
    }
    // sizes stage_in and stage_out, binds every array, queues the matrix's upload and the inputs'
    int stage(const float* G_host, int64_t n_rows, int64_t n_cols) {
        const size_t bytes = static_cast<size_t>(n_rows) * n_cols * sizeof(float);
        BYZ_TRY(ctx_->stage_in.ensure(bytes));
        BYZ_TRY(carve_.commit(ctx_->stage_out));
        BYZ_HIP(hipMemcpyAsync(ctx_->stage_in.ptr, G_host, bytes, hipMemcpyHostToDevice, stream()));
        for (int i = 0; i < carve_.slots(); ++i)
            if (copies_[i].from != nullptr)
                BYZ_HIP(hipMemcpyAsync(at(i), copies_[i].from, copies_[i].bytes, hipMemcpyHostToDevice, stream()));
        return BYZ_OK;
    }
    float* G() const { return ctx_->stage_in.as<float>(); }
    hipStream_t stream() const { return nullptr; }
    // the two endings.  finish: the downloads queued, then the device scalars read back and the status word checked (`all`: the
    // whole block, for a wrapper that reports a field of it; the core alone otherwise)
    int finish(DeviceScalars* all = nullptr) {
        BYZ_TRY(download());
        return all != nullptr ? read_scalars(ctx_, all, sizeof *all, stream()) : check_core(ctx_, stream());
    }
    // finish_sync: the downloads queued, then the stream synchronised and nothing else
    int finish_sync() {
        BYZ_TRY(download());
        BYZ_HIP(hipStreamSynchronize(stream()));
        return BYZ_OK;
    }

  private:
    struct Copy { const void* from; void* to; size_t bytes; };
    char* at(int slot) const { return static_cast<char*>(ctx_->stage_out.ptr) + carve_.offset(slot); }   // as commit() bound it
    int download() {
        for (int i = 0; i < carve_.slots(); ++i)
            if (copies_[i].to != nullptr)
                BYZ_HIP(hipMemcpyAsync(copies_[i].to, at(i), copies_[i].bytes, hipMemcpyDeviceToHost, stream()));
        return BYZ_OK;
    }
    byz_ctx* ctx_;
    Carve carve_;
    Copy copies_[Carve::kMaxSlots];
};

int krum_select(byz_ctx* ctx, const float* dist, int64_t n, int64_t users_count, int64_t corrupted,
                int32_t* winner_dev, hipStream_t stream) {
    const int64_t prefix = python_prefix_len(n - 1, users_count - corrupted);
    if (krum_small_applies(n, 1))
        return launch_small_select(ctx, dist, n, prefix, nullptr, 0, 0, winner_dev, nullptr, stream);
    BYZ_TRY(launch_row_sort(ctx, dist, n, prefix, 0, false, stream));
    BYZ_TRY(launch_krum_argmin(ctx, n, winner_dev, stream));
    return BYZ_OK;
}

// krum_winner_dev != nullptr: the same row sort also forms the Krum scores of defences.py:33-34 (prefix users_count - corrupted
// of the full rows) and the Krum index goes to krum_winner_dev: configs[4]'s round runs Krum and Bulyan on ONE distance matrix,
// and a second sort of its 10,000 rows costs 7 ms
int bulyan_select(byz_ctx* ctx, const float* dist, int64_t n, int64_t users_count, int64_t corrupted,
                  int32_t* selection_dev, hipStream_t stream, int32_t* krum_winner_dev = nullptr) {
    const int64_t theta = users_count - 2 * corrupted;
    if (theta < 0 || theta > n) {
        set_error("bulyan: selection size %lld does not fit %lld rows", (long long)theta, (long long)n);
        return BYZ_E_INVALID;
    }
    // every pick scores a row by its (n_t - f) smallest of (n_t - 1) live distances (defences.py:26,34 with
    // users_count - len(selection_set) passed down from defences.py:61): the number of dropped, largest
    // entries is the same at every step
    int64_t drop = (n - 1) - users_count + corrupted;
    if (drop < 0) drop = 0;
    if (drop > n - 1) drop = n - 1;
    const int64_t krum_prefix = krum_winner_dev != nullptr ? python_prefix_len(n - 1, users_count - corrupted) : 0;
    BYZ_TRY(launch_row_sort(ctx, dist, n, krum_prefix, drop, true, stream));
    if (krum_winner_dev != nullptr) BYZ_TRY(launch_krum_argmin(ctx, n, krum_winner_dev, stream));
    BYZ_TRY(launch_bulyan_loop(ctx, dist, n, theta, drop, users_count, corrupted, selection_dev, &device_scalars(ctx)->core.bulyan, stream));
    CoreScalars core;
    BYZ_TRY(read_core(ctx, &core, stream));
    const int32_t status = core.bulyan.status;
    ctx->bulyan_rescored = core.bulyan.rescored;
    if (status == 2) {
        set_error("bulyan: the selection loop's workgroups lost contact with each other (exchange timed out)");
        return BYZ_E_HIP;
    }
    if (status != 0) {
        set_error("bulyan: no row scored below 1e20 (the reference raises KeyError(-1) here)");
        return BYZ_E_NO_WINNER;
    }
    return BYZ_OK;
}

// Multi-Krum (Blanchard et al. 2017, section 4): the Krum score of every row (krum_select: defences.py:33-34, prefix users_count -
// corrupted_count), rows ranked by (score, visit position), the first m taken.  selection_dev (optional): the m rows in ranking
// order; ctx->multi_krum_rows: the same rows ascending, the list the row-list mean walks.
int check_multi_krum_m(int64_t n, int64_t m) {
    if (m < 1 || m > n) {
        set_error("multi_krum: m = %lld outside 1..%lld (the row count)", (long long)m, (long long)n);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

int multi_krum_select(byz_ctx* ctx, const float* dist, int64_t n, int64_t users_count, int64_t corrupted, int64_t m,
                      int32_t* selection_dev, hipStream_t stream) {
    BYZ_TRY(check_multi_krum_m(n, m));
    if (n > kLargeMaxRows) {
        set_error("selection kernels support at most %lld rows, got %lld", (long long)kLargeMaxRows, (long long)n);
        return BYZ_E_UNSUPPORTED;
    }
    BYZ_TRY(ctx->multi_krum_rows.ensure(static_cast<size_t>(n) * sizeof(int32_t)));
    BYZ_TRY(krum_select(ctx, dist, n, users_count, corrupted, krum_winner_word(ctx), stream));
    return launch_multi_krum_rank(ctx, n, m, selection_dev, ctx->multi_krum_rows.as<int32_t>(), stream);
}

// ---- multi-GPU, columns layout: the one exchange of the path through the host's all-reduce -------------------
int reduce_over_ranks(byz_allreduce_f64_fn allreduce, void* user, double* buf, int64_t count, void* stream, const char* what) {
    const int rc = allreduce(user, buf, count, stream);
    if (rc != 0) {
        set_error("%s: the caller's all-reduce returned %d", what, rc);
        return BYZ_E_COLLECTIVE;
    }
    return BYZ_OK;
}

// dist (n x n) from the column slices of all ranks: Gram of the local slice -> all-reduce -> distances -> the near-duplicate
// pairs of the all-reduced Gram re-evaluated on the difference (per-rank sums over the local columns -> all-reduce -> apply).
// The sequence of sharded.py's global_distances + engine.distances_from_gram, in one call.
int sharded_distances(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, byz_allreduce_f64_fn allreduce,
                      void* user, float* dist, void* stream) {
    hipStream_t s = as_stream(stream);
    BYZ_TRY(ctx->gram.ensure(static_cast<size_t>(n_rows) * n_rows * sizeof(double)));
    double* gram = ctx->gram.as<double>();
    BYZ_TRY(launch_gram(ctx, G, n_rows, n_cols, ld, gram, s));
    // rows that are identical in THIS slice need not be identical in the others: what launch_gram's duplicate search proved
    // holds for the local columns only, and the all-reduced Gram is an external one as far as the distances are concerned
    ctx->row_map_rows = 0;
    BYZ_TRY(reduce_over_ranks(allreduce, user, gram, n_rows * n_rows, stream, "sharded distances (Gram)"));
    BYZ_TRY(launch_distances_from_gram(ctx, gram, n_rows, dist, s, nullptr, 0, 0));
    int64_t count = 0;
    BYZ_TRY(near_pair_count(ctx, &count, s));   // (the same all-reduced Gram on every rank: the same count, the same list)
    if (count > 0) {
        double* sq = ctx->near_sq.as<double>();
        BYZ_TRY(launch_near_pair_sqdist(ctx, G, n_cols, ld, nullptr, sq, s));
        BYZ_TRY(reduce_over_ranks(allreduce, user, sq, count, stream, "sharded distances (near pairs)"));
        BYZ_TRY(launch_near_pair_apply(ctx, sq, n_rows, dist, s));
    }
    return BYZ_OK;
}

// ---- one composition per defence; allreduce == nullptr: one GPU holds every column ---------------------------------------------
// dist (n x n) of G's rows: over the ranks' column slices when an all-reduce is given, by the small-N kernel where it applies
// (no Gram, no duplicate search: the row map describes nothing afterwards), else the Gram and the distances from it.
int distances(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, byz_allreduce_f64_fn allreduce, void* user,
              float* dist, void* stream) {
    if (allreduce != nullptr) return sharded_distances(ctx, G, n_rows, n_cols, ld, allreduce, user, dist, stream);
    hipStream_t s = as_stream(stream);
    if (krum_small_applies(n_rows, n_cols)) {
        ctx->row_map_rows = 0;
        return launch_small_distances(ctx, G, n_rows, n_cols, ld, dist, s);
    }
    BYZ_TRY(ctx->gram.ensure(static_cast<size_t>(n_rows) * n_rows * sizeof(double)));
    BYZ_TRY(launch_gram(ctx, G, n_rows, n_cols, ld, ctx->gram.as<double>(), s));
    return launch_distances_from_gram(ctx, ctx->gram.as<double>(), n_rows, dist, s, G, n_cols, ld);
}

int krum(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count, int64_t corrupted_count,
         byz_allreduce_f64_fn allreduce, void* user, float* out_row, int32_t* index_host, void* stream) {
    hipStream_t s = as_stream(stream);
    BYZ_TRY(ensure_distance_workspaces(ctx, n_rows));
    float* dist = ctx->dist.as<float>();
    int32_t* winner = krum_winner_word(ctx);
    if (allreduce == nullptr && krum_small_applies(n_rows, n_cols)) {
        // the reference's own sizes: two launches (krum_small.hip), the row copy is part of the second
        ctx->row_map_rows = 0;
        const int64_t prefix = python_prefix_len(n_rows - 1, users_count - corrupted_count);
        if (ctx->num_cus >= n_rows) {
            BYZ_TRY(launch_small_krum(ctx, G, n_rows, n_cols, ld, dist, prefix, winner, out_row, s));
        } else {
            // the two-launch form has every row's workgroup wait for all the others' scores: they must all be resident at once
            // (one workgroup per CU).  On a device or partition with fewer CUs than rows (a CPX partition has 32) the first wave
            // of workgroups would spin to the limit and the call fail with the status word set: take the
            // four-launch form, which has no wait across workgroups.
            BYZ_TRY(launch_small_distances(ctx, G, n_rows, n_cols, ld, dist, s));
            BYZ_TRY(launch_small_select(ctx, dist, n_rows, prefix, G, n_cols, ld, winner, out_row, s));
        }
    } else {
        BYZ_TRY(distances(ctx, G, n_rows, n_cols, ld, allreduce, user, dist, stream));
        BYZ_TRY(krum_select(ctx, dist, n_rows, users_count, corrupted_count, winner, s));
        if (out_row) BYZ_TRY(launch_copy_row(ctx, G, ld, n_rows, n_cols, winner, out_row, s));
    }
    return read_winner(ctx, index_host, s);
}

int bulyan(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count, int64_t corrupted_count,
           byz_allreduce_f64_fn allreduce, void* user, float* out, int32_t* selection_out, void* stream) {
    hipStream_t s = as_stream(stream);
    const int64_t theta = users_count - 2 * corrupted_count;
    BYZ_TRY(ensure_distance_workspaces(ctx, n_rows));
    BYZ_TRY(ctx->selection.ensure(static_cast<size_t>(n_rows) * sizeof(int32_t)));
    BYZ_TRY(distances(ctx, G, n_rows, n_cols, ld, allreduce, user, ctx->dist.as<float>(), stream));
    int32_t* sel = ctx->selection.as<int32_t>();
    BYZ_TRY(bulyan_select(ctx, ctx->dist.as<float>(), n_rows, users_count, corrupted_count, sel, s));
    if (selection_out)
        BYZ_HIP(hipMemcpyAsync(selection_out, sel, static_cast<size_t>(theta) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    // defences.py:70: trimmed_mean(np.array(selection_set), len(selection_set), 2*corrupted_count); sharded: on the local columns
    // of the selected rows
    const int64_t keep = python_prefix_len(theta, theta - 2 * corrupted_count - 1);
    return launch_trimmed_mean(ctx, G, theta, n_cols, ld, sel, keep, out, s);
}

int multi_krum(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
               int64_t corrupted_count, int64_t m, byz_allreduce_f64_fn allreduce, void* user, float* out, int32_t* selection,
               void* stream) {
    hipStream_t s = as_stream(stream);
    BYZ_TRY(ensure_distance_workspaces(ctx, n_rows));
    BYZ_TRY(distances(ctx, G, n_rows, n_cols, ld, allreduce, user, ctx->dist.as<float>(), stream));
    BYZ_TRY(multi_krum_select(ctx, ctx->dist.as<float>(), n_rows, users_count, corrupted_count, m, selection, s));
    // sharded: the selection is the same on every rank (one all-reduced Gram); each rank averages its own columns of the selected rows
    return launch_column_mean_rows(ctx, G, ctx->multi_krum_rows.as<int32_t>(), m, n_cols, ld, out, s);
}

int gram_share(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index, int share_count,
               int share_index, double* gram, bool accumulate, void* stream) {
    BYZ_TRY(enter(ctx));
    // with row_index the logical matrix has n_rows rows taken from anywhere in G: only the pointer and ld are checkable
    BYZ_REQUIRE(G && n_rows > 0 && n_cols > 0 && ld >= n_cols, "%s: bad matrix", accumulate ? "gram_share_add" : "gram_share");
    return launch_gram_share(ctx, G, n_rows, n_cols, ld, row_index, share_count, share_index, gram, as_stream(stream), accumulate);
}

}  // namespace
}  // namespace byz

using namespace byz;

extern "C" {

int byz_abi_version(void) { return BYZ_ABI_VERSION; }
const char* byz_last_error(void) { return g_error; }

int byz_ctx_create(int device, byz_ctx** out) {
    if (!out) {
        set_error("byz_ctx_create: null output");
        return BYZ_E_INVALID;
    }
    *out = nullptr;
    int count = 0;
    BYZ_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) {
        set_error("byz_ctx_create: device %d not present (%d visible)", device, count);
        return BYZ_E_INVALID;
    }
    BYZ_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    BYZ_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("libbyzagg is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
        return BYZ_E_UNSUPPORTED;
    }
    byz_ctx* ctx = new byz_ctx();
    ctx->device = device;
    ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (ctx->scalars.ensure(sizeof(DeviceScalars)) != BYZ_OK || hipMemset(ctx->scalars.ptr, 0, sizeof(DeviceScalars)) != hipSuccess) {
        delete ctx;   // (frees what was allocated)
        set_error("byz_ctx_create: cannot allocate the device scalars");
        return BYZ_E_HIP;
    }
    *out = ctx;
    return BYZ_OK;
}

void byz_ctx_destroy(byz_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    byz_timing_reset(ctx);
    if (ctx->assemble_copied != nullptr) (void)hipEventDestroy(ctx->assemble_copied);
    delete ctx;   // every workspace frees itself (common.hpp: Buffer)
}

int byz_ctx_device(const byz_ctx* ctx) { return ctx ? ctx->device : -1; }

int byz_limits(int64_t* max_rows_select, int64_t* max_rows_trimmed) {
    if (max_rows_select) *max_rows_select = select_max_rows();
    if (max_rows_trimmed) *max_rows_trimmed = trimmed_mean_max_rows();
    return BYZ_OK;
}

int byz_ctx_reserve(byz_ctx* ctx, int64_t n_rows, int64_t n_cols) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(n_rows > 0 && n_cols > 0, "byz_ctx_reserve: bad shape");
    BYZ_TRY(ensure_distance_workspaces(ctx, n_rows));
    BYZ_TRY(ctx->scores.ensure(static_cast<size_t>(n_rows) * sizeof(float)));
    BYZ_TRY(ctx->selection.ensure(static_cast<size_t>(n_rows) * sizeof(int32_t)));
    if (!select_large_applies(n_rows)) {   // (beyond 16,384 rows the selection grows its own tables: large_rows.hip)
        BYZ_TRY(ctx->sorted_idx.ensure(static_cast<size_t>(n_rows) * n_rows * sizeof(uint16_t)));
        BYZ_TRY(ctx->rank_t.ensure(static_cast<size_t>(n_rows) * n_rows * sizeof(uint16_t)));
        BYZ_TRY(ctx->rank_rows.ensure(static_cast<size_t>(n_rows) * n_rows * sizeof(uint16_t)));
    }
    BYZ_TRY(ctx->row_total.ensure(static_cast<size_t>(n_rows) * sizeof(double)));
    BYZ_TRY(ctx->row_top.ensure(static_cast<size_t>(2 * n_rows) * sizeof(double)));
    BYZ_TRY(ctx->stage_out.ensure(static_cast<size_t>(n_cols) * 3 * sizeof(float)));
    BYZ_TRY(ctx->pinned.ensure(static_cast<size_t>(n_rows) * sizeof(int32_t) + 64));
    if (krum_small_applies(n_rows, n_cols)) BYZ_TRY(reserve_small_workspaces(ctx));
    {   // the Gram's schedule words and the duplicate-row table
        const int64_t T = ceil_div(n_rows, 128);
        BYZ_TRY(ctx->gram_tickets.ensure(static_cast<size_t>(T * (T + 1) / 2 + 8) * sizeof(int32_t)));
        BYZ_TRY(ctx->dup_rep.ensure(static_cast<size_t>(n_rows + 1) * sizeof(int32_t)));
    }
    return BYZ_OK;
}

// ---- raw memory ----------------------------------------------------------------------------------
int byz_malloc(byz_ctx* ctx, int64_t bytes, void** dev_ptr) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dev_ptr && bytes > 0, "byz_malloc: bad arguments");
    BYZ_HIP(hipMalloc(dev_ptr, static_cast<size_t>(bytes)));
    return BYZ_OK;
}
int byz_free(byz_ctx* ctx, void* dev_ptr) {
    BYZ_TRY(enter(ctx));
    if (dev_ptr) BYZ_HIP(hipFree(dev_ptr));
    return BYZ_OK;
}
int byz_upload(byz_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dst_dev && src_host && bytes >= 0, "byz_upload: bad arguments");
    BYZ_HIP(hipMemcpyAsync(dst_dev, src_host, static_cast<size_t>(bytes), hipMemcpyHostToDevice, as_stream(stream)));
    return BYZ_OK;
}
int byz_download(byz_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dst_host && src_dev && bytes >= 0, "byz_download: bad arguments");
    BYZ_HIP(hipMemcpyAsync(dst_host, src_dev, static_cast<size_t>(bytes), hipMemcpyDeviceToHost, as_stream(stream)));
    BYZ_HIP(hipStreamSynchronize(as_stream(stream)));
    return BYZ_OK;
}
int byz_upload_2d(byz_ctx* ctx, void* dst_dev, int64_t dst_pitch_bytes, const void* src_host,
                  int64_t src_pitch_bytes, int64_t width_bytes, int64_t rows, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dst_dev && src_host && rows >= 0 && width_bytes >= 0, "byz_upload_2d: bad arguments");
    BYZ_HIP(hipMemcpy2DAsync(dst_dev, static_cast<size_t>(dst_pitch_bytes), src_host,
                             static_cast<size_t>(src_pitch_bytes), static_cast<size_t>(width_bytes),
                             static_cast<size_t>(rows), hipMemcpyHostToDevice, as_stream(stream)));
    return BYZ_OK;
}
int byz_stream_sync(byz_ctx* ctx, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_HIP(hipStreamSynchronize(as_stream(stream)));
    return BYZ_OK;
}

// ---- device entry points -------------------------------------------------------------------------
int byz_no_defense_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, float* out,
                       void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "no_defense"));
    return launch_column_mean(ctx, G, n_rows, n_cols, ld, out, as_stream(stream));
}

int byz_gram_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, double* gram,
                 void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "gram"));
    return launch_gram(ctx, G, n_rows, n_cols, ld, gram, as_stream(stream));
}

int byz_gram_share_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                       const int32_t* row_index, int share_count, int share_index, double* gram, void* stream) {
    return gram_share(ctx, G, n_rows, n_cols, ld, row_index, share_count, share_index, gram, false, stream);
}

int byz_gram_share_add_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                           const int32_t* row_index, int share_count, int share_index, double* gram, void* stream) {
    return gram_share(ctx, G, n_rows, n_cols, ld, row_index, share_count, share_index, gram, true, stream);
}

int byz_distances_from_gram_dev(byz_ctx* ctx, const double* gram, int64_t n_rows, float* dist, void* stream) {
    BYZ_TRY(enter(ctx));
    ctx->row_map_rows = 0;   // an external Gram: nothing is known about its rows
    return launch_distances_from_gram(ctx, gram, n_rows, dist, as_stream(stream), nullptr, 0, 0);
}

int byz_near_pairs_count(byz_ctx* ctx, int64_t* count_host, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(count_host, "near_pairs_count: null output");
    return near_pair_count(ctx, count_host, as_stream(stream));
}

int byz_near_pairs_sqdist_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                              const int32_t* row_index, double* sq_dev, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "near_pairs_sqdist"));
    BYZ_REQUIRE(sq_dev && ctx->near_pair_capacity > 0, "near_pairs_sqdist: no pair list (call byz_distances_from_gram_dev first)");
    return launch_near_pair_sqdist(ctx, G, n_cols, ld, row_index, sq_dev, as_stream(stream));
}

int byz_near_pairs_apply_dev(byz_ctx* ctx, const double* sq_dev, int64_t n_rows, float* dist, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(sq_dev && dist && n_rows > 0 && ctx->near_pair_capacity > 0, "near_pairs_apply: bad arguments");
    return launch_near_pair_apply(ctx, sq_dev, n_rows, dist, as_stream(stream));
}

int byz_ctx_check(byz_ctx* ctx, void* stream) {
    BYZ_TRY(enter(ctx));
    return check_core(ctx, as_stream(stream));
}

int byz_bulyan_rescored(const byz_ctx* ctx, int64_t* rows_host) {
    if (!ctx || !rows_host) {
        set_error("bulyan_rescored: null argument");
        return BYZ_E_INVALID;
    }
    *rows_host = ctx->bulyan_rescored;
    return BYZ_OK;
}

int byz_pairwise_distances_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                               float* dist, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "pairwise_distances"));
    BYZ_REQUIRE(dist, "pairwise_distances: null output");
    return distances(ctx, G, n_rows, n_cols, ld, nullptr, nullptr, dist, stream);
}

int byz_krum_select_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int64_t users_count,
                        int64_t corrupted_count, int32_t* index_host, float* scores_dev, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist && n_rows > 0, "krum_select: bad arguments");
    hipStream_t s = as_stream(stream);
    BYZ_TRY(krum_select(ctx, dist, n_rows, users_count, corrupted_count, krum_winner_word(ctx), s));
    if (scores_dev)
        BYZ_HIP(hipMemcpyAsync(scores_dev, ctx->scores.ptr, static_cast<size_t>(n_rows) * sizeof(float),
                               hipMemcpyDeviceToDevice, s));
    return read_winner(ctx, index_host, s);
}

int byz_krum_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
                 int64_t corrupted_count, int check_assert, float* out_row, int32_t* index_host, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "krum"));
    BYZ_TRY(check_krum_assert(check_assert, users_count, corrupted_count));
    return krum(ctx, G, n_rows, n_cols, ld, users_count, corrupted_count, nullptr, nullptr, out_row, index_host, stream);
}

int byz_trimmed_mean_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                         const int32_t* row_index, int64_t corrupted_count, float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "trimmed_mean"));
    // defences.py:45: number_to_consider = int(rows - corrupted) - 1, then a Python slice [:k]
    const int64_t keep = python_prefix_len(n_rows, n_rows - corrupted_count - 1);
    return launch_trimmed_mean(ctx, G, n_rows, n_cols, ld, row_index, keep, out, as_stream(stream));
}

int byz_coordinate_median_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                              float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    return launch_rank_select(ctx, G, n_rows, n_cols, ld, row_index, 0, true, out, as_stream(stream));
}

int byz_rank_trimmed_mean_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                              int64_t trim_count, float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    return launch_rank_select(ctx, G, n_rows, n_cols, ld, row_index, trim_count, false, out, as_stream(stream));
}

int byz_window_mean_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                        const float* centre, int64_t keep, float* out, float* radius, void* stream) {
    BYZ_TRY(enter(ctx));
    return launch_centre_window(ctx, G, n_rows, n_cols, ld, row_index, centre, keep, out, radius, as_stream(stream));
}

// Phocas: the window of n - b values around the bits byz_rank_trimmed_mean_dev returns.  Everything is checked before the first
// launch; the centre goes to the caller's vector when there is one, else to the workspace.
int byz_phocas_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                   int64_t trim_count, float* out, float* centre_out, float* radius, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "phocas"));
    BYZ_REQUIRE(out, "phocas: null output");
    BYZ_TRY(check_row_ceiling("phocas", n_rows));
    BYZ_REQUIRE(trim_count >= 0 && 2 * trim_count < n_rows, "phocas: trim_count %lld must satisfy 0 <= 2 b < %lld rows",
                (long long)trim_count, (long long)n_rows);
    float* centre = centre_out;
    if (centre == nullptr) {
        Carve c;
        c.take(&centre, n_cols);
        BYZ_TRY(c.commit(ctx->phocas));
    }
    hipStream_t s = as_stream(stream);
    BYZ_TRY(launch_rank_select(ctx, G, n_rows, n_cols, ld, row_index, trim_count, false, centre, s));
    return launch_centre_window(ctx, G, n_rows, n_cols, ld, row_index, centre, n_rows - trim_count, out, radius, s);
}

int byz_trimmed_mean_redone(byz_ctx* ctx, int64_t* tiles_host, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(tiles_host, "trimmed_mean_redone: null output");
    *tiles_host = 0;
    if (ctx->redo_tiles.ptr == nullptr || !ctx->redo_valid) return BYZ_OK;
    int32_t count = 0;
    BYZ_TRY(read_i32(ctx, ctx->redo_tiles.as<int32_t>(), &count, 1, as_stream(stream)));
    *tiles_host = count;
    return BYZ_OK;
}

int byz_bulyan_select_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int64_t users_count,
                          int64_t corrupted_count, int32_t* selection, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist && selection && n_rows > 0, "bulyan_select: bad arguments");
    return bulyan_select(ctx, dist, n_rows, users_count, corrupted_count, selection, as_stream(stream));
}

int byz_krum_bulyan_select_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int64_t users_count,
                               int64_t corrupted_count, int32_t* krum_index_host, int32_t* selection, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist && selection && krum_index_host && n_rows > 0, "krum_bulyan_select: bad arguments");
    hipStream_t s = as_stream(stream);
    BYZ_TRY(bulyan_select(ctx, dist, n_rows, users_count, corrupted_count, selection, s, krum_winner_word(ctx)));
    return read_winner(ctx, krum_index_host, s);
}

int byz_bulyan_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
                   int64_t corrupted_count, float* out, int32_t* selection_out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "bulyan"));
    BYZ_REQUIRE(out, "bulyan: null output");
    BYZ_TRY(check_bulyan_precondition(users_count, corrupted_count));
    return bulyan(ctx, G, n_rows, n_cols, ld, users_count, corrupted_count, nullptr, nullptr, out, selection_out, stream);
}

// ---- Multi-Krum (Blanchard et al. 2017, section 4; beyond the reference) -----------------------------------------------------
int byz_mean_rows_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                      int64_t count, float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "mean_rows"));
    BYZ_REQUIRE(row_index && out && count >= 1, "mean_rows: null row list or output, or count %lld < 1", (long long)count);
    return launch_column_mean_rows(ctx, G, row_index, count, n_cols, ld, out, as_stream(stream));
}

int byz_multi_krum_select_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int64_t users_count, int64_t corrupted_count,
                              int64_t m, int32_t* selection, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist && selection && n_rows > 0, "multi_krum_select: bad arguments");
    return multi_krum_select(ctx, dist, n_rows, users_count, corrupted_count, m, selection, as_stream(stream));
}

int byz_multi_krum_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
                       int64_t corrupted_count, int64_t m, int check_assert, float* out, int32_t* selection, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "multi_krum"));
    BYZ_REQUIRE(out, "multi_krum: null output");
    BYZ_TRY(check_krum_assert(check_assert, users_count, corrupted_count));
    BYZ_TRY(check_multi_krum_m(n_rows, m));
    return multi_krum(ctx, G, n_rows, n_cols, ld, users_count, corrupted_count, m, nullptr, nullptr, out, selection, stream);
}

// ---- multi-GPU, columns layout: the same compositions over the ranks' column slices ------------------------------------------
int byz_pairwise_distances_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                                       byz_allreduce_f64_fn allreduce, void* user, float* dist, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "pairwise_distances_sharded"));
    BYZ_REQUIRE(dist && allreduce, "pairwise_distances_sharded: null output or null all-reduce");
    return sharded_distances(ctx, G, n_rows, n_cols, ld, allreduce, user, dist, stream);
}

int byz_krum_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
                         int64_t corrupted_count, int check_assert, byz_allreduce_f64_fn allreduce, void* user, float* out_row,
                         int32_t* index_host, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "krum_sharded"));
    BYZ_REQUIRE(allreduce, "krum_sharded: null all-reduce");
    BYZ_TRY(check_krum_assert(check_assert, users_count, corrupted_count));
    return krum(ctx, G, n_rows, n_cols, ld, users_count, corrupted_count, allreduce, user, out_row, index_host, stream);
}

int byz_bulyan_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
                           int64_t corrupted_count, byz_allreduce_f64_fn allreduce, void* user, float* out,
                           int32_t* selection_out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "bulyan_sharded"));
    BYZ_REQUIRE(out && allreduce, "bulyan_sharded: null output or null all-reduce");
    BYZ_TRY(check_bulyan_precondition(users_count, corrupted_count));
    return bulyan(ctx, G, n_rows, n_cols, ld, users_count, corrupted_count, allreduce, user, out, selection_out, stream);
}

int byz_multi_krum_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
                               int64_t corrupted_count, int64_t m, int check_assert, byz_allreduce_f64_fn allreduce, void* user,
                               float* out, int32_t* selection, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "multi_krum_sharded"));
    BYZ_REQUIRE(out && allreduce, "multi_krum_sharded: null output or null all-reduce");
    BYZ_TRY(check_krum_assert(check_assert, users_count, corrupted_count));
    BYZ_TRY(check_multi_krum_m(n_rows, m));
    return multi_krum(ctx, G, n_rows, n_cols, ld, users_count, corrupted_count, m, allreduce, user, out, selection, stream);
}

// ---- geometric median (smoothed Weiszfeld; RFA, Pillutla et al.; beyond the reference) ------------------------------------
namespace {

int check_geomed(const byz_geomed_params* params, int64_t n_rows, const char* who) {
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    // (written so that a NaN fails every test)
    if (!(params->nu > 0.0) || params->max_iter < 0 || !(params->ftol >= 0.0)) {
        set_error("%s: nu = %g must be > 0, max_iter = %lld >= 0, ftol = %g >= 0", who, params->nu, (long long)params->max_iter,
                  params->ftol);
        return BYZ_E_INVALID;
    }
    BYZ_TRY(check_row_ceiling(who, n_rows));
    // every update's launches are enqueued up front, stop or no stop: the cap bounds what a call can queue
    if (params->max_iter > BYZ_GEOMED_MAX_ITER) {
        set_error("%s: max_iter = %lld beyond %d (every update's launches are enqueued whatever the stop)", who,
                  (long long)params->max_iter, BYZ_GEOMED_MAX_ITER);
        return BYZ_E_UNSUPPORTED;
    }
    return BYZ_OK;
}

// What the row-distance loops (the geometric median, centered clipping, FLTrust, byz_row_sqdist_dev, byz_row_dots_dev) keep in
// ctx->rows.  planes = 2 is FLTrust's: two sums a row.
struct RowScratch {
    double* partials;   // planes x chunks x n: the (row, column chunk) partials of rowsq
    double* a;          // planes * n + 1: the squared distances (the geometric median's fallback flag behind the rows); FLTrust:
                        // p (n), q (n), q0 (1), one all-reduce's worth
    double* b;          // planes * n: the weights, or the scales; FLTrust: ts (n), w (n)
    double* root;       // planes = 2 only, 64: the chunk partials of the root's squared norm
};

// sized by the chunks geomed_chunks picks for this shape: at most 64 per row and plane, about num_cus * 256 + n in all
int row_scratch(byz_ctx* ctx, int64_t n, int64_t n_cols, RowScratch* out, int planes = 1) {
    int64_t chunk_cols = 0;
    const int64_t chunks = geomed_chunks(ctx, n, n_cols, &chunk_cols);
    Carve c;
    c.take(&out->partials, chunks * n * planes);
    c.take(&out->a, planes * n + 1);
    c.take(&out->b, planes * n);
    c.take(&out->root, planes == 2 ? geomed_chunks(ctx, 1, n_cols, &chunk_cols) : 0);
    return c.commit(ctx->rows);
}

// The whole call; allreduce == nullptr: one GPU holds every column.  Nothing here waits for the device.
int geometric_median(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, const byz_geomed_params* params,
                     byz_allreduce_f64_fn allreduce, void* user, float* out, double* weights, void* stream) {
    hipStream_t s = as_stream(stream);
    RowScratch t;
    BYZ_TRY(row_scratch(ctx, n, n_cols, &t));
    double *sq = t.a, *w = t.b;
    GeomedReport* report = &device_scalars(ctx)->geomed;
    const int32_t* done = &report->done;
    const int32_t* fallback = &report->fallback;
    BYZ_HIP(hipMemsetAsync(report, 0, sizeof *report, s));
    mark(ctx, kReportGeomed, s);
    // mean0: no_defense's kernel, then its finiteness; the fallback's launches return at once when it is finite
    BYZ_TRY(launch_column_mean(ctx, G, n, n_cols, ld, out, s));
    if (allreduce == nullptr) {
        BYZ_TRY(launch_geomed_finite_check(ctx, out, n_cols, nullptr, s));
        BYZ_TRY(launch_row_sqdist(ctx, G, n, n_cols, ld, nullptr, t.partials, sq, nullptr, fallback, s));
        BYZ_TRY(launch_geomed_fallback(ctx, sq, n, w, nullptr, s));
    } else {
        // a rank whose own columns are finite adds 0 to every row's squared norm (finite: the sum's finiteness is the
        // others'); the flag rides behind the rows, so that the decision is taken on all-reduced data on every rank
        BYZ_HIP(hipMemsetAsync(sq, 0, static_cast<size_t>(n + 1) * sizeof(double), s));
        BYZ_TRY(launch_geomed_finite_check(ctx, out, n_cols, sq + n, s));
        BYZ_TRY(launch_row_sqdist(ctx, G, n, n_cols, ld, nullptr, t.partials, sq, nullptr, fallback, s));
        BYZ_TRY(reduce_over_ranks(allreduce, user, sq, n + 1, stream, "geometric median (finiteness)"));
        BYZ_TRY(launch_geomed_fallback(ctx, sq, n, w, sq + n, s));
    }
    BYZ_TRY(launch_weighted_mean(ctx, G, n, n_cols, ld, w, out, nullptr, fallback, s));
    // the objective at the start, then the updates
    for (int64_t k = 0; k <= params->max_iter; ++k) {
        if (k > 0) BYZ_TRY(launch_weighted_mean(ctx, G, n, n_cols, ld, w, out, done, nullptr, s));
        BYZ_TRY(launch_row_sqdist(ctx, G, n, n_cols, ld, out, t.partials, sq, done, nullptr, s));
        if (allreduce != nullptr) BYZ_TRY(reduce_over_ranks(allreduce, user, sq, n, stream, "geometric median (distances)"));
        BYZ_TRY(launch_geomed_step(ctx, sq, n, w, params->nu, params->ftol, k, params->max_iter, s));
    }
    if (weights != nullptr) BYZ_TRY(launch_geomed_weights(ctx, w, n, weights, s));
    return BYZ_OK;
}

}  // namespace

int byz_row_sqdist_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* z, double* sq,
                       void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "row_sqdist"));
    BYZ_REQUIRE(z && sq, "row_sqdist: null vector or output");
    BYZ_TRY(check_row_ceiling("row_sqdist", n_rows));
    RowScratch t;
    BYZ_TRY(row_scratch(ctx, n_rows, n_cols, &t));
    return launch_row_sqdist(ctx, G, n_rows, n_cols, ld, z, t.partials, sq, nullptr, nullptr, as_stream(stream));
}

int byz_weighted_mean_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const double* w, float* out,
                          void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "weighted_mean"));
    BYZ_REQUIRE(w && out, "weighted_mean: null weights or output");
    BYZ_TRY(check_row_ceiling("weighted_mean", n_rows));
    return launch_weighted_mean(ctx, G, n_rows, n_cols, ld, w, out, nullptr, nullptr, as_stream(stream));
}

int byz_geometric_median_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                             const byz_geomed_params* params, float* out, double* weights, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "geometric_median"));
    BYZ_REQUIRE(out, "geometric_median: null output");
    BYZ_TRY(check_geomed(params, n_rows, "geometric_median"));
    return geometric_median(ctx, G, n_rows, n_cols, ld, params, nullptr, nullptr, out, weights, stream);
}

int byz_geometric_median_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                                     const byz_geomed_params* params, byz_allreduce_f64_fn allreduce, void* user, float* out,
                                     double* weights, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "geometric_median_sharded"));
    BYZ_REQUIRE(out && allreduce, "geometric_median_sharded: null output or null all-reduce");
    BYZ_TRY(check_geomed(params, n_rows, "geometric_median_sharded"));
    return geometric_median(ctx, G, n_rows, n_cols, ld, params, allreduce, user, out, weights, stream);
}

int byz_geometric_median_info(byz_ctx* ctx, int64_t* iterations, int64_t* excluded_rows, double* objective) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportGeomed, nullptr, &all));
    if (iterations) *iterations = all.geomed.iterations;
    if (excluded_rows) *excluded_rows = all.geomed.excluded;
    if (objective) *objective = all.geomed.objective;
    return BYZ_OK;
}

// ---- centered clipping (Karimireddy, He and Jaggi 2021, Algorithm 2; beyond the reference) --------------------------------
namespace {

int check_cclip(const byz_cclip_params* params, int64_t n_rows, const char* who) {
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    // (written so that a NaN fails the test; +inf passes)
    if (!(params->tau > 0.0) || params->iters < 0) {
        set_error("%s: tau = %g must be > 0, iters = %lld >= 0", who, params->tau, (long long)params->iters);
        return BYZ_E_INVALID;
    }
    BYZ_TRY(check_row_ceiling(who, n_rows));
    if (params->iters > BYZ_CCLIP_MAX_ITER) {
        set_error("%s: iters = %lld beyond %d (every iteration's launches are enqueued up front)", who, (long long)params->iters,
                  BYZ_CCLIP_MAX_ITER);
        return BYZ_E_UNSUPPORTED;
    }
    return BYZ_OK;
}

// out must not overlap G (the update stores the new centre while other workgroups still read the matrix)
int check_cclip_output(const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* out, const char* who) {
    const float* g_end = G + (n_rows - 1) * ld + n_cols;
    if (out < g_end && out + n_cols > G) {
        set_error("%s: the output overlaps the matrix", who);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

// The whole call; allreduce == nullptr: one GPU holds every column.  Nothing here waits for the device.  The centre lives in
// `out` throughout.  Per iteration rowsq, the scales, the update: 2 * iters passes over G.  Nothing measures the rows against the
// final centre: the scales and the counts reported are those the last update used.
int centered_clip(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, const byz_cclip_params* params,
                  byz_allreduce_f64_fn allreduce, void* user, const float* start, float* out, double* scales, void* stream) {
    hipStream_t s = as_stream(stream);
    RowScratch t;
    BYZ_TRY(row_scratch(ctx, n, n_cols, &t));
    double *sq = t.a, *scale = t.b;
    mark(ctx, kReportCclip, s);
    const size_t vec_bytes = static_cast<size_t>(n_cols) * sizeof(float);
    if (start == nullptr) BYZ_HIP(hipMemsetAsync(out, 0, vec_bytes, s));
    else if (start != out) BYZ_HIP(hipMemcpyAsync(out, start, vec_bytes, hipMemcpyDeviceToDevice, s));
    if (params->iters == 0) BYZ_TRY(launch_cclip_scales(ctx, nullptr, n, params->tau, scale, s));      // scales 1, counts 0
    for (int64_t l = 0; l < params->iters; ++l) {
        BYZ_TRY(launch_row_sqdist(ctx, G, n, n_cols, ld, out, t.partials, sq, nullptr, nullptr, s));
        if (allreduce != nullptr) BYZ_TRY(reduce_over_ranks(allreduce, user, sq, n, stream, "centered clipping (distances)"));
        BYZ_TRY(launch_cclip_scales(ctx, sq, n, params->tau, scale, s));
        BYZ_TRY(launch_clip_update(ctx, G, n, n_cols, ld, out, scale, out, s));
    }
    if (scales != nullptr)
        BYZ_HIP(hipMemcpyAsync(scales, scale, static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToDevice, s));
    return BYZ_OK;
}

}  // namespace

int byz_clip_update_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* v,
                        const double* scales, float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "clip_update"));
    BYZ_REQUIRE(v && scales && out, "clip_update: null vector, scales or output");
    BYZ_TRY(check_row_ceiling("clip_update", n_rows));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "clip_update"));
    return launch_clip_update(ctx, G, n_rows, n_cols, ld, v, scales, out, as_stream(stream));
}

int byz_centered_clip_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                          const byz_cclip_params* params, const float* start, float* out, double* scales, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "centered_clip"));
    BYZ_REQUIRE(out, "centered_clip: null output");
    BYZ_TRY(check_cclip(params, n_rows, "centered_clip"));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "centered_clip"));
    return centered_clip(ctx, G, n_rows, n_cols, ld, params, nullptr, nullptr, start, out, scales, stream);
}

int byz_centered_clip_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                                  const byz_cclip_params* params, byz_allreduce_f64_fn allreduce, void* user, const float* start,
                                  float* out, double* scales, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "centered_clip_sharded"));
    BYZ_REQUIRE(out && allreduce, "centered_clip_sharded: null output or null all-reduce");
    BYZ_TRY(check_cclip(params, n_rows, "centered_clip_sharded"));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "centered_clip_sharded"));
    return centered_clip(ctx, G, n_rows, n_cols, ld, params, allreduce, user, start, out, scales, stream);
}

int byz_centered_clip_info(byz_ctx* ctx, int64_t* clipped_rows, int64_t* excluded_rows) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportCclip, nullptr, &all));
    if (clipped_rows) *clipped_rows = all.cclip.clipped;
    if (excluded_rows) *excluded_rows = all.cclip.excluded;
    return BYZ_OK;
}

// ---- FLTrust (Cao, Fang, Liu and Gong, NDSS 2021; beyond the reference) -------------------------------------------------
namespace {

// The whole call; allreduce == nullptr: one GPU holds every column.  Nothing here waits for the device.  Two passes over G:
// the dots, then the sum; the root's squared norm and the trust scores are two tiny launches between them.
int fltrust(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, const float* root, byz_allreduce_f64_fn allreduce,
            void* user, float* out, double* trust, double* weights, void* stream) {
    hipStream_t s = as_stream(stream);
    RowScratch t;
    BYZ_TRY(row_scratch(ctx, n, n_cols, &t, 2));
    double *pq = t.a, *ts = t.b, *w = t.b + n;
    mark(ctx, kReportFltrust, s);
    BYZ_TRY(launch_row_sqdist(ctx, root, 1, n_cols, n_cols, nullptr, t.root, pq + 2 * n, nullptr, nullptr, s));
    BYZ_TRY(launch_row_dots(ctx, G, n, n_cols, ld, root, t.partials, pq, pq + n, s));
    if (allreduce != nullptr) BYZ_TRY(reduce_over_ranks(allreduce, user, pq, 2 * n + 1, stream, "fltrust (dots and norms)"));
    BYZ_TRY(launch_fltrust_trust(ctx, pq, n, ts, w, s));
    BYZ_TRY(launch_scaled_rows_sum(ctx, G, n, n_cols, ld, w, &device_scalars(ctx)->fltrust.trust_sum, out, s));      // (out may be root: its last reader is behind)
    const size_t row_bytes = static_cast<size_t>(n) * sizeof(double);
    if (trust != nullptr) BYZ_HIP(hipMemcpyAsync(trust, ts, row_bytes, hipMemcpyDeviceToDevice, s));
    if (weights != nullptr) BYZ_HIP(hipMemcpyAsync(weights, w, row_bytes, hipMemcpyDeviceToDevice, s));
    return BYZ_OK;
}

}  // namespace

int byz_row_dots_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* r, double* dot,
                     double* sq, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "row_dots"));
    BYZ_REQUIRE(r && dot && sq, "row_dots: null vector or output");
    BYZ_TRY(check_row_ceiling("row_dots", n_rows));
    RowScratch t;
    BYZ_TRY(row_scratch(ctx, n_rows, n_cols, &t, 2));
    return launch_row_dots(ctx, G, n_rows, n_cols, ld, r, t.partials, dot, sq, as_stream(stream));
}

int byz_scaled_rows_sum_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const double* w,
                            const double* divisor, float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "scaled_rows_sum"));
    BYZ_REQUIRE(w && divisor && out, "scaled_rows_sum: null weights, divisor or output");
    BYZ_TRY(check_row_ceiling("scaled_rows_sum", n_rows));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "scaled_rows_sum"));
    return launch_scaled_rows_sum(ctx, G, n_rows, n_cols, ld, w, divisor, out, as_stream(stream));
}

int byz_fltrust_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* root, float* out,
                    double* trust, double* weights, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "fltrust"));
    BYZ_REQUIRE(root && out, "fltrust: null root or output");
    BYZ_TRY(check_row_ceiling("fltrust", n_rows));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "fltrust"));
    return fltrust(ctx, G, n_rows, n_cols, ld, root, nullptr, nullptr, out, trust, weights, stream);
}

int byz_fltrust_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* root,
                            byz_allreduce_f64_fn allreduce, void* user, float* out, double* trust, double* weights,
                            void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "fltrust_sharded"));
    BYZ_REQUIRE(root && out && allreduce, "fltrust_sharded: null root, output or all-reduce");
    BYZ_TRY(check_row_ceiling("fltrust_sharded", n_rows));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "fltrust_sharded"));
    return fltrust(ctx, G, n_rows, n_cols, ld, root, allreduce, user, out, trust, weights, stream);
}

int byz_fltrust_info(byz_ctx* ctx, int64_t* trusted_rows, int64_t* excluded_rows, int32_t* root_ok, double* trust_sum) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportFltrust, nullptr, &all));
    if (trusted_rows) *trusted_rows = all.fltrust.trusted;
    if (excluded_rows) *excluded_rows = all.fltrust.excluded;
    if (root_ok) *root_ok = all.fltrust.root_ok;
    if (trust_sum) *trust_sum = all.fltrust.trust_sum;
    return BYZ_OK;
}

// ---- SignGuard (Xu, Huang, Song and Lan, ICDCS 2022; beyond the reference) -------------------------------------------------
namespace {

int check_signguard(const byz_signguard_params* p, int64_t n_rows, const int32_t* sample, const char* who) {
    if (!p) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    BYZ_TRY(check_row_ceiling(who, n_rows));
    if (!(p->lower >= 0.0) || !(p->upper > p->lower) || !(p->bandwidth >= 0.0) || p->window_start < 0 || p->window_len < 1) {
        set_error("%s: lower = %g must be >= 0, upper = %g > lower, bandwidth = %g >= 0, window_start = %lld >= 0, window_len = "
                  "%lld >= 1", who, p->lower, p->upper, p->bandwidth, (long long)p->window_start, (long long)p->window_len);
        return BYZ_E_INVALID;
    }
    if (!(p->bandwidth > 0.0) && (!sample || p->n_sample < 1 || p->n_sample > BYZ_SIGNGUARD_MAX_SAMPLES || p->n_sample > n_rows)) {
        set_error("%s: the bandwidth is estimated from 1..min(n_rows, %d) sampled rows, got %lld (sample %p)", who,
                  BYZ_SIGNGUARD_MAX_SAMPLES, (long long)p->n_sample, (const void*)sample);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

// The whole call; allreduce == nullptr: one GPU holds every column and [win_start, win_start + win_len) is the window itself.
// Nothing here waits for the device.  Two passes over G: the census, then the sum over the kept rows.
int signguard(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, const byz_signguard_params* p, int64_t win_start,
              int64_t win_len, const int32_t* sample, byz_allreduce_f64_fn allreduce, void* user, float* out, int32_t* keep,
              double* weights, int32_t* labels, void* stream) {
    hipStream_t s = as_stream(stream);
    SgScratch t;
    BYZ_TRY(signguard_workspace(ctx, n, n_cols, &t));
    mark(ctx, kReportSignguard, s);
    BYZ_TRY(launch_row_signs(ctx, t, G, n, n_cols, ld, win_start, win_len, nullptr, nullptr, t.pznq, s));
    if (allreduce != nullptr) BYZ_TRY(reduce_over_ranks(allreduce, user, t.pznq, 4 * n, stream, "signguard (counts and norms)"));
    BYZ_TRY(launch_signguard_select(ctx, t, t.pznq, n, p->window_len, p->lower, p->upper, p->bandwidth, sample, p->n_sample,
                                    keep ? keep : t.keep, t.w, labels ? labels : t.labels, nullptr, s));
    BYZ_TRY(launch_scaled_rows_sum(ctx, G, n, n_cols, ld, t.w, &device_scalars(ctx)->sg.kept_f64, out, s));
    if (weights != nullptr)
        BYZ_HIP(hipMemcpyAsync(weights, t.w, static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToDevice, s));
    return BYZ_OK;
}

}  // namespace

int byz_row_signs_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t window_start,
                      int64_t window_len, int64_t* counts, double* q, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "row_signs"));
    BYZ_REQUIRE(counts && q, "row_signs: null output");
    BYZ_TRY(check_row_ceiling("row_signs", n_rows));
    SgScratch t;
    BYZ_TRY(signguard_workspace(ctx, n_rows, n_cols, &t));
    return launch_row_signs(ctx, t, G, n_rows, n_cols, ld, window_start, window_len, reinterpret_cast<long long*>(counts), q, nullptr,
                            as_stream(stream));
}

int byz_signguard_select_dev(byz_ctx* ctx, const int64_t* counts, const double* q, int64_t n_rows, const byz_signguard_params* params,
                             const int32_t* sample, int32_t* keep, double* weights, int32_t* labels, double* mk, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(counts && q && n_rows > 0, "signguard_select: null counts or norms, or no rows");
    BYZ_TRY(check_signguard(params, n_rows, sample, "signguard_select"));
    hipStream_t s = as_stream(stream);
    SgScratch t;
    BYZ_TRY(signguard_workspace(ctx, n_rows, 0, &t));
    mark(ctx, kReportSignguard, s);
    BYZ_TRY(launch_signguard_counts_f64(ctx, reinterpret_cast<const long long*>(counts), q, n_rows, t.pznq, s));
    return launch_signguard_select(ctx, t, t.pznq, n_rows, params->window_len, params->lower, params->upper, params->bandwidth, sample,
                                   params->n_sample, keep ? keep : t.keep, weights ? weights : t.w, labels ? labels : t.labels, mk, s);
}

int byz_signguard_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_signguard_params* params,
                      const int32_t* sample, float* out, int32_t* keep, double* weights, int32_t* labels, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "signguard"));
    BYZ_REQUIRE(out, "signguard: null output");
    BYZ_TRY(check_signguard(params, n_rows, sample, "signguard"));
    BYZ_REQUIRE(params->window_start <= n_cols && params->window_len <= n_cols - params->window_start,
                "signguard: the window [%lld, %lld + %lld) is outside the %lld columns", (long long)params->window_start,
                (long long)params->window_start, (long long)params->window_len, (long long)n_cols);
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "signguard"));
    return signguard(ctx, G, n_rows, n_cols, ld, params, params->window_start, params->window_len, sample, nullptr, nullptr, out, keep,
                     weights, labels, stream);
}

int byz_signguard_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                              const byz_signguard_params* params, int64_t local_window_start, int64_t local_window_len,
                              const int32_t* sample, byz_allreduce_f64_fn allreduce, void* user, float* out, int32_t* keep,
                              double* weights, int32_t* labels, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "signguard_sharded"));
    BYZ_REQUIRE(out && allreduce, "signguard_sharded: null output or all-reduce");
    BYZ_TRY(check_signguard(params, n_rows, sample, "signguard_sharded"));
    BYZ_REQUIRE(local_window_start >= 0 && local_window_len >= 0 && local_window_start <= n_cols &&
                    local_window_len <= n_cols - local_window_start && local_window_len <= params->window_len,
                "signguard_sharded: the local window [%lld, %lld + %lld) is outside the slice's %lld columns or longer than the "
                "global window", (long long)local_window_start, (long long)local_window_start, (long long)local_window_len,
                (long long)n_cols);
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "signguard_sharded"));
    return signguard(ctx, G, n_rows, n_cols, ld, params, local_window_start, local_window_len, sample, allreduce, user, out, keep,
                     weights, labels, stream);
}

int byz_signguard_info(byz_ctx* ctx, int64_t* kept_rows, int64_t* norm_failed_rows, int64_t* outside_rows, int64_t* clusters,
                       int64_t* seeds, double* bandwidth, double* median_norm) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportSignguard, nullptr, &all));
    if (kept_rows) *kept_rows = all.sg.kept;
    if (norm_failed_rows) *norm_failed_rows = all.sg.norm_failed;
    if (outside_rows) *outside_rows = all.sg.outside;
    if (clusters) *clusters = all.sg.clusters;
    if (seeds) *seeds = all.sg.seeds;
    if (bandwidth) *bandwidth = all.sg.bandwidth;
    if (median_norm) *median_norm = all.sg.median;
    return BYZ_OK;
}

// ---- nearest-neighbour mixing (Allouah et al., AISTATS 2023; beyond the reference) -----------------------------------------
namespace {

// k = users_count - corrupted_count rows a list at most; the n x n keys and mask end at kNnmMaxRows rows (checked on the
// arguments alone, before any pointer is looked at)
int check_nnm(const char* who, int64_t n_rows, int64_t k) {
    if (n_rows > kNnmMaxRows) {
        set_error("%s: at most %lld rows, got %lld", who, (long long)kNnmMaxRows, (long long)n_rows);
        return BYZ_E_UNSUPPORTED;
    }
    if (n_rows < 1 || k < 1 || k > n_rows) {
        set_error("%s: k = users_count - corrupted_count = %lld outside 1..%lld (the row count)", who, (long long)k, (long long)n_rows);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

// Y (y_rows x n_cols, leading dimension ldy) must not overlap G: a workgroup stores its part of Y while others still read G
int check_matrix_output(const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* Y, int64_t y_rows, int64_t ldy,
                        const char* who) {
    if (!Y || ldy < n_cols) {
        set_error("%s: bad output (ptr %p, ldy %lld < %lld columns)", who, (const void*)Y, (long long)ldy, (long long)n_cols);
        return BYZ_E_INVALID;
    }
    const float* g_end = G + (n_rows - 1) * ld + n_cols;
    const float* y_end = Y + (y_rows - 1) * ldy + n_cols;
    if (Y < g_end && y_end > G) {
        set_error("%s: the output overlaps the matrix", who);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}
int check_nnm_output(const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* Y, int64_t ldy, const char* who) {
    return check_matrix_output(G, n_rows, n_cols, ld, Y, n_rows, ldy, who);
}

// The whole call; allreduce == nullptr: one GPU holds every column.  Distances (over the ranks' slices when sharded: the one
// exchange), the lists -- the same on every rank --, the mix on the local columns.
int nnm(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, int64_t k, byz_allreduce_f64_fn allreduce, void* user,
        float* Y, int64_t ldy, int32_t* nbr_out, void* stream) {
    hipStream_t s = as_stream(stream);
    BYZ_TRY(ensure_distance_workspaces(ctx, n));
    const size_t list_bytes = static_cast<size_t>(n) * k * sizeof(int32_t);
    BYZ_TRY(ctx->nnm_lists.ensure(list_bytes + static_cast<size_t>(n) * sizeof(int32_t)));
    int32_t* nbr = ctx->nnm_lists.as<int32_t>();
    int32_t* counts = nbr + n * k;
    mark(ctx, kReportNnm, s);
    BYZ_TRY(distances(ctx, G, n, n_cols, ld, allreduce, user, ctx->dist.as<float>(), stream));
    BYZ_TRY(launch_nnm_neighbours(ctx, ctx->dist.as<float>(), n, k, nbr, counts, s));
    BYZ_TRY(launch_nnm_mix(ctx, G, n, n_cols, ld, nbr, counts, k, Y, ldy, s));
    if (nbr_out != nullptr) BYZ_HIP(hipMemcpyAsync(nbr_out, nbr, list_bytes, hipMemcpyDeviceToDevice, s));
    return BYZ_OK;
}

}  // namespace

int byz_nnm_neighbours_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int64_t k, int32_t* nbr, int32_t* counts, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_nnm("nnm_neighbours", n_rows, k));
    BYZ_REQUIRE(dist && nbr, "nnm_neighbours: null distances or output");
    mark(ctx, kReportNnm, as_stream(stream));
    return launch_nnm_neighbours(ctx, dist, n_rows, k, nbr, counts, as_stream(stream));
}

int byz_nnm_mix_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* nbr,
                    const int32_t* counts, int64_t k, float* Y, int64_t ldy, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_nnm("nnm_mix", n_rows, k));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "nnm_mix"));
    BYZ_REQUIRE(nbr, "nnm_mix: null neighbour lists");
    BYZ_TRY(check_nnm_output(G, n_rows, n_cols, ld, Y, ldy, "nnm_mix"));
    return launch_nnm_mix(ctx, G, n_rows, n_cols, ld, nbr, counts, k, Y, ldy, as_stream(stream));
}

int byz_nnm_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
                int64_t corrupted_count, float* Y, int64_t ldy, int32_t* nbr, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_nnm("nnm", n_rows, users_count - corrupted_count));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "nnm"));
    BYZ_TRY(check_nnm_output(G, n_rows, n_cols, ld, Y, ldy, "nnm"));
    return nnm(ctx, G, n_rows, n_cols, ld, users_count - corrupted_count, nullptr, nullptr, Y, ldy, nbr, stream);
}

int byz_nnm_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
                        int64_t corrupted_count, byz_allreduce_f64_fn allreduce, void* user, float* Y, int64_t ldy, int32_t* nbr,
                        void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_nnm("nnm_sharded", n_rows, users_count - corrupted_count));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "nnm_sharded"));
    BYZ_REQUIRE(allreduce, "nnm_sharded: null all-reduce");
    BYZ_TRY(check_nnm_output(G, n_rows, n_cols, ld, Y, ldy, "nnm_sharded"));
    return nnm(ctx, G, n_rows, n_cols, ld, users_count - corrupted_count, allreduce, user, Y, ldy, nbr, stream);
}

int byz_nnm_info(byz_ctx* ctx, int64_t* solo_rows, int64_t* short_rows) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportNnm, nullptr, &all));
    if (solo_rows) *solo_rows = all.nnm.solo;
    if (short_rows) *short_rows = all.nnm.short_rows;
    return BYZ_OK;
}

// ---- the robust learning rate (Ozdayi, Kantarcioglu and Gel, AAAI 2021; beyond the reference) ----------------------------------
namespace {

// theta counts clients: 0 .. n_rows (checked on the arguments alone)
int check_rlr_theta(const char* who, int64_t theta, int64_t n_rows) {
    if (theta < 0 || theta > n_rows) {
        set_error("%s: theta = %lld outside 0..%lld (the row count)", who, (long long)theta, (long long)n_rows);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

}  // namespace

int byz_sign_votes_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t* votes, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "sign_votes"));
    BYZ_REQUIRE(votes, "sign_votes: null output");
    BYZ_TRY(check_row_ceiling("sign_votes", n_rows));
    mark(ctx, kReportRlr, as_stream(stream));
    return launch_sign_votes(ctx, G, n_rows, n_cols, ld, 0, nullptr, votes, as_stream(stream));
}

int byz_sign_flip_dev(byz_ctx* ctx, const float* agg, const int32_t* votes, int64_t n_cols, int64_t theta, float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(agg && votes && out && n_cols > 0, "sign_flip: null vector or no columns (%lld)", (long long)n_cols);
    BYZ_TRY(check_rlr_theta("sign_flip", theta, kLargeMaxRows));
    mark(ctx, kReportRlr, as_stream(stream));
    return launch_sign_flip(ctx, agg, votes, n_cols, theta, out, as_stream(stream));
}

int byz_robust_lr_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t theta, float* out,
                      int32_t* votes, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "robust_lr"));
    BYZ_REQUIRE(out, "robust_lr: null output");
    BYZ_TRY(check_row_ceiling("robust_lr", n_rows));
    BYZ_TRY(check_rlr_theta("robust_lr", theta, n_rows));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "robust_lr"));
    mark(ctx, kReportRlr, as_stream(stream));
    return launch_sign_votes(ctx, G, n_rows, n_cols, ld, theta, out, votes, as_stream(stream));
}

int byz_robust_lr_info(byz_ctx* ctx, int64_t* flipped_cols) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportRlr, nullptr, &all));
    if (flipped_cols) *flipped_cols = static_cast<int64_t>(all.rlr.flipped);
    return BYZ_OK;
}

// ---- s-bucketing (Karimireddy, He and Jaggi, ICLR 2022; beyond the reference) ---------------------------------------------------
namespace {

// the row ceiling first and on the arguments alone, then the shapes: 1 <= s <= n_rows
int check_bucketing(const char* who, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t s) {
    BYZ_TRY(check_row_ceiling(who, n_rows));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, who));
    if (s < 1 || s > n_rows) {
        set_error("%s: s = %lld outside 1..%lld (the row count)", who, (long long)s, (long long)n_rows);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

}  // namespace

int byz_bucket_means_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* perm, int64_t s,
                         float* Y, int64_t ldy, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_bucketing("bucket_means", G, n_rows, n_cols, ld, s));
    BYZ_TRY(check_matrix_output(G, n_rows, n_cols, ld, Y, ceil_div(n_rows, s), ldy, "bucket_means"));
    return launch_bucket_means(ctx, G, n_rows, n_cols, ld, perm, s, Y, ldy, as_stream(stream));
}

// ---- SparseFed: global top-k with error feedback (Panda et al., AISTATS 2022; beyond the reference) --------------------------------
namespace {

bool vectors_overlap(const float* a, const float* b, int64_t n) { return a && b && a < b + n && b < a + n; }

// an output may coincide with ONE input exactly (residual with x, out with add); an output that touches anything else is refused
int check_topk(const char* who, const float* x, const float* add, int64_t n, int64_t k_max, int64_t k, const float* out,
               const float* residual) {
    if (k < 0 || k > k_max) {
        set_error("%s: k = %lld outside 0..%lld (the length)", who, (long long)k, (long long)k_max);
        return BYZ_E_INVALID;
    }
    const bool bad = vectors_overlap(out, x, n) || (out != add && vectors_overlap(out, add, n)) || vectors_overlap(out, residual, n) ||
                     (residual != x && vectors_overlap(residual, x, n)) || vectors_overlap(residual, add, n);
    if (bad) {
        set_error("%s: an output overlaps another vector (residual may be x, out may be add, nothing else)", who);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

}  // namespace

int byz_topk_sparsify_dev(byz_ctx* ctx, const float* x, const float* add, int64_t n, int64_t k, float* out, float* residual,
                          void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(x && out && n > 0, "topk_sparsify: null vector or no columns (%lld)", (long long)n);
    BYZ_TRY(check_topk("topk_sparsify", x, add, n, n, k, out, residual));
    mark(ctx, kReportTopk, as_stream(stream));
    return launch_topk_sparsify(ctx, x, add, n, k, 0, 1, nullptr, nullptr, out, residual, 0, stream);
}

int byz_topk_sparsify_sharded_dev(byz_ctx* ctx, const float* x, const float* add, int64_t n_local, int64_t n_total, int64_t k,
                                  int rank_index, int rank_count, byz_allreduce_f64_fn allreduce, void* user, float* out,
                                  float* residual, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(allreduce, "topk_sparsify_sharded: null all-reduce");
    BYZ_REQUIRE(n_total > 0 && n_local >= 0 && n_local <= n_total, "topk_sparsify_sharded: %lld local columns of %lld",
                (long long)n_local, (long long)n_total);
    BYZ_REQUIRE(rank_count >= 1 && rank_count <= 65536 && rank_index >= 0 && rank_index < rank_count,
                "topk_sparsify_sharded: rank %d of %d", rank_index, rank_count);
    BYZ_REQUIRE(n_local == 0 || (x && out), "topk_sparsify_sharded: null vector");
    BYZ_TRY(check_topk("topk_sparsify_sharded", x, add, n_local, n_total, k, out, residual));
    mark(ctx, kReportTopk, as_stream(stream));
    return launch_topk_sparsify(ctx, x, add, n_local, k, rank_index, rank_count, allreduce, user, out, residual, 0, stream);
}

int byz_topk_info(byz_ctx* ctx, int64_t* selected, uint32_t* threshold_key, int64_t* ties, int64_t* ties_taken) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportTopk, nullptr, &all));
    if (selected) *selected = static_cast<int64_t>(all.topk.selected);
    if (ties) *ties = static_cast<int64_t>(all.topk.ties);
    if (ties_taken) *ties_taken = static_cast<int64_t>(all.topk.taken);
    if (threshold_key) *threshold_key = static_cast<uint32_t>(all.topk.key);
    return BYZ_OK;
}

int byz_sparsefed_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_sparsefed_params* params,
                      float* residual, float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "sparsefed"));
    BYZ_REQUIRE(params && residual && out, "sparsefed: null parameters, memory or output");
    const byz_cclip_params clip = {params->clip, 1};
    BYZ_TRY(check_cclip(&clip, n_rows, "sparsefed"));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "sparsefed"));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, residual, "sparsefed"));
    BYZ_TRY(check_topk("sparsefed", residual, nullptr, n_cols, n_cols, params->k, out, nullptr));
    float* agg = topk_aggregate_workspace(ctx, n_cols);
    if (agg == nullptr) return BYZ_E_HIP;
    BYZ_TRY(centered_clip(ctx, G, n_rows, n_cols, ld, &clip, nullptr, nullptr, nullptr, agg, nullptr, stream));
    mark(ctx, kReportTopk, as_stream(stream));
    return launch_topk_sparsify(ctx, residual, agg, n_cols, params->k, 0, 1, nullptr, nullptr, out, residual, n_cols, stream);
}

// ---- clip and noise, "weak DP" (Sun et al. 2019; FLAME's last stage; beyond the reference) ------------------------------------------
namespace {

constexpr int64_t kNoiseMaxColumn = int64_t{1} << 62;

// (written so that a NaN sigma fails the test)
int check_noise(const char* who, double sigma, int64_t column_offset, int64_t n) {
    if (!(sigma >= 0.0) || !__builtin_isfinite(sigma)) {
        set_error("%s: sigma = %g must be finite and >= 0", who, sigma);
        return BYZ_E_INVALID;
    }
    if (n < 1 || column_offset < 0 || n > kNoiseMaxColumn - column_offset) {
        set_error("%s: %lld columns from global column %lld (at least one, from 0 on, up to 2^62)", who, (long long)n,
                  (long long)column_offset);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

int check_weak_dp(const char* who, const byz_weak_dp_params* params, int64_t n_rows, int64_t n_cols) {
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    if (!params->adaptive && !(params->clip > 0.0)) {      // (a NaN fails; +inf passes, as centered clipping's tau)
        set_error("%s: clip = %g must be > 0 in the fixed mode", who, params->clip);
        return BYZ_E_INVALID;
    }
    BYZ_TRY(check_noise(who, params->sigma, params->column_offset, n_cols));
    return check_row_ceiling(who, n_rows);
}

}  // namespace

int byz_gaussian_noise_dev(byz_ctx* ctx, const float* x, int64_t n, const byz_noise_params* params, const double* scale_dev,
                           float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(x && out && params, "gaussian_noise: null vector or parameters");
    BYZ_TRY(check_noise("gaussian_noise", params->sigma, params->column_offset, n));
    BYZ_REQUIRE(out == x || !vectors_overlap(x, out, n), "gaussian_noise: the output overlaps x (it may BE x, nothing else)");
    hipStream_t s = as_stream(stream);
    if (params->sigma == 0.0 && scale_dev == nullptr) {      // x's bits verbatim (an addition of 0.0 would turn -0.0 into +0.0)
        if (out != x) BYZ_HIP(hipMemcpyAsync(out, x, static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToDevice, s));
        return BYZ_OK;
    }
    return launch_gaussian_noise(ctx, x, n, params->sigma, params->seed, params->round, params->column_offset, scale_dev, out, s);
}

int byz_noise_words_dev(byz_ctx* ctx, const byz_noise_params* params, int64_t n, uint32_t* words, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(words && params, "noise_words: null output or parameters");
    BYZ_TRY(check_noise("noise_words", 0.0, params->column_offset, n));
    return launch_noise_words(ctx, params->seed, params->round, params->column_offset, n, words, as_stream(stream));
}

int byz_clip_scales_dev(byz_ctx* ctx, const double* sq, int64_t n_rows, const byz_weak_dp_params* params, double* scales,
                        double* clip_dev, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(sq && scales && n_rows > 0, "clip_scales: null norms or scales, or no rows (%lld)", (long long)n_rows);
    BYZ_REQUIRE(params && (params->adaptive || params->clip > 0.0), "clip_scales: null parameters, or clip not > 0 in the fixed mode");
    BYZ_TRY(check_row_ceiling("clip_scales", n_rows));
    mark(ctx, kReportWeakDp, as_stream(stream));
    return launch_clip_scales(ctx, sq, n_rows, params->clip, params->adaptive != 0, scales, clip_dev, as_stream(stream));
}

int byz_weak_dp_info(byz_ctx* ctx, int64_t* clipped_rows, int64_t* excluded_rows, double* clip) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportWeakDp, nullptr, &all));
    if (clipped_rows) *clipped_rows = all.weak_dp.clipped;
    if (excluded_rows) *excluded_rows = all.weak_dp.excluded;
    if (clip) *clip = all.weak_dp.clip;
    return BYZ_OK;
}

// centered_clip's one iteration from zero with the scales' clip chosen by the mode, then the noise in place on out
int byz_weak_dp_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_weak_dp_params* params,
                    float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "weak_dp"));
    BYZ_REQUIRE(out, "weak_dp: null output");
    BYZ_TRY(check_weak_dp("weak_dp", params, n_rows, n_cols));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "weak_dp"));
    hipStream_t s = as_stream(stream);
    const bool adaptive = params->adaptive != 0;
    RowScratch t;
    BYZ_TRY(row_scratch(ctx, n_rows, n_cols, &t));
    double *sq = t.a, *scale = t.b;
    mark(ctx, kReportWeakDp, s);
    BYZ_HIP(hipMemsetAsync(out, 0, static_cast<size_t>(n_cols) * sizeof(float), s));
    BYZ_TRY(launch_row_sqdist(ctx, G, n_rows, n_cols, ld, out, t.partials, sq, nullptr, nullptr, s));
    BYZ_TRY(launch_clip_scales(ctx, sq, n_rows, params->clip, adaptive, scale, nullptr, s));
    BYZ_TRY(launch_clip_update(ctx, G, n_rows, n_cols, ld, out, scale, out, s));
    if (params->sigma == 0.0) return BYZ_OK;               // the clipped mean's bits
    return launch_gaussian_noise(ctx, out, n_cols, params->sigma, params->seed, params->round, params->column_offset,
                                 adaptive ? &device_scalars(ctx)->weak_dp.clip : nullptr, out, s);
}

// ---- FLAME (Nguyen et al., USENIX Security 2022; beyond the reference) -------------------------------------------------------
namespace {

// the ceiling of the kernels whose one workgroup owns every row (owner_loop.hpp): FLAME, the linkage, Multi-Metrics, FABA, AFA
int check_owned_rows(const char* who, int64_t n) {
    if (n > kOwnerMaxRows) {
        set_error("%s: at most %lld rows, got %lld", who, (long long)kOwnerMaxRows, (long long)n);
        return BYZ_E_UNSUPPORTED;
    }
    return BYZ_OK;
}

int check_flame_select(const char* who, int64_t n, int64_t m, int64_t ms) {
    BYZ_TRY(check_owned_rows(who, n));
    if (n < 2 || m < 2 || m > n || 2 * m <= n) {
        set_error("%s: min_cluster_size = %lld must lie in 2..n and exceed n / 2 (n = %lld): one majority cluster", who, (long long)m,
                  (long long)n);
        return BYZ_E_INVALID;
    }
    if (ms > kFlameMaxSamples) {
        set_error("%s: min_samples = %lld beyond %lld", who, (long long)ms, (long long)kFlameMaxSamples);
        return BYZ_E_UNSUPPORTED;
    }
    if (ms < 0 || ms > n - 1) {
        set_error("%s: min_samples = %lld outside 0..n - 1 (n = %lld)", who, (long long)ms, (long long)n);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

int64_t flame_cluster_size(const byz_flame_params* params, int64_t n) {
    return params->min_cluster_size == 0 ? n / 2 + 1 : params->min_cluster_size;
}

int check_flame(const char* who, const byz_flame_params* params, int64_t n_rows, int64_t n_cols) {
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    BYZ_TRY(check_owned_rows(who, n_rows));
    BYZ_TRY(check_noise(who, params->lambda, params->column_offset, n_cols));
    return check_flame_select(who, n_rows, flame_cluster_size(params, n_rows), params->min_samples);
}

// the cosine distances of G's rows into dist, the Gram in ctx->gram; with an all-reduce the Gram of the ranks' column slices
int cosine_distances(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, byz_allreduce_f64_fn allreduce, void* user,
                     float* dist, void* stream) {
    hipStream_t s = as_stream(stream);
    BYZ_TRY(ctx->gram.ensure(static_cast<size_t>(n) * n * sizeof(double)));
    double* gram = ctx->gram.as<double>();
    BYZ_TRY(launch_gram(ctx, G, n, n_cols, ld, gram, s));
    if (allreduce != nullptr) {
        ctx->row_map_rows = 0;      // (what the duplicate search proved holds for the local columns only)
        BYZ_TRY(reduce_over_ranks(allreduce, user, gram, n * n, stream, "flame (Gram)"));
    }
    return launch_cosine_from_gram(ctx, gram, n, dist, s);
}

// The whole call; allreduce == nullptr: one GPU holds every column.  Every launch of the stages added here is enqueued up
// front; the one wait is the Gram's own duplicate search (dedup.hip: find_unique_rows reads a count back to size its launch),
// the same wait byz_gram_dev and byz_pairwise_distances_dev make.  A caller's dist_in skips the Gram and with it that wait.
int flame(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, const byz_flame_params* params,
          byz_allreduce_f64_fn allreduce, void* user, const float* dist_in, float* out, int32_t* admitted_out, void* stream) {
    hipStream_t s = as_stream(stream);
    FlameScratch f;
    BYZ_TRY(flame_workspace(ctx, n, &f));
    RowScratch t;
    BYZ_TRY(row_scratch(ctx, n, n_cols, &t));
    double *sq = t.a, *scale = t.b;
    mark(ctx, kReportFlame, s);
    mark(ctx, kReportWeakDp, s);
    const float* dist = dist_in;
    if (dist == nullptr) {
        BYZ_TRY(ctx->dist.ensure(static_cast<size_t>(n) * n * sizeof(float)));
        BYZ_TRY(cosine_distances(ctx, G, n, n_cols, ld, allreduce, user, ctx->dist.as<float>(), stream));
        dist = ctx->dist.as<float>();
    }
    BYZ_TRY(launch_flame_select(ctx, f, dist, n, flame_cluster_size(params, n), params->min_samples, admitted_out, s));
    BYZ_HIP(hipMemsetAsync(out, 0, static_cast<size_t>(n_cols) * sizeof(float), s));
    BYZ_TRY(launch_row_sqdist(ctx, G, n, n_cols, ld, out, t.partials, sq, nullptr, nullptr, s));
    if (allreduce != nullptr) BYZ_TRY(reduce_over_ranks(allreduce, user, sq, n, stream, "flame (norms)"));
    BYZ_TRY(launch_clip_scales(ctx, sq, n, 0.0, true, scale, &f.info->clip, s));     // the paper's median: over all n rows
    BYZ_TRY(launch_flame_weights(ctx, f.admitted, scale, n, f.w, s));
    BYZ_TRY(launch_scaled_rows_sum(ctx, G, n, n_cols, ld, f.w, &f.info->admitted_f64, out, s));
    if (params->lambda == 0.0) return BYZ_OK;              // the clipped mean's bits
    return launch_gaussian_noise(ctx, out, n_cols, params->lambda, params->seed, params->round, params->column_offset,
                                 &device_scalars(ctx)->weak_dp.clip, out, s);
}

}  // namespace

int byz_cosine_distances_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, float* dist, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "cosine_distances"));
    BYZ_REQUIRE(dist, "cosine_distances: null output");
    BYZ_TRY(check_owned_rows("cosine_distances", n_rows));
    return cosine_distances(ctx, G, n_rows, n_cols, ld, nullptr, nullptr, dist, stream);
}

int byz_cosine_from_gram_dev(byz_ctx* ctx, const double* gram, int64_t n_rows, float* dist, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(gram && dist && n_rows > 0, "cosine_from_gram: null Gram or output, or no rows (%lld)", (long long)n_rows);
    BYZ_TRY(check_owned_rows("cosine_from_gram", n_rows));
    return launch_cosine_from_gram(ctx, gram, n_rows, dist, as_stream(stream));
}

int byz_flame_core_distances_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int64_t min_samples, float* core, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist && core, "flame_core_distances: null distances or output");
    BYZ_TRY(check_flame_select("flame_core_distances", n_rows, n_rows, min_samples));
    FlameScratch f;
    BYZ_TRY(flame_workspace(ctx, n_rows, &f));
    return launch_flame_core(ctx, dist, n_rows, min_samples, core, f.isolated, as_stream(stream));
}

int byz_flame_select_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int64_t min_cluster_size, int64_t min_samples,
                         int32_t* admitted, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist && admitted, "flame_select: null distances or output");
    BYZ_TRY(check_flame_select("flame_select", n_rows, min_cluster_size, min_samples));
    FlameScratch f;
    BYZ_TRY(flame_workspace(ctx, n_rows, &f));
    mark(ctx, kReportFlame, as_stream(stream));
    BYZ_HIP(hipMemsetAsync(&f.info->clip, 0, sizeof(double), as_stream(stream)));
    return launch_flame_select(ctx, f, dist, n_rows, min_cluster_size, min_samples, admitted, as_stream(stream));
}

int byz_flame_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_flame_params* params,
                  const float* dist, float* out, int32_t* admitted, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "flame"));
    BYZ_REQUIRE(out, "flame: null output");
    BYZ_TRY(check_flame("flame", params, n_rows, n_cols));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "flame"));
    return flame(ctx, G, n_rows, n_cols, ld, params, nullptr, nullptr, dist, out, admitted, stream);
}

int byz_flame_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_flame_params* params,
                          byz_allreduce_f64_fn allreduce, void* user, const float* dist, float* out, int32_t* admitted,
                          void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "flame_sharded"));
    BYZ_REQUIRE(out && allreduce, "flame_sharded: null output or null all-reduce");
    BYZ_TRY(check_flame("flame_sharded", params, n_rows, n_cols));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "flame_sharded"));
    return flame(ctx, G, n_rows, n_cols, ld, params, allreduce, user, dist, out, admitted, stream);
}

int byz_flame_info(byz_ctx* ctx, int64_t* admitted_rows, int64_t* broken_rows, double* w_star, double* clip) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportFlame, "flame_info: no FLAME selection on this context yet", &all));
    const FlameInfo& info = all.flame;
    if (admitted_rows) *admitted_rows = info.admitted;
    if (broken_rows) *broken_rows = info.broken_rows;
    if (w_star) *w_star = static_cast<double>(info.w_star);
    if (clip) *clip = info.clip;
    return BYZ_OK;
}

// ---- Agglomerative clustering and ClippedClustering (Li, Ngai & Voigt 2023; beyond the reference) ---------------------------------
namespace {

int check_linkage(const char* who, int64_t n, int method, const double* fill) {
    BYZ_TRY(check_owned_rows(who, n));
    if (n < 2) {
        set_error("%s: at least 2 rows, got %lld", who, (long long)n);
        return BYZ_E_INVALID;
    }
    if (method != BYZ_LINKAGE_AVERAGE && method != BYZ_LINKAGE_COMPLETE && method != BYZ_LINKAGE_SINGLE) {
        set_error("%s: method = %d is none of average (0), complete (1), single (2)", who, method);
        return BYZ_E_INVALID;
    }
    if (!fill || !std::isfinite(*fill) || !(*fill >= 0.0)) {
        set_error("%s: fill = %g must be finite and >= 0", who, fill ? *fill : 0.0);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

int check_clipped_clustering(const char* who, const byz_clipped_clustering_params* params, int64_t n_rows) {
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    if (!params->adaptive && !(params->clip > 0.0)) {      // (a NaN fails; +inf passes, as weak DP's clip)
        set_error("%s: clip = %g must be > 0 in the fixed mode", who, params->clip);
        return BYZ_E_INVALID;
    }
    return check_linkage(who, n_rows, params->method, &params->fill);
}

// The whole call; allreduce == nullptr: one GPU holds every column.  It waits where flame() waits: inside the Gram's duplicate
// search, and nowhere when the caller passes the distances.
int clipped_clustering(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, const byz_clipped_clustering_params* params,
                       byz_allreduce_f64_fn allreduce, void* user, const float* dist_in, const double* sq_in, float* out,
                       int32_t* admitted_out, void* stream) {
    hipStream_t s = as_stream(stream);
    LinkageScratch f;
    BYZ_TRY(linkage_workspace(ctx, n, &f));
    RowScratch t;
    BYZ_TRY(row_scratch(ctx, n, n_cols, &t));
    double* scale = t.b;
    mark(ctx, kReportLinkage, s);
    mark(ctx, kReportClippedClustering, s);
    mark(ctx, kReportWeakDp, s);
    const float* dist = dist_in;
    if (dist == nullptr) {
        BYZ_TRY(ctx->dist.ensure(static_cast<size_t>(n) * n * sizeof(float)));
        BYZ_TRY(cosine_distances(ctx, G, n, n_cols, ld, allreduce, user, ctx->dist.as<float>(), stream));
        dist = ctx->dist.as<float>();
    }
    BYZ_TRY(launch_clipped_clustering_select(ctx, f, dist, n, params->method, params->fill, admitted_out, s));
    BYZ_HIP(hipMemsetAsync(out, 0, static_cast<size_t>(n_cols) * sizeof(float), s));
    const double* sq = sq_in;
    if (sq == nullptr) {
        BYZ_TRY(launch_row_sqdist(ctx, G, n, n_cols, ld, out, t.partials, t.a, nullptr, nullptr, s));
        if (allreduce != nullptr) BYZ_TRY(reduce_over_ranks(allreduce, user, t.a, n, stream, "clipped_clustering (norms)"));
        sq = t.a;
    }
    BYZ_TRY(launch_clip_scales(ctx, sq, n, params->clip, params->adaptive != 0, scale, &f.info->clip, s));
    BYZ_TRY(launch_flame_weights(ctx, f.admitted, scale, n, f.w, s));
    return launch_scaled_rows_sum(ctx, G, n, n_cols, ld, f.w, &f.info->admitted_f64, out, s);
}

}  // namespace

int byz_linkage_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int method, const double* fill, int32_t* pair, double* height,
                    int32_t* size, int32_t* usable_rows, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist && pair && height && size, "linkage: null distances or output");
    BYZ_TRY(check_linkage("linkage", n_rows, method, fill));
    LinkageScratch f;
    BYZ_TRY(linkage_workspace(ctx, n_rows, &f));
    mark(ctx, kReportLinkage, as_stream(stream));
    ctx->last[kReportClippedClustering].stream = as_stream(stream);   // (one LinkageInfo: its other info call follows the last writer too)
    return launch_linkage(ctx, f, dist, n_rows, method, *fill, pair, height, size, usable_rows, as_stream(stream));
}

int byz_linkage_info(byz_ctx* ctx, int64_t* merges, int64_t* rescans, int64_t* max_rescans) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportLinkage, "linkage_info: no linkage on this context yet", &all));
    const LinkageInfo& info = all.linkage;
    if (merges) *merges = info.steps;
    if (rescans) *rescans = info.rescans;
    if (max_rescans) *max_rescans = info.max_rescans;
    return BYZ_OK;
}

int byz_linkage_cut_dev(byz_ctx* ctx, const int32_t* pair, int64_t n_rows, const int32_t* usable_rows, int64_t n_clusters,
                        int32_t* labels, int32_t* cluster_sizes, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(pair && usable_rows && labels && cluster_sizes, "linkage_cut: null merges, flags or output");
    BYZ_TRY(check_owned_rows("linkage_cut", n_rows));
    BYZ_REQUIRE(n_rows >= 2 && n_clusters >= 1 && n_clusters <= n_rows, "linkage_cut: %lld clusters of %lld rows (at least 2 rows, 1..n clusters)",
                (long long)n_clusters, (long long)n_rows);
    return launch_linkage_cut(ctx, pair, n_rows, usable_rows, n_clusters, labels, cluster_sizes, as_stream(stream));
}

int byz_clipped_clustering_select_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int method, const double* fill,
                                      int32_t* admitted, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist && admitted, "clipped_clustering_select: null distances or output");
    BYZ_TRY(check_linkage("clipped_clustering_select", n_rows, method, fill));
    LinkageScratch f;
    BYZ_TRY(linkage_workspace(ctx, n_rows, &f));
    mark(ctx, kReportLinkage, as_stream(stream));
    mark(ctx, kReportClippedClustering, as_stream(stream));
    BYZ_HIP(hipMemsetAsync(&f.info->clip, 0, sizeof(double), as_stream(stream)));
    return launch_clipped_clustering_select(ctx, f, dist, n_rows, method, *fill, admitted, as_stream(stream));
}

int byz_clipped_clustering_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                               const byz_clipped_clustering_params* params, const float* dist, const double* sq, float* out,
                               int32_t* admitted, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "clipped_clustering"));
    BYZ_REQUIRE(out, "clipped_clustering: null output");
    BYZ_TRY(check_clipped_clustering("clipped_clustering", params, n_rows));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "clipped_clustering"));
    return clipped_clustering(ctx, G, n_rows, n_cols, ld, params, nullptr, nullptr, dist, sq, out, admitted, stream);
}

int byz_clipped_clustering_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld,
                                       const byz_clipped_clustering_params* params, byz_allreduce_f64_fn allreduce, void* user,
                                       const float* dist, float* out, int32_t* admitted, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "clipped_clustering_sharded"));
    BYZ_REQUIRE(out && allreduce, "clipped_clustering_sharded: null output or null all-reduce");
    BYZ_TRY(check_clipped_clustering("clipped_clustering_sharded", params, n_rows));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "clipped_clustering_sharded"));
    return clipped_clustering(ctx, G, n_rows, n_cols, ld, params, allreduce, user, dist, nullptr, out, admitted, stream);
}

int byz_clipped_clustering_info(byz_ctx* ctx, int64_t* admitted_rows, int64_t* usable_rows, double* top_height, double* second_height,
                                double* clip) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportClippedClustering, "clipped_clustering_info: no ClippedClustering selection on this context yet", &all));
    const LinkageInfo& info = all.linkage;
    if (admitted_rows) *admitted_rows = info.admitted;
    if (usable_rows) *usable_rows = info.usable;
    if (top_height) *top_height = info.top_height;
    if (second_height) *second_height = info.second_height;
    if (clip) *clip = info.clip;
    return BYZ_OK;
}

// ---- FABA (Xia, Chen, Yu & Ma, IJCAI 2019; beyond the reference) ------------------------------------------------------------------
namespace {

int check_faba(const char* who, int64_t n, int64_t remove_count, int power) {
    BYZ_TRY(check_owned_rows(who, n));
    if (n < 2) {
        set_error("%s: at least 2 rows, got %lld", who, (long long)n);
        return BYZ_E_INVALID;
    }
    if (remove_count < 0 || remove_count > n - 1) {
        set_error("%s: remove_count = %lld outside 0..n - 1 (n = %lld)", who, (long long)remove_count, (long long)n);
        return BYZ_E_INVALID;
    }
    if (power != 1 && power != 2) {
        set_error("%s: power = %d is neither 1 (the distances) nor 2 (their squares)", who, power);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

}  // namespace

int byz_faba_select_dev(byz_ctx* ctx, const float* dist, int64_t n_rows, int64_t remove_count, int power, int32_t* kept,
                        int32_t* order, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist && kept, "faba_select: null distances or output");
    BYZ_TRY(check_faba("faba_select", n_rows, remove_count, power));
    FabaScratch f;
    BYZ_TRY(faba_workspace(ctx, n_rows, &f));
    mark(ctx, kReportFaba, as_stream(stream));
    return launch_faba_select(ctx, f, dist, n_rows, remove_count, power, kept, order, as_stream(stream));
}

// It waits where byz_pairwise_distances_dev waits (the Gram's duplicate search), and nowhere when the caller passes the distances.
int byz_faba_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t remove_count, const float* dist_in,
                 float* out, int32_t* kept, int32_t* order, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "faba"));
    BYZ_REQUIRE(out, "faba: null output");
    BYZ_TRY(check_faba("faba", n_rows, remove_count, 2));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "faba"));
    hipStream_t s = as_stream(stream);
    FabaScratch f;
    BYZ_TRY(faba_workspace(ctx, n_rows, &f));
    mark(ctx, kReportFaba, s);
    const float* dist = dist_in;
    if (dist == nullptr) {
        BYZ_TRY(ensure_distance_workspaces(ctx, n_rows));
        BYZ_TRY(distances(ctx, G, n_rows, n_cols, ld, nullptr, nullptr, ctx->dist.as<float>(), stream));
        dist = ctx->dist.as<float>();
    }
    BYZ_TRY(launch_faba_select(ctx, f, dist, n_rows, remove_count, 2, kept, order, s));
    return launch_scaled_rows_sum(ctx, G, n_rows, n_cols, ld, f.w, &f.info->kept_f64, out, s);
}

int byz_faba_info(byz_ctx* ctx, int64_t* removed_rows, int64_t* kept_rows, int64_t* forced_rows, double* last_score, double* divisor) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportFaba, "faba_info: no FABA selection on this context yet", &all));
    const FabaReport& info = all.faba;
    if (removed_rows) *removed_rows = info.removed;
    if (kept_rows) *kept_rows = info.kept;
    if (forced_rows) *forced_rows = info.forced;
    if (last_score) *last_score = info.last_score;
    if (divisor) *divisor = info.kept_f64;
    return BYZ_OK;
}

// ---- AFA (Munoz-Gonzalez, Co & Lupu, arXiv:1909.05125; beyond the reference) -----------------------------------------------------
namespace {

int check_afa(const char* who, int64_t n, const byz_afa_params* params) {
    BYZ_TRY(check_owned_rows(who, n));
    if (n < 2) {
        set_error("%s: at least 2 rows, got %lld", who, (long long)n);
        return BYZ_E_INVALID;
    }
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    if (!(std::isfinite(params->xi0) && params->xi0 >= 0.0 && std::isfinite(params->delta_xi) && params->delta_xi >= 0.0) ||
        params->max_rounds < 0) {
        set_error("%s: xi0 = %g and delta_xi = %g must be finite and >= 0, max_rounds = %lld >= 0", who, params->xi0, params->delta_xi,
                  (long long)params->max_rounds);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

}  // namespace

int byz_afa_select_dev(byz_ctx* ctx, const double* gram, int64_t n_rows, const double* weights, const byz_afa_params* params,
                       int32_t* kept, int32_t* round_of, double* score, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(gram && kept, "afa_select: null Gram or output");
    BYZ_TRY(check_afa("afa_select", n_rows, params));
    AfaScratch a;
    BYZ_TRY(afa_workspace(ctx, n_rows, &a));
    mark(ctx, kReportAfa, as_stream(stream));
    return launch_afa_select(ctx, a, gram, n_rows, weights, params->xi0, params->delta_xi, params->max_rounds, kept, round_of, score,
                             as_stream(stream));
}

// It waits where byz_gram_dev waits (the Gram's duplicate search), and nowhere when the caller passes the Gram.
int byz_afa_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const double* weights,
                const byz_afa_params* params, const double* gram_in, float* out, int32_t* kept, int32_t* round_of, double* score,
                void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "afa"));
    BYZ_REQUIRE(out, "afa: null output");
    BYZ_TRY(check_afa("afa", n_rows, params));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "afa"));
    hipStream_t s = as_stream(stream);
    AfaScratch a;
    BYZ_TRY(afa_workspace(ctx, n_rows, &a));
    mark(ctx, kReportAfa, s);
    const double* gram = gram_in;
    if (gram == nullptr) {
        BYZ_TRY(ctx->gram.ensure(static_cast<size_t>(n_rows) * n_rows * sizeof(double)));
        BYZ_TRY(launch_gram(ctx, G, n_rows, n_cols, ld, ctx->gram.as<double>(), s));
        gram = ctx->gram.as<double>();
    }
    BYZ_TRY(launch_afa_select(ctx, a, gram, n_rows, weights, params->xi0, params->delta_xi, params->max_rounds, kept, round_of, score, s));
    return launch_scaled_rows_sum(ctx, G, n_rows, n_cols, ld, a.w, &a.info->divisor, out, s);
}

int byz_afa_info(byz_ctx* ctx, int64_t* counts6, double* stats4, double* divisor) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportAfa, "afa_info: no AFA selection on this context yet", &all));
    const AfaReport& info = all.afa;
    if (counts6) {
        const int32_t counts[6] = {info.rounds, info.kept, info.removed, info.excluded, info.branch, info.degenerate};
        for (int i = 0; i < 6; ++i) counts6[i] = counts[i];
    }
    if (stats4) {
        stats4[0] = info.mean;
        stats4[1] = info.med;
        stats4[2] = info.sd;
        stats4[3] = info.thr;
    }
    if (divisor) *divisor = info.divisor;
    return BYZ_OK;
}

// ---- Auror (Shen, Tople & Saxena, ACSAC 2016; beyond the reference) ---------------------------------------------------------------
namespace {

int check_auror(const char* who, int64_t n, const byz_auror_params* params) {
    if (n > kAurorMaxRows) {
        set_error("%s: at most %lld rows, got %lld", who, (long long)kAurorMaxRows, (long long)n);
        return BYZ_E_UNSUPPORTED;
    }
    if (n < 1) {
        set_error("%s: at least 1 row, got %lld", who, (long long)n);
        return BYZ_E_INVALID;
    }
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    if (!(std::isfinite(params->alpha) && params->alpha >= 0.0 && params->tau >= 0.0 && params->tau <= 1.0) || params->max_iter < 1 ||
        (params->accumulate != 0 && params->accumulate != 1)) {
        set_error("%s: alpha = %g must be finite and >= 0, 0 <= tau = %g <= 1, max_iter = %lld >= 1, accumulate = %lld 0 or 1", who,
                  params->alpha, params->tau, (long long)params->max_iter, (long long)params->accumulate);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

long long* as_ll(int64_t* p) { return reinterpret_cast<long long*>(p); }
const long long* as_const_ll(const int64_t* p) { return reinterpret_cast<const long long*>(p); }

}  // namespace

int byz_auror_votes_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_auror_params* params,
                        int64_t* votes, int32_t* bad, int64_t* counts, double* gap, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "auror_votes"));
    BYZ_REQUIRE(votes && bad && counts, "auror_votes: null votes, bad flags or counts");
    BYZ_TRY(check_auror("auror_votes", n_rows, params));
    return launch_auror_votes(ctx, G, n_rows, n_cols, ld, params->alpha, params->max_iter, params->accumulate != 0, as_ll(votes), bad,
                              as_ll(counts), gap, as_stream(stream));
}

int byz_auror_select_dev(byz_ctx* ctx, const int64_t* votes, const int32_t* bad, const int64_t* counts, int64_t n_rows,
                         const byz_auror_params* params, int32_t* kept, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(votes && bad && counts && kept, "auror_select: null votes, bad flags, counts or output");
    BYZ_TRY(check_auror("auror_select", n_rows, params));
    AurorScratch a;
    BYZ_TRY(auror_workspace(ctx, n_rows, &a));
    mark(ctx, kReportAuror, as_stream(stream));
    return launch_auror_select(ctx, a, as_const_ll(votes), bad, as_const_ll(counts), n_rows, params->tau, kept, as_stream(stream));
}

int byz_auror_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_auror_params* params,
                  int64_t* votes, int32_t* bad, int64_t* counts, float* out, int32_t* kept, double* gap, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "auror"));
    BYZ_REQUIRE(out, "auror: null output");
    BYZ_TRY(check_auror("auror", n_rows, params));
    const bool history = votes != nullptr;
    BYZ_REQUIRE((bad != nullptr) == history && (counts != nullptr) == history, "auror: votes, bad flags and counts come together or not at all");
    BYZ_REQUIRE(history || params->accumulate == 0, "auror: accumulate = 1 needs the caller's votes, bad flags and counts");
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "auror"));
    hipStream_t s = as_stream(stream);
    AurorScratch a;
    BYZ_TRY(auror_workspace(ctx, n_rows, &a));
    mark(ctx, kReportAuror, s);
    long long* v = history ? as_ll(votes) : a.votes;
    long long* c = history ? as_ll(counts) : a.counts;
    int32_t* b = history ? bad : a.bad;
    BYZ_TRY(launch_auror_votes(ctx, G, n_rows, n_cols, ld, params->alpha, params->max_iter, params->accumulate != 0, v, b, c, gap, s));
    BYZ_TRY(launch_auror_select(ctx, a, v, b, c, n_rows, params->tau, kept, s));
    return launch_scaled_rows_sum(ctx, G, n_rows, n_cols, ld, a.w, &a.info->kept_f64, out, s);
}

int byz_auror_info(byz_ctx* ctx, int64_t* indicative, int64_t* removed_rows, int64_t* kept_rows, int64_t* bad_rows, int64_t* capped_cols) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportAuror, "auror_info: no Auror selection on this context yet", &all));
    const AurorReport& info = all.auror;
    if (indicative) *indicative = info.indicative;
    if (removed_rows) *removed_rows = info.removed;
    if (kept_rows) *kept_rows = info.kept;
    if (bad_rows) *bad_rows = info.bad_rows;
    if (capped_cols) *capped_cols = info.capped;
    return BYZ_OK;
}

// ---- FoolsGold (Fung, Yoon & Beschastnikh, arXiv:1808.04866; beyond the reference) -----------------------------------------------
namespace {

int check_foolsgold(const char* who, int64_t n, const byz_foolsgold_params* params) {
    if (n < 1) {
        set_error("%s: at least 1 row, got %lld", who, (long long)n);
        return BYZ_E_INVALID;
    }
    BYZ_TRY(check_row_ceiling(who, n));
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    if (!(std::isfinite(params->kappa) && params->kappa > 0.0) ||
        (params->normalise != BYZ_FOOLSGOLD_NORMALISE_COUNT && params->normalise != BYZ_FOOLSGOLD_NORMALISE_SUM)) {
        set_error("%s: kappa = %g must be finite and > 0, normalise = %lld one of 0 (count) and 1 (sum)", who, params->kappa,
                  (long long)params->normalise);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

// the window [col_start, col_start + col_count) inside n_cols columns, and the history beside it
int check_foolsgold_window(const char* who, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* H, int64_t ld_h,
                           int64_t col_start, int64_t col_count) {
    if (col_start < 0 || col_count < 1 || col_start > n_cols - col_count) {
        set_error("%s: the window [%lld, %lld + %lld) lies outside the %lld columns", who, (long long)col_start, (long long)col_start,
                  (long long)col_count, (long long)n_cols);
        return BYZ_E_INVALID;
    }
    if (H != nullptr) {
        if (ld_h < col_count) {
            set_error("%s: the history's ld %lld is below its %lld columns", who, (long long)ld_h, (long long)col_count);
            return BYZ_E_INVALID;
        }
        const float* g_end = G + (n_rows - 1) * ld + n_cols;
        const float* h_end = H + (n_rows - 1) * ld_h + col_count;
        if (H < g_end && h_end > G) {
            set_error("%s: the history overlaps the matrix", who);
            return BYZ_E_INVALID;
        }
    }
    return BYZ_OK;
}

}  // namespace

int byz_rows_add_dev(byz_ctx* ctx, float* H, int64_t ld_h, const float* G, int64_t n_rows, int64_t n_cols_window, int64_t ld_g,
                     int64_t col_start, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(H && G && n_rows >= 1 && n_cols_window >= 1 && col_start >= 0 && ld_h >= n_cols_window &&
                    ld_g >= col_start + n_cols_window,
                "rows_add: bad arguments (%lld x %lld from column %lld, ld %lld and %lld)", (long long)n_rows, (long long)n_cols_window,
                (long long)col_start, (long long)ld_h, (long long)ld_g);
    BYZ_TRY(check_foolsgold_window("rows_add", G, n_rows, col_start + n_cols_window, ld_g, H, ld_h, col_start, n_cols_window));
    return launch_rows_add(ctx, H, ld_h, G + col_start, n_rows, n_cols_window, ld_g, as_stream(stream));
}

int byz_foolsgold_weights_dev(byz_ctx* ctx, const double* gram, int64_t n_rows, const byz_foolsgold_params* params, double* weights,
                              double* maxcs, double* alpha, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(gram && weights, "foolsgold_weights: null Gram or output");
    BYZ_TRY(check_foolsgold("foolsgold_weights", n_rows, params));
    FoolsgoldScratch t;
    BYZ_TRY(foolsgold_workspace(ctx, n_rows, &t));
    mark(ctx, kReportFoolsgold, as_stream(stream));
    ctx->foolsgold_rows = n_rows;
    return launch_foolsgold_weights(ctx, t, gram, n_rows, params->kappa, static_cast<int>(params->normalise), weights, maxcs, alpha,
                                    as_stream(stream));
}

int byz_foolsgold_trace_dev(byz_ctx* ctx, int64_t n_rows, double* rescaled, int32_t* usable, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(ctx->last[kReportFoolsgold].ran && n_rows == ctx->foolsgold_rows,
                "foolsgold_trace: the last FoolsGold weights on this context had %lld rows, not %lld", (long long)ctx->foolsgold_rows,
                (long long)n_rows);
    FoolsgoldScratch t;
    BYZ_TRY(foolsgold_workspace(ctx, n_rows, &t));      // (the same layout in the same buffer: nothing grows)
    hipStream_t s = as_stream(stream);
    if (rescaled) BYZ_HIP(hipMemcpyAsync(rescaled, t.rescaled, static_cast<size_t>(n_rows) * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (usable) BYZ_HIP(hipMemcpyAsync(usable, t.flags, static_cast<size_t>(n_rows) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return BYZ_OK;
}

// It waits where byz_gram_dev waits (the Gram's duplicate search), and nowhere when the caller passes the Gram.
int byz_foolsgold_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, float* H, int64_t ld_h,
                      int64_t col_start, int64_t col_count, const byz_foolsgold_params* params, const double* gram_in, float* out,
                      double* weights, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "foolsgold"));
    BYZ_REQUIRE(out, "foolsgold: null output");
    BYZ_TRY(check_foolsgold("foolsgold", n_rows, params));
    BYZ_TRY(check_foolsgold_window("foolsgold", G, n_rows, n_cols, ld, H, ld_h, col_start, col_count));
    BYZ_TRY(check_cclip_output(G, n_rows, n_cols, ld, out, "foolsgold"));
    if (H != nullptr) BYZ_TRY(check_cclip_output(H, n_rows, col_count, ld_h, out, "foolsgold"));
    hipStream_t s = as_stream(stream);
    FoolsgoldScratch t;
    BYZ_TRY(foolsgold_workspace(ctx, n_rows, &t));
    mark(ctx, kReportFoolsgold, s);
    ctx->foolsgold_rows = n_rows;
    if (H != nullptr) BYZ_TRY(launch_rows_add(ctx, H, ld_h, G + col_start, n_rows, col_count, ld, s));
    const double* gram = gram_in;
    if (gram == nullptr) {
        BYZ_TRY(ctx->gram.ensure(static_cast<size_t>(n_rows) * n_rows * sizeof(double)));
        if (H != nullptr) BYZ_TRY(launch_gram(ctx, H, n_rows, col_count, ld_h, ctx->gram.as<double>(), s));
        else BYZ_TRY(launch_gram(ctx, G + col_start, n_rows, col_count, ld, ctx->gram.as<double>(), s));
        gram = ctx->gram.as<double>();
    }
    BYZ_TRY(launch_foolsgold_weights(ctx, t, gram, n_rows, params->kappa, static_cast<int>(params->normalise), weights, nullptr, nullptr, s));
    return launch_scaled_rows_sum(ctx, G, n_rows, n_cols, ld, t.w, &t.info->divisor, out, s);
}

int byz_foolsgold_info(byz_ctx* ctx, int64_t* counts5, double* stats2) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportFoolsgold, "foolsgold_info: no FoolsGold weights on this context yet", &all));
    const FoolsgoldReport& info = all.foolsgold;
    if (counts5) {
        const int32_t counts[5] = {info.usable, info.excluded, info.at_zero, info.at_one, info.degenerate};
        for (int i = 0; i < 5; ++i) counts5[i] = counts[i];
    }
    if (stats2) {
        stats2[0] = info.top;
        stats2[1] = info.divisor;
    }
    return BYZ_OK;
}

// ---- Multi-Metrics (Huang et al., ICCV 2023; beyond the reference) ------------------------------------------------------------
namespace {

int check_mm_keep(const char* who, int64_t n, int64_t keep) {
    BYZ_TRY(check_owned_rows(who, n));
    if (n < 1 || keep < 1 || keep > n) {
        set_error("%s: keep = %lld outside 1..%lld (the row count)", who, (long long)keep, (long long)n);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

// the L1 sums of G's rows into the workspace's n x n doubles (with an all-reduce: of the ranks' column slices), then dist
int manhattan_distances(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, byz_allreduce_f64_fn allreduce, void* user,
                        float* dist, void* stream) {
    hipStream_t s = as_stream(stream);
    double *partial, *sums;
    BYZ_TRY(manhattan_workspace(ctx, n, n_cols, &partial, &sums));
    BYZ_TRY(launch_manhattan_sums(ctx, G, n, n_cols, ld, partial, sums, s));
    if (allreduce != nullptr) BYZ_TRY(reduce_over_ranks(allreduce, user, sums, n * n, stream, "multi_metrics (L1 sums)"));
    return launch_manhattan_from_sums(ctx, sums, n, dist, s);
}

// The whole call; allreduce == nullptr: one GPU holds every column.  ONE Gram serves the Euclidean and the cosine matrix: the
// distances' own path leaves it in ctx->gram untouched (launch_distances_from_gram reads it), and cosine_from_gram reads the
// same doubles byz_cosine_distances_dev would have computed, launch_gram being deterministic.  Where the Euclidean matrix
// comes from the small-N kernel, which forms no Gram, the Gram is computed here for the cosine matrix alone -- once, either way.
// Sharded: the Gram's all-reduce (and the near pairs', when there are any) inside the distances, then the L1 sums'.
int multi_metrics(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, int64_t keep, byz_allreduce_f64_fn allreduce,
                  void* user, float* out, int32_t* flags_out, void* stream) {
    hipStream_t s = as_stream(stream);
    MmScratch t;
    BYZ_TRY(multi_metrics_workspace(ctx, n, true, &t));
    BYZ_TRY(ensure_distance_workspaces(ctx, n));
    mark(ctx, kReportMultiMetrics, s);
    float* euc = ctx->dist.as<float>();
    double* gram = ctx->gram.as<double>();
    BYZ_TRY(distances(ctx, G, n, n_cols, ld, allreduce, user, euc, stream));
    if (allreduce == nullptr && krum_small_applies(n, n_cols)) BYZ_TRY(launch_gram(ctx, G, n, n_cols, ld, gram, s));
    BYZ_TRY(launch_cosine_from_gram(ctx, gram, n, t.cos, s));
    BYZ_TRY(launch_mm_usable_from_gram(ctx, gram, n, t.usable, s));
    BYZ_TRY(manhattan_distances(ctx, G, n, n_cols, ld, allreduce, user, t.man, stream));
    BYZ_TRY(launch_mm_features(ctx, t.man, euc, t.cos, t.usable, n, t.feat, s));
    BYZ_TRY(launch_mm_select(ctx, t, t.feat, n, keep, flags_out, nullptr, s));
    // sharded: the selection is the same on every rank; each rank averages its own columns of the chosen rows
    BYZ_TRY(launch_column_mean_rows_counted(ctx, G, t.rows, t.count, n_cols, ld, out, s));
    return launch_mm_zero_if_empty(ctx, t.count, n_cols, out, s);
}

int check_multi_metrics(const char* who, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t keep, const float* out) {
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, who));
    BYZ_REQUIRE(out, "%s: null output", who);
    BYZ_TRY(check_mm_keep(who, n_rows, keep));
    return check_cclip_output(G, n_rows, n_cols, ld, out, who);
}

}  // namespace

int byz_manhattan_distances_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, float* dist, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "manhattan_distances"));
    BYZ_REQUIRE(dist, "manhattan_distances: null output");
    BYZ_TRY(check_owned_rows("manhattan_distances", n_rows));
    return manhattan_distances(ctx, G, n_rows, n_cols, ld, nullptr, nullptr, dist, stream);
}

int byz_manhattan_sums_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, double* sums, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "manhattan_sums"));
    BYZ_REQUIRE(sums, "manhattan_sums: null output");
    BYZ_TRY(check_owned_rows("manhattan_sums", n_rows));
    double *partial, *unused;
    BYZ_TRY(manhattan_workspace(ctx, n_rows, n_cols, &partial, &unused));
    return launch_manhattan_sums(ctx, G, n_rows, n_cols, ld, partial, sums, as_stream(stream));
}

int byz_manhattan_from_sums_dev(byz_ctx* ctx, const double* sums, int64_t n_rows, float* dist, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(sums && dist && n_rows > 0, "manhattan_from_sums: null sums or output, or no rows (%lld)", (long long)n_rows);
    BYZ_TRY(check_owned_rows("manhattan_from_sums", n_rows));
    return launch_manhattan_from_sums(ctx, sums, n_rows, dist, as_stream(stream));
}

int byz_multi_metrics_features_dev(byz_ctx* ctx, const float* man, const float* euc, const float* cos, int64_t n_rows, double* features,
                                   void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(man && euc && cos && features && n_rows > 0, "multi_metrics_features: a null matrix or output, or no rows (%lld)",
                (long long)n_rows);
    BYZ_TRY(check_owned_rows("multi_metrics_features", n_rows));
    MmScratch t;
    BYZ_TRY(multi_metrics_workspace(ctx, n_rows, false, &t));
    BYZ_TRY(launch_mm_usable_from_cos(ctx, cos, n_rows, t.usable, as_stream(stream)));
    return launch_mm_features(ctx, man, euc, cos, t.usable, n_rows, features, as_stream(stream));
}

int byz_multi_metrics_select_dev(byz_ctx* ctx, const double* features, int64_t n_rows, int64_t keep, int32_t* flags, double* scores,
                                 void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(features && flags, "multi_metrics_select: null features or output");
    BYZ_TRY(check_mm_keep("multi_metrics_select", n_rows, keep));
    MmScratch t;
    BYZ_TRY(multi_metrics_workspace(ctx, n_rows, false, &t));
    mark(ctx, kReportMultiMetrics, as_stream(stream));
    return launch_mm_select(ctx, t, features, n_rows, keep, flags, scores, as_stream(stream));
}

int byz_multi_metrics_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t keep, float* out,
                          int32_t* flags, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_multi_metrics("multi_metrics", G, n_rows, n_cols, ld, keep, out));
    return multi_metrics(ctx, G, n_rows, n_cols, ld, keep, nullptr, nullptr, out, flags, stream);
}

int byz_multi_metrics_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t keep,
                                  byz_allreduce_f64_fn allreduce, void* user, float* out, int32_t* flags, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_multi_metrics("multi_metrics_sharded", G, n_rows, n_cols, ld, keep, out));
    BYZ_REQUIRE(allreduce, "multi_metrics_sharded: null all-reduce");
    return multi_metrics(ctx, G, n_rows, n_cols, ld, keep, allreduce, user, out, flags, stream);
}

int byz_multi_metrics_info(byz_ctx* ctx, int64_t* kept_rows, int64_t* usable_rows, int32_t* degenerate, double* det) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportMultiMetrics, "multi_metrics_info: no Multi-Metrics selection on this context yet", &all));
    const MmInfo& info = all.mm;
    if (kept_rows) *kept_rows = info.kept;
    if (usable_rows) *usable_rows = info.usable;
    if (degenerate) *degenerate = info.degenerate;
    if (det) *det = info.det;
    return BYZ_OK;
}

// ---- DnC, the spectral defence (Shejwalkar & Houmansadr 2021, Algorithm 2; beyond the reference) ----------------------------
namespace {

int check_dnc(const byz_dnc_params* params, int64_t n_rows, int64_t n_cols, const char* who) {
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    if (params->n_iters < 1 || params->sub_dim < 1 || params->sub_dim > n_cols || params->power_iters < 0 ||
        params->remove_count < 0 || params->remove_count > n_rows - 1) {
        set_error("%s: n_iters = %lld must be >= 1, sub_dim = %lld in 1..%lld (the columns), power_iters = %lld >= 0, remove_count = "
                  "%lld in 0..%lld", who, (long long)params->n_iters, (long long)params->sub_dim, (long long)n_cols,
                  (long long)params->power_iters, (long long)params->remove_count, (long long)(n_rows - 1));
        return BYZ_E_INVALID;
    }
    BYZ_TRY(check_row_ceiling(who, n_rows));
    if (params->sub_dim > BYZ_DNC_MAX_SAMPLED / n_rows) {
        set_error("%s: %lld rows x %lld sampled columns exceed the workspace bound of %lld values", who, (long long)n_rows,
                  (long long)params->sub_dim, (long long)BYZ_DNC_MAX_SAMPLED);
        return BYZ_E_UNSUPPORTED;
    }
    // every product's launches are enqueued up front
    if (params->power_iters + 1 > BYZ_DNC_MAX_PRODUCTS / params->n_iters) {
        set_error("%s: n_iters * (power_iters + 1) = %lld * %lld beyond %d", who, (long long)params->n_iters,
                  (long long)(params->power_iters + 1), BYZ_DNC_MAX_PRODUCTS);
        return BYZ_E_UNSUPPORTED;
    }
    return BYZ_OK;
}

// The selection of the whole call into the workspace (t.good, the count in the context's word); local_counts == nullptr: every
// iteration has params->sub_dim columns.  Nothing here waits for the device.
int dnc_select(byz_ctx* ctx, const float* G, int64_t n, int64_t ld, const byz_dnc_params* params, const int64_t* columns,
               const int64_t* local_counts, byz_allreduce_f64_fn allreduce, void* user, int32_t* good_out, int32_t* count_out,
               DncScratch* t, void* stream) {
    hipStream_t s = as_stream(stream);
    int64_t widest = local_counts ? 0 : params->sub_dim;
    if (local_counts)
        for (int64_t k = 0; k < params->n_iters; ++k) {
            BYZ_REQUIRE(local_counts[k] >= 0 && local_counts[k] <= params->sub_dim, "dnc: local count %lld of iteration %lld outside 0..%lld",
                        (long long)local_counts[k], (long long)k, (long long)params->sub_dim);
            widest = local_counts[k] > widest ? local_counts[k] : widest;
        }
    BYZ_REQUIRE(columns || widest == 0, "dnc: null column list");
    BYZ_TRY(dnc_workspace(ctx, n, widest, t));
    mark(ctx, kReportDnc, s);
    const int64_t n_keep = n - params->remove_count;
    const int64_t* cols = columns;
    for (int64_t k = 0; k < params->n_iters; ++k) {
        const int64_t b = local_counts ? local_counts[k] : params->sub_dim;
        BYZ_TRY(launch_dnc_scores(ctx, *t, G, n, ld, cols, b, params->power_iters, allreduce, user, stream));
        BYZ_TRY(launch_dnc_rank(ctx, *t, n, n_keep, k == 0, s));
        cols += b;
    }
    return launch_dnc_compact(ctx, *t, n, good_out, count_out, s);
}

int dnc(byz_ctx* ctx, const float* G, int64_t n, int64_t n_cols, int64_t ld, const byz_dnc_params* params, const int64_t* columns,
        const int64_t* local_counts, byz_allreduce_f64_fn allreduce, void* user, float* out, int32_t* good_out, void* stream) {
    DncScratch t;
    BYZ_TRY(dnc_select(ctx, G, n, ld, params, columns, local_counts, allreduce, user, good_out, nullptr, &t, stream));
    // the kept rows are known on the device alone: the row-list mean reads their count there
    return launch_column_mean_rows_counted(ctx, G, t.good, &device_scalars(ctx)->dnc.kept, n_cols, ld, out, as_stream(stream));
}

}  // namespace

int byz_dnc_scores_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int64_t* columns,
                       int64_t sub_dim, int64_t power_iters, double* scores, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "dnc_scores"));
    BYZ_REQUIRE(columns && scores, "dnc_scores: null column list or output");
    const byz_dnc_params params = {1, sub_dim, power_iters, 0};
    BYZ_TRY(check_dnc(&params, n_rows, n_cols, "dnc_scores"));
    DncScratch t;
    BYZ_TRY(dnc_workspace(ctx, n_rows, sub_dim, &t));
    BYZ_TRY(launch_dnc_scores(ctx, t, G, n_rows, ld, columns, sub_dim, power_iters, nullptr, nullptr, stream));
    BYZ_HIP(hipMemcpyAsync(scores, t.scores, static_cast<size_t>(n_rows) * sizeof(double), hipMemcpyDeviceToDevice, as_stream(stream)));
    return BYZ_OK;
}

int byz_dnc_select_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_dnc_params* params,
                       const int64_t* columns, int32_t* good, int32_t* count, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "dnc_select"));
    BYZ_REQUIRE(columns && good, "dnc_select: null column list or output");
    BYZ_TRY(check_dnc(params, n_rows, n_cols, "dnc_select"));
    DncScratch t;
    return dnc_select(ctx, G, n_rows, ld, params, columns, nullptr, nullptr, nullptr, good, count, &t, stream);
}

int byz_dnc_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_dnc_params* params,
                const int64_t* columns, float* out, int32_t* good, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "dnc"));
    BYZ_REQUIRE(columns && out, "dnc: null column list or output");
    BYZ_TRY(check_dnc(params, n_rows, n_cols, "dnc"));
    return dnc(ctx, G, n_rows, n_cols, ld, params, columns, nullptr, nullptr, nullptr, out, good, stream);
}

int byz_dnc_sharded_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_dnc_params* params,
                        const int64_t* columns_local, const int64_t* local_counts, byz_allreduce_f64_fn allreduce, void* user,
                        float* out, int32_t* good, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "dnc_sharded"));
    BYZ_REQUIRE(out && allreduce && local_counts, "dnc_sharded: null output, all-reduce or local counts");
    // (sub_dim is the global figure here: it may exceed this rank's columns, the local counts may not)
    BYZ_TRY(check_dnc(params, n_rows, INT64_MAX, "dnc_sharded"));
    for (int64_t k = 0; k < params->n_iters; ++k)
        BYZ_REQUIRE(local_counts[k] <= n_cols, "dnc_sharded: %lld local columns of %lld", (long long)local_counts[k], (long long)n_cols);
    return dnc(ctx, G, n_rows, n_cols, ld, params, columns_local, local_counts, allreduce, user, out, good, stream);
}

int byz_dnc_info(byz_ctx* ctx, int64_t* kept_rows, int64_t* inactive_rows) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportDnc, nullptr, &all));
    if (kept_rows) *kept_rows = all.dnc.kept;
    if (inactive_rows) *inactive_rows = all.dnc.inactive;
    return BYZ_OK;
}

int byz_drift_attack_dev(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, float num_std,
                         float* drift, float* mean, float* stdev, int write_back, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "drift_attack"));
    hipStream_t s = as_stream(stream);
    float* vec = drift;
    if (write_back && !vec) {
        BYZ_TRY(ctx->stage_out.ensure(static_cast<size_t>(n_cols) * 3 * sizeof(float)));
        vec = ctx->stage_out.as<float>();
    }
    BYZ_TRY(launch_column_drift(ctx, G, n_rows, n_cols, ld, num_std, vec, mean, stdev, s));
    if (write_back) BYZ_TRY(launch_broadcast_rows(ctx, G, n_rows, n_cols, ld, vec, s));
    return BYZ_OK;
}

// ---- the attacks of Fang, Cao, Jia and Gong (USENIX Security 2020; beyond the reference) -----------------------------------------
namespace {

// What the attacks keep in ctx->fang.  m = 0 (the trimmed-mean attack): the column vectors alone.
struct FangScratch {
    float *a, *b, *c, *vec;          // n_cols each: mean or mu; lo or sigma; hi; the direction s, then the attack vector
    double *t, *q;                   // m each: g_i . s and |g_i|^2 of the benign rows
    float* block;                    // m x m: the benign rows' distances
    unsigned long long* bounds;      // 2: the bits of min_i S_i and of max_i q_i
};

int fang_workspace(byz_ctx* ctx, int64_t n_cols, int64_t m, FangScratch* out) {
    Carve c;
    c.take(&out->a, n_cols);
    c.take(&out->b, n_cols);
    c.take(&out->c, n_cols);
    c.take(&out->vec, n_cols);
    c.take(&out->t, m);
    c.take(&out->q, m);
    c.take(&out->block, m * m);
    c.take(&out->bounds, 2);
    return c.commit(ctx->fang);
}

// (written so that a NaN fails every test)
int check_fang(const char* who, const byz_fang_params* params, int64_t n_cols) {
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    if (!params->partial && !(params->b > 1.0 && __builtin_isfinite(params->b))) {
        set_error("%s: b = %g must be finite and > 1", who, params->b);
        return BYZ_E_INVALID;
    }
    if (params->partial && !(params->k_lo >= 0.0 && params->k_hi >= params->k_lo && __builtin_isfinite(params->k_hi))) {
        set_error("%s: 0 <= k_lo = %g <= k_hi = %g, both finite, violated", who, params->k_lo, params->k_hi);
        return BYZ_E_INVALID;
    }
    if (params->round >> 32 != 0) {
        set_error("%s: round = %llu must be below 2^32 (the attacker row takes the counter's top word)", who,
                  (unsigned long long)params->round);
        return BYZ_E_INVALID;
    }
    if (n_cols < 1 || params->column_offset > static_cast<uint64_t>(kNoiseMaxColumn) ||
        static_cast<uint64_t>(n_cols) > static_cast<uint64_t>(kNoiseMaxColumn) - params->column_offset) {
        set_error("%s: %lld columns from global column %llu (at least one, up to 2^62)", who, (long long)n_cols,
                  (unsigned long long)params->column_offset);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

FangDraw fang_draw(const byz_fang_params* params) {
    return {params->b, params->k_lo, params->k_hi, params->seed, params->round, static_cast<int64_t>(params->column_offset)};
}

int check_attackers(const char* who, int64_t n_rows, int64_t n_attackers) {
    if (n_attackers < 0 || n_attackers > n_rows) {
        set_error("%s: %lld attacker rows of %lld rows", who, (long long)n_attackers, (long long)n_rows);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

}  // namespace

int byz_column_extremes_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers, float* mean,
                            float* lo, float* hi, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "column_extremes"));
    BYZ_TRY(check_attackers("column_extremes", n_rows, n_attackers));
    BYZ_REQUIRE(mean || lo || hi, "column_extremes: no output asked for");
    return launch_column_extremes(ctx, G, n_rows, n_cols, ld, n_attackers, mean, lo, hi, as_stream(stream));
}

int byz_fang_fill_dev(byz_ctx* ctx, float* G, int64_t n_attackers, int64_t n_cols, int64_t ld, const byz_fang_params* params,
                      const float* a, const float* b, const float* c, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_attackers, n_cols, ld, "fang_fill"));
    BYZ_TRY(check_fang("fang_fill", params, n_cols));
    BYZ_REQUIRE(a && b && (params->partial || c), "fang_fill: null column vector");
    return launch_fang_fill(ctx, G, n_attackers, n_cols, ld, fang_draw(params), params->partial != 0, a, b, c, as_stream(stream));
}

// full knowledge: column_extremes over all the rows, then the fill; partial: the drift attack's statistics of the attacker rows
// (write_back = 0, no drifted vector), then the fill.  Nothing synchronises.
int byz_fang_trmean_attack_dev(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers,
                               const byz_fang_params* params, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "fang_trmean_attack"));
    BYZ_TRY(check_attackers("fang_trmean_attack", n_rows, n_attackers));
    BYZ_TRY(check_fang("fang_trmean_attack", params, n_cols));
    BYZ_REQUIRE(params->partial || n_attackers < n_rows, "fang_trmean_attack: full knowledge needs a benign row (%lld rows, all the attacker's)",
                (long long)n_rows);
    if (n_attackers == 0) return BYZ_OK;
    hipStream_t s = as_stream(stream);
    FangScratch w;
    BYZ_TRY(fang_workspace(ctx, n_cols, 0, &w));
    if (params->partial) BYZ_TRY(launch_column_drift(ctx, G, n_attackers, n_cols, ld, 0.0f, nullptr, w.a, w.b, s));
    else BYZ_TRY(launch_column_extremes(ctx, G, n_rows, n_cols, ld, n_attackers, w.a, w.b, w.c, s));
    return launch_fang_fill(ctx, G, n_attackers, n_cols, ld, fang_draw(params), params->partial != 0, w.a, w.b, w.c, s);
}

int byz_fang_trmean_attack_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t n_attackers,
                                const byz_fang_params* params, float* rows_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "fang_trmean_attack"));
    BYZ_TRY(check_attackers("fang_trmean_attack", n_rows, n_attackers));
    BYZ_TRY(check_fang("fang_trmean_attack", params, n_cols));
    BYZ_REQUIRE(rows_host || n_attackers == 0, "fang_trmean_attack: null output");
    HostStage st(ctx);   // (the matrix alone: the result is its first rows)
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_fang_trmean_attack_dev(ctx, st.G(), n_rows, n_cols, n_cols, n_attackers, params, st.stream()));
    if (n_attackers > 0)
        BYZ_HIP(hipMemcpyAsync(rows_host, st.G(), static_cast<size_t>(n_attackers) * n_cols * sizeof(float), hipMemcpyDeviceToHost,
                               st.stream()));
    return st.finish();
}

// The Krum attack.  The benign block's distances, t and q once; then one step = the attacker's rows and columns of the matrix
// for lambda (no Gram) + the library's own Krum selection, whose index the host reads: that read per step, and the one of the
// two bounds before the first, are the call's synchronisations (and the one the Gram's duplicate search makes, as everywhere).
int byz_fang_krum_attack_dev(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers,
                             const double* threshold, float* dist_out, double* t_out, double* q_out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "fang_krum_attack"));
    BYZ_REQUIRE(threshold && *threshold > 0.0 && __builtin_isfinite(*threshold), "fang_krum_attack: the threshold must be finite and > 0");
    BYZ_REQUIRE(n_attackers >= 1 && n_rows > 2 * n_attackers + 1, "fang_krum_attack: n = %lld rows must exceed 2 c + 1 with c = %lld >= 1 attackers",
                (long long)n_rows, (long long)n_attackers);
    BYZ_TRY(check_row_ceiling("fang_krum_attack", n_rows));
    hipStream_t s = as_stream(stream);
    const int64_t n = n_rows, c = n_attackers, m = n - c;
    FangScratch w;
    BYZ_TRY(fang_workspace(ctx, n_cols, m, &w));
    BYZ_TRY(ensure_distance_workspaces(ctx, n));
    float* dist = dist_out ? dist_out : ctx->dist.as<float>();
    const float* benign = G + c * ld;
    // s from the mean of ALL rows (no_defense's bits), t and q of the benign rows, their distances, the two bounds
    BYZ_TRY(launch_column_mean(ctx, G, n, n_cols, ld, w.a, s));
    BYZ_TRY(launch_sign_vector(ctx, w.a, n_cols, 1.0f, -1.0f, w.vec, s));
    RowScratch rows;
    BYZ_TRY(row_scratch(ctx, m, n_cols, &rows, 2));
    BYZ_TRY(launch_row_dots(ctx, benign, m, n_cols, ld, w.vec, rows.partials, w.t, w.q, s));
    BYZ_TRY(distances(ctx, benign, m, n_cols, ld, nullptr, nullptr, w.block, stream));
    BYZ_TRY(launch_fang_krum_bound(ctx, w.block, w.q, m, w.bounds, s));
    int32_t raw[4];
    BYZ_TRY(read_i32(ctx, reinterpret_cast<const int32_t*>(w.bounds), raw, 4, s));
    double s_min, q_max;
    std::memcpy(&s_min, raw, sizeof(double));
    std::memcpy(&q_max, raw + 2, sizeof(double));
    const double lambda0 = fang_lambda0(s_min, q_max, n, c, n_cols);
    BYZ_REQUIRE(__builtin_isfinite(lambda0), "fang_krum_attack: the bound lambda_0 = %g is not finite (a benign row holds a value that is not)", lambda0);
    BYZ_HIP(hipMemcpy2DAsync(dist + c * n + c, static_cast<size_t>(n) * sizeof(float), w.block, static_cast<size_t>(m) * sizeof(float),
                             static_cast<size_t>(m) * sizeof(float), static_cast<size_t>(m), hipMemcpyDeviceToDevice, s));
    double lambda = lambda0;
    int64_t steps = 0;
    int32_t chosen = -1;
    bool succeeded = false;
    for (;;) {
        BYZ_TRY(launch_fang_krum_fill(ctx, dist, n, c, n_cols, w.q, w.t, lambda, s));
        BYZ_TRY(krum_select(ctx, dist, n, n, c, krum_winner_word(ctx), s));
        BYZ_TRY(read_winner(ctx, &chosen, s));
        ++steps;
        succeeded = chosen >= 0 && chosen < c;
        if (succeeded || lambda < *threshold || steps >= 4096) break;
        lambda = lambda / 2.0;
    }
    // every attacker row = -lambda s
    BYZ_TRY(launch_sign_vector(ctx, w.a, n_cols, static_cast<float>(-lambda), static_cast<float>(lambda), w.vec, s));
    BYZ_TRY(launch_broadcast_rows(ctx, G, c, n_cols, ld, w.vec, s));
    const size_t row_bytes = static_cast<size_t>(m) * sizeof(double);
    if (t_out) BYZ_HIP(hipMemcpyAsync(t_out, w.t, row_bytes, hipMemcpyDeviceToDevice, s));
    if (q_out) BYZ_HIP(hipMemcpyAsync(q_out, w.q, row_bytes, hipMemcpyDeviceToDevice, s));
    mark(ctx, kReportFangKrum, s);
    ctx->fang_lambda0 = lambda0;
    ctx->fang_lambda = lambda;
    ctx->fang_steps = steps;
    ctx->fang_chosen = chosen;
    ctx->fang_succeeded = succeeded ? 1 : 0;
    return BYZ_OK;
}

int byz_fang_krum_info(byz_ctx* ctx, double* lambda0, double* lambda, int64_t* steps, int64_t* chosen, int32_t* succeeded) {
    DeviceScalars all;      // (the five values are the host's; the read synchronises the last call's stream: the rows' overwrite is behind it)
    BYZ_TRY(read_report(ctx, kReportFangKrum, "fang_krum_info: no Krum attack on this context yet", &all));
    if (lambda0) *lambda0 = ctx->fang_lambda0;
    if (lambda) *lambda = ctx->fang_lambda;
    if (steps) *steps = ctx->fang_steps;
    if (chosen) *chosen = ctx->fang_chosen;
    if (succeeded) *succeeded = ctx->fang_succeeded;
    return BYZ_OK;
}

// ---- the Min-Max / Min-Sum attacks of Shejwalkar and Houmansadr (NDSS 2021; beyond the reference) ----------------------------------
namespace {

// What the attacks keep in ctx->minmax.  a, b and c lie behind one another: one all-reduce's worth.
struct MinmaxScratch {
    float *mu, *sigma, *p;           // n_cols each
    double* abc;                     // 2 r + 1: a, b, c
    double* norm_sq;                 // 1: |mu|^2
    float *dmax, *dmax_part;         // 1; kMinmaxMaxPartials: the distance maximum and its workgroups' values
};

int minmax_workspace(byz_ctx* ctx, int64_t n_cols, int64_t r, MinmaxScratch* out) {
    Carve c;
    c.take(&out->mu, n_cols);
    c.take(&out->sigma, n_cols);
    c.take(&out->p, n_cols);
    c.take(&out->abc, 2 * r + 1);
    c.take(&out->norm_sq, 1);
    c.take(&out->dmax, 1);
    c.take(&out->dmax_part, kMinmaxMaxPartials);
    return c.commit(ctx->minmax);
}

int check_minmax(const char* who, const byz_minmax_params* params, int64_t n_rows, int64_t n_attackers, const void* p_custom) {
    if (!params) {
        set_error("%s: null parameters", who);
        return BYZ_E_INVALID;
    }
    if (params->kind != BYZ_MINMAX_KIND_MINMAX && params->kind != BYZ_MINMAX_KIND_MINSUM) {
        set_error("%s: unknown kind %d", who, params->kind);
        return BYZ_E_INVALID;
    }
    if (params->perturbation < BYZ_MINMAX_PERTURB_UNIT || params->perturbation > BYZ_MINMAX_PERTURB_CUSTOM) {
        set_error("%s: unknown perturbation %d", who, params->perturbation);
        return BYZ_E_INVALID;
    }
    if ((params->perturbation == BYZ_MINMAX_PERTURB_CUSTOM) != (p_custom != nullptr)) {
        set_error("%s: the custom perturbation and its vector come together or not at all", who);
        return BYZ_E_INVALID;
    }
    if (n_attackers < 0 || n_attackers > n_rows) {
        set_error("%s: %lld attacker rows of %lld rows", who, (long long)n_attackers, (long long)n_rows);
        return BYZ_E_INVALID;
    }
    if (params->partial && n_attackers < 1) {
        set_error("%s: partial knowledge needs an attacker row", who);
        return BYZ_E_INVALID;
    }
    return BYZ_OK;
}

// The whole call; allreduce == nullptr: one GPU holds every column.  Nothing here waits for the device but the distances.
int minmax_attack(byz_ctx* ctx, float* G, int64_t n, int64_t n_cols, int64_t ld, int64_t m, const byz_minmax_params* params,
                  const float* p_custom, float* dist, byz_allreduce_f64_fn allreduce, void* user, void* stream, const char* who) {
    BYZ_TRY(check_minmax(who, params, n, m, p_custom));
    const bool max_kind = params->kind == BYZ_MINMAX_KIND_MINMAX;
    BYZ_REQUIRE(!(max_kind && params->dist_given) || dist, "%s: dist_given without a distance matrix", who);
    if (m == 0) return BYZ_OK;
    const int64_t r = params->partial ? m : n;
    BYZ_TRY(check_row_ceiling(who, r));
    hipStream_t s = as_stream(stream);
    MinmaxScratch w;
    BYZ_TRY(minmax_workspace(ctx, n_cols, r, &w));
    RowScratch rows;
    BYZ_TRY(row_scratch(ctx, r, n_cols, &rows, 2));
    double *a = w.abc, *b = w.abc + r, *c = w.abc + 2 * r;
    BYZ_TRY(launch_column_drift(ctx, G, r, n_cols, ld, 0.0f, nullptr, w.mu, w.sigma, s));
    const float* p = p_custom;
    if (p == nullptr) {
        if (params->perturbation == BYZ_MINMAX_PERTURB_UNIT) {
            BYZ_TRY(launch_row_sqdist(ctx, w.mu, 1, n_cols, n_cols, nullptr, rows.root, w.norm_sq, nullptr, nullptr, s));
            if (allreduce != nullptr) BYZ_TRY(reduce_over_ranks(allreduce, user, w.norm_sq, 1, stream, "minmax attack (the mean's norm)"));
        }
        BYZ_TRY(launch_perturbation(ctx, w.mu, w.sigma, w.norm_sq, params->perturbation, n_cols, w.p, s));
        p = w.p;
    }
    BYZ_TRY(launch_row_sqdist(ctx, p, 1, n_cols, n_cols, nullptr, rows.root, c, nullptr, nullptr, s));
    BYZ_TRY(launch_row_moments(ctx, G, r, n_cols, ld, w.mu, p, rows.partials, a, b, s));
    if (allreduce != nullptr) BYZ_TRY(reduce_over_ranks(allreduce, user, w.abc, 2 * r + 1, stream, "minmax attack (moments)"));
    if (max_kind) {
        if (r == 1) {
            BYZ_HIP(hipMemsetAsync(w.dmax, 0, sizeof(float), s));
        } else if (params->dist_given) {
            BYZ_TRY(launch_dist_max(ctx, dist, r, n, w.dmax_part, w.dmax, s));
        } else {
            if (dist == nullptr) BYZ_TRY(ctx->dist.ensure(static_cast<size_t>(r) * r * sizeof(float)));      // (distances() sizes the Gram itself)
            float* d = dist ? dist : ctx->dist.as<float>();
            BYZ_TRY(distances(ctx, G, r, n_cols, ld, allreduce, user, d, stream));
            BYZ_TRY(launch_dist_max(ctx, d, r, r, w.dmax_part, w.dmax, s));
        }
    }
    mark(ctx, kReportMinmax, s);
    BYZ_TRY(launch_minmax_solve(ctx, a, b, c, w.dmax, r, params->kind, s));
    return launch_minmax_fill(ctx, G, m, n_cols, ld, w.mu, p, s);
}

}  // namespace

int byz_row_moments_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* z, const float* p,
                        double* a, double* b, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "row_moments"));
    BYZ_REQUIRE(z && p && a && b, "row_moments: null vector or output");
    BYZ_TRY(check_row_ceiling("row_moments", n_rows));
    RowScratch t;
    BYZ_TRY(row_scratch(ctx, n_rows, n_cols, &t, 2));
    return launch_row_moments(ctx, G, n_rows, n_cols, ld, z, p, t.partials, a, b, as_stream(stream));
}

int byz_minmax_attack_dev(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers,
                          const byz_minmax_params* params, const float* p_custom, float* dist, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "minmax_attack"));
    return minmax_attack(ctx, G, n_rows, n_cols, ld, n_attackers, params, p_custom, dist, nullptr, nullptr, stream, "minmax_attack");
}

int byz_minmax_attack_sharded_dev(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers,
                                  const byz_minmax_params* params, const float* p_custom, float* dist, byz_allreduce_f64_fn allreduce,
                                  void* user, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "minmax_attack_sharded"));
    BYZ_REQUIRE(allreduce, "minmax_attack_sharded: null all-reduce");
    return minmax_attack(ctx, G, n_rows, n_cols, ld, n_attackers, params, p_custom, dist, allreduce, user, stream,
                         "minmax_attack_sharded");
}

int byz_minmax_info(byz_ctx* ctx, double* gamma, double* bound, double* c, int64_t* binding_row, int64_t* known_rows,
                    int32_t* degenerate, int32_t* broken) {
    DeviceScalars all;
    BYZ_TRY(read_report(ctx, kReportMinmax, "minmax_info: no Min-Max or Min-Sum attack on this context yet", &all));
    const MinmaxReport& info = all.minmax;
    if (gamma) *gamma = info.gamma;
    if (bound) *bound = info.bound;
    if (c) *c = info.c;
    if (binding_row) *binding_row = info.row;
    if (known_rows) *known_rows = info.r;
    if (degenerate) *degenerate = info.degenerate;
    if (broken) *broken = info.broken;
    return BYZ_OK;
}

int byz_minmax_attack_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t n_attackers,
                           const byz_minmax_params* params, const float* p_custom_host, float* vector_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "minmax_attack"));
    BYZ_TRY(check_minmax("minmax_attack", params, n_rows, n_attackers, p_custom_host));
    BYZ_REQUIRE(vector_host && n_attackers >= 1, "minmax_attack: null output or no attacker row");
    HostStage st(ctx);
    float* p_dev = nullptr;
    st.in(&p_dev, p_custom_host, n_cols);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_minmax_attack_dev(ctx, st.G(), n_rows, n_cols, n_cols, n_attackers, params, p_dev, nullptr, st.stream()));
    BYZ_HIP(hipMemcpyAsync(vector_host, st.G(), static_cast<size_t>(n_cols) * sizeof(float), hipMemcpyDeviceToHost, st.stream()));
    return st.finish();
}

int byz_column_chain_dev(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const float* carry_in,
                         const float* mean, float* out_sum, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "column_chain"));
    BYZ_REQUIRE(out_sum, "column_chain: null output");
    return launch_column_chain(ctx, G, n_rows, n_cols, ld, carry_in, mean, out_sum, as_stream(stream));
}

int byz_column_finish_dev(byz_ctx* ctx, const float* sum, const float* sumsq, int64_t total_rows, float num_std, int64_t n_cols,
                          float* mean, float* stdev, float* drift, void* stream) {
    BYZ_TRY(enter(ctx));
    return launch_column_finish(ctx, sum, sumsq, total_rows, num_std, n_cols, mean, stdev, drift, as_stream(stream));
}

int byz_drift_axpy_dev(byz_ctx* ctx, float* mean, const float* stdev, int64_t n, float num_std, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(mean && stdev && n > 0, "drift_axpy: bad arguments");
    return launch_drift_axpy(ctx, mean, stdev, n, num_std, as_stream(stream));
}

int byz_server_update_dev(byz_ctx* ctx, float* weights, float* velocity, const float* agg, int64_t n,
                          float momentum, float learning_rate, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(weights && velocity && agg && n > 0, "server_update: bad arguments");
    return launch_server_update(ctx, weights, velocity, agg, n, momentum, learning_rate, as_stream(stream));
}

// ---- the steps either side of the path -------------------------------------------
int byz_backdoor_initial_params_dev(byz_ctx* ctx, const float* original_params, const float* grads_mean, int64_t n,
                                    float learning_rate, float* out, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(original_params && grads_mean && out && n > 0, "backdoor_initial_params: bad arguments");
    return launch_backdoor_initial(ctx, original_params, grads_mean, n, learning_rate, out, as_stream(stream));
}

int byz_backdoor_clip_dev(byz_ctx* ctx, const float* grads_mean, const float* grads_stdev, const float* original_params,
                          const float* mal_net_params, int64_t n, float learning_rate, float num_std, float* out,
                          void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(grads_mean && grads_stdev && original_params && mal_net_params && out && n > 0,
                "backdoor_clip: bad arguments");
    return launch_backdoor_clip(ctx, grads_mean, grads_stdev, original_params, mal_net_params, n, learning_rate,
                                num_std, out, as_stream(stream));
}

int byz_assemble_row_dev(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row,
                         int64_t n_segments, const float* const* segments_dev, const int64_t* lengths, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "assemble_row"));
    BYZ_REQUIRE(row >= 0 && row < n_rows, "assemble_row: row %lld outside 0..%lld", (long long)row, (long long)n_rows - 1);
    BYZ_REQUIRE(n_segments > 0 && segments_dev && lengths, "assemble_row: no segments");
    return launch_assemble_row(ctx, G + row * ld, n_cols, n_segments, segments_dev, lengths, as_stream(stream));
}

int byz_assemble_rows_dev(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t first_row,
                          int64_t n_clients, int64_t n_segments, const float* const* segments_dev, const int64_t* lengths,
                          void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "assemble_rows"));
    BYZ_REQUIRE(first_row >= 0 && n_clients > 0 && first_row + n_clients <= n_rows,
                "assemble_rows: rows %lld .. %lld outside 0..%lld", (long long)first_row, (long long)(first_row + n_clients - 1),
                (long long)n_rows - 1);
    BYZ_REQUIRE(n_segments > 0 && segments_dev && lengths, "assemble_rows: no segments");
    return launch_assemble_rows(ctx, G + first_row * ld, n_cols, ld, n_clients, n_segments, segments_dev, lengths,
                                as_stream(stream));
}

int byz_assemble_rows_again_dev(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t first_row,
                                int64_t n_clients, int64_t n_segments, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "assemble_rows_again"));
    BYZ_REQUIRE(first_row >= 0 && n_clients > 0 && first_row + n_clients <= n_rows,
                "assemble_rows_again: rows %lld .. %lld outside 0..%lld", (long long)first_row,
                (long long)(first_row + n_clients - 1), (long long)n_rows - 1);
    return launch_assemble_rows_again(ctx, G + first_row * ld, n_cols, ld, n_clients, n_segments, as_stream(stream));
}

int byz_assemble_columns_dev(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_segments,
                             const float* const* segments_dev, const int64_t* lengths, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "assemble_columns"));
    BYZ_REQUIRE(n_segments > 0 && segments_dev && lengths, "assemble_columns: no segments");
    return launch_assemble_columns(ctx, G, n_rows, n_cols, ld, n_segments, segments_dev, lengths, as_stream(stream));
}

int byz_assemble_row_host(byz_ctx* ctx, float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row,
                          const float* grads_host, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G, n_rows, n_cols, ld, "assemble_row"));
    BYZ_REQUIRE(row >= 0 && row < n_rows && grads_host, "assemble_row: row %lld outside 0..%lld", (long long)row,
                (long long)n_rows - 1);
    BYZ_HIP(hipMemcpyAsync(G + row * ld, grads_host, static_cast<size_t>(n_cols) * sizeof(float), hipMemcpyHostToDevice,
                           as_stream(stream)));
    return BYZ_OK;
}

// ---- host-pointer convenience --------------------------------------------------------------------
int byz_defend_host(byz_ctx* ctx, int name, const float* G_host, int64_t n_rows, int64_t n_cols,
                    int64_t users_count, int64_t corrupted_count, int check_assert, float* out_host,
                    int32_t* aux_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "defend"));
    BYZ_REQUIRE(name >= 0 && name <= 3, "defend: unknown defence %d", name);
    // preconditions first: the reference asserts before touching the data
    BYZ_TRY(check_krum_assert(name == 1 && check_assert, users_count, corrupted_count));
    if (name == 3) BYZ_TRY(check_bulyan_precondition(users_count, corrupted_count));
    HostStage st(ctx);
    float* out;
    st.inout<float>(&out, nullptr, out_host, n_cols);   // (every defence but Krum writes it whether asked for or not)
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    float* G = st.G();
    hipStream_t s = st.stream();
    int32_t index = 0;
    switch (name) {
        case 0: BYZ_TRY(byz_no_defense_dev(ctx, G, n_rows, n_cols, n_cols, out, s)); break;
        case 1:
            BYZ_TRY(byz_krum_dev(ctx, G, n_rows, n_cols, n_cols, users_count, corrupted_count, 0,
                                 out_host ? out : nullptr, &index, s));
            if (aux_host) aux_host[0] = index;
            break;
        case 2: BYZ_TRY(byz_trimmed_mean_dev(ctx, G, n_rows, n_cols, n_cols, nullptr, corrupted_count, out, s)); break;
        case 3: {
            BYZ_TRY(byz_bulyan_dev(ctx, G, n_rows, n_cols, n_cols, users_count, corrupted_count, out, nullptr, s));
            if (aux_host) {
                const int64_t theta = users_count - 2 * corrupted_count;
                BYZ_TRY(read_i32(ctx, ctx->selection.as<int32_t>(), aux_host, theta, s));
            }
            break;
        }
    }
    return out_host ? st.finish_sync() : BYZ_OK;   // (nothing to wait for when no vector goes back)
}

int byz_pairwise_distances_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                                float* dist_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "pairwise_distances"));
    BYZ_REQUIRE(dist_host, "pairwise_distances: null output");
    HostStage st(ctx);   // (the matrix alone: the result is ctx->dist)
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    hipStream_t s = st.stream();
    BYZ_TRY(ensure_distance_workspaces(ctx, n_rows));
    BYZ_TRY(byz_pairwise_distances_dev(ctx, st.G(), n_rows, n_cols, n_cols, ctx->dist.as<float>(), s));
    BYZ_HIP(hipMemcpyAsync(dist_host, ctx->dist.ptr, static_cast<size_t>(n_rows) * n_rows * sizeof(float),
                           hipMemcpyDeviceToHost, s));
    BYZ_HIP(hipStreamSynchronize(s));
    return BYZ_OK;
}

int byz_krum_select_host(byz_ctx* ctx, const float* dist_host, int64_t n_rows, int64_t users_count,
                         int64_t corrupted_count, int32_t* index_host) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(dist_host && index_host && n_rows > 0, "krum_select: bad arguments");
    hipStream_t s = nullptr;
    BYZ_TRY(ensure_distance_workspaces(ctx, n_rows));
    BYZ_HIP(hipMemcpyAsync(ctx->dist.ptr, dist_host, static_cast<size_t>(n_rows) * n_rows * sizeof(float),
                           hipMemcpyHostToDevice, s));
    return byz_krum_select_dev(ctx, ctx->dist.as<float>(), n_rows, users_count, corrupted_count, index_host,
                               nullptr, s);
}

int byz_drift_attack_host(byz_ctx* ctx, const float* rows_host, int64_t n_rows, int64_t n_cols, float num_std,
                          float* drift_host, float* mean_host, float* std_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(rows_host, n_rows, n_cols, n_cols, "drift_attack"));
    HostStage st(ctx);
    float *drift, *mean, *stdev;   // (the kernel writes all three, asked for or not)
    st.inout<float>(&drift, nullptr, drift_host, n_cols);
    st.inout<float>(&mean, nullptr, mean_host, n_cols);
    st.inout<float>(&stdev, nullptr, std_host, n_cols);
    BYZ_TRY(st.stage(rows_host, n_rows, n_cols));
    BYZ_TRY(launch_column_drift(ctx, st.G(), n_rows, n_cols, n_cols, num_std, drift, mean, stdev, st.stream()));
    return st.finish();
}

int byz_multi_krum_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t users_count,
                        int64_t corrupted_count, int64_t m, float* out_host, int32_t* selection_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "multi_krum"));
    BYZ_REQUIRE(out_host || selection_host, "multi_krum: neither an output nor a selection asked for");
    // the aggregate asserts as defences.krum does; a selection alone does not (krum(..., return_index=True))
    BYZ_TRY(check_krum_assert(out_host != nullptr, users_count, corrupted_count));
    BYZ_TRY(check_multi_krum_m(n_rows, m));
    HostStage st(ctx);
    float* out;
    st.inout<float>(&out, nullptr, out_host, n_cols);   // (the device call always forms the aggregate)
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(ctx->selection.ensure(static_cast<size_t>(n_rows) * sizeof(int32_t)));
    int32_t* sel = ctx->selection.as<int32_t>();
    BYZ_TRY(byz_multi_krum_dev(ctx, st.G(), n_rows, n_cols, n_cols, users_count, corrupted_count, m, 0, out, sel, st.stream()));
    if (selection_host) BYZ_TRY(read_i32(ctx, sel, selection_host, m, st.stream()));
    return st.finish();
}

// the two coordinate-wise rank rules on a host matrix (median: trim_count ignored)
static int rank_select_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t trim_count, bool median,
                            float* out_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, median ? "coordinate_median" : "rank_trimmed_mean"));
    BYZ_REQUIRE(out_host, "%s: null output", median ? "coordinate_median" : "rank_trimmed_mean");
    if (n_rows > kLargeMaxRows || (!median && (trim_count < 0 || 2 * trim_count >= n_rows)))      // refused before anything is staged
        return launch_rank_select(ctx, G_host, n_rows, n_cols, n_cols, nullptr, trim_count, median, out_host, nullptr);
    HostStage st(ctx);
    float* out;
    st.out(&out, out_host, n_cols);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(launch_rank_select(ctx, st.G(), n_rows, n_cols, n_cols, nullptr, trim_count, median, out, st.stream()));
    return st.finish_sync();
}

int byz_coordinate_median_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, float* out_host) {
    return rank_select_host(ctx, G_host, n_rows, n_cols, 0, true, out_host);
}

int byz_rank_trimmed_mean_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t trim_count,
                               float* out_host) {
    return rank_select_host(ctx, G_host, n_rows, n_cols, trim_count, false, out_host);
}

int byz_window_mean_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const float* centre_host, int64_t keep,
                         float* out_host, float* radius_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "window_mean"));
    BYZ_REQUIRE(centre_host && out_host, "window_mean: null centre or output");
    BYZ_TRY(check_centre_window("window_mean", n_rows, keep));      // refused before anything is staged
    HostStage st(ctx);
    float *centre, *out, *radius;
    st.in<float>(&centre, centre_host, n_cols);
    st.out(&out, out_host, n_cols);
    st.out(&radius, radius_host, n_cols);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(launch_centre_window(ctx, st.G(), n_rows, n_cols, n_cols, nullptr, centre, keep, out, radius, st.stream()));
    return st.finish_sync();
}

int byz_phocas_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t trim_count, float* out_host,
                    float* centre_out_host, float* radius_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "phocas"));
    BYZ_REQUIRE(out_host, "phocas: null output");
    BYZ_TRY(check_row_ceiling("phocas", n_rows));
    BYZ_REQUIRE(trim_count >= 0 && 2 * trim_count < n_rows, "phocas: trim_count %lld must satisfy 0 <= 2 b < %lld rows",
                (long long)trim_count, (long long)n_rows);
    HostStage st(ctx);
    float *out, *centre, *radius;
    st.out(&out, out_host, n_cols);
    st.inout<float>(&centre, nullptr, centre_out_host, n_cols);      // (always carved: the window is taken around it)
    st.out(&radius, radius_host, n_cols);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_phocas_dev(ctx, st.G(), n_rows, n_cols, n_cols, nullptr, trim_count, out, centre, radius, st.stream()));
    return st.finish_sync();
}

int byz_geometric_median_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_geomed_params* params,
                              float* out_host, double* weights_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "geometric_median"));
    BYZ_REQUIRE(out_host, "geometric_median: null output");
    BYZ_TRY(check_geomed(params, n_rows, "geometric_median"));
    HostStage st(ctx);
    float* out;
    double* weights;
    st.out(&out, out_host, n_cols);
    st.out(&weights, weights_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_geometric_median_dev(ctx, st.G(), n_rows, n_cols, n_cols, params, out, weights, st.stream()));
    return st.finish();
}

int byz_centered_clip_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_cclip_params* params,
                           const float* start_host, float* out_host, double* scales_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "centered_clip"));
    BYZ_REQUIRE(out_host, "centered_clip: null output");
    BYZ_TRY(check_cclip(params, n_rows, "centered_clip"));
    HostStage st(ctx);
    float* out;
    double* scales;
    st.inout(&out, start_host, out_host, n_cols);   // the start is staged into the output vector: the device call runs in place on it
    st.out(&scales, scales_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_centered_clip_dev(ctx, st.G(), n_rows, n_cols, n_cols, params, start_host ? out : nullptr, out, scales, st.stream()));
    return st.finish();
}

int byz_fltrust_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const float* root_host, float* out_host,
                     double* trust_host, double* weights_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "fltrust"));
    BYZ_REQUIRE(root_host && out_host, "fltrust: null root or output");
    BYZ_TRY(check_row_ceiling("fltrust", n_rows));
    HostStage st(ctx);
    float* out;
    double *trust, *weights;
    st.inout(&out, root_host, out_host, n_cols);   // the root is staged into the output vector: the device call runs in place on it
    st.out(&trust, trust_host, n_rows);
    st.out(&weights, weights_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_fltrust_dev(ctx, st.G(), n_rows, n_cols, n_cols, out, out, trust, weights, st.stream()));
    return st.finish();
}

int byz_signguard_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_signguard_params* params,
                       const int32_t* sample_host, float* out_host, int32_t* keep_host, double* weights_host, int32_t* labels_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "signguard"));
    BYZ_REQUIRE(out_host, "signguard: null output");
    BYZ_TRY(check_signguard(params, n_rows, sample_host, "signguard"));
    const bool estimate = !(params->bandwidth > 0.0);
    if (estimate) {
        std::vector<char> seen(static_cast<size_t>(n_rows), 0);
        for (int64_t j = 0; j < params->n_sample; ++j) {
            const int32_t r = sample_host[j];
            BYZ_REQUIRE(r >= 0 && r < n_rows && !seen[r], "signguard: sample[%lld] = %d is out of range or a repeat", (long long)j, r);
            seen[r] = 1;
        }
    }
    HostStage st(ctx);
    float* out;
    double* weights;
    int32_t *keep, *labels;
    st.out(&out, out_host, n_cols);
    st.inout<double>(&weights, nullptr, weights_host, n_rows);   // (as before, the device call gets all three, asked for or not)
    st.inout<int32_t>(&keep, nullptr, keep_host, n_rows);
    st.inout<int32_t>(&labels, nullptr, labels_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    SgScratch t;   // the sample goes where the selection reads it, not into the staging area
    BYZ_TRY(signguard_workspace(ctx, n_rows, n_cols, &t));
    if (estimate)
        BYZ_HIP(hipMemcpyAsync(t.sample, sample_host, static_cast<size_t>(params->n_sample) * sizeof(int32_t), hipMemcpyHostToDevice,
                               st.stream()));
    BYZ_TRY(byz_signguard_dev(ctx, st.G(), n_rows, n_cols, n_cols, params, estimate ? t.sample : nullptr, out, keep, weights, labels,
                              st.stream()));
    return st.finish();
}

int byz_nnm_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t users_count, int64_t corrupted_count,
                 float* Y_host, int32_t* nbr_host) {
    BYZ_TRY(enter(ctx));
    const int64_t k = users_count - corrupted_count;
    BYZ_TRY(check_nnm("nnm", n_rows, k));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "nnm"));
    BYZ_REQUIRE(Y_host, "nnm: null output");
    HostStage st(ctx);
    float* Y;
    int32_t* nbr;
    st.out(&Y, Y_host, n_rows * n_cols);
    st.out(&nbr, nbr_host, n_rows * k);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_nnm_dev(ctx, st.G(), n_rows, n_cols, n_cols, users_count, corrupted_count, Y, n_cols, nbr, st.stream()));
    return st.finish();
}

int byz_robust_lr_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t theta, float* out_host,
                       int32_t* votes_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "robust_lr"));
    BYZ_REQUIRE(out_host, "robust_lr: null output");
    BYZ_TRY(check_row_ceiling("robust_lr", n_rows));
    BYZ_TRY(check_rlr_theta("robust_lr", theta, n_rows));
    HostStage st(ctx);
    float* out;
    int32_t* votes;
    st.out(&out, out_host, n_cols);
    st.out(&votes, votes_host, n_cols);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_robust_lr_dev(ctx, st.G(), n_rows, n_cols, n_cols, theta, out, votes, st.stream()));
    return st.finish();
}

int byz_bucket_means_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const int32_t* perm_host, int64_t s,
                          float* Y_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_bucketing("bucket_means", G_host, n_rows, n_cols, n_cols, s));
    BYZ_REQUIRE(Y_host, "bucket_means: null output");
    if (perm_host != nullptr) {     // a permutation of 0 .. n_rows - 1: every entry in range, none twice
        std::vector<bool> seen(static_cast<size_t>(n_rows), false);
        for (int64_t i = 0; i < n_rows; ++i) {
            const int64_t e = perm_host[i];
            BYZ_REQUIRE(e >= 0 && e < n_rows && !seen[static_cast<size_t>(e)],
                        "bucket_means: perm is no permutation of 0..%lld (entry %lld is %lld)", (long long)(n_rows - 1), (long long)i,
                        (long long)e);
            seen[static_cast<size_t>(e)] = true;
        }
    }
    HostStage st(ctx);
    float* Y;
    int32_t* perm;
    st.out(&Y, Y_host, ceil_div(n_rows, s) * n_cols);
    st.in(&perm, perm_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_bucket_means_dev(ctx, st.G(), n_rows, n_cols, n_cols, perm, s, Y, n_cols, st.stream()));
    return st.finish();
}

int byz_topk_sparsify_host(byz_ctx* ctx, const float* x_host, const float* add_host, int64_t n, int64_t k, float* out_host,
                           float* residual_host) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(x_host && out_host && n > 0, "topk_sparsify: null vector or no columns (%lld)", (long long)n);
    BYZ_TRY(check_topk("topk_sparsify", x_host, add_host, n, n, k, out_host, residual_host));
    HostStage st(ctx);     // x is the staged "matrix" (one row); the device call is out of place, so the host vectors may coincide
    float *add, *out, *residual;
    st.in(&add, add_host, n);
    st.out(&out, out_host, n);
    st.out(&residual, residual_host, n);
    BYZ_TRY(st.stage(x_host, 1, n));
    BYZ_TRY(byz_topk_sparsify_dev(ctx, st.G(), add, n, k, out, residual, st.stream()));
    return st.finish();
}

int byz_sparsefed_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_sparsefed_params* params,
                       float* residual_host, float* out_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "sparsefed"));
    BYZ_REQUIRE(params && residual_host && out_host, "sparsefed: null parameters, memory or output");
    const byz_cclip_params clip = {params->clip, 1};
    BYZ_TRY(check_cclip(&clip, n_rows, "sparsefed"));
    BYZ_TRY(check_topk("sparsefed", residual_host, nullptr, n_cols, n_cols, params->k, out_host, nullptr));
    HostStage st(ctx);
    float *residual, *out;
    st.inout(&residual, static_cast<const float*>(residual_host), residual_host, n_cols);
    st.out(&out, out_host, n_cols);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_sparsefed_dev(ctx, st.G(), n_rows, n_cols, n_cols, params, residual, out, st.stream()));
    return st.finish();
}

int byz_gaussian_noise_host(byz_ctx* ctx, const float* x_host, int64_t n, const byz_noise_params* params, float* out_host) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(x_host && out_host && params, "gaussian_noise: null vector or parameters");
    BYZ_TRY(check_noise("gaussian_noise", params->sigma, params->column_offset, n));
    BYZ_REQUIRE(out_host == x_host || !vectors_overlap(x_host, out_host, n), "gaussian_noise: the output overlaps x (it may BE x, nothing else)");
    HostStage st(ctx);     // x is the staged "matrix" (one row); the device call is out of place, so the host vectors may coincide
    float* out;
    st.out(&out, out_host, n);
    BYZ_TRY(st.stage(x_host, 1, n));
    BYZ_TRY(byz_gaussian_noise_dev(ctx, st.G(), n, params, nullptr, out, st.stream()));
    return st.finish();
}

int byz_weak_dp_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_weak_dp_params* params,
                     float* out_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "weak_dp"));
    BYZ_REQUIRE(out_host, "weak_dp: null output");
    BYZ_TRY(check_weak_dp("weak_dp", params, n_rows, n_cols));
    HostStage st(ctx);
    float* out;
    st.out(&out, out_host, n_cols);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_weak_dp_dev(ctx, st.G(), n_rows, n_cols, n_cols, params, out, st.stream()));
    return st.finish();
}

int byz_flame_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_flame_params* params,
                   const float* dist_host, float* out_host, int32_t* admitted_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "flame"));
    BYZ_REQUIRE(out_host, "flame: null output");
    BYZ_TRY(check_flame("flame", params, n_rows, n_cols));
    HostStage st(ctx);
    float *out, *dist;
    int32_t* admitted;
    st.out(&out, out_host, n_cols);
    st.in(&dist, dist_host, n_rows * n_rows);
    st.out(&admitted, admitted_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_flame_dev(ctx, st.G(), n_rows, n_cols, n_cols, params, dist, out, admitted, st.stream()));
    return st.finish();
}

int byz_clipped_clustering_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                                const byz_clipped_clustering_params* params, const float* dist_host, const double* sq_host,
                                float* out_host, int32_t* admitted_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "clipped_clustering"));
    BYZ_REQUIRE(out_host, "clipped_clustering: null output");
    BYZ_TRY(check_clipped_clustering("clipped_clustering", params, n_rows));
    HostStage st(ctx);
    float *out, *dist;
    double* sq;
    int32_t* admitted;
    st.out(&out, out_host, n_cols);
    st.in(&dist, dist_host, n_rows * n_rows);
    st.in(&sq, sq_host, n_rows);
    st.out(&admitted, admitted_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_clipped_clustering_dev(ctx, st.G(), n_rows, n_cols, n_cols, params, dist, sq, out, admitted, st.stream()));
    return st.finish();
}

int byz_faba_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t remove_count, const float* dist_host,
                  float* out_host, int32_t* kept_host, int32_t* order_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "faba"));
    BYZ_REQUIRE(out_host, "faba: null output");
    BYZ_TRY(check_faba("faba", n_rows, remove_count, 2));
    HostStage st(ctx);
    float *out, *dist;
    int32_t *kept, *order;
    st.out(&out, out_host, n_cols);
    st.in(&dist, dist_host, n_rows * n_rows);
    st.out(&kept, kept_host, n_rows);
    st.out(&order, order_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_faba_dev(ctx, st.G(), n_rows, n_cols, n_cols, remove_count, dist, out, kept, order, st.stream()));
    return st.finish();
}

int byz_afa_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const double* weights_host,
                 const byz_afa_params* params, const double* gram_host, float* out_host, int32_t* kept_host, int32_t* round_of_host,
                 double* score_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "afa"));
    BYZ_REQUIRE(out_host, "afa: null output");
    BYZ_TRY(check_afa("afa", n_rows, params));
    HostStage st(ctx);
    float* out;
    double *weights, *gram, *score;
    int32_t *kept, *round_of;
    st.out(&out, out_host, n_cols);
    st.in(&weights, weights_host, n_rows);
    st.in(&gram, gram_host, n_rows * n_rows);
    st.out(&score, score_host, n_rows);
    st.out(&kept, kept_host, n_rows);
    st.out(&round_of, round_of_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_afa_dev(ctx, st.G(), n_rows, n_cols, n_cols, weights, params, gram, out, kept, round_of, score, st.stream()));
    return st.finish();
}

int byz_auror_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_auror_params* params, float* out_host,
                   int32_t* kept_host, int64_t* votes_host, int32_t* bad_host, int64_t* counts_host, double* gap_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "auror"));
    BYZ_REQUIRE(out_host, "auror: null output");
    BYZ_TRY(check_auror("auror", n_rows, params));
    const bool add = params->accumulate != 0;
    BYZ_REQUIRE(!add || (votes_host && bad_host && counts_host), "auror: accumulate = 1 needs the caller's votes, bad flags and counts");
    HostStage st(ctx);
    float* out;
    double* gap;
    int64_t *votes, *counts;
    int32_t *kept, *bad;
    st.out(&out, out_host, n_cols);
    st.out(&kept, kept_host, n_rows);
    st.out(&gap, gap_host, n_cols);
    // the history: always on the device (the call writes all three), uploaded when it is added to
    st.inout(&votes, add ? votes_host : nullptr, votes_host, n_rows);
    st.inout(&bad, add ? bad_host : nullptr, bad_host, n_rows);
    st.inout(&counts, add ? counts_host : nullptr, counts_host, 4);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_auror_dev(ctx, st.G(), n_rows, n_cols, n_cols, params, votes, bad, counts, out, kept, gap, st.stream()));
    return st.finish();
}

int byz_foolsgold_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, float* H_host, int64_t col_start,
                       int64_t col_count, const byz_foolsgold_params* params, const double* gram_host, float* out_host,
                       double* weights_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "foolsgold"));
    BYZ_REQUIRE(out_host, "foolsgold: null output");
    BYZ_TRY(check_foolsgold("foolsgold", n_rows, params));
    BYZ_TRY(check_foolsgold_window("foolsgold", G_host, n_rows, n_cols, n_cols, nullptr, 0, col_start, col_count));
    HostStage st(ctx);
    float *out, *H = nullptr;
    double *gram, *weights;
    st.out(&out, out_host, n_cols);
    if (H_host != nullptr) st.inout(&H, static_cast<const float*>(H_host), H_host, n_rows * col_count);     // added to in place
    st.in(&gram, gram_host, n_rows * n_rows);
    st.out(&weights, weights_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_foolsgold_dev(ctx, st.G(), n_rows, n_cols, n_cols, H, col_count, col_start, col_count, params, gram, out, weights,
                              st.stream()));
    return st.finish();
}

int byz_multi_metrics_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t keep, float* out_host,
                           int32_t* flags_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "multi_metrics"));
    BYZ_REQUIRE(out_host, "multi_metrics: null output");
    BYZ_TRY(check_mm_keep("multi_metrics", n_rows, keep));
    HostStage st(ctx);
    float* out;
    int32_t* flags;
    st.out(&out, out_host, n_cols);
    st.out(&flags, flags_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_multi_metrics_dev(ctx, st.G(), n_rows, n_cols, n_cols, keep, out, flags, st.stream()));
    return st.finish();
}

int byz_dnc_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_dnc_params* params,
                 const int64_t* columns_host, float* out_host, int32_t* good_host, int64_t* kept_host) {
    BYZ_TRY(enter(ctx));
    BYZ_TRY(check_matrix(G_host, n_rows, n_cols, n_cols, "dnc"));
    BYZ_REQUIRE(columns_host && out_host, "dnc: null column list or output");
    BYZ_TRY(check_dnc(params, n_rows, n_cols, "dnc"));
    const int64_t listed = params->n_iters * params->sub_dim;
    for (int64_t k = 0; k < listed; ++k) {
        const int64_t c = columns_host[k];
        const bool first = k % params->sub_dim == 0;
        BYZ_REQUIRE(c >= 0 && c < n_cols && (first || c > columns_host[k - 1]),
                    "dnc: column list entry %lld = %lld out of range or not ascending", (long long)k, (long long)c);
    }
    HostStage st(ctx);
    float* out;
    int64_t* columns;
    int32_t* good;
    st.out(&out, out_host, n_cols);
    st.in(&columns, columns_host, listed);
    st.out(&good, good_host, n_rows);
    BYZ_TRY(st.stage(G_host, n_rows, n_cols));
    BYZ_TRY(byz_dnc_dev(ctx, st.G(), n_rows, n_cols, n_cols, params, columns, out, good, st.stream()));
    DeviceScalars all;
    BYZ_TRY(st.finish(&all));
    if (kept_host) *kept_host = all.dnc.kept;
    return BYZ_OK;
}

// ---- timing --------------------------------------------------------------------------------------
static const char* const kKernelNames[BYZ_K_COUNT] = {
    "column_stats", "gram_tile", "gram_reduce", "distances", "row_sort",
    "krum_argmin",  "bulyan_loop", "trimmed_mean", "misc", "plane_split"};

const char* byz_kernel_name(int kernel) {
    return (kernel >= 0 && kernel < BYZ_K_COUNT) ? kKernelNames[kernel] : "?";
}

int byz_timing_enable(byz_ctx* ctx, int on) {
    BYZ_TRY(enter(ctx));
    ctx->timing = on != 0;
    return BYZ_OK;
}

int byz_timing_reset(byz_ctx* ctx) {
    if (!ctx) return BYZ_E_INVALID;
    for (auto& slot : ctx->slots) {
        for (auto& ev : slot.pending) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
        slot.pending.clear();
        slot.total_ms = 0.0;
        slot.launches = 0;
    }
    return BYZ_OK;
}

int byz_timing_read(byz_ctx* ctx, int kernel, double* total_ms, int64_t* launches) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(kernel >= 0 && kernel < BYZ_K_COUNT, "timing: bad kernel id");
    auto& slot = ctx->slots[kernel];
    for (auto& ev : slot.pending) {
        BYZ_HIP(hipEventSynchronize(ev.second));
        float ms = 0.0f;
        BYZ_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
        slot.total_ms += ms;
        slot.launches += 1;
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    slot.pending.clear();
    if (total_ms) *total_ms = slot.total_ms;
    if (launches) *launches = slot.launches;
    return BYZ_OK;
}

int byz_selftest_lane_exchange_dev(byz_ctx* ctx, int32_t* out_dev, int32_t* n_patterns_host, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(out_dev && n_patterns_host, "selftest: bad arguments");
    return launch_lane_selftest(ctx, out_dev, n_patterns_host, as_stream(stream));
}

int byz_selftest_owner_loop_dev(byz_ctx* ctx, int32_t* out_dev, int32_t* n_rows_host, void* stream) {
    BYZ_TRY(enter(ctx));
    BYZ_REQUIRE(out_dev && n_rows_host, "selftest: bad arguments");
    return launch_owner_loop_selftest(ctx, out_dev, n_rows_host, as_stream(stream));
}

int byz_gram_unit_table(int64_t n_rows, int32_t* units_host, int64_t capacity_units, int64_t* n_units) {
    static_assert(kGramUnitWords == BYZ_GRAM_UNIT_WORDS, "the header describes GramUnit");
    if (n_rows < 1 || n_rows > 32767ll * 128 || !n_units || capacity_units < 0) return BYZ_E_INVALID;
    std::vector<GramUnit> units;
    std::vector<int32_t> slot_slab;
    build_gram_units(ceil_div(n_rows, 128), ceil_div(n_rows, 32), true, 1, 0, units, slot_slab);
    *n_units = static_cast<int64_t>(units.size());
    if (units_host) {
        const int64_t count = *n_units < capacity_units ? *n_units : capacity_units;
        std::memcpy(units_host, units.data(), static_cast<size_t>(count) * sizeof(GramUnit));
    }
    return BYZ_OK;
}

}  // extern "C"
