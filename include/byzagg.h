/*
 * byzagg -- C ABI of the MI355X (gfx950) Byzantine-robust aggregation engine.
 *
 * This is the drop-in boundary for the hot path of shaneson0/attacking_federate_learning:
 * what `defences.py` and `malicious.py` compute on the host with numpy, this library
 * computes on one GPU with hand-written HIP kernels.  Plain C types only: pointers, sizes,
 * a stream handle passed as `void*` (a `hipStream_t`, NULL = the default stream).  No torch
 * types cross this line.  The reference is pure Python, so a maintainer binds these with
 * ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - G is the (n_rows x n_cols) fp32 gradient matrix, row-major, leading dimension `ld`
 *     (elements).  It corresponds to `Server.users_grads` (reference server.py:34-35).
 *   - "_dev" pointers are device pointers; "_host" entry points take host pointers and do the
 *     staging copies themselves (pinned bounce buffers owned by the context).
 *   - Every call is asynchronous on `stream` unless it has a host output, in which case it
 *     returns after that output is valid.
 *   - Return value: BYZ_OK (0) or a negative BYZ_E_* code; `byz_last_error()` has the text.
 *     BYZ_E_PRECONDITION mirrors the reference's `assert`s (defences.py:25, 56): the Python
 *     shim turns it into AssertionError.
 *   - The context owns all workspaces (distance matrix, sort buffers, split-K slabs).  They
 *     grow on demand outside the kernels; `byz_ctx_reserve` pre-sizes them so that no
 *     allocation happens on the hot path.
 *   - One call in flight per context (the reference is single-threaded and synchronous).
 */
#ifndef BYZAGG_H
#define BYZAGG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BYZ_ABI_VERSION 1

enum {
    BYZ_OK = 0,
    BYZ_E_INVALID = -1,      /* bad argument (null pointer, negative size, ld < n_cols ...)   */
    BYZ_E_PRECONDITION = -2, /* the reference would raise AssertionError                       */
    BYZ_E_HIP = -3,          /* a HIP runtime call failed                                      */
    BYZ_E_UNSUPPORTED = -4,  /* size beyond what this build supports (see byz_limits)          */
    BYZ_E_NO_WINNER = -5,    /* Krum found no score < 1e20 (reference: index -1 / KeyError)    */
    BYZ_E_COLLECTIVE = -6    /* the caller's all-reduce (byz_allreduce_f64_fn) reported failure */
};

typedef struct byz_ctx byz_ctx;

/* ---- context -------------------------------------------------------------------------- */
int byz_abi_version(void);
const char* byz_last_error(void);                       /* thread-local text of the last failure */
int byz_ctx_create(int device, byz_ctx** out);
void byz_ctx_destroy(byz_ctx* ctx);
int byz_ctx_reserve(byz_ctx* ctx, int64_t n_rows, int64_t n_cols);
int byz_ctx_device(const byz_ctx* ctx);
/* Synchronises `stream` and reports what a kernel of an asynchronous call could only flag on the device:  */
/* BYZ_E_HIP when a Gram chunk never got its accumulation ticket (the distances of that call are invalid), */
/* BYZ_E_UNSUPPORTED when the near-duplicate pair list overflowed.  Entry points with a host output do this */
/* themselves.                                                                                             */
int byz_ctx_check(byz_ctx* ctx, void* stream);
/* largest supported row count for the selection kernels (rows of G: Krum, Bulyan) and for trimmed_mean: */
/* 2^20 both -- an index width, not a kernel's capacity: the reference has no limit (defences.py:23-70),   */
/* and beyond the 16,384 rows the LDS-resident kernels hold (BASELINE's largest configuration has 10,000   */
/* clients) the rows are sorted in global memory and the Bulyan loop runs in batches of picks              */
/* (csrc/large_rows.hip: the same results; Bulyan's selection of 20,000 rows: 0.9 s); memory -- 24 N^2     */
/* bytes of tables -- is what ends it in practice.  Beyond 2^20 the calls return BYZ_E_UNSUPPORTED.        */
/* trimmed_mean runs its fast kernels up to 5376 rows.                                                     */
int byz_limits(int64_t* max_rows_select, int64_t* max_rows_trimmed);

/* ---- raw device memory, so that a host without torch can still drive the library ------- */
int byz_malloc(byz_ctx* ctx, int64_t bytes, void** dev_ptr);
int byz_free(byz_ctx* ctx, void* dev_ptr);
int byz_upload(byz_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes, void* stream);
int byz_download(byz_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes, void* stream);
int byz_upload_2d(byz_ctx* ctx, void* dst_dev, int64_t dst_pitch_bytes, const void* src_host,
                  int64_t src_pitch_bytes, int64_t width_bytes, int64_t rows, void* stream);
int byz_stream_sync(byz_ctx* ctx, void* stream);

/* ---- defences.no_defense (reference defences.py:13-14) --------------------------------- */
/* out_dev[c] = mean over rows of G[:, c].                                                  */
int byz_no_defense_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols,
                       int64_t ld, float* out_dev, void* stream);

/* ---- defences._krum_create_distances (reference defences.py:16-21) --------------------- */
/* dist_dev: (n_rows x n_rows) fp32, row-major, unsquared L2 distances, diagonal = +inf     */
/* (the reference stores no self-distance).  Gram via fp32 MFMA, chunk partials in fp64.    */
int byz_pairwise_distances_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols,
                               int64_t ld, float* dist_dev, void* stream);
/* The two halves of the above, exposed for the D-sharded multi-GPU path: every rank computes */
/* the Gram of its column slice in fp64, the host all-reduces it, then every rank converts.   */
int byz_gram_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                 double* gram_dev, void* stream);
/* One rank's SHARE of a Gram, for ranks that all hold the same rows (the client-sharded path after an   */
/* all-gather of a column panel): every share_count-th 128 x 128 tile of the lower triangle starting with */
/* share_index is computed, the rest of gram_dev is written as zero, so that the SUM over the ranks is    */
/* the panel's Gram.  row_index_dev (optional): logical row r is G[row_index[r]] (skips padding rows of   */
/* the gathered panel).                                                                                    */
int byz_gram_share_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                       const int32_t* row_index_dev, int share_count, int share_index, double* gram_dev,
                       void* stream);
/* The same share ADDED into gram_dev (which the caller zeroed before the first panel): the sum over column  */
/* panels accumulates in the caller's one N x N buffer, in panel order, instead of through a separate N x N    */
/* addition pass per panel; entries of other ranks' tiles are left untouched.                                 */
int byz_gram_share_add_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                           const int32_t* row_index_dev, int share_count, int share_index, double* gram_dev,
                           void* stream);
int byz_distances_from_gram_dev(byz_ctx* ctx, const double* gram_dev, int64_t n_rows,
                                float* dist_dev, void* stream);
/* Near-duplicate pairs.  c_ii + c_jj - 2 c_ij cannot resolve rows that nearly coincide, the reference's  */
/* norm of the difference (defences.py:20) can.  byz_pairwise_distances_dev (and krum / bulyan) therefore  */
/* re-evaluate every pair with d^2 < (c_ii + c_jj)/16 on the difference itself.  A caller that only holds   */
/* a column slice of G (byz_distances_from_gram_dev on an all-reduced Gram) finishes the same step itself:  */
/* count -> per-rank sums of squared differences over the local columns -> (all-reduce) -> apply.           */
/* The list is ordered (ascending i, then j): slot p is the same pair on every GPU that holds the same Gram. */
/* A count > 0 OBLIGES the caller to finish with byz_near_pairs_apply_dev: until then listed entries hold    */
/* the Gram identity's value (possibly 0 by cancellation) and identical rows are not yet canonicalised.      */
int byz_near_pairs_count(byz_ctx* ctx, int64_t* count_host, void* stream);
int byz_near_pairs_sqdist_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                              const int32_t* row_index_dev, double* sq_dev, void* stream);
int byz_near_pairs_apply_dev(byz_ctx* ctx, const double* sq_dev, int64_t n_rows, float* dist_dev,
                             void* stream);

/* ---- defences.krum (reference defences.py:23-42) --------------------------------------- */
/* Selection loop only: ascending sort of every row's distances, sequential fp32 sum of the */
/* first (users_count - corrupted_count), candidates visited in order 1,0,2,3,... with a    */
/* strict '<' against 1e20.  *index_host = winner or -1.  scores_dev (optional, n_rows).    */
int byz_krum_select_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int64_t users_count,
                        int64_t corrupted_count, int32_t* index_host, float* scores_dev,
                        void* stream);
/* Whole function.  check_assert != 0 applies `users_count >= 2*corrupted_count + 1`        */
/* (the reference skips it when return_index=True).  out_row_dev (optional) receives a copy */
/* of the winning row (index -1 selects the last row, as numpy's G[-1] does).               */
int byz_krum_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                 int64_t users_count, int64_t corrupted_count, int check_assert,
                 float* out_row_dev, int32_t* index_host, void* stream);

/* ---- defences.trimmed_mean (reference defences.py:44-52) ------------------------------- */
/* Per column: fp32 median, keep the k = n_rows - corrupted_count - 1 values closest to it  */
/* (ties in |x - med| by row order), out = mean(kept - med) + med.  row_index_dev (optional)*/
/* selects and orders the rows: row r of the logical matrix is G[row_index[r]].  k follows  */
/* Python slice semantics (k == 0 -> NaN, k < 0 -> drop from the far end).                  */
int byz_trimmed_mean_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols,
                         int64_t ld, const int32_t* row_index_dev, int64_t corrupted_count,
                         float* out_dev, void* stream);

/* 16-column tiles of the last byz_trimmed_mean_dev (or Bulyan second stage) that the fast ring selection */
/* handed to the general kernel (ties at the window edge, outliers, non-finite values); synchronises.    */
int byz_trimmed_mean_redone(byz_ctx* ctx, int64_t* tiles_host, void* stream);

/* ---- the coordinate-wise median and the rank-trimmed mean (Yin et al. 2018; not in the reference) ---- */
/* Per column of the logical matrix (row r is G[row_index[r]] when row_index_dev is given), n = n_rows:   */
/*   median        np.median(col) for float32 input, bit for bit: the middle value for odd n, for even n  */
/*                 fl32(fl32(a + b) * 0.5f) of the two middle values; NaN if the column holds a NaN of    */
/*                 either sign.  +0.0 and -0.0 compare equal: which of the two comes back is unspecified. */
/*   rank-trimmed  kept = np.sort(col)[b : n - b] with b = trim_count, 0 <= b and 2 b < n (else           */
/*                 BYZ_E_INVALID); out = fl32(sum of kept in fp64 / (n - 2 b)).  NaN of either sign sorts */
/*                 behind +inf as np.sort has it, so up to b NaNs or infinities on a side are trimmed     */
/*                 away; a NaN that survives makes the column NaN, +inf and -inf both kept give NaN, one  */
/*                 of them kept gives that infinity.  The sum is S = sum{x : lo < x < hi} + c_lo * lo +   */
/*                 c_hi * hi in fp64 in a fixed order (lo, hi the order statistics of ranks b and         */
/*                 n - 1 - b, c_lo, c_hi >= 1 their kept copies), rounded to fp32 once after the division:*/
/*                 the same bits on every run and for every matrix width.  With ref the exactly rounded   */
/*                 mean of kept and mabs the mean of |kept|:                                              */
/*                 |out - ref| <= 2^-23 |ref| + 2^-30 mabs + 2^-149.  A column whose kept values are all  */
/*                 equal returns that value exactly; b = 0 is the column mean (in fp64: not no_defense's  */
/*                 bits); for NaN-free columns, odd n and b = (n - 1) / 2 it is the median exactly.       */
/* More than 2^20 rows (byz_limits' trimmed figure): BYZ_E_UNSUPPORTED.  Asynchronous on `stream`.        */
int byz_coordinate_median_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols,
                              int64_t ld, const int32_t* row_index_dev, float* out_dev, void* stream);
int byz_rank_trimmed_mean_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols,
                              int64_t ld, const int32_t* row_index_dev, int64_t trim_count,
                              float* out_dev, void* stream);

/* ---- the mean of the values nearest a centre; Phocas (Xie, Koyejo and Gupta 2018; not in the reference) */
/* Per column of the logical matrix (row r is G[row_index[r]] when row_index_dev is given), n = n_rows,   */
/* c = centre_dev[column] (given, not found) and 1 <= keep <= n (else BYZ_E_INVALID):                     */
/*   d      = fl32(col - c)                     one fp32 subtraction, never an FMA                        */
/*   a      = |d|                                                                                         */
/*   order  = np.argsort(a, kind='stable')      ties in |d| by LOGICAL row order; every NaN difference    */
/*                                              behind +inf, in row order                                 */
/*   kept   = order[:keep]                                                                                */
/*   radius = a[order[keep - 1]]                radius_dev (optional, n_cols floats): exact bits; when it */
/*                                              is NaN, which NaN is unspecified                          */
/*   out    = fl32(sum of col[kept] in fp64 / keep)                                                       */
/* The sum runs in a fixed order and is rounded to fp32 once after the division: the same bits on every   */
/* run and for every ld, base alignment and matrix width.  With ref the exactly rounded mean of col[kept] */
/* and mabs the mean of |col[kept]|: |out - ref| <= 2^-23 |ref| + 2^-30 mabs + 2^-149.  A kept NaN makes  */
/* the column NaN, +inf and -inf both kept give NaN, one of them kept gives that infinity.  A non-finite  */
/* centre is no special case (a NaN centre keeps the first `keep` rows).  A column whose kept values are  */
/* all equal returns that value exactly.  More than 2^20 rows: BYZ_E_UNSUPPORTED.  Asynchronous on        */
/* `stream`; nothing is launched when an argument is refused.                                             */
int byz_window_mean_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                        const int32_t* row_index_dev, const float* centre_dev, int64_t keep,
                        float* out_dev, float* radius_dev, void* stream);
/* Phocas: the window of keep = n_rows - trim_count values around the bits byz_rank_trimmed_mean_dev      */
/* returns for b = trim_count (0 <= b and 2 b < n, else BYZ_E_INVALID) -- by definition, so this call and */
/* the two calls made by hand agree bit for bit.  centre_out_dev (optional, n_cols floats): that trimmed  */
/* mean; radius_dev (optional) as above.  Must not alias each other or out_dev.                           */
int byz_phocas_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                   const int32_t* row_index_dev, int64_t trim_count, float* out_dev,
                   float* centre_out_dev, float* radius_dev, void* stream);

/* ---- defences.bulyan (reference defences.py:55-70) ------------------------------------- */
/* Selection loop on a distance matrix: theta = users_count - 2*corrupted_count picks, each */
/* the Krum winner among the rows still present.  Exact fp64 running scores pick the winner  */
/* outright when it is clear; otherwise the contenders are re-scored with the reference's    */
/* sequential fp32 sums (defences.py:33-34), so the selection is the reference's own.        */
/* selection_dev: theta int32 indices in selection order.                                   */
int byz_bulyan_select_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int64_t users_count,
                          int64_t corrupted_count, int32_t* selection_dev, void* stream);
/* Krum's index AND Bulyan's selection from one distance matrix with ONE sort of its rows (BASELINE       */
/* configs[4] runs both defences on the same distances): *krum_index_host as byz_krum_select_dev gives it, */
/* selection_dev as byz_bulyan_select_dev.                                                                  */
int byz_krum_bulyan_select_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int64_t users_count,
                               int64_t corrupted_count, int32_t* krum_index_host, int32_t* selection_dev,
                               void* stream);
/* Rows the last selection loop had to re-score in the reference's sequential fp32 arithmetic because   */
/* their exact scores lay within that arithmetic's rounding band (0 for well separated clients).        */
int byz_bulyan_rescored(const byz_ctx* ctx, int64_t* rows_host);
/* Whole function (asserts users_count >= 4*corrupted_count + 3).  selection_dev optional.  */
int byz_bulyan_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                   int64_t users_count, int64_t corrupted_count, float* out_dev,
                   int32_t* selection_dev, void* stream);

/* ---- Multi-Krum (Blanchard et al. 2017, section 4; not in the reference) ----------------- */
/* Every row's Krum score s_i -- exactly what byz_krum_select_dev writes to scores_dev: the    */
/* sequential fp32 sum of row i's first min(n_rows - 1, users_count - corrupted_count)         */
/* ascending distances (the reference's n - f, so that m = 1 is Krum) -- ranks the rows by     */
/* (s_i, visit position 1, 0, 2, 3, ...): every NaN after every number, -0.0 as +0.0, scores   */
/* >= 1e20 and +inf by value.  selection_dev: the first m rows in RANKING order; selection[0]  */
/* is Krum's index whenever Krum has one (it returns -1 when no score is below 1e20, Multi-Krum */
/* still ranks those rows).  The aggregate is np.mean(G[np.sort(selection)], axis=0): the      */
/* selected rows summed in ascending row order, sequential fp32 from +0.0, divided by (float)m  */
/* -- m = n_rows gives byz_no_defense_dev's bits.  1 <= m <= n_rows (BYZ_E_INVALID otherwise); */
/* n_rows up to byz_limits' selection limit.                                                   */
/* The mean of the rows row_index_dev[0..count) of G (device int32, each in [0, n_rows): the   */
/* caller vouches for it) in list order, no_defense's arithmetic; row_index in ascending order */
/* is Multi-Krum's aggregate.  The clients layout calls it on its re-sharded slices.           */
int byz_mean_rows_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                      const int32_t* row_index_dev, int64_t count, float* out_dev, void* stream);
/* Selection only, on a distance matrix (selection_dev: m int32).                            */
int byz_multi_krum_select_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int64_t users_count,
                              int64_t corrupted_count, int64_t m, int32_t* selection_dev, void* stream);
/* Whole function.  check_assert != 0 applies `users_count >= 2*corrupted_count + 1` as Krum  */
/* does.  out_dev: n_cols floats; selection_dev (optional): m int32 in ranking order.          */
int byz_multi_krum_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                       int64_t users_count, int64_t corrupted_count, int64_t m, int check_assert,
                       float* out_dev, int32_t* selection_dev, void* stream);

/* ---- geometric median (smoothed Weiszfeld; RFA, Pillutla et al.; not in the reference) --- */
/* G: n_rows x n_cols fp32, leading dimension ld; n_rows up to byz_limits' selection limit    */
/* (BYZ_E_UNSUPPORTED beyond), n_cols any.  The pieces:                                       */
/*   wmean(G, w)[c] = fl32(S_c / W): S_c the fp64 sum over the rows with w_i != 0 of          */
/*     w_i * (double)x_ic, W = sum w_i, both added sequentially in row order, no fused        */
/*     multiply-add; a row of weight 0 is skipped, not multiplied (0 * inf never reaches a     */
/*     column).  Every weight 0: the output is NaN.                                            */
/*   rowsq(G, z)[i] = sum_c ((double)x_ic - (double)z_c)^2 in fp64, on the difference (not    */
/*     |x|^2 - 2 x.z + |z|^2), in a fixed order: two calls give the same bits.                 */
/* The median:                                                                                 */
/*   mean0 = byz_no_defense_dev's bits.  Every mean0[c] finite: every row active, z = mean0.   */
/*   Otherwise s0 = rowsq(G, 0), active_i = isfinite(s0_i), z = wmean(G, active ? 1 : 0).     */
/*   No active row: out all NaN, iterations 0.  d = sqrt(rowsq(G, z)), F = sum of d over the   */
/*   active rows; for k = 1 .. max_iter: beta_i = active ? 1 / max(nu, d_i) : 0,               */
/*   z = wmean(G, beta) (fp32), d = sqrt(rowsq(G, z)), F_new = sum of active d,                */
/*   stop = |F - F_new| <= ftol * F_new, F = F_new, break on stop.  out = z.                   */
/* F, the stop test and beta are fp64 on the device: nothing synchronises, every launch of the */
/* loop is enqueued and those after the stop return at once.  A finite input costs            */
/* 2 + 2 * iterations passes over G.  weights_dev (optional, n_rows fp64): beta / sum(beta) of */
/* the last update, or uniform over the active rows when there was none (all 0 when no row is  */
/* active).  nu > 0, max_iter >= 0, ftol >= 0 (BYZ_E_INVALID otherwise, NaN included).  The    */
/* parameters travel in a struct: the ABI's by-value arguments are int, int64_t, float and     */
/* pointers.  Cost: 4 launches per update are enqueued for all max_iter updates, whatever the   */
/* stop (a launch after the stop returns in a few microseconds), so a large max_iter with       */
/* ftol > 0 still pays for its launches; max_iter beyond BYZ_GEOMED_MAX_ITER returns            */
/* BYZ_E_UNSUPPORTED.                                                                          */
#define BYZ_GEOMED_MAX_ITER 65536
typedef struct byz_geomed_params {
    double nu;          /* smoothing: the distances are floored at nu                          */
    int64_t max_iter;   /* Weiszfeld updates at most                                           */
    double ftol;        /* relative change of the objective that stops the loop                */
} byz_geomed_params;
/* One rank's part of rowsq over its columns (z_dev: n_cols floats; sq_dev: n_rows fp64).     */
int byz_row_sqdist_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                       const float* z_dev, double* sq_dev, void* stream);
/* wmean (w_dev: n_rows fp64; the caller vouches that they are finite and >= 0).              */
int byz_weighted_mean_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                          const double* w_dev, float* out_dev, void* stream);
/* The median (out_dev: n_cols floats).  Asynchronous; byz_geometric_median_info reads back   */
/* the last call's iterations, excluded (inactive) rows and objective F, and synchronises.     */
int byz_geometric_median_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                             const byz_geomed_params* params, float* out_dev, double* weights_dev,
                             void* stream);
int byz_geometric_median_info(byz_ctx* ctx, int64_t* iterations, int64_t* excluded_rows,
                              double* objective);
/* The median of a host matrix (out_host: n_cols floats; weights_host optional, n_rows fp64). */
int byz_geometric_median_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                              const byz_geomed_params* params, float* out_host, double* weights_host);

/* ---- centered clipping (Karimireddy, He & Jaggi, ICML 2021, Algorithm 2; not in the reference) ---- */
/* Every row is pulled towards a centre and no row moves the aggregate by more than tau / n:             */
/*   v_{l+1} = v_l + (1/n) sum_i (x_i - v_l) min(1, tau / |x_i - v_l|).                                 */
/* The centre is the caller's: the previous round's aggregate (the history the paper's title speaks of), */
/* or the zero vector, for which one iteration is the norm-clipped mean (Sun et al. 2019).              */
/* G: n x n_cols fp32 (n = n_rows up to byz_limits' selection limit, BYZ_E_UNSUPPORTED beyond), leading  */
/* dimension ld.  tau > 0, +inf allowed (NaN or tau <= 0: BYZ_E_INVALID); 0 <= iters (negative:          */
/* BYZ_E_INVALID) <= BYZ_CCLIP_MAX_ITER (beyond: BYZ_E_UNSUPPORTED).  start_dev: n_cols floats, optional */
/* (NULL: the zero vector); the caller vouches that it is finite.  From v_0 = start, for l = 0 .. iters-1:*/
/*   q = rowsq(G, v_l) (the geometric median's contract above: fp64, on the difference, fixed order),    */
/*   d_i = sqrt(q_i);  s_i = 1 if d_i <= tau, tau / d_i if tau < d_i < inf;                              */
/*   a row whose d_i is not finite (inf or NaN) is EXCLUDED: s_i = 0 and the row is skipped, not          */
/*   multiplied (0 * inf never reaches a column); it still counts in the divisor n -- a row clipped from  */
/*   infinitely far away contributes nothing;                                                             */
/*   v_{l+1}[c] = fl32((double)v_l[c] + S_c / n), S_c the fp64 sum over the rows with s_i != 0 of         */
/*   s_i * ((double)x_ic - (double)v_l[c]): on the difference, in a fixed order, no fused multiply-add.   */
/* out = v_iters (iters = 0: the bits of start).  Two calls give the same bits; so do a strided view and  */
/* its dense copy.  out_dev may be start_dev; it must not overlap G (BYZ_E_INVALID).  scales_dev          */
/* (optional, n fp64): the s of the LAST iteration (iters = 0: all 1).  byz_centered_clip_info reads that */
/* iteration's clipped rows (tau < d_i < inf) and excluded rows (iters = 0: both 0) and synchronises;     */
/* nothing else does: every launch is enqueued up front.  Cost: rowsq and the update per iteration, 2 *   */
/* iters passes over G.  Nothing measures the rows against the final centre: the scales and counts       */
/* reported are the ones the last update used.  The parameters travel in a struct: the ABI passes no      */
/* doubles by value.                                                                                      */
#define BYZ_CCLIP_MAX_ITER 65536
typedef struct byz_cclip_params {
    double tau;       /* clipping radius                                                                */
    int64_t iters;    /* clipping iterations                                                            */
} byz_cclip_params;
/* The piece: out[c] = fl32((double)v[c] + S_c / n_rows) with the caller's scales (n_rows fp64, finite;  */
/* a row of scale 0 is neither loaded nor multiplied), S_c added sequentially in row order.  out_dev may  */
/* be v_dev.  With byz_row_sqdist_dev it composes the iteration for every height.                         */
int byz_clip_update_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                        const float* v_dev, const double* scales_dev, float* out_dev, void* stream);
int byz_centered_clip_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                          const byz_cclip_params* params, const float* start_dev, float* out_dev,
                          double* scales_dev, void* stream);
int byz_centered_clip_info(byz_ctx* ctx, int64_t* clipped_rows, int64_t* excluded_rows);
/* Centered clipping of a host matrix (start_host optional, out_host: n_cols floats, scales_host          */
/* optional: n_rows fp64).  Synchronous.                                                                  */
int byz_centered_clip_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                           const byz_cclip_params* params, const float* start_host, float* out_host,
                           double* scales_host);

/* ---- FLTrust (Cao, Fang, Liu & Gong, NDSS 2021; not in the reference) ---- */
/* Trust bootstrapping: every row is compared with a gradient r the SERVER computed on its own small root      */
/* dataset.  A row's trust score is the ReLU of its cosine with r, a trusted row is rescaled to r's norm, and   */
/* the aggregate is the trust-weighted mean of the rescaled rows.  The one rule here with no bound on the number */
/* of malicious rows: a row pointing away from r gets no weight however many rows agree with it.  Computing r   */
/* is the caller's job.  G: n x n_cols fp32 (n = n_rows up to byz_limits' selection limit, BYZ_E_UNSUPPORTED     */
/* beyond), leading dimension ld; root_dev: n_cols fp32.  Everything below is fp64 on the device:               */
/*   p_i = sum_c (double)x_ic * (double)r_c     q_i = sum_c (double)x_ic^2     q0 = sum_c (double)r_c^2          */
/*   root_ok  = isfinite(q0) && q0 > 0                                                                          */
/*   usable_i = isfinite(p_i) && isfinite(q_i) && q_i > 0                                                       */
/*   c_i  = p_i / (sqrt(q_i) * sqrt(q0))            (this order of operations, no fused multiply-add)           */
/*   ts_i = root_ok && usable_i && c_i > 0 ? c_i : 0    (the ReLU of the cosine; not clamped at 1)              */
/*   w_i  = ts_i != 0 ? ts_i * (sqrt(q0) / sqrt(q_i)) : 0     (trust x rescaling to the root's norm)            */
/*   T    = sum_i ts_i                              (a fixed order, the same on every call)                     */
/*   S_c  = sum over the rows with w_i != 0 of w_i * (double)x_ic, added in row order, no fused multiply-add    */
/*   out[c] = T > 0 ? fl32(S_c / T) : 0                                                                         */
/* p, q and q0 are summed in rowsq's fixed order (lane sums, a fixed butterfly, the column chunks in chunk       */
/* order): two calls give the same bits, and so do a strided view and its dense copy.  A row with w_i = 0 is     */
/* neither loaded nor multiplied in the second pass (0 * inf never reaches a column).  The paper leaves the case */
/* of no trusted row undefined; here it is a zero step: when no row is trusted, or the root is zero or not       */
/* finite, out is 0 in every column and never NaN.  out_dev may be root_dev; it must not overlap G               */
/* (BYZ_E_INVALID).  trust_dev and weights_dev (optional, n fp64 each): ts and w.  byz_fltrust_info reads the    */
/* last call's trusted rows (ts_i > 0), excluded rows (p_i or q_i not finite), root_ok and T, and synchronises;  */
/* nothing else does: every launch is enqueued up front.  Cost: two passes over G.                               */
/* The first pass as a piece: dot_dev[i] = p_i and sq_dev[i] = q_i (n_rows fp64 each) in ONE read of G; on one    */
/* rank of the columns layout, its partial sums over its columns.                                                */
int byz_row_dots_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                     const float* r_dev, double* dot_dev, double* sq_dev, void* stream);
/* The second pass as a piece: out[c] = T > 0 ? fl32(S_c / T) : 0 with the caller's weights (n_rows fp64, finite; */
/* a row of weight 0 is neither loaded nor multiplied) and T = *divisor_dev (one device fp64).                   */
int byz_scaled_rows_sum_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                            const double* w_dev, const double* divisor_dev, float* out_dev, void* stream);
int byz_fltrust_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                    const float* root_dev, float* out_dev, double* trust_dev, double* weights_dev, void* stream);
int byz_fltrust_info(byz_ctx* ctx, int64_t* trusted_rows, int64_t* excluded_rows, int32_t* root_ok,
                     double* trust_sum);
/* FLTrust of a host matrix and a host root (out_host: n_cols floats; trust_host and weights_host optional:      */
/* n_rows fp64).  Synchronous.                                                                                  */
int byz_fltrust_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const float* root_host,
                     float* out_host, double* trust_host, double* weights_host);

/* ---- SignGuard (Xu, Huang, Song & Lan, "Byzantine-robust Federated Learning through Collaborative Malicious Gradient       */
/* Filtering", ICDCS 2022; not in the reference) ----                                                                       */
/* A row built to sit among its neighbours in DISTANCE (the reference's "A Little Is Enough" attack, mean - z * std) still   */
/* has visibly different shares of positive, zero and negative coordinates.  SignGuard filters the rows whose norm is far    */
/* from the median norm, clusters the rows on those three shares taken over a window of the columns, keeps the largest       */
/* cluster, clips the kept rows to the median norm and averages them.  Nothing is of order n^2: one read of G and one        */
/* weighted sum over the kept rows.  The library draws nothing: the caller passes the window and the sampled rows, so that    */
/* a call is deterministic.  G: n x n_cols fp32 (n = n_rows up to byz_limits' selection limit, BYZ_E_UNSUPPORTED beyond),     */
/* leading dimension ld.  Everything after the census is fp64 on the device, in the stated order, no fused multiply-add.     */
/* The census, over the window [window_start, window_start + window_len) of the columns (m = window_len):                    */
/*   q_i = sum_c (double)x_ic^2 over ALL columns, in rowsq's fixed order: the bits of byz_row_dots_dev's sq_dev;             */
/*   pos_i, zero_i, neg_i = the window's values that are > 0, == 0, < 0, decided on the BITS as the robust learning rate's   */
/*   votes are: +0.0 and -0.0 are zeros, denormals and infinities count by their sign, a NaN counts nowhere.  Exact.         */
/* The selection:                                                                                                           */
/*   norm_i = sqrt(q_i);  M = np.median of the norms of the rows with a finite q_i (an even count: the mean of the two       */
/*   middle values; no such row: M = NaN and no row passes);                                                                */
/*   norm_ok_i = isfinite(q_i) && lower * M < norm_i && norm_i < upper * M          (both strict)                            */
/*   P_i = pos_i / m, Z_i = zero_i / m, N_i = neg_i / m;                                                                    */
/*   x_i = (P_i / (max_j P_j + 1e-8), Z_i / (max_j Z_j + 1e-8), N_i / (max_j N_j + 1e-8))  for EVERY row (the authors'        */
/*   normalisation);  distances below are ((dx*dx + dy*dy) + dz*dz), compared squared against h*h.                           */
/*   Bandwidth: h = params->bandwidth when that is > 0.  Otherwise, over the s = n_sample sampled rows (distinct row numbers, */
/*   device int32; 1 <= s <= BYZ_SIGNGUARD_MAX_SAMPLES, BYZ_E_INVALID otherwise) and k = max(1, s / 2): h = the mean, in      */
/*   sample order, of the k-th smallest of the s distances sqrt(.) from a sampled row to the sampled rows, itself included    */
/*   -- scikit-learn's estimate_bandwidth(quantile = 0.5) on that sample.  If h is 0, not finite, or below 2^-20 (the bins    */
/*   pack 21 bits a coordinate), the selection is FLAT: every row has label 0, one cluster, no seeds.                        */
/*   Mean shift, flat kernel, bin seeding (scikit-learn's MeanShift(bandwidth = h, bin_seeding = True, cluster_all = False),  */
/*   as the authors run it): the seeds are h * b for every distinct b = rint(x_i / h) (ties to even).  From a seed, the       */
/*   members are the rows at squared distance <= h*h, the new centre is the members' sum (a fixed order) divided by their     */
/*   count; stop when the move sqrt(.) is <= 1e-3 * h or after 300 updates.  A seed whose last member count is 0 is dropped. */
/*   The centres are ordered by member count descending, then by their coordinates descending lexicographically; going        */
/*   through them in that order, a centre still standing removes every later centre at squared distance <= h*h.  A row's      */
/*   label is the number, in that order, of the nearest standing centre, the first on ties, or -1 when that centre is         */
/*   farther than h.  benign = the label >= 0 with the most rows, the lowest on ties.                                        */
/*   keep_i = norm_ok_i && label_i == benign;  K = the number of kept rows;  w_i = keep_i ? min(1, M / norm_i) : 0.          */
/* The sum: out[c] = K > 0 ? fl32(S_c / K) : 0, S_c = the sum over the rows with w_i != 0 of w_i * (double)x_ic in row order  */
/* (byz_scaled_rows_sum_dev).  No kept row gives the zero vector, never NaN (FLTrust's convention); a dropped row is neither  */
/* loaded nor multiplied.  lower = 0.1 and upper = 3.0 are the paper's values; the window of a tenth of the columns, the      */
/* quantile 0.5 and the 50 sampled rows are the authors' code's.  0 <= lower, lower < upper (+inf allowed), bandwidth >= 0    */
/* (NaN anywhere: BYZ_E_INVALID); window_start >= 0, window_len >= 1, inside the columns.  out_dev must not overlap G.        */
/* Everything is asynchronous on `stream`; only byz_signguard_info synchronises.  Two calls give the same bits; so do a       */
/* strided view and its dense copy.  The parameters travel in a struct: the ABI passes no doubles by value.                  */
#define BYZ_SIGNGUARD_MAX_SAMPLES 1024
typedef struct byz_signguard_params {
    int64_t window_start;   /* first column of the census window                                                          */
    int64_t window_len;     /* m: its length, the divisor of the shares (sharded: the GLOBAL window's length)               */
    double lower, upper;    /* the norm filter's bounds, in units of the median norm                                       */
    double bandwidth;       /* > 0: h; 0: estimated from the sampled rows                                                   */
    int64_t n_sample;       /* s: the sampled rows (read only when bandwidth is 0)                                          */
} byz_signguard_params;
/* The census as a piece: counts_dev = 3 * n_rows int64 (pos, then zero, then neg), q_dev = n_rows fp64, in ONE read of G.   */
/* window_len = 0 is allowed (all counts 0); on one rank of the columns layout, its part of q and of the window.             */
int byz_row_signs_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t window_start,
                      int64_t window_len, int64_t* counts_dev, double* q_dev, void* stream);
/* The selection as a piece, from counts and q of that form (the caller vouches that the counts are >= 0 and <= window_len): */
/* keep_dev (n int32, 0 / 1), weights_dev (n fp64), labels_dev (n int32), each optional; mk_dev (optional): two fp64, M and K. */
int byz_signguard_select_dev(byz_ctx* ctx, const int64_t* counts_dev, const double* q_dev, int64_t n_rows,
                             const byz_signguard_params* params, const int32_t* sample_dev, int32_t* keep_dev,
                             double* weights_dev, int32_t* labels_dev, double* mk_dev, void* stream);
int byz_signguard_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                      const byz_signguard_params* params, const int32_t* sample_dev, float* out_dev, int32_t* keep_dev,
                      double* weights_dev, int32_t* labels_dev, void* stream);
/* The last selection on this context: the kept rows, the rows failing the norm filter, the rows outside the benign cluster,  */
/* the clusters found, the seeds, h and M.  Synchronises that call's stream; nothing else does.                              */
int byz_signguard_info(byz_ctx* ctx, int64_t* kept_rows, int64_t* norm_failed_rows, int64_t* outside_rows, int64_t* clusters,
                       int64_t* seeds, double* bandwidth, double* median_norm);
/* SignGuard of a host matrix (sample_host: params->n_sample int32, checked: distinct and in range, BYZ_E_INVALID otherwise;  */
/* out_host: n_cols floats; keep_host, weights_host, labels_host optional).  Synchronous.                                    */
int byz_signguard_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_signguard_params* params,
                       const int32_t* sample_host, float* out_host, int32_t* keep_host, double* weights_host,
                       int32_t* labels_host);

/* ---- nearest-neighbour mixing, NNM (Allouah, Farhadkhani, Guerraoui, Gupta, Pinot & Stephan, "Fixing by Mixing", AISTATS  */
/* 2023; not in the reference) ----                                                                                        */
/* A PRE-aggregation: every row of G is replaced by the mean of its k = users_count - corrupted_count nearest rows, itself  */
/* included, and the mixed n x n_cols matrix Y is what Krum, a trimmed mean, the median or the geometric median then see;  */
/* the paper shows that this makes those rules order-optimal under heterogeneous data.  G: n x n_cols fp32 (n = n_rows),    */
/* leading dimension ld.  1 <= k <= n (BYZ_E_INVALID otherwise); n up to 16,384 (BYZ_E_UNSUPPORTED beyond, decided on the   */
/* argument alone: the sort keys and the mask are n x n).                                                                  */
/* Neighbour lists, from a distance matrix as byz_pairwise_distances_dev writes it (n x n fp32, diagonal +inf):             */
/*   row i's candidates are the other rows j, ordered by the key (distance bits in order-preserving form, then j): -0.0     */
/*   counts as +0.0 and every NaN sorts behind +inf; the first k - 1 candidates are taken, those whose distance is not      */
/*   finite are dropped, i itself is added, and the list is stored in ASCENDING row order with its length k_i <= k.  The     */
/*   key order is total, so ties (an attack's identical rows) are decided the same way on every run.  A row with a          */
/*   non-finite value has only non-finite distances: it is in nobody's list and its own list is {i}.                        */
/* Mix: Y[i] = np.mean(G[list_i], axis=0) bit for bit: the listed rows added in ascending row order, sequential fp32 from   */
/*   +0.0, divided (a true division) by (float)k_i -- byz_mean_rows_dev's and byz_no_defense_dev's arithmetic.  list_i =    */
/*   {i}: row i of Y is row i of G copied verbatim, NaN and inf included.  A value of a row outside list_i never reaches    */
/*   Y[i] (0 * inf does not either).  So k = n makes every row of Y byz_no_defense_dev's bits, and k = 1 gives Y = G.       */
/*   The sum is ONE accumulator chain of the fp32-input matrix instruction over j = 0 .. n - 1 (a multiplier of exactly 1    */
/*   or 0: fma(1, x, c) = fl32(c + x), fma(0, x, c) = c); the rows of G are read through isfinite(x) ? x : 0, which changes  */
/*   no value that is used.  Cost: 2 n^2 n_cols flops on the matrix pipe, whatever k.                                       */
/* Y must not overlap G (BYZ_E_INVALID), ldy >= n_cols.  Everything is asynchronous on `stream`; only byz_nnm_info           */
/* synchronises.                                                                                                           */
/* The lists: nbr_dev n_rows x k int32, row i = list_i ascending, the unused tail -1; counts_dev (optional) n_rows int32.   */
int byz_nnm_neighbours_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int64_t k, int32_t* nbr_dev,
                           int32_t* counts_dev, void* stream);
/* The mix for ANY lists of that form (each entry in [0, n_rows), ascending, no row twice: the caller vouches; an entry out  */
/* of range is ignored).  counts_dev optional: without it a list ends at its first negative entry.  The caller may walk the  */
/* columns in panels -- G_dev + c0, Y_dev + c0, the same ld and ldy -- which is how a matrix too large to hold twice is      */
/* mixed; the panels' results are the one call's bits.                                                                      */
int byz_nnm_mix_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* nbr_dev,
                    const int32_t* counts_dev, int64_t k, float* Y_dev, int64_t ldy, void* stream);
/* Distances, lists, mix.  nbr_dev (optional): n_rows x (users_count - corrupted_count) int32.                              */
int byz_nnm_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t users_count,
                int64_t corrupted_count, float* Y_dev, int64_t ldy, int32_t* nbr_dev, void* stream);
/* The last neighbour search: solo_rows = rows with k_i == 1 < k, short_rows = rows with k_i < k; synchronises its stream.  */
int byz_nnm_info(byz_ctx* ctx, int64_t* solo_rows, int64_t* short_rows);
/* NNM of a host matrix (Y_host: n_rows x n_cols floats; nbr_host optional, as nbr_dev).  Synchronous.                      */
int byz_nnm_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t users_count,
                 int64_t corrupted_count, float* Y_host, int32_t* nbr_host);

/* ---- the robust learning rate, RLR (Ozdayi, Kantarcioglu & Gel, "Defending against Backdoors in Federated Learning with  */
/* Robust Learning Rate", AAAI 2021; not in the reference) ----                                                            */
/* The defence designed for the backdoor attack.  Per coordinate the server sums the SIGNS of the clients' updates; where   */
/* the absolute value of that sum is below a threshold theta, the learning rate of that coordinate is negated for the       */
/* round.  No rule of its own: it wraps an aggregate (the paper wraps FedAvg, clipping and the median).  With the           */
/* reference's update v = momentum v - lr agg, negating agg[c] is the negated learning rate of coordinate c.  G: n x n_cols  */
/* fp32 (n = n_rows up to the selection limit of byz_limits, BYZ_E_UNSUPPORTED beyond), leading dimension ld:                */
/*   votes[c] = #{ r : G[r][c] > 0 } - #{ r : G[r][c] < 0 }                                   (int32)                        */
/*   flip[c]  = |votes[c]| < theta                                                                                          */
/*   out[c]   = flip[c] ? agg[c] with its sign bit inverted : agg[c] verbatim                                                */
/* A value's vote is decided on its bits with integer comparisons (sign bit; magnitude in (0, 0x7f800000]): +0.0, -0.0 and   */
/* NaN cast no vote, +-inf and denormals vote by their sign, whatever the denormal mode.  The flip is an XOR of the sign     */
/* bit: a zero becomes -0.0, a NaN keeps its payload; a non-finite aggregate passes through (agg is not sanitised).  theta   */
/* is an integer in [0, n_rows] (BYZ_E_INVALID outside); theta = 0 returns agg's bits untouched.  The paper fixes no formula */
/* for theta; corrupted_count + 1, the smallest threshold that corrupted_count colluding clients cannot reach on their own,  */
/* is the Python layer's default and this package's choice.  sign(votes) is signSGD's majority vote (Bernstein et al. 2019). */
/* Everything is asynchronous on `stream`; only byz_robust_lr_info synchronises.  The vote is local to a column: a rank of    */
/* the columns layout calls these entry points on its own columns, so no sharded entry point exists (a panel's results are   */
/* the one call's bits).                                                                                                    */
/* The vote alone (votes_dev: n_cols int32): one read of G.                                                                 */
int byz_sign_votes_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t* votes_dev,
                       void* stream);
/* The flip of ANY aggregate (agg_dev: n_cols fp32, e.g. a trimmed mean's or a median's result) by given votes; out_dev may   */
/* be agg_dev.  0 <= theta <= the selection limit (the row count is not known here).                                         */
int byz_sign_flip_dev(byz_ctx* ctx, const float* agg_dev, const int32_t* votes_dev, int64_t n_cols, int64_t theta,
                      float* out_dev, void* stream);
/* Fused, agg = the column mean: out_dev = byz_no_defense_dev's bits (a sequential fp32 chain from +0.0 in row order, then   */
/* / (float)n_rows) with the flips applied, the vote counted in the same walk: G is read once.  votes_dev_or_null: n_cols    */
/* int32.  out_dev must not overlap G (BYZ_E_INVALID).                                                                      */
int byz_robust_lr_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t theta,
                      float* out_dev, int32_t* votes_dev_or_null, void* stream);
/* The columns flipped by the last of the three calls above on this context (byz_sign_votes_dev has no threshold: 0);        */
/* synchronises that call's stream.                                                                                         */
int byz_robust_lr_info(byz_ctx* ctx, int64_t* flipped_cols);
/* The fused call on a host matrix (out_host: n_cols floats; votes_host_or_null: n_cols int32).  Synchronous.                */
int byz_robust_lr_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t theta, float* out_host,
                       int32_t* votes_host_or_null);

/* ---- s-bucketing (Karimireddy, He & Jaggi, "Byzantine-Robust Learning on Heterogeneous Datasets via Bucketing", ICLR      */
/* 2022; not in the reference) ----                                                                                        */
/* A PRE-aggregation: the clients are shuffled, every s consecutive ones are replaced by their mean, and the B = ceil(n/s)  */
/* bucket means are what Krum, the median, the geometric median or centered clipping then see (behind the median it is      */
/* median-of-means).  G: n x n_cols fp32 (n = n_rows up to byz_limits' selection limit, BYZ_E_UNSUPPORTED beyond, decided   */
/* on the argument alone), leading dimension ld.  perm: a permutation of 0 .. n-1 as int32, NULL for the identity.          */
/* 1 <= s <= n (BYZ_E_INVALID otherwise).  Bucket b holds the rows perm[b s .. min((b+1) s, n) - 1] in that order; the last  */
/* bucket may be short; c_b is a bucket's length.                                                                           */
/*   Y[b] = np.mean(G[perm[b*s : (b+1)*s]], axis=0) bit for bit: the bucket's rows added in list order, sequential fp32     */
/*   from +0.0, divided (a true division) by (float)c_b -- byz_mean_rows_dev's and byz_no_defense_dev's arithmetic.  So     */
/*   s = n with the identity makes the single row of Y byz_no_defense_dev's bits, and s = 1 makes Y a row-permuted copy of  */
/*   G: x + 0.0 and then / 1.0f change no bit except that -0.0 becomes +0.0 (the chain starts at +0.0; not special-cased).  */
/* Nothing is sanitised: a NaN or an infinity in a row reaches its bucket's mean in that column as IEEE arithmetic gives it, */
/* and no other element of Y.  A poisoned row spoils one bucket, which the rule behind treats as one bad row: the paper's    */
/* accounting, in which at most f of the B buckets are contaminated.                                                        */
/* Y: B x n_cols, leading dimension ldy >= n_cols; it must not overlap G (BYZ_E_INVALID).  Everything is asynchronous on     */
/* `stream`; nothing synchronises with the host.  Cost: one read of G and one write of Y.                                   */
/* On the device entry point the caller vouches for perm; an entry outside [0, n) is skipped without being used as a row     */
/* number (it cannot fault) and the divisor stays c_b.  The caller may walk the columns in panels -- G_dev + c0, Y_dev + c0, */
/* the same ld and ldy --; the panels' results are the one call's bits.  The operation is local to a column: with the same   */
/* perm on every rank, a rank of the columns layout calls this entry point on its own columns and no collective is needed,   */
/* so no sharded entry point exists.                                                                                        */
int byz_bucket_means_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                         const int32_t* perm_dev_or_null, int64_t s, float* Y_dev, int64_t ldy, void* stream);
/* The same on a host matrix (Y_host: B x n_cols floats).  perm_host_or_null is checked: anything but a permutation of       */
/* 0 .. n-1 is BYZ_E_INVALID.  Synchronous.                                                                                 */
int byz_bucket_means_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                          const int32_t* perm_host_or_null, int64_t s, float* Y_host);

/* ---- SparseFed: global top-k with error feedback (Panda, Mahloujifar, Bhagoji, Chakraborty & Mittal, "SparseFed:          */
/* Mitigating Model Poisoning Attacks in Federated Learning with Sparsification", AISTATS 2022; not in the reference) ----   */
/* The second defence against the backdoor attack, certified against model poisoning: every client is clipped to norm L and  */
/* the clipped updates are averaged; the average is added to an error-feedback memory W; only the k coordinates of W with    */
/* the largest magnitude are applied and cleared, the rest stay in W for later rounds.                                       */
/* The new piece is a selection ALONG a vector of n fp32 values, byz_topk_sparsify_dev:                                      */
/*   w[c]   = add given ? fl32(x[c] + add[c]) : x[c]                    one fp32 addition: the error-feedback step fused in   */
/*   key[c] = bits(w[c]) & 0x7fffffff                                   31 bits, compared as integers                         */
/*   the k columns first in the order (key descending, column index ascending) are SELECTED                                  */
/*   out[c] = selected ? w[c] : +0.0          residual[c] = selected ? +0.0 : w[c]            w's bits verbatim               */
/* The key is decided on the bits whatever the denormal mode: +0.0 and -0.0 tie at key 0, denormals rank by their bits, both  */
/* infinities rank above every finite value and a NaN of either sign above the infinities, where its bits fall.  NOTHING IS  */
/* SANITISED (bucketing's and the robust learning rate's convention): a NaN in the memory is selected first and shows in the */
/* step instead of being parked in W for ever; a selected -0.0 or NaN payload comes back as it is.  Equivalently, with T the */
/* k-th largest key: every column with key > T is selected (`above` of them) and of the `ties` columns with key == T the      */
/* first k - above in index order.  The order is total: two runs, an aligned and a misaligned caller and the sharded path    */
/* select the same set.  k = 0: out all +0.0, residual = w.  k = n: out = w, residual all +0.0.                               */
/* n >= 1, k in [0, n] (BYZ_E_INVALID outside); add_dev_or_null and residual_dev_or_null are optional.  residual_dev may be   */
/* x_dev and out_dev may be add_dev (the in-place round: W updated where it lies, the step written over the aggregate); the   */
/* two inputs may overlap each other; any other overlap of an output with another vector: BYZ_E_INVALID, nothing written.     */
/* A three-pass radix select (11 + 10 + 10 bits) with integer atomics only, so no bit depends on the scheduling; every launch */
/* is enqueued up front and nothing synchronises with the host.  Cost: four reads of x (and add), five when the ties at T    */
/* are rationed, and one write of out (and residual).                                                                        */
int byz_topk_sparsify_dev(byz_ctx* ctx, const float* x_dev, const float* add_dev_or_null, int64_t n, int64_t k,
                          float* out_dev, float* residual_dev_or_null, void* stream);
/* The last top-k call on this context: selected (== k), the threshold key T (0xffffffff for k = 0: above every key), the    */
/* ties at T and how many of them were taken (the sharded call: the global figures).  Synchronises that call's stream.       */
int byz_topk_info(byz_ctx* ctx, int64_t* selected, uint32_t* threshold_key, int64_t* ties, int64_t* ties_taken);
/* The same on host vectors (out_host: n floats; add_host_or_null, residual_host_or_null optional; residual_host may be       */
/* x_host and out_host may be add_host).  Synchronous.                                                                       */
int byz_topk_sparsify_host(byz_ctx* ctx, const float* x_host, const float* add_host_or_null, int64_t n, int64_t k,
                           float* out_host, float* residual_host_or_null);

/* SparseFed's round.  agg = byz_centered_clip_dev(G, tau = clip, iters = 1, start = NULL) into a context workspace (its     */
/* contract and its checks: clip > 0, +inf allowed; non-finite rows excluded and still counted in n), then                   */
/* byz_topk_sparsify_dev(x = residual, add = agg, n_cols, k, out, residual) in place on residual_dev (n_cols floats, in/out,  */
/* the caller's memory W; the caller zeroes it before the first round).  out_dev must not overlap G or residual_dev, and      */
/* residual_dev must not overlap G (BYZ_E_INVALID).  byz_centered_clip_info and byz_topk_info describe the call.  No doubles  */
/* by value, as elsewhere.                                                                                                   */
typedef struct byz_sparsefed_params {
    double clip;    /* the clients' norm bound L: > 0, +inf allowed */
    int64_t k;      /* coordinates applied per round: 0 .. n_cols   */
} byz_sparsefed_params;
int byz_sparsefed_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                      const byz_sparsefed_params* params, float* residual_dev, float* out_dev, void* stream);
/* The same on a host matrix (residual_host: n_cols floats, in/out; out_host: n_cols floats).  Synchronous.                  */
int byz_sparsefed_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_sparsefed_params* params,
                       float* residual_host, float* out_host);

/* ---- Clip and noise, "weak DP" (Sun, Kairouz, Suresh & McMahan, "Can You Really Backdoor Federated Learning?", 2019;      */
/* FLAME's last stage, Nguyen et al., USENIX Security 2022; DP-FedAvg's server step; not in the reference) ----              */
/* The baseline the backdoor defences measure themselves against: every client clipped to a norm bound, the clipped updates  */
/* averaged, Gaussian noise added to the average.  The clipped mean is byz_centered_clip_dev from zero with one iteration;   */
/* the new piece is the noise, drawn ON THE DEVICE from a counter-based Philox4x32-10 stream (Salmon et al., SC'11) that is  */
/* addressed by GLOBAL COLUMN:                                                                                               */
/*   key = (low, high word of seed);  counter = (low word of b, high word of b, low word of round, high word of round),      */
/*   b = global_column >> 2;  word i (0..3) of block b belongs to global column 4 b + i                                      */
/*   normals, all in fp64, one Box-Muller pair p in {0, 1} per two words x:                                                  */
/*     u1 = (x[2p] + 0.5) * 2^-32,  u2 = (x[2p+1] + 0.5) * 2^-32,  r = sqrt(-2 log(u1)),  t = fl64(6.283185307179586 * u2),  */
/*     z[4b + 2p] = r cos(t),  z[4b + 2p + 1] = r sin(t)                                                                     */
/*   out[c] = fl32((double)x[c] + sigma_eff * z[column_offset + c]),  sigma_eff = sigma * (scale_dev ? *scale_dev : 1.0)     */
/* The integers are the same bit for bit for one call, a misaligned caller and any split of the columns over ranks (each     */
/* rank passes the global index of its first column as column_offset); the normals are those integers through the device's   */
/* fp64 log, sin and cos, which agree with another math library's to a few fp64 ulp, far below the one fp32 rounding.        */
/* `round` is the caller's round counter: one seed, fresh noise every round.  scale_dev_or_null is ONE device double read by  */
/* the kernel (the adaptive clip), so no call here synchronises with the host.                                               */
/* n >= 1, column_offset >= 0, column_offset + n <= 2^62, sigma finite and >= 0: BYZ_E_INVALID otherwise, nothing written.    */
/* out_dev may be x_dev (in place); any other overlap: BYZ_E_INVALID.  sigma == 0 with no scale writes x's bits verbatim.     */
/* A NaN or an infinity in x stays where it is: nothing is sanitised.  No doubles by value, as elsewhere.                     */
typedef struct byz_noise_params {
    double sigma;           /* the standard deviation: finite, >= 0 (times *scale_dev when given)  */
    uint64_t seed;          /* the stream's key                                                     */
    uint64_t round;         /* the caller's round counter: counter words 2 and 3                    */
    int64_t column_offset;  /* the global column of x[0]: >= 0                                      */
} byz_noise_params;
int byz_gaussian_noise_dev(byz_ctx* ctx, const float* x_dev, int64_t n, const byz_noise_params* params,
                           const double* scale_dev_or_null, float* out_dev, void* stream);
/* The raw stream: words_dev[c] = the 32-bit word of global column column_offset + c (n of them; sigma is not read).          */
int byz_noise_words_dev(byz_ctx* ctx, const byz_noise_params* params, int64_t n, uint32_t* words_dev, void* stream);
/* The same on host vectors (out_host may be x_host).  Synchronous.                                                          */
int byz_gaussian_noise_host(byz_ctx* ctx, const float* x_host, int64_t n, const byz_noise_params* params, float* out_host);

typedef struct byz_weak_dp_params {
    double clip;            /* fixed mode: the clients' norm bound, > 0 (+inf allowed); adaptive mode: not read        */
    double sigma;           /* fixed mode: the noise's standard deviation; adaptive mode: FLAME's lambda, the noise's   */
                            /* standard deviation is sigma * clip; finite, >= 0                                         */
    int64_t adaptive;       /* 0: clip as given; otherwise clip = the median of the finite rows' norms                  */
    uint64_t seed;
    uint64_t round;
    int64_t column_offset;  /* the global column of column 0 of G: >= 0                                                 */
} byz_weak_dp_params;
/* The clipping piece.  sq_dev: the n_rows fp64 squared norms q of byz_row_sqdist_dev with a zero centre.  d_i = sqrt(q_i).   */
/* Fixed mode: clip = params->clip.  Adaptive mode: clip = np.median of d_i over the rows with finite q_i (the middle value,  */
/* or the mean of the two middle values: SignGuard's definition and its key-and-sort route); no finite row: clip = 0.         */
/* scales_dev[i] = 1 (d_i <= clip), clip / d_i (clip < d_i < inf), 0 (q_i not finite: the row is excluded and still counted   */
/* in n, centered clipping's convention); clip = 0: every scale 0.  clip_dev_or_null receives the one fp64 clip.  In the      */
/* fixed mode the scales are those byz_centered_clip_dev (iters = 1, start = NULL) reports, bit for bit.  Only clip (fixed   */
/* mode) and adaptive are read.  n_rows up to 2^20.                                                                          */
int byz_clip_scales_dev(byz_ctx* ctx, const double* sq_dev, int64_t n_rows, const byz_weak_dp_params* params,
                        double* scales_dev, double* clip_dev_or_null, void* stream);
/* The last byz_clip_scales_dev or byz_weak_dp_dev on this context: the rows clipped (clip < d < inf), the rows excluded,     */
/* the clip used.  Synchronises that call's stream.                                                                          */
int byz_weak_dp_info(byz_ctx* ctx, int64_t* clipped_rows, int64_t* excluded_rows, double* clip);
/* The whole defence: byz_row_sqdist_dev's norms (zero centre), byz_clip_scales_dev, byz_clip_update_dev from the zero        */
/* vector, then the noise in place on out_dev with sigma_eff = sigma (fixed) or sigma * clip (adaptive, read on the device). */
/* In the fixed mode the result before the noise has byz_centered_clip_dev(iters = 1)'s bits, and sigma = 0 returns them.    */
/* Every launch is enqueued up front; nothing synchronises with the host.  out_dev must not overlap G (BYZ_E_INVALID).       */
/* There is NO SHARDED ENTRY POINT: the noise is local to a column given column_offset, and the norms are the one all-reduce */
/* of n_rows doubles that byz_centered_clip_sharded_dev already makes.  A host of the columns layout calls                   */
/* byz_centered_clip_sharded_dev (iters = 1, no start) and byz_gaussian_noise_dev with its slice's column_offset in the      */
/* fixed mode; in the adaptive mode byz_row_sqdist_dev, its all-reduce, byz_clip_scales_dev, byz_clip_update_dev and         */
/* byz_gaussian_noise_dev with scale_dev = the clip.                                                                         */
int byz_weak_dp_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                    const byz_weak_dp_params* params, float* out_dev, void* stream);
/* The same on a host matrix (out_host: n_cols floats).  Synchronous.                                                        */
int byz_weak_dp_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_weak_dp_params* params,
                     float* out_host);

/* ---- FLAME (Nguyen et al., "FLAME: Taming Backdoors in Federated Learning", USENIX Security 2022; not in the reference) ---- */
/* The backdoor defence that robust_lr, sparsefed and weak_dp are measured against: (1) pairwise COSINE distances between the    */
/* clients, (2) HDBSCAN (Campello, Moulavi & Sander 2013) with min_cluster_size = n / 2 + 1, everything outside the one majority  */
/* cluster rejected, (3) the admitted clients clipped to the median norm of ALL clients and averaged, (4) Gaussian noise of       */
/* standard deviation lambda * clip.  Stages 3 and 4 are byz_clip_scales_dev (adaptive) and byz_gaussian_noise_dev.               */
/* Cosine distances, from the fp64 Gram g as byz_gram_dev writes it (n x n, both triangles):                                      */
/*   c_ij = fl32(max(0, 1 - g_ij / (sqrt(g_ii) * sqrt(g_jj)))), in fp64 in this order of operations, rounded once.  The diagonal  */
/*   is +inf, byz_pairwise_distances_dev's convention.  A row with g_ii not finite or <= 0 (a zero or non-finite client) is       */
/*   BROKEN: its whole row and column are +inf; a non-finite g_ij gives +inf as well.  Entry (i, j) is computed from the lower    */
/*   triangle's g at (max(i, j), min(i, j)), so the matrix is symmetric bit for bit.  n up to 16,384 (BYZ_E_UNSUPPORTED beyond).  */
int byz_cosine_distances_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, float* dist_dev,
                             void* stream);
/* The second half alone: what a host of the columns layout calls after its all-reduce of the ranks' Grams.                       */
int byz_cosine_from_gram_dev(byz_ctx* ctx, const double* gram_dev, int64_t n_rows, float* dist_dev, void* stream);
/* The clustering, on ANY symmetric matrix in byz_pairwise_distances_dev's form (n x n fp32, diagonal +inf), Euclidean included.  */
/* With m = min_cluster_size, 2 m > n, two clusters cannot coexist and HDBSCAN (metric precomputed, allow_single_cluster) is      */
/* exactly this rule, with ms = min_samples in the `hdbscan` package's sense (scikit-learn's min_samples is ms + 1):              */
/*   core_i = the ms-th smallest off-diagonal entry of row i (ms = 0: 0); order: the distance (-0.0 as +0.0, every NaN behind     */
/*            +inf, -inf taken for +inf), then the column                                                                         */
/*   R_ij   = max(C_ij, core_i, core_j), the mutual reachability                                                                  */
/*   w*     = the smallest threshold at which the graph {R_ij <= w*} has a connected component of at least m vertices             */
/*   admitted_dev[i] = 1 for the rows of that component (edges tied at w* count), 0 for every other row; no finite threshold      */
/*            gives such a component: nobody is admitted and w* = +inf.                                                          */
/* The components of a threshold graph are those of any minimum spanning tree cut at the same threshold: the call builds ONE MST  */
/* (Prim, one workgroup, exactly n - 1 steps, no atomics and no loop whose length depends on the data), sorts its edges and walks */
/* them with a union-find.  By construction roughly m rows are admitted: the densest majority.  Identical rows sit together at   */
/* distance 0 and are admitted or rejected as a block: FLAME is a backdoor defence, not an answer to the drift attack.            */
/* 2 <= n <= 16,384 (BYZ_E_UNSUPPORTED beyond, decided on the argument alone); 2 <= m <= n < 2 m and 0 <= ms <= n - 1             */
/* (BYZ_E_INVALID otherwise); ms > 32: BYZ_E_UNSUPPORTED.  Nothing is written when a call is refused.  Asynchronous on `stream`.  */
int byz_flame_select_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int64_t min_cluster_size, int64_t min_samples,
                         int32_t* admitted_dev, void* stream);
/* Its first step alone: core_dev[i] = core_i above (n_rows floats), the same limits on n_rows and min_samples.  Exported so     */
/* that the core distances can be tested on their own; it leaves what byz_flame_info reports untouched.                           */
int byz_flame_core_distances_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int64_t min_samples, float* core_dev,
                                 void* stream);
typedef struct byz_flame_params {
    double lambda;             /* the noise's standard deviation is lambda * clip: finite, >= 0                        */
    int64_t min_samples;       /* ms above: 0..32, at most n_rows - 1                                                  */
    int64_t min_cluster_size;  /* m above; 0: n_rows / 2 + 1, the paper's                                              */
    uint64_t seed;             /* the noise's Philox key                                                               */
    uint64_t round;            /* the caller's round counter                                                           */
    int64_t column_offset;     /* the global column of column 0 of G: >= 0                                             */
} byz_flame_params;
/* The whole defence: byz_cosine_distances_dev (dist_dev_or_null == NULL; otherwise that n x n matrix REPLACES the cosine stage,  */
/* e.g. the angles between the clients' MODELS, which the paper compares), byz_flame_select_dev, byz_row_sqdist_dev with a zero   */
/* centre, byz_clip_scales_dev (adaptive: clip = the median norm of all the finite rows) giving s_i, w_i = admitted_i ? s_i : 0,  */
/* byz_scaled_rows_sum_dev with the divisor L = the admitted rows (L = 0: the zero vector, never NaN), then                       */
/* byz_gaussian_noise_dev in place with sigma = lambda and scale_dev = the clip.  The noise is added whoever is admitted;         */
/* lambda == 0 returns the clipped mean's bits.  admitted_dev_or_null: n_rows int32 of 0 / 1.  Every launch of the stages added   */
/* here is enqueued up front and byz_flame_info is the call that reads anything back.  ONE EXCEPTION, inherited: the Gram         */
/* (byz_gram_dev's path) waits once for its duplicate-row search, as byz_pairwise_distances_dev does; with dist_dev_or_null given  */
/* there is no Gram and no wait at all.  out_dev must not overlap G (BYZ_E_INVALID).  No doubles by value.                         */
/* Timers: BYZ_K_COUNT is part of the ABI that version 1 promises, so the new kernels report into existing slots --               */
/* BYZ_K_DISTANCES: the cosine conversion; BYZ_K_ROW_SORT: the core distances, the edge sort and the admission; BYZ_K_MISC:        */
/* Prim (alone in a byz_flame_select_dev call; byz_flame_dev's clip scales and weights kernels report there too).                 */
int byz_flame_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_flame_params* params,
                  const float* dist_dev_or_null, float* out_dev, int32_t* admitted_dev_or_null, void* stream);
/* The last byz_flame_select_dev or byz_flame_dev on this context: the rows admitted, the rows of the distance matrix without a   */
/* finite off-diagonal entry (the cosine stage's broken rows), w* (+inf: nobody admitted) and the clip (byz_flame_dev; 0 after a  */
/* selection alone).  Synchronises that call's stream.  BYZ_E_INVALID before the first such call.                                 */
int byz_flame_info(byz_ctx* ctx, int64_t* admitted_rows, int64_t* broken_rows, double* w_star, double* clip);
/* The same on a host matrix (dist_host_or_null: n_rows x n_rows floats; out_host: n_cols floats; admitted_host_or_null).         */
/* Synchronous.                                                                                                                   */
int byz_flame_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_flame_params* params,
                   const float* dist_host_or_null, float* out_host, int32_t* admitted_host_or_null);

/* ---- Multi-Metrics (Huang, Li, Wang, Chen, Zhang & Li, "Multi-metrics adaptively identifies backdoors in Federated Learning",  */
/* ICCV 2023; not in the reference) ----                                                                                           */
/* The fourth backdoor defence beside FLAME, robust_lr and sparsefed: L2 and cosine distances lose contrast in high dimensions,   */
/* the L1 distance keeps it.  Every client is described by its summed Manhattan, Euclidean and cosine distance to the others; the */
/* three features are whitened by their own covariance; the keep clients of smallest squared Mahalanobis norm are averaged.       */
/* The Manhattan matrix, which no Gram gives: m_ij = sum_c |g_ic - g_jc|, computed on the vector pipe in fp32 chains of at most   */
/* BYZ_MANHATTAN_CHAIN terms folded into fp64, rounded once to fp32.  Worst-case relative error (BYZ_MANHATTAN_CHAIN + 2) * 2^-24 */
/* = 7.75e-6.  The diagonal is +inf (byz_pairwise_distances_dev's convention); a pair whose sum is not finite -- a NaN or an      */
/* infinity in either row, or overflow -- is +inf; a zero row is an ordinary row.  Symmetric bit for bit.  Chains are assigned by  */
/* column index: the same matrix behind another ld or a moved base pointer, or a second run, gives the same bits.  n up to 16,384  */
/* (BYZ_E_UNSUPPORTED beyond, nothing written).  Any entry that takes a distance matrix (byz_krum_select_dev,                      */
/* byz_multi_krum_select_dev, byz_nnm_neighbours_dev, byz_flame_select_dev) takes this one.                                        */
#define BYZ_MANHATTAN_CHAIN 128
int byz_manhattan_distances_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, float* dist_dev,
                                void* stream);
/* The two halves, for a host of the columns layout: the L1 sums of a column slice (n x n fp64, both triangles) are ADDITIVE over  */
/* the slices; after the all-reduce the second half rounds the lower triangle's sums once and mirrors them.                        */
int byz_manhattan_sums_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, double* sums_dev,
                           void* stream);
int byz_manhattan_from_sums_dev(byz_ctx* ctx, const double* sums_dev, int64_t n_rows, float* dist_dev, void* stream);
/* The features, in fp64, from three n x n matrices in byz_pairwise_distances_dev's form (Manhattan, Euclidean, cosine; a caller   */
/* may pass any three): row i is USABLE when row i of cos_dev has a finite off-diagonal entry -- with byz_cosine_distances_dev's  */
/* matrix: g_ii finite and > 0, as long as two rows are usable.  features_dev[3 i ..] = (sum m_ij, sum e_ij, sum c_ij) over the   */
/* usable j != i, added in ascending j in 256 interleaved chains that meet in a fixed tree; (inf, inf, inf) for a row that is not  */
/* usable.                                                                                                                         */
int byz_multi_metrics_features_dev(byz_ctx* ctx, const float* man_dev, const float* euc_dev, const float* cos_dev, int64_t n_rows,
                                   double* features_dev, void* stream);
/* The selection on ANY n x 3 feature matrix (fp64): U = the rows whose three features are finite, u = |U|.  With y = x - x_first  */
/* (the first usable row's features: the variance does not see the shift, and a constant feature's deviation is exactly 0):       */
/*   s_k = the sample standard deviation (ddof = 1) of feature k, R = the features' correlation matrix (the covariance of x / s),  */
/*   score_i = z_i^T R^-1 z_i with z_i = x_i / s -- the paper's squared Mahalanobis norm, uncentred, computed through the         */
/*   correlation matrix so that the features' scales do not enter the conditioning; R^-1 = adj R / det R in closed form.           */
/* DEGENERATE -- u < 4, an s_k that is zero or not finite, det R <= 1e-12 -- score_i = x_i0, the Manhattan feature.  A row outside */
/* U scores +inf and is never chosen.  Chosen: the min(u, keep) smallest by (score ascending, row ascending; a NaN last).          */
/* flags_dev: n_rows int32 of 0 / 1; scores_dev_or_null: n_rows doubles.  1 <= keep <= n_rows (BYZ_E_INVALID otherwise), n_rows    */
/* up to 16,384 (BYZ_E_UNSUPPORTED beyond); nothing is written when a call is refused.  Asynchronous on `stream`.                  */
int byz_multi_metrics_select_dev(byz_ctx* ctx, const double* features_dev, int64_t n_rows, int64_t keep, int32_t* flags_dev,
                                 double* scores_dev_or_null, void* stream);
/* The whole defence: byz_pairwise_distances_dev, byz_cosine_distances_dev and byz_manhattan_distances_dev's matrices (ONE Gram    */
/* serves the first two, their bits unchanged), the features with U = the rows whose g_ii is finite and > 0, the selection, then   */
/* out_dev = byz_mean_rows_dev over the chosen rows ascending: np.mean(G[chosen], axis = 0) bit for bit.  Nobody usable: the zero  */
/* vector.  flags_dev_or_null: n_rows int32 of 0 / 1.  Nothing here synchronises with the host and byz_multi_metrics_info is the   */
/* call that reads anything back; the one wait is the Gram's own duplicate-row search, as in byz_flame_dev.  out_dev must not      */
/* overlap G (BYZ_E_INVALID).  Timers: BYZ_K_DISTANCES: the L1 tile kernel, its reduction and the two conversions;                 */
/* BYZ_K_ROW_SORT: the ranking and the compaction; BYZ_K_MISC: the usable flags, the features and the scores.                      */
int byz_multi_metrics_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t keep, float* out_dev,
                          int32_t* flags_dev_or_null, void* stream);
/* The last byz_multi_metrics_select_dev or byz_multi_metrics_dev on this context: the rows chosen (min(u, keep)), the usable      */
/* rows u, whether the degenerate rule scored them, and det R (0 when it was never formed).  Synchronises that call's stream.      */
/* BYZ_E_INVALID before the first such call.                                                                                       */
int byz_multi_metrics_info(byz_ctx* ctx, int64_t* kept_rows, int64_t* usable_rows, int32_t* degenerate, double* det);
/* The same on a host matrix (out_host: n_cols floats; flags_host_or_null: n_rows int32).  Synchronous.                            */
int byz_multi_metrics_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t keep, float* out_host,
                           int32_t* flags_host_or_null);

/* ---- Agglomerative clustering and ClippedClustering (Li, Ngai & Voigt, "An Experimental Study of Byzantine-Robust Aggregation     */
/* Schemes in Federated Learning", IEEE Trans. Big Data 2023; the `Clippedclustering` aggregator of Blades; not in the reference) ---- */
/* The rule's four stages: (1) every client clipped to the median norm, (2) pairwise COSINE distances, (3) agglomerative clustering  */
/* with AVERAGE linkage cut into two clusters, (4) the mean of the larger cluster.  Stages 1, 2 and 4 are byz_clip_scales_dev,       */
/* byz_cosine_distances_dev and byz_scaled_rows_sum_dev; stage 3 is the linkage below, a primitive over ANY symmetric matrix in      */
/* byz_pairwise_distances_dev's form (n x n fp32, the diagonal ignored): cosine, Euclidean or Manhattan.                             */
/* The linkage, exactly:                                                                                                             */
/*   entry (i, j), i != j, is READ from the lower triangle, at (max(i, j), min(i, j)): the matrix is symmetric by construction.      */
/*   Row i is USABLE when it has a finite off-diagonal entry (the cosine stage's notion of a row that is not broken).  A row that is */
/*   not usable takes no part: it is never merged and its label is -1.                                                               */
/*   W, the working copy, is fp64: an entry that is not finite, or is negative, becomes `fill` (finite, >= 0; ClippedClustering      */
/*   passes 2.0, the largest cosine distance, as Blades does); -0.0 counts as +0.0.                                                  */
/*   Every step merges the active pair smallest in (W[a][b], a, b), a < b: the distance, then the lower slot, then the higher one.   */
/*   The merged cluster keeps slot a (so a cluster's slot is its lowest row), slot b retires, and for every other active k, in fp64  */
/*   in exactly this order of operations, with the sizes s_a and s_b held as doubles:                                                */
/*     BYZ_LINKAGE_AVERAGE   W[a][k] = (s_a * W[a][k] + s_b * W[b][k]) / (s_a + s_b)   (two products, a sum, a quotient: scipy's)     */
/*     BYZ_LINKAGE_COMPLETE  W[a][k] = max(W[a][k], W[b][k])                                                                         */
/*     BYZ_LINKAGE_SINGLE    W[a][k] = min(W[a][k], W[b][k])                                                                         */
/*   u usable rows give u - 1 merges: pair_dev[2 t], pair_dev[2 t + 1] = the slots a < b of merge t, height_dev[t] = W[a][b],        */
/*   size_dev[t] = the merged size.  pair_dev holds 2 (n_rows - 1) int32, height_dev n_rows - 1 doubles, size_dev n_rows - 1 int32;  */
/*   behind the u - 1 merges they hold -1, +inf and 0.  usable_rows_dev (optional): n_rows int32 of 0 / 1.                           */
/* One workgroup runs the u - 1 steps with a nearest-partner cache per slot (Muellner 2011): no floating-point atomics, no grid or   */
/* host synchronisation; the caches a merge invalidates are rebuilt from a row of W each, at most n_rows a step, the one loop whose  */
/* length depends on the data.  method: 0 average, 1 complete, 2 single (BYZ_E_INVALID otherwise); *fill (a HOST double, read        */
/* before the call returns: the ABI takes no doubles by value) finite and >= 0 (BYZ_E_INVALID otherwise); 2 <= n_rows <= 16,384      */
/* (below: BYZ_E_INVALID; beyond: BYZ_E_UNSUPPORTED, decided on the argument alone).  Nothing is written when a call is refused.     */
/* Asynchronous on `stream`.  Timers: BYZ_K_ROW_SORT: the working copy, the first caches and the cut; BYZ_K_MISC: the linkage.       */
#define BYZ_LINKAGE_AVERAGE 0
#define BYZ_LINKAGE_COMPLETE 1
#define BYZ_LINKAGE_SINGLE 2
int byz_linkage_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int method, const double* fill, int32_t* pair_dev,
                    double* height_dev, int32_t* size_dev, int32_t* usable_rows_dev, void* stream);
/* The last byz_linkage_dev or ClippedClustering call on this context: its merges, the nearest-partner caches it rebuilt from a row  */
/* of W, and the most of them in one step.  Synchronises that call's stream.  BYZ_E_INVALID before the first such call.              */
int byz_linkage_info(byz_ctx* ctx, int64_t* merges, int64_t* rescans, int64_t* max_rescans);
/* The cut into n_clusters = c clusters, 1 <= c <= n_rows (BYZ_E_INVALID otherwise; with u < c usable rows every usable row is its    */
/* own cluster): the first u - c merges of pair_dev (2 (n_rows - 1) int32, byz_linkage_dev's) replayed; labels_dev[i] in 0..c-1,   */
/* the clusters numbered by their lowest row in ascending order, -1 for a row that is not usable; cluster_sizes_dev: c int32.  One   */
/* workgroup; a pair outside 0 <= a < b < n_rows is skipped.  2 <= n_rows <= 16,384.  Asynchronous on `stream`.                     */
int byz_linkage_cut_dev(byz_ctx* ctx, const int32_t* pair_dev, int64_t n_rows, const int32_t* usable_rows_dev, int64_t n_clusters,
                        int32_t* labels_dev, int32_t* cluster_sizes_dev, void* stream);
/* ClippedClustering's selection: the linkage, the cut into two, admitted_dev[i] = 1 for the rows of the LARGER cluster and 0 for     */
/* every other row.  Equal sizes: the cluster of the lowest usable row (this library's rule: Blades' tie goes to scikit-learn's      */
/* label 0, which is not a property of the data).  One usable row: it alone is admitted; none: nobody.  With two or more usable      */
/* rows somebody is always rejected.  The limits and refusals of byz_linkage_dev.                                                    */
int byz_clipped_clustering_select_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int method, const double* fill,
                                      int32_t* admitted_dev, void* stream);
typedef struct byz_clipped_clustering_params {
    double clip;       /* the fixed mode's clip: > 0 (+inf: nobody is clipped)                                  */
    int32_t adaptive;  /* != 0: clip = the median of this round's finite norms instead (FLAME's mode)            */
    int32_t method;    /* BYZ_LINKAGE_*: the paper's is average                                                 */
    double fill;       /* the distance taken for an entry that is not finite or is negative: finite, >= 0 (2.0) */
} byz_clipped_clustering_params;
/* The whole rule: byz_cosine_distances_dev (dist_dev_or_null == NULL; otherwise that n x n matrix REPLACES the cosine stage, as in   */
/* byz_flame_dev), byz_clipped_clustering_select_dev, byz_row_sqdist_dev with a zero centre (sq_dev_or_null == NULL; otherwise the   */
/* caller's n_rows squared norms, which spares that pass), byz_clip_scales_dev giving s_i, w_i = admitted_i ? s_i : 0, and           */
/* byz_scaled_rows_sum_dev with the divisor L = the admitted rows (L = 0: the zero vector, never NaN).  Scaling a row by a positive  */
/* number does not change its cosines, so the cosine stage runs on the UNCLIPPED rows (Blades clips first).                          */
/* admitted_dev_or_null: n_rows int32 of 0 / 1.  It waits as byz_flame_dev does: once, inside the Gram's duplicate-row search, and   */
/* not at all when dist_dev_or_null is given.  out_dev must not overlap G (BYZ_E_INVALID).  The limits of byz_linkage_dev.           */
int byz_clipped_clustering_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                               const byz_clipped_clustering_params* params, const float* dist_dev_or_null,
                               const double* sq_dev_or_null, float* out_dev, int32_t* admitted_dev_or_null, void* stream);
/* The last byz_clipped_clustering_select_dev or byz_clipped_clustering_dev on this context: the rows admitted, the usable rows, the  */
/* heights of the last merge and of the one before (0 where there is none) and the clip (0 after a selection alone).  Synchronises  */
/* that call's stream.  BYZ_E_INVALID before the first such call.                                                                    */
int byz_clipped_clustering_info(byz_ctx* ctx, int64_t* admitted_rows, int64_t* usable_rows, double* top_height, double* second_height,
                                double* clip);
/* The same on a host matrix (dist_host_or_null: n_rows x n_rows floats; sq_host_or_null: n_rows doubles; out_host: n_cols floats;   */
/* admitted_host_or_null).  Synchronous.                                                                                             */
int byz_clipped_clustering_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                                const byz_clipped_clustering_params* params, const float* dist_host_or_null,
                                const double* sq_host_or_null, float* out_host, int32_t* admitted_host_or_null);

/* ---- FABA (Xia, Chen, Yu & Ma, "FABA: An Algorithm for Fast Aggregation against Byzantine Attacks in Distributed Neural Networks", */
/* IJCAI 2019; not in the reference) ----                                                                                            */
/* The rule: take the mean of the rows still kept, drop the row farthest from it, r times; average the rest.  For a set S of m rows  */
/* and a row i of S, |g_i - mean(S)|^2 = (1/m) sum_{j in S} |g_i - g_j|^2 - (1/(2 m^2)) sum_{j,k in S} |g_j - g_k|^2, and the second */
/* term is the same for every i: the farthest row is the row with the largest SUM of squared distances to the kept rows, and the      */
/* rule runs on an n x n matrix in byz_pairwise_distances_dev's form (fp32, the diagonal ignored, taken as symmetric) without reading */
/* the gradients again.  The selection, exactly (C: the matrix, r: remove_count, power 1 or 2):                                      */
/*   An off-diagonal entry c is USABLE when it is finite and >= 0 (-0.0 is, and counts as +0.0).  Its term is e = (double)c for       */
/*   power 1 and (double)c * (double)c for power 2 (exact in fp64).                                                                  */
/*   Row i starts with bad_i = the entries C[i][j], j != i, that are not usable, and s_i = the fp64 sum of the terms of those that    */
/*   are, in this order: 64 chains, chain l the sum, from +0.0, of the terms of the columns j = l, l + 64, l + 128, ... ascending     */
/*   (the diagonal and entries that are not usable skipped); then chain[l] += chain[l + h] for every l < h, for h = 32, 16, 8, 4, 2,  */
/*   1 in turn; s_i = chain[0].                                                                                                      */
/*   A step removes the kept row q that is first in the order (bad descending, s descending by value, row ascending) and then, for    */
/*   every other row i, reads c = C[q][i]: bad_i -= 1 where c is not usable, s_i = s_i - e(c) (one fp64 subtraction) where it is.     */
/*   The loop makes r steps and goes on while the largest bad of the kept rows is positive, so that no row with an unusable entry    */
/*   against a kept row is averaged.  A matrix WITHOUT ANY usable off-diagonal entry judges nobody: every row is removed.            */
/*   Rows removed = max(r, what the bad counts force) <= n_rows.                                                                     */
/* Consequences: with power 2 on Euclidean distances this is FABA; rows whose entries are all NaN or +inf (broken gradients) go       */
/* first, lowest row first, and count towards r; identical rows tie and go lowest row first; power 1 is "largest summed distance",   */
/* for the cosine and Manhattan matrices.  FABA removes what is far from the crowd: rows that sit inside it (the drift attack's)      */
/* pass, as they pass Krum.                                                                                                          */
/* kept_dev: n_rows int32 of 0 / 1.  order_dev_or_null: n_rows int32, the removed rows in removal order, then -1.                    */
/* One workgroup runs the steps (an argmax, one row read and one subtraction a row): no floating-point atomics, no grid or host      */
/* synchronisation, at most n_rows steps.  2 <= n_rows <= 16,384 (below: BYZ_E_INVALID; beyond: BYZ_E_UNSUPPORTED, decided on the      */
/* argument alone); 0 <= remove_count <= n_rows - 1 and power in {1, 2} (BYZ_E_INVALID otherwise).  Nothing is written when a call   */
/* is refused.  Asynchronous on `stream`.  Timers: BYZ_K_ROW_SORT: the initial sums; BYZ_K_MISC: the loop.                           */
int byz_faba_select_dev(byz_ctx* ctx, const float* dist_dev, int64_t n_rows, int64_t remove_count, int power, int32_t* kept_dev,
                        int32_t* order_dev_or_null, void* stream);
/* The whole rule: byz_pairwise_distances_dev (dist_dev_or_null == NULL; otherwise that n x n matrix REPLACES the stage), the         */
/* selection above with power 2, and byz_scaled_rows_sum_dev with the 0 / 1 flags as fp64 weights and the kept count, an fp64 read   */
/* on the device, as the divisor: its bits.  Nobody kept: the zero vector, never NaN.  It waits as byz_pairwise_distances_dev does,  */
/* and not at all when dist_dev_or_null is given.  out_dev (n_cols floats) must not overlap G (BYZ_E_INVALID).                       */
int byz_faba_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t remove_count,
                 const float* dist_dev_or_null, float* out_dev, int32_t* kept_dev_or_null, int32_t* order_dev_or_null, void* stream);
/* The last byz_faba_select_dev or byz_faba_dev on this context: the rows removed, the rows kept, the rows removed beyond             */
/* remove_count because a bad count forced it, s of the last removed row (0: nobody was removed) and the divisor of the sum.          */
/* Synchronises that call's stream.  BYZ_E_INVALID before the first such call.                                                       */
int byz_faba_info(byz_ctx* ctx, int64_t* removed_rows, int64_t* kept_rows, int64_t* forced_rows, double* last_score, double* divisor);
/* The same on a host matrix (dist_host_or_null: n_rows x n_rows floats; out_host: n_cols floats; kept_host_or_null and               */
/* order_host_or_null: n_rows int32).  Synchronous.                                                                                  */
int byz_faba_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t remove_count,
                  const float* dist_host_or_null, float* out_host, int32_t* kept_host_or_null, int32_t* order_host_or_null);

/* ---- AFA, Adaptive Federated Averaging (Munoz-Gonzalez, Co & Lupu, "Byzantine-Robust Federated Machine Learning through Adaptive   */
/* Model Averaging", arXiv:1909.05125, Algorithm 1; not in the reference) ----                                                        */
/* The rule: every row's cosine with the weighted aggregate of the rows still kept; the rows whose cosine lies more than xi standard  */
/* deviations from the median are removed, on the side the mean of the cosines points away from; xi grows by delta_xi and the round   */
/* repeats until it removes nobody.  It needs no count of attackers.  With the kept set S, weights w and the Gram C (C[k][j] = g_k .   */
/* g_j), g_k . agg is proportional to u_k = sum_{j in S} w_j C[k][j] and |agg|^2 to A = sum_{k in S} w_k u_k, and removing row q takes  */
/* w_q C[q][k] off every u_k: the rule runs on the n x n fp64 Gram in byz_gram_dev's form (row-major, taken as symmetric: a round      */
/* reads C[q][k] of a removed row q only) and never reads the gradients.  The selection, exactly (every operation an fp64 operation   */
/* rounded once, no contraction; w: weights_dev_or_null, NULL: all ones):                                                             */
/*   Row k is USABLE when C[k][k] is finite and > 0 and w[k] is finite and > 0.  Every other row is EXCLUDED before the first round:  */
/*   never kept, never averaged, never summed over, reported apart from the removed rows (a NaN or zero gradient, a weight of 0).     */
/*   r_k = sqrt(C[k][k]).  u_k starts as the sum of w_j * C[k][j] over the usable j in this order: 64 chains, chain l the sum, from   */
/*   +0.0, of the products of the columns j = l, l + 64, l + 128, ... ascending (excluded columns skipped); then chain[l] += chain[l   */
/*   + h] for every l < h, for h = 32, 16, 8, 4, 2, 1 in turn; u_k = chain[0].                                                        */
/*   A SUM OVER THE KEPT ROWS (A, sum s, sum (s - mean)^2, the divisor) has one order: 1024 chains, chain t the sum, from +0.0, of    */
/*   the terms of the kept rows t, t + 1024, t + 2048, ... ascending; inside every aligned group of 64 chains chain[l] += chain[l +  */
/*   h] for l < h, h = 32, 16, 8, 4, 2, 1; then the 16 groups' sums W: W[v] += W[v + h] for v < h, h = 8, 4, 2, 1; the sum is W[0].  */
/*   Round 1, 2, ... on the kept set S of m rows, xi = xi0 in round 1:                                                                */
/*     A = sum_{k in S} w_k * u_k.  A not finite or <= 0: the loop ends here, `degenerate` set, S as it stands.                       */
/*     s_k = u_k / (r_k * sqrt(A));  mean = (sum s_k) / m;  sd = sqrt((sum (s_k - mean)^2) / m)  (np.std: population form, two       */
/*     passes);  med = np.median of the s_k: the order statistic (m - 1) / 2 for odd m, (lo + hi) / 2 of the order statistics m / 2  */
/*     - 1 and m / 2 for even m.  The order is by value: -0.0 equals +0.0 and is read back as +0.0; an s_k that is a NaN (it cannot   */
/*     occur for usable rows and a finite A) sorts behind +inf, and a med, sd or thr that is a NaN removes nobody.                    */
/*     mean < med: thr = med - xi * sd and R = { k in S : s_k < thr };  otherwise: thr = med + xi * sd and R = { k in S : s_k > thr }. */
/*     Both comparisons are strict: the median row is never removed, S never empties, and sd = 0 removes nobody.                      */
/*     The rows of R leave S.  R empty, or the round's number = max_rounds (0: no cap): the loop ends.  Otherwise, for every q in R   */
/*     in ascending row order and every kept k: u_k = u_k - w_q * C[q][k]; then xi = xi + delta_xi and the next round starts.         */
/*   At most n_rows rounds, n_rows - 1 of them removing.  A matrix whose rows are all unusable (all zeros, say) is not refused:       */
/*   everybody is excluded, no round runs, the weights are all 0 and the aggregate is the zero vector.                                */
/* kept_dev: n_rows int32 of 0 / 1.  round_of_dev_or_null: n_rows int32, the round that removed the row, 0 for an excluded row, -1   */
/* for a kept one.  score_dev_or_null: n_rows fp64, the last s_k the row had (+0.0 where it never had one).                           */
/* One workgroup runs the rounds: no floating-point atomics, no grid or host synchronisation.  2 <= n_rows <= 16,384 (below:          */
/* BYZ_E_INVALID; beyond: BYZ_E_UNSUPPORTED, decided on the argument alone); xi0 and delta_xi finite and >= 0, max_rounds >= 0        */
/* (BYZ_E_INVALID otherwise).  Nothing is written when a call is refused.  Asynchronous on `stream`.  Timers: BYZ_K_ROW_SORT: the     */
/* usable rows and the initial u; BYZ_K_MISC: the rounds.                                                                            */
typedef struct byz_afa_params {
    double xi0;          /* the first round's xi (the paper: 2) */
    double delta_xi;     /* added to xi after every removing round (the paper: 0.5) */
    int64_t max_rounds;  /* 0: until a round removes nobody */
} byz_afa_params;
int byz_afa_select_dev(byz_ctx* ctx, const double* gram_dev, int64_t n_rows, const double* weights_dev_or_null,
                       const byz_afa_params* params, int32_t* kept_dev, int32_t* round_of_dev_or_null, double* score_dev_or_null,
                       void* stream);
/* The whole rule: byz_gram_dev (gram_dev_or_null == NULL; otherwise that n x n fp64 matrix REPLACES the stage), the selection above, */
/* and byz_scaled_rows_sum_dev with the weights w_k * kept_k and their sum (the order above), an fp64 read on the device, as the      */
/* divisor: its bits.  Nobody kept: the zero vector, never NaN.  It waits as byz_gram_dev does, and not at all when gram_dev_or_null  */
/* is given.  out_dev (n_cols floats) must not overlap G (BYZ_E_INVALID).                                                             */
int byz_afa_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, const double* weights_dev_or_null,
                const byz_afa_params* params, const double* gram_dev_or_null, float* out_dev, int32_t* kept_dev_or_null,
                int32_t* round_of_dev_or_null, double* score_dev_or_null, void* stream);
/* The last byz_afa_select_dev or byz_afa_dev on this context.  counts6: rounds run, rows kept, removed and excluded, the branch of   */
/* the last removing round (-1: below the median, +1: above, 0: no round removed anybody), degenerate (0 / 1).  stats4: the last      */
/* complete round's mean, med, sd and thr (0 before the first).  divisor: the kept rows' weights summed.  Any pointer may be NULL.    */
/* Synchronises that call's stream.  BYZ_E_INVALID before the first such call.                                                        */
int byz_afa_info(byz_ctx* ctx, int64_t* counts6, double* stats4, double* divisor);
/* The same on a host matrix (weights_host_or_null: n_rows fp64; gram_host_or_null: n_rows x n_rows fp64; out_host: n_cols floats;    */
/* kept_host_or_null and round_of_host_or_null: n_rows int32; score_host_or_null: n_rows fp64).  Synchronous.                         */
int byz_afa_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const double* weights_host_or_null,
                 const byz_afa_params* params, const double* gram_host_or_null, float* out_host, int32_t* kept_host_or_null,
                 int32_t* round_of_host_or_null, double* score_host_or_null);

/* ---- Auror (Shen, Tople & Saxena, "AUROR: Defending Against Poisoning Attacks in Collaborative Deep Learning Systems", ACSAC 2016;  */
/* not in the reference) ----                                                                                                         */
/* The rule is column-local: every column's n values are split into two clusters, a column whose two centres end far apart is         */
/* INDICATIVE, and a row that sits in the smaller cluster of most indicative columns is removed.  It is the classic answer to         */
/* targeted poisoning (a label flip, a backdoor), which moves a few coordinates a lot.  It is NO answer to the drift attack: in a     */
/* unimodal column of spread sigma the two centres end about 1.6 sigma apart, so with alpha below that every column is indicative and  */
/* honest rows are removed.  alpha therefore has no default: byz_auror_votes_dev's gap output is there to choose it from.             */
/* The votes, exactly.  Per column, with x the FINITE values of the column and m their count (fp64 operations rounded once each):      */
/*   A non-finite value abstains in its column, and its row is BAD; the row's finite values still take part in their own columns.     */
/*   m < 2 or min == max (-0.0 == +0.0): the column is not clustered, its gap is 0, it is not indicative.                              */
/*   Otherwise c0 = (double)min, c1 = (double)max, and sweep k = 1, 2, ..., max_iter:                                                  */
/*     t = 0.5 * (c0 + c1).  Cluster 1 is the values with (double)x > t; a value equal to t is in cluster 0.  m1 = the count of       */
/*     cluster 1, S1 and S0 the fp64 sums of the two clusters, c1 = S1 / m1, c0 = S0 / (m - m1).  min <= t < max throughout, so        */
/*     neither cluster is empty.  The column stops after a sweep k >= 2 whose m1 equals the previous sweep's (an integer: the order   */
/*     of the sums has no say in it), and after sweep max_iter in any case; stopped there WITHOUT that equality it is CAPPED.          */
/*     The order of a sum: the rows of one row group (rows g, g + RG, g + 2 RG, ... with RG the launch geometry's row groups: 16 up   */
/*     to 256 rows and beyond 4096, 32 up to 1024, 64 up to 4096) ascending from +0.0, then the row groups ascending from +0.0.        */
/*   The final assignment is the last sweep's (its t, its m1), gap = c1 - c0 its centres' distance.  The column is indicative iff      */
/*   gap > alpha.  In an indicative column the cluster with FEWER members is suspicious (equal counts: nobody), and every row in it    */
/*   gets one vote.                                                                                                                   */
/* votes_dev: n_rows int64.  bad_dev: n_rows int32 of 0 / 1.  counts_dev: 4 int64 = {indicative, clustered, capped columns, 0}.        */
/* gap_dev_or_null: n_cols fp64.  accumulate = 0 overwrites votes, bad and counts; accumulate = 1 adds to the votes and counts and     */
/* keeps a bad flag that is set (the paper gathers its evidence over several rounds): the caller's arrays then hold an earlier call's  */
/* results for the same n_rows, or zeros.  gap is always overwritten.                                                                 */
/* 1 <= n_rows <= 16,384 (beyond: BYZ_E_UNSUPPORTED, decided on the argument alone); alpha finite and >= 0, 0 <= tau <= 1,             */
/* max_iter >= 1, accumulate 0 or 1 (BYZ_E_INVALID otherwise, NaN included).  Nothing is written when a call is refused.               */
/* One read of the matrix up to 4096 rows (a workgroup's columns stay in registers over the sweeps), one read a sweep beyond.  Integer */
/* atomics only, one 64-bit add a row and workgroup at most.  Asynchronous on `stream`.  Timer: BYZ_K_MISC.                            */
typedef struct byz_auror_params {
    double alpha;        /* a column is indicative when its centres end more than this apart */
    double tau;          /* a row is removed when it has more than tau * indicative votes (the paper: 0.5) */
    int64_t max_iter;    /* sweeps a column at most (32 covers Gaussian columns of up to 4097 rows) */
    int64_t accumulate;  /* 1: add to votes, bad and counts */
} byz_auror_params;
int byz_auror_votes_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_auror_params* params,
                        int64_t* votes_dev, int32_t* bad_dev, int64_t* counts_dev, double* gap_dev_or_null, void* stream);
/* The selection: row i is removed iff bad[i] != 0, or counts[0] > 0 and (double)votes[i] > tau * (double)counts[0].  With no          */
/* indicative column nobody is removed for votes.  kept_dev: n_rows int32 of 0 / 1.  One workgroup.  Asynchronous on `stream`.         */
int byz_auror_select_dev(byz_ctx* ctx, const int64_t* votes_dev, const int32_t* bad_dev, const int64_t* counts_dev, int64_t n_rows,
                         const byz_auror_params* params, int32_t* kept_dev, void* stream);
/* The whole rule: the votes, the selection, and byz_scaled_rows_sum_dev with the 0 / 1 flags as fp64 weights and the kept count, an   */
/* fp64 read on the device, as the divisor: its bits.  Nobody kept: the zero vector, never NaN.  votes_dev, bad_dev and counts_dev     */
/* are the caller's history, all three or none (none: the context's own, and accumulate must be 0).  out_dev (n_cols floats) must not  */
/* overlap G (BYZ_E_INVALID).  Nothing synchronises with the host.                                                                    */
int byz_auror_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, const byz_auror_params* params,
                  int64_t* votes_dev_or_null, int32_t* bad_dev_or_null, int64_t* counts_dev_or_null, float* out_dev,
                  int32_t* kept_dev_or_null, double* gap_dev_or_null, void* stream);
/* The last byz_auror_select_dev or byz_auror_dev on this context: the indicative columns the selection read (accumulated: over the    */
/* rounds), the rows removed (bad rows included) and kept, the bad rows, the capped columns.  Any pointer may be NULL.  Synchronises   */
/* that call's stream: the only Auror call that does.  BYZ_E_INVALID before the first such call.                                       */
int byz_auror_info(byz_ctx* ctx, int64_t* indicative, int64_t* removed_rows, int64_t* kept_rows, int64_t* bad_rows, int64_t* capped_cols);
/* The same on a host matrix (out_host: n_cols floats; kept_host_or_null: n_rows int32; votes_host_or_null: n_rows int64;              */
/* bad_host_or_null: n_rows int32; counts_host_or_null: 4 int64; gap_host_or_null: n_cols fp64).  With accumulate = 1 the three        */
/* history arrays are read and written, and all three are required (BYZ_E_INVALID otherwise).  Synchronous.                           */
int byz_auror_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_auror_params* params, float* out_host,
                   int32_t* kept_host_or_null, int64_t* votes_host_or_null, int32_t* bad_host_or_null, int64_t* counts_host_or_null,
                   double* gap_host_or_null);

/* ---- FoolsGold (Fung, Yoon & Beschastnikh, "Mitigating Sybils in Federated Learning Poisoning", arXiv:1808.04866; RAID 2020, "The    */
/* Limitations of Federated Learning in Sybil Settings"; not in the reference) ----                                                    */
/* Sybils are several clients that push one shared objective round after round: clients whose ACCUMULATED updates point the same way   */
/* get their weight cut.  It needs no count of attackers.  The decision runs on ONE n x n fp64 Gram and never on the gradients; the    */
/* Gram is taken over a per-client history matrix that lives on the device across rounds (or over this round's gradients).             */
/* The rule (R).  Input: an n x n fp64 Gram C, taken as symmetric (row i is read; C_ii is the diagonal), and kappa, finite and > 0,     */
/* the paper's confidence (default 1).  All arithmetic is fp64, one operation at a time, no contraction.                               */
/*   1. Usable rows.  Row i is EXCLUDED if C_ii is not finite or is negative: its weight is 0 and no other row sees it as a j.         */
/*   2. Norms.  r_i = sqrt(C_ii).  A usable row with C_ii == 0 (a client with no history) has cs_ij = cs_ji = 0 for every j.           */
/*   3. Cosines.  cs_ij = C_ij / (r_i * r_j) for usable i != j with both norms > 0.  A cs_ij that is NaN is taken as 0 (C_ij          */
/*      non-finite under finite diagonals).  Nothing is clamped to [-1, 1].                                                            */
/*   4. Row maximum.  m_i = max(0, max_{j != i} cs_ij): the authors' cosine_similarity - eye, the diagonal takes part as 0, so m_i    */
/*      >= 0 always.                                                                                                                   */
/*   5. Pardoning, applied on the fly (no second n x n table).  p_ij = (m_i < m_j) ? (cs_ij * m_i) / m_j : cs_ij, in that order of    */
/*      operations;  a_i = max(0, max_{j != i} p_ij).  m_j > m_i >= 0, so the divisor is never 0.                                      */
/*      A maximum, here and in 4, starts from +0.0 and takes x when x > what it holds: a NaN p_ij (-inf * 0) and a -0.0 never enter.   */
/*   6. Raw weight.  v_i = min(1, max(0, 1 - a_i)).                                                                                    */
/*   7. Rescale.  top = max_i v_i over the usable rows.  Fewer than 2 usable rows: every usable row gets weight 1, stop.  top == 0:    */
/*      every weight is 0 and `degenerate` = 1 (everybody's twin; the authors' code yields NaN here), stop.                            */
/*   8. Logit and clip.  w_i = v_i / top; w_i == 1: w_i = 0.99.  w_i == 0: l_i = 0.  Otherwise l_i = kappa * (log(w_i / (1 - w_i))    */
/*      + 0.5).  Then l_i = min(1, max(0, l_i)).                                                                                       */
/*   9. Aggregate.  out[c] = fl32(sum_i l_i * G[i][c] / T) over THIS ROUND's gradients G (not the history), by                        */
/*      byz_scaled_rows_sum_dev, with its bits.  normalise = COUNT (default): T = the number of usable rows; with every weight 1 the   */
/*      rule is the mean (no_defense).  normalise = SUM: T = sum_i l_i in ascending row order, from +0.0 (Blades' variant).  T is     */
/*      formed and read on the device; T == 0 gives the zero vector, never NaN.                                                        */
/* Steps 4 to 8 are the authors' published foolsgold() with its loop order removed: the pardoned maximum does not depend on the order  */
/* because m is fixed before the loop.  Not built: the paper's feature-importance weighting of the cosines; partial participation      */
/* (clients are rows by position and every client reports every round).                                                                */
/* The history.  H is an n x w fp32 matrix on the device, zero at the start; row i is client i; w is the column window [col_start,    */
/* col_start + w) of the gradients.  Every call first does H[i][c] = fl32(H[i][c] + G[i][col_start + c]) (numpy's float32 += bits),    */
/* then the Gram is byz_gram_dev(H).  Without a history the Gram is that of G's window itself.  A non-finite value this round makes   */
/* the client's history row non-finite for good, and rule 1 excludes it until the caller zeroes H.                                     */
/* Row limit: 1 <= n_rows <= 2^20, what byz_gram_dev and byz_scaled_rows_sum_dev accept (beyond: BYZ_E_UNSUPPORTED); no kernel here    */
/* needs a lower cap.  No floating-point atomics; no host synchronisation except in byz_foolsgold_info.  Nothing is written when a     */
/* call is refused.  Asynchronous on `stream`.  Timers: BYZ_K_MISC: the history update and the weights kernel; BYZ_K_ROW_SORT: the     */
/* norms, the row maxima and the pardoned maxima.                                                                                      */
#define BYZ_FOOLSGOLD_NORMALISE_COUNT 0
#define BYZ_FOOLSGOLD_NORMALISE_SUM 1
typedef struct byz_foolsgold_params {
    double kappa;        /* the confidence: finite and > 0 (the paper: 1) */
    int64_t normalise;   /* BYZ_FOOLSGOLD_NORMALISE_COUNT or _SUM */
} byz_foolsgold_params;
/* The history update alone: H (n_rows x n_cols_window, ld_h) += G[:, col_start : col_start + n_cols_window] (G: ld_g).  Any ld and    */
/* any 4-byte base alignment on either operand: 16-byte accesses on both when both bases (G's at the window) and both ld allow it,     */
/* otherwise 16-byte accesses on H between its own boundaries and dword reads of G.  H must not overlap G (BYZ_E_INVALID).             */
int byz_rows_add_dev(byz_ctx* ctx, float* H_dev, int64_t ld_h, const float* G_dev, int64_t n_rows, int64_t n_cols_window, int64_t ld_g,
                     int64_t col_start, void* stream);
/* Steps 1 to 8 on a Gram: weights_dev (n_rows fp64) = l, 0 for an excluded row.  maxcs_dev_or_null: n_rows fp64, m.                  */
/* alpha_dev_or_null: n_rows fp64, a.  Four launches: the norms, the row maxima, the pardoned maxima, one workgroup for the rest.      */
int byz_foolsgold_weights_dev(byz_ctx* ctx, const double* gram_dev, int64_t n_rows, const byz_foolsgold_params* params,
                              double* weights_dev, double* maxcs_dev_or_null, double* alpha_dev_or_null, void* stream);
/* The last weights stage's intermediate vectors, copied on `stream` (tests and diagnosis): rescaled_dev_or_null, n_rows fp64, w of    */
/* step 8 (1 for the usable rows when fewer than 2 are usable, 0 for an excluded row and when degenerate); usable_dev_or_null, n_rows  */
/* int32 of 0 / 1.  n_rows must be the last stage's (BYZ_E_INVALID otherwise, and before the first).                                   */
int byz_foolsgold_trace_dev(byz_ctx* ctx, int64_t n_rows, double* rescaled_dev_or_null, int32_t* usable_dev_or_null, void* stream);
/* The whole rule: the history update (H_dev_or_null == NULL: none), byz_gram_dev of the history or of G's window (gram_dev_or_null    */
/* != NULL: that n x n fp64 matrix REPLACES the stage; the history is still updated), the weights, and byz_scaled_rows_sum_dev with    */
/* them and T.  0 <= col_start, 1 <= col_count, col_start + col_count <= n_cols, ld_h >= col_count (BYZ_E_INVALID otherwise).  It      */
/* waits as byz_gram_dev does, and not at all when gram_dev_or_null is given.  out_dev (n_cols floats) must overlap neither G nor H.   */
int byz_foolsgold_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, float* H_dev_or_null, int64_t ld_h,
                      int64_t col_start, int64_t col_count, const byz_foolsgold_params* params, const double* gram_dev_or_null,
                      float* out_dev, double* weights_dev_or_null, void* stream);
/* The last byz_foolsgold_weights_dev or byz_foolsgold_dev on this context.  counts5: usable rows, excluded rows, usable rows at       */
/* weight 0, usable rows at weight 1, degenerate (0 / 1).  stats2: top (0 when nobody is usable) and T.  Either may be NULL.           */
/* Synchronises that call's stream.  BYZ_E_INVALID before the first such call.                                                         */
int byz_foolsgold_info(byz_ctx* ctx, int64_t* counts5, double* stats2);
/* The same on a host matrix (H_host_or_null: n_rows x col_count floats, contiguous, read and written; gram_host_or_null: n_rows x     */
/* n_rows fp64; out_host: n_cols floats; weights_host_or_null: n_rows fp64).  Synchronous.                                             */
int byz_foolsgold_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, float* H_host_or_null, int64_t col_start,
                       int64_t col_count, const byz_foolsgold_params* params, const double* gram_host_or_null, float* out_host,
                       double* weights_host_or_null);

/* ---- DnC, the spectral defence (Shejwalkar & Houmansadr, NDSS 2021, Algorithm 2; not in the reference) ---- */
/* Colluding rows that each stay below every distance and per-coordinate threshold still line up along ONE    */
/* direction of the centred gradient matrix: its top right singular vector.  DnC scores every row by its      */
/* squared projection on that vector, computed on a sample of the columns, removes the highest scores, repeats */
/* with fresh samples and averages the rows that every iteration kept.  The library draws nothing: the caller  */
/* passes the sampled columns, so that a call is deterministic.                                                */
/* Inputs: G (n x n_cols fp32, n = n_rows); n_iters >= 1; for every iteration t a list of sub_dim DISTINCT,    */
/* ASCENDING column indices in [0, n_cols) -- columns_dev, one device int64 array of n_iters * sub_dim entries, */
/* iteration-major; the caller vouches for range and order --; power_iters >= 0; 0 <= remove_count <= n - 1.   */
/* For every iteration t, with x_ij the sampled values of row i:                                               */
/*   row i is ACTIVE when every x_ij is finite; n_a = the number of active rows;                               */
/*   mu_j = (sum over the active i, ascending, of (double)x_ij) / n_a;  c_ij = (double)x_ij - mu_j (fp64);     */
/*   M = C C^T over the active rows (fp64);  i0 = the active row with the largest M_ii, the lowest index on a  */
/*   tie;  u = e_i0;  power_iters times: y = M u, u = y / |y|_2;  then y = M u, lambda = u.y,                  */
/*   s_i = y_i^2 / lambda -- the squared projection (c_i . v)^2 of centred row i on v = C^T u / |C^T u|, the   */
/*   top right singular vector once the iteration has converged.  If M_i0i0, any |y| or lambda is 0, every     */
/*   active score is 0.  An inactive row scores +inf.                                                          */
/*   Rows are ranked by (s_i, i) ascending (exactly, on the fp64 scores); keep_t = the first n - remove_count.  */
/* good = the intersection of the keep_t, ascending; out = the mean of the rows `good` with byz_mean_rows_dev's */
/* arithmetic: the bits of np.mean(G[good], axis=0).  No row left (possible only when n_iters * remove_count   */
/* >= n): out is NaN in every column, the kept count 0.  More inactive rows than remove_count: the lowest-      */
/* indexed of them are kept, as the ranking says, and reach the mean.                                           */
/* The device never forms M: y = M u is w = C^T u (over the sampled columns) then y = C w, both in fp64 in a     */
/* fixed order (two calls give the same bits); the values differ from the N-space arithmetic above by fp64      */
/* rounding only (measured: DESIGN.md 3.4d).  Nothing synchronises with the host: the kept count stays on the   */
/* device until byz_dnc_info reads it.  Every launch is enqueued up front: 5 + 4 (power_iters + 1) + 2 per      */
/* iteration.  Limits (BYZ_E_UNSUPPORTED beyond): n_rows up to byz_limits' selection limit; n_rows * sub_dim up  */
/* to BYZ_DNC_MAX_SAMPLED values (the fp64 workspace: 8 bytes each); n_iters * (power_iters + 1) up to          */
/* BYZ_DNC_MAX_PRODUCTS.  The parameters travel in a struct, as the geometric median's do.                      */
#define BYZ_DNC_MAX_SAMPLED 268435456
#define BYZ_DNC_MAX_PRODUCTS 65536
typedef struct byz_dnc_params {
    int64_t n_iters;       /* iterations: samples of the columns, intersected                              */
    int64_t sub_dim;       /* sampled columns per iteration (1 .. n_cols)                                  */
    int64_t power_iters;   /* normalised products before the scoring one                                   */
    int64_t remove_count;  /* rows every iteration removes                                                 */
} byz_dnc_params;
/* One iteration's scores (scores_dev: n_rows fp64) for one list of sub_dim columns.                        */
int byz_dnc_scores_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                       const int64_t* columns_dev, int64_t sub_dim, int64_t power_iters, double* scores_dev,
                       void* stream);
/* The selection: good_dev (n_rows int32) receives the kept rows ascending, -1 behind them; count_dev        */
/* (optional, one device int32) their number.                                                                */
int byz_dnc_select_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                       const byz_dnc_params* params, const int64_t* columns_dev, int32_t* good_dev,
                       int32_t* count_dev, void* stream);
/* The whole function (out_dev: n_cols floats; good_dev optional, as above).                                 */
int byz_dnc_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                const byz_dnc_params* params, const int64_t* columns_dev, float* out_dev, int32_t* good_dev,
                void* stream);
/* The last call's kept rows and the rows its last iteration found inactive; synchronises that call's stream. */
int byz_dnc_info(byz_ctx* ctx, int64_t* kept_rows, int64_t* inactive_rows);

/* ---- multi-GPU, columns layout: one context per GPU, the HOST owns the communicator ---- */
/* SURVEY.md 8(e)'s "cheaper equivalent": every rank holds ALL n_rows clients over its own slice of the      */
/* columns (G_local: n_rows x n_cols_local).  The path has ONE exchange: the n_rows x n_rows fp64 Gram of    */
/* the slices is summed over the ranks (plus, when clients nearly coincide, the short list of squared        */
/* differences of byz_near_pairs_*); the selection then runs replicated on every rank and the trimmed mean   */
/* on the local columns, so out_local is this rank's slice of the reference's result.  The library links no  */
/* collective library: the host passes its own in-place SUM all-reduce over the ranks, which must enqueue on */
/* `stream` and return 0 --                                                                                   */
/*     ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, comm, (hipStream_t)stream)   (RCCL over xGMI)      */
/* with `comm` from ncclCommInitRank (one process per GPU) or ncclCommInitAll (one thread per GPU) reached     */
/* through `user`.  Every rank makes the same calls in the same order (the pair count is read from the same    */
/* all-reduced Gram on every rank).  A failing callback makes the call return BYZ_E_COLLECTIVE.  What          */
/* attacking_federate_learning_amd/sharded.py composes in Python over torch.distributed, for hosts without it. */
/* no_defense, trimmed_mean, the drift attack and the robust learning rate's vote and flip are independent per */
/* column: call the single-GPU entry points on the local slice.                                                */
typedef int (*byz_allreduce_f64_fn)(void* user, double* buf_dev, int64_t count, void* stream);
int byz_pairwise_distances_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows,
                                       int64_t n_cols_local, int64_t ld, byz_allreduce_f64_fn allreduce,
                                       void* user, float* dist_dev, void* stream);
/* defences.krum over the slices: *index_host is the reference's index (the same on every rank),              */
/* out_row_local_dev (optional) this rank's n_cols_local columns of the winning row.                           */
int byz_krum_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local,
                         int64_t ld, int64_t users_count, int64_t corrupted_count, int check_assert,
                         byz_allreduce_f64_fn allreduce, void* user, float* out_row_local_dev,
                         int32_t* index_host, void* stream);
/* defences.bulyan over the slices: out_local_dev = this rank's n_cols_local columns of the aggregate,         */
/* selection_dev (optional) the theta selected clients in selection order (the same on every rank).            */
int byz_bulyan_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local,
                           int64_t ld, int64_t users_count, int64_t corrupted_count,
                           byz_allreduce_f64_fn allreduce, void* user, float* out_local_dev,
                           int32_t* selection_dev, void* stream);

/* Multi-Krum over the slices: the same selection on every rank (selection_dev optional, m     */
/* int32 in ranking order), out_local_dev = this rank's n_cols_local columns of the aggregate.  */
int byz_multi_krum_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local,
                               int64_t ld, int64_t users_count, int64_t corrupted_count, int64_t m,
                               int check_assert, byz_allreduce_f64_fn allreduce, void* user,
                               float* out_local_dev, int32_t* selection_dev, void* stream);

/* The geometric median over the slices: out_local_dev = this rank's columns of the median.   */
/* One all-reduce of n_rows + 1 doubles for the finiteness fallback (every rank's squared      */
/* norms where its own columns are not finite, and its flag), then one of n_rows per-row       */
/* partials per rowsq: 2 + max_iter calls in all, on every rank, whatever the iteration the    */
/* loop stops at (the stop is decided on all-reduced data, the same on every rank).            */
int byz_geometric_median_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows,
                                     int64_t n_cols_local, int64_t ld, const byz_geomed_params* params,
                                     byz_allreduce_f64_fn allreduce, void* user, float* out_local_dev,
                                     double* weights_dev, void* stream);

/* Centered clipping over the slices: every rank holds its columns of G and of start             */
/* (start_local_dev optional: zeros); out_local_dev = this rank's columns of the result.  A rank's  */
/* row distances cover its own columns: one all-reduce of n_rows doubles (the per-row partials)     */
/* per distance computation makes them whole -- `iters` calls in all, on every rank, whatever the   */
/* data (none for iters = 0).  The scales (scales_dev optional) are then the same on every rank and */
/* the update is local to the columns.                                                              */
int byz_centered_clip_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows,
                                  int64_t n_cols_local, int64_t ld, const byz_cclip_params* params,
                                  byz_allreduce_f64_fn allreduce, void* user, const float* start_local_dev,
                                  float* out_local_dev, double* scales_dev, void* stream);

/* FLTrust over the slices: every rank holds its columns of G and of the root; out_local_dev = this rank's       */
/* columns of the result.  A rank's p, q and q0 cover its own columns: ONE all-reduce of 2 * n_rows + 1 doubles     */
/* (p, q, q0, in that order) makes them whole -- one call, on every rank, whatever the data.  The trust scores      */
/* (trust_dev, weights_dev optional) are then the same on every rank and the sum is local to the columns.           */
int byz_fltrust_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local, int64_t ld,
                            const float* root_local_dev, byz_allreduce_f64_fn allreduce, void* user,
                            float* out_local_dev, double* trust_dev, double* weights_dev, void* stream);

/* SignGuard over the slices: every rank holds its columns of G.  A rank counts the part of the GLOBAL window that falls in   */
/* its slice -- local_window_start and local_window_len, within the slice; a length of 0 is allowed -- and params->window_len  */
/* is the global m.  ONE all-reduce of 4 * n_rows doubles (pos, zero, neg, q, in that order; a count is exact as a double)     */
/* makes them whole -- one call, on every rank, whatever the data.  The selection is then replicated on every rank and the    */
/* sum is local to the columns.  The result differs from byz_signguard_dev's by the order of q's partial sums only.            */
int byz_signguard_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local, int64_t ld,
                              const byz_signguard_params* params, int64_t local_window_start, int64_t local_window_len,
                              const int32_t* sample_dev, byz_allreduce_f64_fn allreduce, void* user, float* out_local_dev,
                              int32_t* keep_dev, double* weights_dev, int32_t* labels_dev, void* stream);

/* NNM over the slices (the columns layout; a clients layout is not offered): byz_pairwise_distances_sharded_dev's exchange  */
/* and nothing more.  The lists (nbr_dev optional) are then the same on every rank and the mix is local to the columns:        */
/* Y_local_dev (n_rows x n_cols_local, leading dimension ldy) = this rank's columns of the mixed matrix.                       */
int byz_nnm_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local, int64_t ld,
                        int64_t users_count, int64_t corrupted_count, byz_allreduce_f64_fn allreduce, void* user,
                        float* Y_local_dev, int64_t ldy, int32_t* nbr_dev, void* stream);

/* DnC over the slices.  The caller maps every iteration's global sample onto the ranks: local_counts (HOST,  */
/* n_iters entries) is the number of iteration t's sampled columns this rank owns -- 0 is allowed --, and      */
/* columns_local_dev their indices within the slice, ascending, the iterations one after the other            */
/* (sum of local_counts entries; may be NULL when that sum is 0).  params->sub_dim is the global figure and    */
/* bounds every local count.  Column means and w = C^T u are local to the owner of a column; what is summed     */
/* over the ranks are n_rows-vectors: the activity flags, the diagonal of M and every product y.  That is       */
/* n_iters * (power_iters + 3) all-reduce calls of n_rows doubles each, on every rank, whatever the data.  The  */
/* selection (good_dev optional, byz_dnc_info) is the same on every rank; out_local_dev = this rank's columns   */
/* of the mean.  The scores differ from the single-GPU call's by the order of the fp64 partial sums only.       */
int byz_dnc_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local, int64_t ld,
                        const byz_dnc_params* params, const int64_t* columns_local_dev,
                        const int64_t* local_counts, byz_allreduce_f64_fn allreduce, void* user,
                        float* out_local_dev, int32_t* good_dev, void* stream);

/* Top-k over the slices: the one step here that is NOT local to a column.  Rank rank_index of rank_count holds n_local      */
/* consecutive columns (0 is allowed; the vectors may then be NULL); the slices follow one another in rank order, so a        */
/* column's global index is ordered by (rank, local index).  k and n_total are the GLOBAL figures (0 <= k <= n_total,         */
/* n_local <= n_total, 0 <= rank_index < rank_count; BYZ_E_INVALID otherwise).  Per select pass ONE all-reduce of the pass's  */
/* bins as doubles (a count is exact as a double), then ONE of rank_count doubles (every rank's ties at T in its own slot,    */
/* zero elsewhere: a gather by summation) from which a rank takes its share of the tie quota after the ranks before it.       */
/* That is FOUR calls, of 2048, 1024, 1024 and rank_count doubles in that order: constants of the build, the same on every   */
/* rank whatever the data, k = 0 and k = n_total included.  The selected set is byz_topk_sparsify_dev's on the concatenated  */
/* vector, bit for bit.  The overlap rules are byz_topk_sparsify_dev's.  There is no byz_sparsefed_sharded_dev: a host calls */
/* byz_centered_clip_sharded_dev (iters = 1, no start) and then this entry point with x = its slice of W, add = its slice of */
/* the aggregate.                                                                                                            */
int byz_topk_sparsify_sharded_dev(byz_ctx* ctx, const float* x_local_dev, const float* add_local_dev_or_null, int64_t n_local,
                                  int64_t n_total, int64_t k, int rank_index, int rank_count, byz_allreduce_f64_fn allreduce,
                                  void* user, float* out_local_dev, float* residual_local_dev_or_null, void* stream);
/* FLAME over the ranks' column slices: TWO all-reduces, the n x n Gram and the n squared norms (the Gram alone is skipped when   */
/* dist_dev_or_null is given); everything after them is replicated (the selection, the scales) or local to the columns (the sum, */
/* and the noise, which is addressed by global column: params->column_offset is the global index of this rank's first column).   */
/* The ranks' outputs concatenate to byz_flame_dev's vector up to the fp64 rounding of the all-reduced sums.                     */
int byz_flame_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local, int64_t ld,
                          const byz_flame_params* params, byz_allreduce_f64_fn allreduce, void* user,
                          const float* dist_dev_or_null, float* out_local_dev, int32_t* admitted_dev_or_null, void* stream);
/* Multi-Metrics over the ranks' column slices: the L1 sums are additive over the slices, so beside the Gram's all-reduce (and the  */
/* near-duplicate pairs', when there are any) there is ONE more of n x n doubles, issued after it.  The features, the scores and   */
/* the selection are replicated; the final mean is local to the columns.  The ranks' outputs concatenate to                        */
/* byz_multi_metrics_dev's vector up to the fp64 rounding of the all-reduced sums.  A rank-local argument error returns before any */
/* collective.                                                                                                                     */
int byz_multi_metrics_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local, int64_t ld,
                                  int64_t keep, byz_allreduce_f64_fn allreduce, void* user, float* out_local_dev,
                                  int32_t* flags_dev_or_null, void* stream);

/* ClippedClustering over the ranks' column slices: TWO all-reduces, the n x n Gram and the n squared norms (the Gram's is skipped    */
/* when dist_dev_or_null is given); the selection and the scales are replicated on every rank, the sum is local to the columns.      */
/* The ranks' outputs concatenate to byz_clipped_clustering_dev's vector up to the fp64 rounding of the all-reduced sums.            */
int byz_clipped_clustering_sharded_dev(byz_ctx* ctx, const float* G_local_dev, int64_t n_rows, int64_t n_cols_local, int64_t ld,
                                       const byz_clipped_clustering_params* params, byz_allreduce_f64_fn allreduce, void* user,
                                       const float* dist_dev_or_null, float* out_local_dev, int32_t* admitted_dev_or_null,
                                       void* stream);

/* ---- malicious.Attack.attack / DriftAttack._attack_grads (malicious.py:10-36) ---------- */
/* Column mean and population std over the n_rows rows of G (the malicious clients' honest  */
/* gradients), drifted vector = mean - num_std * std.  Any output pointer may be NULL.      */
/* write_back != 0 also overwrites every row of G with the drifted vector (what             */
/* collect_gradients would copy in, server.py:81-83).                                       */
int byz_drift_attack_dev(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                         float num_std, float* drift_dev, float* mean_dev, float* std_dev,
                         int write_back, void* stream);
/* The same statistics when the rows are spread over several owners (the clients layout of   */
/* sharded.py: the malicious clients' rows sit on the first ranks).  numpy adds in row order,  */
/* so the additions form ONE chain through all owners: each calls byz_column_chain_dev on its  */
/* rows with the previous owner's output as carry_in (NULL for the first) -- out_sum[c] =      */
/* carry_in[c] + its rows' values in row order, or with `mean` their fl(fl(x - mean)^2) -- and */
/* the last owner ends a chain with byz_column_finish_dev: sum != NULL: mean = sum / total_rows */
/* (written); sumsq != NULL: std = sqrt(sumsq / total_rows), drift = mean - num_std * std (mean */
/* read where sum is NULL).  Bit for bit what byz_drift_attack_dev returns on the stacked rows. */
int byz_column_chain_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                         const float* carry_in_dev, const float* mean_dev, float* out_sum_dev, void* stream);
int byz_column_finish_dev(byz_ctx* ctx, const float* sum_dev, const float* sumsq_dev, int64_t total_rows,
                          float num_std, int64_t n_cols, float* mean_dev, float* std_dev, float* drift_dev,
                          void* stream);
/* The hook alone (malicious.py:34-36): mean[:] -= num_std * std[:], in place on the device. */
int byz_drift_axpy_dev(byz_ctx* ctx, float* mean_dev, const float* std_dev, int64_t n,
                       float num_std, void* stream);

/* ---- The attacks of Fang, Cao, Jia & Gong, "Local Model Poisoning Attacks to Byzantine-Robust Federated Learning" (USENIX    */
/* Security 2020, sections 4.2 and 4.3; not in the reference) ----                                                                */
/* The adaptive baseline beside A Little Is Enough: one attack tailored to the trimmed mean and the median, one to Krum.  G is    */
/* n_rows x n_cols; rows 0 .. c - 1 (c = n_attackers) are the attacker's and hold their honest gradients on entry, rows c ..      */
/* n_rows - 1 are benign.  The paper works on local MODELS; a gradient g moves the model by -lr g, so its "changing direction"    */
/* s = -1 is a column mean above 0 here and its "above the largest benign model" is "below the smallest benign gradient".         */
/*                                                                                                                                */
/* A. Trimmed-mean / median attack, full knowledge (section 4.3).  Per column j:                                                  */
/*   mean_j = np.mean(G[:, j]) over ALL rows: byz_no_defense_dev's bits.                                                          */
/*   lo_j = np.fmin.reduce(G[c:, j]), hi_j = np.fmax.reduce(G[c:, j]) over the BENIGN rows: a NaN is skipped, a column with no     */
/*   benign number gives NaN (of zeros of both signs the first one met stays).                                                    */
/*   mean_j > 0: every attacker value is drawn from [lo / b, lo] when lo > 0, else from [b lo, lo];                                */
/*   otherwise (mean_j <= 0, -0.0, NaN): from [hi, b hi] when hi > 0, else from [hi, hi / b].                                       */
/*   The ends A <= B are fp64: one product or quotient of b and the fp32 extreme.                                                 */
/* B. The same attack, partial knowledge: mu_j, sigma_j = the attacker rows' np.mean and np.var ** 0.5 (byz_drift_attack_dev's     */
/*   bits, write_back = 0).  mu_j > 0: drawn from [mu - k_hi sigma, mu - k_lo sigma], otherwise from [mu + k_lo sigma, mu + k_hi   */
/*   sigma]; the ends are (double)mu -+ fl64(k * (double)sigma).  One attacker has sigma = 0: the value is the end itself.        */
/* The draw: u = (word + 0.5) * 2^-32 in fp64 (exact, inside (0, 1)); value = fl32(A + fl64(u * fl64(B - A))).  Rounding is         */
/*   monotone, so fl32(A) <= value <= fl32(B).  An end that is not finite gives the extreme itself (lo_j, hi_j, or the k_lo end): */
/*   no inf - inf, never a new NaN.  The word of (attacker row i, global column j) is word j & 3 of the Philox4x32-10 block        */
/*   (key = seed, counter = (low, high word of j >> 2, round, i)): byz_noise_words_dev's stream with `round | i << 32` as its     */
/*   round.  `round` therefore has 32 bits (BYZ_E_INVALID beyond).  Every attacker row draws independently, the paper's "sample c */
/*   numbers"; one call, a misaligned caller and any split of the columns over ranks draw the same bits.                          */
/* There is NO SHARDED ENTRY POINT for A and B: given column_offset they are local to a column, a rank of the columns layout      */
/*   calls byz_fang_trmean_attack_dev on its slice with the global index of its first column.                                     */
typedef struct byz_fang_params {
    double b;               /* full knowledge: the interval's factor, finite and > 1 (the paper's 2)            */
    double k_lo, k_hi;      /* partial knowledge: 0 <= k_lo <= k_hi, finite (the paper's 3 and 4)                */
    int partial;            /* 0: full knowledge (A); otherwise partial knowledge (B)                            */
    uint64_t seed, round, column_offset;   /* the Philox key; the round counter, < 2^32; the global column of     */
                            /* column 0 of G, column_offset + n_cols <= 2^62                                      */
} byz_fang_params;
/* mean_dev, lo_dev, hi_dev (n_cols floats each, any of them NULL, not all) of rule A in ONE read of G; 0 <= n_attackers <=       */
/* n_rows (n_attackers = n_rows: no benign row, lo = hi = NaN).                                                                   */
int byz_column_extremes_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers,
                            float* mean_dev, float* lo_dev, float* hi_dev, void* stream);
/* The draw alone, into the n_attackers >= 1 rows of G_dev.  Full knowledge: a = mean, b = lo, c = hi; partial: a = mu, b =       */
/* sigma, c is not read.                                                                                                          */
int byz_fang_fill_dev(byz_ctx* ctx, float* G_dev, int64_t n_attackers, int64_t n_cols, int64_t ld, const byz_fang_params* params,
                      const float* a_dev, const float* b_dev, const float* c_dev_or_null, void* stream);
/* The attack, in place on rows 0 .. n_attackers - 1: byz_column_extremes_dev (full) or the attacker rows' statistics (partial)   */
/* into a context workspace, then byz_fang_fill_dev.  n_attackers = 0 does nothing; full knowledge needs n_attackers < n_rows.    */
/* Every launch is enqueued up front; nothing synchronises with the host.                                                        */
int byz_fang_trmean_attack_dev(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers,
                               const byz_fang_params* params, void* stream);
/* The same on a host matrix, which is left as it is: rows_host receives the n_attackers x n_cols attacked rows.  Synchronous.    */
int byz_fang_trmean_attack_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t n_attackers,
                                const byz_fang_params* params, float* rows_host);
/* C. Krum attack, full knowledge (section 4.2).  s_j = +1 where mean_j > 0 (rule A's mean), else -1; every attacker row becomes  */
/* the ONE vector -lambda s.  The paper's other c - 1 rows "within epsilon of the first" are copies of it here, as in every       */
/* public implementation.  Upper bound (Theorem 1, with w_Re the zero gradient), all in fp64:                                     */
/*   lambda_0 = min_i S_i / ((n - 2c - 1) sqrt(d)) + sqrt(max_i q_i) / sqrt(d),  q_i = |g_i|^2 of benign row i (byz_row_dots_dev), */
/*   S_i = the sum, in column order, of benign i's n - c - 2 smallest distances to the other benign rows: its row of              */
/*   byz_pairwise_distances_dev of the benign block without the first of its largest entries.                                     */
/* lambda = lambda_0, lambda_0 / 2, ...: a step writes the attacker's c rows and columns of the n x n fp32 distance matrix from   */
/*   d(benign i, -lambda s)^2 = q_i + fl(fl(2 lambda) t_i) + fl(fl(lambda lambda) d),  t_i = g_i . s (byz_row_dots_dev),           */
/*   summed left to right in fp64, then fl32(sqrt(max(., 0))); attacker-attacker entries are 0, the diagonal +inf as              */
/*   byz_pairwise_distances_dev writes it; the benign block is computed ONCE, no step costs a Gram.  Then the library's own        */
/*   byz_krum_select_dev(dist, n, n, c).  The loop stops at the first lambda for which Krum returns an index < c (succeeded = 1),  */
/*   or after the first lambda tried that lies below *threshold (succeeded = 0); the last lambda tried is used either way, and    */
/*   rows 0 .. c - 1 of G are overwritten with -lambda s (fl32(lambda) with the sign).                                            */
/* n_rows > 2 n_attackers + 1 and n_attackers >= 1, *threshold finite and > 0 (the paper's 1e-5): BYZ_E_INVALID otherwise, and    */
/* when lambda_0 is not finite (a benign row holds a value that is not); nothing is written then.  No doubles by value.           */
/* SYNCHRONISES: the host reads the two bounds once and one int32, Krum's index, per step (and the Gram of the benign block       */
/* waits once for its duplicate-row search, as byz_pairwise_distances_dev does).  The last launches, the rows' overwrite, are      */
/* asynchronous on `stream`.  dist_dev_or_null: n x n floats, receives the last step's matrix; t_dev_or_null, q_dev_or_null:      */
/* n_rows - n_attackers doubles each.  Under the columns layout t and q need an all-reduce: not offered here.                     */
int byz_fang_krum_attack_dev(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers,
                             const double* threshold, float* dist_dev_or_null, double* t_dev_or_null, double* q_dev_or_null,
                             void* stream);
/* The last byz_fang_krum_attack_dev on this context: lambda_0, the lambda used, the steps taken (lambda = lambda_0 / 2^(steps-1)), */
/* the index Krum chose at the last step (-1: none) and whether that was an attacker row.  Synchronises that call's stream, as     */
/* byz_flame_info does: the rows' overwrite is complete when it returns.  BYZ_E_INVALID before the first such call.               */
int byz_fang_krum_info(byz_ctx* ctx, double* lambda0, double* lambda, int64_t* steps, int64_t* chosen, int32_t* succeeded);

/* ---- The AGR-agnostic attacks of Shejwalkar & Houmansadr, "Manipulating the Byzantine: Optimizing Model Poisoning Attacks and   */
/* Defenses for Federated Learning" (NDSS 2021, section IV-C): Min-Max and Min-Sum; not in the reference ----                     */
/* Rows as in the Fang attacks: G is n_rows x n_cols, rows 0 .. m - 1 (m = n_attackers) are the attackers' and hold their honest  */
/* gradients on entry.  The KNOWN rows are all n_rows (full knowledge) or rows 0 .. m - 1 (partial != 0); r is their number.      */
/* Every attacker row becomes the ONE vector mal = mu + gamma p with the largest gamma for which                                  */
/*   Min-Max:  max_i |mal - g_i|   <= max_ij |g_i - g_j|                over the known rows,                                      */
/*   Min-Sum:  sum_i |mal - g_i|^2 <= max_i sum_j |g_i - g_j|^2         over the known rows.                                      */
/* D. The rule.  mu, sigma = byz_drift_attack_dev's mean and population std over the known rows (write_back = 0), its bits.       */
/*   The perturbation p (fp32, n_cols):                                                                                           */
/*     unit    p_k = fl32(-(double)mu_k / nrm), nrm = sqrt(sum_k (double)mu_k^2) (byz_row_sqdist_dev's order); nrm == 0: p = 0     */
/*     std     p_k = -sigma_k                                                                                                     */
/*     sign    p_k = -1 where mu_k > 0, +1 where mu_k < 0, +0.0 otherwise (a zero of either sign, a NaN)                           */
/*     custom  the caller's vector                                                                                                */
/*   Only gamma p matters.  The authors' code takes torch.std, the UNBIASED estimate: the same vector, a gamma smaller by         */
/*   sqrt((r - 1) / r).                                                                                                           */
/*   The moments, fp64 in byz_row_sqdist_dev's fixed order (byz_row_moments_dev):                                                 */
/*     a_i = sum_k ((double)x_ik - (double)mu_k)^2,  b_i = sum_k (double)p_k * ((double)mu_k - (double)x_ik),  c = sum_k p_k^2,    */
/*   so that |mal - g_i|^2 = a_i + 2 gamma b_i + gamma^2 c: the paper's search (Algorithm 1) is the root of a quadratic here.     */
/*   gamma = 0 is always feasible (mu lies in the rows' convex hull).  The authors' halving search (start 10, threshold 1e-5)     */
/*   ends within 2e-5 below that root and cannot pass 20 whatever the data; the closed form has no such ceiling.                  */
/*   Min-Max: T = (double)Dmax^2, Dmax the largest finite entry off the diagonal of the known block of                            */
/*     byz_pairwise_distances_dev's fp32 matrix (no finite entry: T = 0).  Per known row q = max(T - a_i, 0),                     */
/*     s = sqrt(b_i^2 + c q), gamma_i = b_i <= 0 ? (s - b_i) / c : q / (s + b_i) -- the form that does not cancel.                */
/*     gamma = min_i gamma_i; the binding row is the lowest such i.                                                               */
/*   Min-Sum: A = sum a_i, B = sum b_i, both in row order and kept as computed (B is 0 in exact arithmetic).  Q = r max_i a_i,    */
/*     s = sqrt(B^2 + (r c) Q), gamma = B <= 0 ? (s - B) / (r c) : Q / (s + B); the bound reported is S = Q + A, which is         */
/*     max_i sum_j |g_i - g_j|^2 because sum_j |g_i - g_j|^2 = r a_i + A about the rows' mean: no n x n table.  The binding row   */
/*     is the lowest row of max a_i.                                                                                              */
/*   Broken (broken = 1, gamma = NaN, the attacker rows are left exactly as they were): some a_i, b_i or c is not finite -- a     */
/*     value of mu that is not finite makes every a_i so -- or A, B, gamma or the bound is not (b^2 beyond fp64).                 */
/*   Degenerate (degenerate = 1, gamma = 0, the rows become mu), when not broken: c == 0, or r == 1.                               */
/*   The rows: fl32((double)mu_k + fl64(gamma * (double)p_k)), no fused multiply-add: numpy reproduces them as bits from the      */
/*     reported gamma.  No new NaN is ever written.                                                                               */
/* Not built: the AGR-tailored attacks of section IV-B, and the paper's learned initialisation of gamma (it has no search here).  */
#define BYZ_MINMAX_KIND_MINMAX 0
#define BYZ_MINMAX_KIND_MINSUM 1
#define BYZ_MINMAX_PERTURB_UNIT 0
#define BYZ_MINMAX_PERTURB_STD 1
#define BYZ_MINMAX_PERTURB_SIGN 2
#define BYZ_MINMAX_PERTURB_CUSTOM 3
typedef struct byz_minmax_params {
    int kind;               /* BYZ_MINMAX_KIND_*                                                                  */
    int perturbation;       /* BYZ_MINMAX_PERTURB_*; CUSTOM if and only if the caller passes a vector             */
    int partial;            /* 0: every row is known; otherwise the attackers' own rows alone (n_attackers >= 1)  */
    int dist_given;         /* Min-Max: 0: the call computes the known rows' r x r distance matrix (into dist_dev */
                            /* when that is not NULL); otherwise dist_dev HOLDS the n_rows x n_rows matrix of all */
                            /* the rows, whose leading r x r block is read: no Gram, and not its wait             */
} byz_minmax_params;
/* a_dev[i], b_dev[i] (n_rows doubles each) of rule D about z_dev (the centre, n_cols floats) along p_dev, in ONE read of G.     */
/* a_dev has byz_row_sqdist_dev's bits.  On one rank of the columns layout: its part over its columns, additive over the ranks.  */
int byz_row_moments_dev(byz_ctx* ctx, const float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, const float* z_dev,
                        const float* p_dev, double* a_dev, double* b_dev, void* stream);
/* The attack, in place on rows 0 .. n_attackers - 1.  n_attackers = 0 does nothing (partial needs n_attackers >= 1); an unknown */
/* kind or perturbation, a custom perturbation without its vector or a vector without it: BYZ_E_INVALID.  More known rows than   */
/* byz_row_sqdist_dev takes: BYZ_E_UNSUPPORTED; Min-Max beyond what byz_pairwise_distances_dev takes: what that returns.  Every  */
/* launch is enqueued up front and nothing synchronises with the host, except that Min-Max without dist_given waits where        */
/* byz_pairwise_distances_dev waits (the Gram's duplicate-row search).  dist_dev_or_null: see dist_given; Min-Sum ignores it.    */
int byz_minmax_attack_dev(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers,
                          const byz_minmax_params* params, const float* p_custom_dev_or_null, float* dist_dev_or_null, void* stream);
/* The same on this rank's column slice (columns layout).  mu, sigma, p and the fill are local to a column; a, b and c are sums    */
/* over the columns: ONE all-reduce of 2 r + 1 doubles, with `unit` one more of 1 double (|mu|^2) before it, and Min-Max the       */
/* all-reduces of the sharded distances.  Every rank gets the same gamma and report.  The clients layout is not offered: the rows */
/* of one client would have to meet every other rank's.                                                                           */
int byz_minmax_attack_sharded_dev(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t n_attackers,
                                  const byz_minmax_params* params, const float* p_custom_dev_or_null, float* dist_dev_or_null,
                                  byz_allreduce_f64_fn allreduce, void* user, void* stream);
/* The last attack on this context: gamma, the bound (T or S), c, the binding row (-1: none), r, and the two flags.  Synchronises */
/* that call's stream: the rows' overwrite is complete when it returns.  BYZ_E_INVALID before the first such call.                */
int byz_minmax_info(byz_ctx* ctx, double* gamma, double* bound, double* c, int64_t* binding_row, int64_t* known_rows,
                    int32_t* degenerate, int32_t* broken);
/* The same on a host matrix, which is left as it is: vector_host receives the ONE attacked vector (n_cols floats; the first      */
/* attacker's honest row when the call is broken).  p_custom_host_or_null: n_cols floats.  Synchronous.  n_attackers >= 1.         */
int byz_minmax_attack_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t n_attackers,
                           const byz_minmax_params* params, const float* p_custom_host_or_null, float* vector_host);

/* ---- next row after the path: Server.defend's update (server.py:89-90) ----------------- */
/* velocity = momentum*velocity - lr*agg ; weights += velocity, fused, in place.            */
int byz_server_update_dev(byz_ctx* ctx, float* weights_dev, float* velocity_dev,
                          const float* agg_dev, int64_t n, float momentum, float learning_rate,
                          void* stream);

/* ---- next: BackdoorAttack._attack_grads without its training loop (backdoor.py:52-65) -- */
/* out = original_params - lr * grads_mean: the parameters the malicious network starts     */
/* from (backdoor.py:54).  fp32, numpy's operation order.                                   */
int byz_backdoor_initial_params_dev(byz_ctx* ctx, const float* original_params_dev,
                                    const float* grads_mean_dev, int64_t n, float learning_rate,
                                    float* out_dev, void* stream);
/* new_grads = ((params - lr*mean) - (mal_net_params + lr*mean)) / lr, clipped to            */
/* mean +- num_std * std (backdoor.py:57-63); np.clip's NaN behaviour.  Bit-identical to    */
/* numpy fp32 on the same inputs.                                                           */
int byz_backdoor_clip_dev(byz_ctx* ctx, const float* grads_mean_dev, const float* grads_stdev_dev,
                          const float* original_params_dev, const float* mal_net_params_dev,
                          int64_t n, float learning_rate, float num_std, float* out_dev,
                          void* stream);

/* ---- next: gradient assembly (user.py:92 np.concatenate + server.py:81-83 row copy) ----- */
/* Row `row` of the device-resident G = the concatenation of n_segments device tensors      */
/* (segments_dev: HOST array of device pointers, lengths: HOST array of element counts,     */
/* summing to n_cols), one launch per 32 tensors.  The _host form takes the client's        */
/* already-concatenated numpy vector (what usr.grads is in the reference).                  */
int byz_assemble_row_dev(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                         int64_t row, int64_t n_segments, const float* const* segments_dev,
                         const int64_t* lengths, void* stream);
/* Many clients in ONE launch, each with its own tensors (server.py:81-83's loop over users):  */
/* rows first_row .. first_row + n_clients - 1; segments_dev is a HOST array of n_clients x      */
/* n_segments device pointers, client-major (client c's tensor s at [c * n_segments + s]);       */
/* lengths (HOST, n_segments, summing to n_cols) is shared by all clients -- one model.  The     */
/* pointer table is copied to a context-owned device buffer on `stream`.                         */
int byz_assemble_rows_dev(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                          int64_t first_row, int64_t n_clients, int64_t n_segments,
                          const float* const* segments_dev, const int64_t* lengths, void* stream);
/* The same launch again with the pointer table of the LAST byz_assemble_rows_dev call on this */
/* context (it stays on the device): for rounds in which no client's gradient tensor moved,    */
/* which is the normal case -- a model's .grad buffers keep their addresses.  The caller       */
/* vouches that the tensors are the ones of that call; n_clients and n_segments must match it  */
/* (BYZ_E_INVALID otherwise, or when there has been no such call).  No host-to-device copy.    */
int byz_assemble_rows_again_dev(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                                int64_t first_row, int64_t n_clients, int64_t n_segments, void* stream);
/* Every client at once (what a batched client step produces): segment s is the row-major    */
/* (n_rows x lengths[s]) gradient of parameter s for all clients; G[:, start_s:start_s+len_s] */
/* := that block.  One launch per 32 parameters.                                             */
int byz_assemble_columns_dev(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                             int64_t n_segments, const float* const* segments_dev,
                             const int64_t* lengths, void* stream);
int byz_assemble_row_host(byz_ctx* ctx, float* G_dev, int64_t n_rows, int64_t n_cols, int64_t ld,
                          int64_t row, const float* grads_host, void* stream);

/* ---- host-pointer convenience (what the numpy drop-in uses) ---------------------------- */
/* G_host is the reference's C-contiguous np.float32 users_grads.  name: 0 NoDefense, 1 Krum, */
/* 2 TrimmedMean, 3 Bulyan (the keys of defences.defend, defences.py:73-75).  out_host: n_cols */
/* floats.  aux_host (optional): Krum -> 1 int32 (index), Bulyan -> theta int32 (selection).  */
int byz_defend_host(byz_ctx* ctx, int name, const float* G_host, int64_t n_rows, int64_t n_cols,
                    int64_t users_count, int64_t corrupted_count, int check_assert,
                    float* out_host, int32_t* aux_host);
int byz_pairwise_distances_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                                float* dist_host);
int byz_krum_select_host(byz_ctx* ctx, const float* dist_host, int64_t n_rows, int64_t users_count,
                         int64_t corrupted_count, int32_t* index_host);
int byz_drift_attack_host(byz_ctx* ctx, const float* rows_host, int64_t n_rows, int64_t n_cols,
                          float num_std, float* drift_host, float* mean_host, float* std_host);

/* Multi-Krum on a host matrix: out_host (optional, n_cols floats), selection_host (optional, */
/* m int32, ranking order), at least one of them.  The aggregate asserts users_count >=         */
/* 2*corrupted_count + 1; a selection alone does not (as krum(..., return_index=True)).        */
int byz_multi_krum_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                        int64_t users_count, int64_t corrupted_count, int64_t m, float* out_host,
                        int32_t* selection_host);

/* The coordinate-wise median and the rank-trimmed mean of a host matrix (C-contiguous fp32);  */
/* out_host: n_cols floats.  Synchronous.                                                      */
int byz_coordinate_median_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                               float* out_host);
int byz_rank_trimmed_mean_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                               int64_t trim_count, float* out_host);

/* byz_window_mean_dev and byz_phocas_dev on a host matrix (C-contiguous fp32): centre_host and out_host  */
/* n_cols floats; radius_host and centre_out_host optional, n_cols floats each.  Synchronous.             */
int byz_window_mean_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols,
                         const float* centre_host, int64_t keep, float* out_host, float* radius_host);
int byz_phocas_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, int64_t trim_count,
                    float* out_host, float* centre_out_host, float* radius_host);

/* DnC on a host matrix: columns_host (n_iters * sub_dim int64, as byz_dnc_dev's list; checked here: each in  */
/* [0, n_cols), strictly ascending within an iteration, BYZ_E_INVALID otherwise), out_host (n_cols floats),    */
/* good_host (optional, n_rows int32: the kept rows ascending, then -1), kept_host (optional).  Synchronous.   */
int byz_dnc_host(byz_ctx* ctx, const float* G_host, int64_t n_rows, int64_t n_cols, const byz_dnc_params* params,
                 const int64_t* columns_host, float* out_host, int32_t* good_host, int64_t* kept_host);

/* ---- per-kernel timing (bench.py's roofline leg) --------------------------------------- */
/* When enabled, every kernel launch is bracketed by HIP events on its own stream.          */
enum {
    BYZ_K_COLUMN_STATS = 0, BYZ_K_GRAM = 1, BYZ_K_GRAM_REDUCE = 2, BYZ_K_DISTANCES = 3,
    BYZ_K_ROW_SORT = 4, BYZ_K_KRUM_ARGMIN = 5, BYZ_K_BULYAN_LOOP = 6, BYZ_K_TRIMMED_MEAN = 7,
    BYZ_K_MISC = 8, BYZ_K_PLANE_SPLIT = 9, BYZ_K_COUNT = 10
};
int byz_timing_enable(byz_ctx* ctx, int on);
int byz_timing_reset(byz_ctx* ctx);
int byz_timing_read(byz_ctx* ctx, int kernel, double* total_ms, int64_t* launches);
const char* byz_kernel_name(int kernel);

/* ---- self-test of the cross-lane exchange primitives (tests only) ----------------------- */
/* out_dev: room for 64 rows of 64 int32; n_patterns (<= 64) rows are written.  Rows 0..10:  */
/* entry [p*64 + lane] = source lane observed by `lane`; rows 11..: what every lane holds    */
/* after one of lane_exchange.hpp's wave reductions (tests/test_gpu_parity.py has the list). */
int byz_selftest_lane_exchange_dev(byz_ctx* ctx, int32_t* out_dev, int32_t* n_patterns_host,
                                   void* stream);
/* The one-workgroup loops' shared pieces (owner_loop.hpp) on one workgroup of 1024 threads.  out_dev: room for 64 rows of   */
/* 1024 int32; n_rows (<= 64) rows are written, entry [r*1024 + t] = thread t's word of row r: the generic exchange, the lane */
/* fold, two block exchanges in a row and the block sum (tests/test_gpu_parity.py has the list).                              */
int byz_selftest_owner_loop_dev(byz_ctx* ctx, int32_t* out_dev, int32_t* n_rows_host, void* stream);

/* ---- the unit table of the long-K Gram's f16x2 tile kernel (host arithmetic; tests and scripts) -------------------- */
/* What byz_gram_dev hands its tile kernel for a matrix of n_rows rows (the whole triangle, deferred slab update): one   */
/* unit per workgroup and 8192-column chunk, in launch order, BYZ_GRAM_UNIT_WORDS int32 each:                            */
/*   [0..11]    the global 32-row block behind each of the twelve row-block slots of an LDS stage                        */
/*   [12 + 3w]  wave w: LDS slot of its first A row block | slot of its first B row block << 8 | live 32 x 32 blocks of  */
/*              its 64 x 64 sub-tile (bit 2 m + n: rows 32 m.., columns 32 n..) << 16 | (row / 64) << 24 |               */
/*              (column / 64) << 25 of the sub-tile inside its 128 x 128 slab                                            */
/*   [13 + 3w]  the slab as ti (ti + 1) / 2 + tj        [14 + 3w]  the slab as ti | tj << 16   (both 0 for an idle wave) */
/* units_host: NULL, or room for capacity_units units; n_units receives the count either way.  No GPU is touched.       */
/* n_rows < 1 or more than 32767 * 128: BYZ_E_INVALID.                                                                   */
#define BYZ_GRAM_UNIT_WORDS 36
int byz_gram_unit_table(int64_t n_rows, int32_t* units_host, int64_t capacity_units, int64_t* n_units);

#ifdef __cplusplus
}
#endif
#endif /* BYZAGG_H */
