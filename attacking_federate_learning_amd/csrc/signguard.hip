// SignGuard (Xu, Huang, Song and Lan, "Byzantine-robust Federated Learning through Collaborative Malicious Gradient Filtering",
// ICDCS 2022; beyond the reference): rows whose norm is far from the median norm are filtered, the rows are clustered on their
// shares of positive, zero and negative coordinates over a window of the columns, and the largest cluster's rows, clipped to
// the median norm, are averaged.  One read of G, one weighted sum over the kept rows, nothing of order N^2.
//
//   census  q_i = sum_c (double)x_ic^2 over ALL columns and the integer counts pos_i, zero_i, neg_i over the window's columns,
//           in one read of G.  rowsq's geometry (geomed.hip): workgroups take (block of 32 rows, chunk of columns), a wave
//           owns 8 rows and walks its chunk in windows of 1024 columns with dwordx4 loads; every (row, chunk) partial comes
//           from one wave (lane sums, the fixed butterfly) and the finishing kernel adds a row's chunks in chunk order.  q is
//           rowsq_partial_kernel<VEC4, kRowsqDots>'s second accumulator operation for operation, so it has byz_row_dots_dev's bits.
//           A value is counted on its BITS, as robust_lr.hip decides its votes: +0.0 and -0.0 are zeros, denormals and
//           infinities count by their sign, a NaN counts nowhere.  A 1024-column step that does not meet the window does no
//           counting work (a wave-uniform test).  Lane counters are int32 (a lane sees at most chunk / 64 + 16 columns); they
//           are widened to int64 where the chunk is finished.
//   select  small kernels, all fp64, no host synchronisation (byzagg.h has the contract): the norms and their median through
//           segment_sort_u64, the features, the bandwidth from the sampled rows, the packed bins sorted and compacted into
//           seeds, the mean shift with one workgroup per POSSIBLE seed (those beyond the device-side seed count return at
//           once: the redo_gate idiom), the centres ranked, suppressed greedily, the labels, the benign cluster, keep and w.
//   sum     launch_scaled_rows_sum (geomed.hip) with w and the device double K.
// This file is compiled with -ffp-contract=off: the stated order of operations, no fused multiply-add.
#include "order_keys.hpp"
#include "row_walk.hpp"

#include <algorithm>

namespace byz {
namespace {

constexpr int kThreads = kWalkThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerWave = 8;
constexpr int kRowBlock = kWaves * kRowsPerWave;    // rows of one census workgroup (rowsq's)
constexpr int kSegs = 4;                            // dwordx4 loads per lane and row in one step
constexpr int kWindow = 64 * 4 * kSegs;             // columns a wave covers at once (1024)
constexpr int kStepThreads = 1024;
constexpr int kShiftThreads = 256;                  // a mean-shift workgroup
constexpr int kBinBits = 21;                        // bits of one coordinate's bin in a packed key
constexpr unsigned long long kNoKey = ~0ull;
constexpr uint32_t kSignBit = 0x80000000u;
constexpr uint32_t kInfBits = 0x7f800000u;

// four consecutive floats at column c (of a chunk that ends at c_end): dwordx4 when whole and aligned, masked otherwise
template <bool VEC4>
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t c, int64_t c_end, float (&x)[4]) {
    if (VEC4 && c + 4 <= c_end) {
        const float4u q = *reinterpret_cast<const float4u*>(p + c);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) x[v] = c + v < c_end ? p[c + v] : 0.0f;
    }
}

// q_part[chunk * n_rows + row]; cnt_part[(plane * chunks + chunk) * n_rows + row], plane = pos, zero, neg.
// [win_lo, win_hi): the window's columns (empty when win_hi <= win_lo).
template <bool VEC4>
__global__ __launch_bounds__(kThreads) void row_signs_partial_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols,
                                                                     int64_t ld, int64_t chunk_cols, int64_t win_lo, int64_t win_hi,
                                                                     double* __restrict__ q_part, long long* __restrict__ cnt_part) {
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kRowBlock + wave * kRowsPerWave;
    if (row0 >= n_rows) return;
    const int64_t c_begin = static_cast<int64_t>(blockIdx.y) * chunk_cols;
    const int64_t c_end = c_begin + chunk_cols < n_cols ? c_begin + chunk_cols : n_cols;
    const int64_t lo = win_lo > c_begin ? win_lo : c_begin, hi = win_hi < c_end ? win_hi : c_end;   // this chunk's part
    double acc_q[kRowsPerWave];
    int32_t n_pos[kRowsPerWave], n_zero[kRowsPerWave], n_neg[kRowsPerWave];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        acc_q[r] = 0.0;
        n_pos[r] = n_zero[r] = n_neg[r] = 0;
    }
    for (int64_t w0 = c_begin; w0 < c_end; w0 += kWindow) {
        const bool counting = w0 < hi && w0 + kWindow > lo;      // uniform: the step meets the window
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            if (row0 + r < n_rows) {
                const float* p = G + (row0 + r) * ld;
                float x[kSegs][4];
#pragma unroll
                for (int k = 0; k < kSegs; ++k) load4<VEC4>(p, w0 + k * 256 + lane * 4, c_end, x[k]);
                double s_q = 0.0;
#pragma unroll
                for (int k = 0; k < kSegs; ++k)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const double xd = static_cast<double>(x[k][v]);
                        s_q = s_q + xd * xd;
                    }
                acc_q[r] = acc_q[r] + s_q;
                if (counting) {
#pragma unroll
                    for (int k = 0; k < kSegs; ++k)
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int64_t c = w0 + k * 256 + lane * 4 + v;
                            const bool inside = c >= lo && c < hi;          // (a masked column reads +0.0 and is outside)
                            const uint32_t u = __float_as_uint(x[k][v]);
                            const uint32_t mag = u & ~kSignBit;
                            const bool by_sign = mag - 1u < kInfBits;       // 0 < mag <= 0x7f800000 (mag = 0 wraps to the top)
                            const bool minus = (u & kSignBit) != 0;
                            n_pos[r] += inside && by_sign && !minus ? 1 : 0;
                            n_neg[r] += inside && by_sign && minus ? 1 : 0;
                            n_zero[r] += inside && mag == 0u ? 1 : 0;
                        }
                }
            }
        }
    }
    const int64_t chunks = gridDim.y;
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        const double s_q = wave_sum_shfl(acc_q[r]);
        const long long pos = wave_sum_shfl<long long>(n_pos[r]), zero = wave_sum_shfl<long long>(n_zero[r]),
                        neg = wave_sum_shfl<long long>(n_neg[r]);
        if (lane == 0 && row0 + r < n_rows) {
            const int64_t at = static_cast<int64_t>(blockIdx.y) * n_rows + row0 + r;
            q_part[at] = s_q;
            cnt_part[at] = pos;
            cnt_part[chunks * n_rows + at] = zero;
            cnt_part[2 * chunks * n_rows + at] = neg;
        }
    }
}

// counts (optional): 3 * n_rows int64, pos, zero, neg; q (optional): n_rows; pznq (optional): 4 * n_rows fp64, pos, zero, neg, q
// (one all-reduce's worth; a count is exact as a double below 2^53)
__global__ __launch_bounds__(256) void row_signs_finish_kernel(const double* __restrict__ q_part, const long long* __restrict__ cnt_part,
                                                               int64_t n_rows, int chunks, long long* __restrict__ counts,
                                                               double* __restrict__ q, double* __restrict__ pznq) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_rows) return;
    double s = 0.0;
    for (int p = 0; p < chunks; ++p) s = s + q_part[p * n_rows + i];
    if (q != nullptr) q[i] = s;
    if (pznq != nullptr) pznq[3 * n_rows + i] = s;
    for (int plane = 0; plane < 3; ++plane) {
        long long c = 0;
        for (int p = 0; p < chunks; ++p) c += cnt_part[(static_cast<int64_t>(plane) * chunks + p) * n_rows + i];
        if (counts != nullptr) counts[plane * n_rows + i] = c;
        if (pznq != nullptr) pznq[plane * n_rows + i] = static_cast<double>(c);
    }
}

__global__ __launch_bounds__(256) void counts_to_f64_kernel(const long long* __restrict__ counts, const double* __restrict__ q,
                                                            int64_t n_rows, double* __restrict__ pznq) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_rows) return;
    for (int plane = 0; plane < 3; ++plane) pznq[plane * n_rows + i] = static_cast<double>(counts[plane * n_rows + i]);
    pznq[3 * n_rows + i] = q[i];
}

// ---- the selection -----------------------------------------------------------------------------------------------------------
// what the selection's kernels hand each other (zeroed in front of the first)
struct SgState {
    unsigned long long max_pos, max_zero, max_neg;
    int32_t finite_rows, seeds, centres, clusters;
};

__device__ __forceinline__ double sqdist3(const double* a, double b0, double b1, double b2) {
    const double d0 = a[0] - b0, d1 = a[1] - b1, d2 = a[2] - b2;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// keys[i] = the norm's order-preserving key (a row whose q is not finite, and the padding: all ones, behind every norm); the
// largest counts and the number of finite rows into the state
__global__ __launch_bounds__(256) void sg_norm_keys_kernel(const double* __restrict__ pznq, int64_t n, int64_t n_pad,
                                                           unsigned long long* __restrict__ keys, SgState* state) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_pad) return;
    if (i >= n) {
        keys[i] = kNoKey;
        return;
    }
    const double q = pznq[3 * n + i];
    const bool finite = __builtin_isfinite(q);
    keys[i] = norm_key(q);                       // order_keys.hpp: a row whose q is not finite sorts with the padding
    atomicMax(&state->max_pos, static_cast<unsigned long long>(pznq[i]));        // (integer maxima and counts commute)
    atomicMax(&state->max_zero, static_cast<unsigned long long>(pznq[n + i]));
    atomicMax(&state->max_neg, static_cast<unsigned long long>(pznq[2 * n + i]));
    if (finite) atomicAdd(&state->finite_rows, 1);
}

// M from the sorted keys; norm_ok and the three features of every row
__global__ __launch_bounds__(256) void sg_features_kernel(const double* __restrict__ pznq, int64_t n,
                                                          const unsigned long long* __restrict__ sorted_keys, const SgState* state,
                                                          double window_len, double lower, double upper, double* __restrict__ feat,
                                                          int32_t* __restrict__ norm_ok, SgReport* report) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t finite_rows = state->finite_rows;
    double M = __builtin_nan("");
    if (finite_rows > 0)      // np.median: the middle value, or the mean of the two middle values
        M = median_of_norm_keys(sorted_keys, finite_rows);
    if (i == 0) report->median = M;
    const double q = pznq[3 * n + i];
    const double norm = sqrt(q);
    norm_ok[i] = __builtin_isfinite(q) && lower * M < norm && norm < upper * M ? 1 : 0;
    const double top[3] = {static_cast<double>(state->max_pos) / window_len + 1e-8,
                           static_cast<double>(state->max_zero) / window_len + 1e-8,
                           static_cast<double>(state->max_neg) / window_len + 1e-8};
#pragma unroll
    for (int k = 0; k < 3; ++k) feat[3 * i + k] = (pznq[k * n + i] / window_len) / top[k];
}

// one workgroup a sampled row: kth[blockIdx.x] = the k-th smallest distance from it to the sampled rows, itself included
// (NaN when a sampled index is out of range: the bandwidth is then not finite and every row gets label 0)
__global__ __launch_bounds__(256) void sg_kth_distance_kernel(const double* __restrict__ feat, int64_t n,
                                                              const int32_t* __restrict__ sample, int s, int k,
                                                              double* __restrict__ kth) {
    __shared__ double d[kSgMaxSamples];
    const int a = sample[blockIdx.x];
    const bool a_ok = a >= 0 && a < n;
    for (int j = threadIdx.x; j < s; j += 256) {
        const int b = sample[j];
        d[j] = a_ok && b >= 0 && b < n ? sqrt(sqdist3(feat + 3 * static_cast<int64_t>(a), feat[3 * static_cast<int64_t>(b)],
                                                      feat[3 * static_cast<int64_t>(b) + 1], feat[3 * static_cast<int64_t>(b) + 2]))
                                       : __builtin_nan("");
    }
    if (threadIdx.x == 0) kth[blockIdx.x] = __builtin_nan("");
    __syncthreads();
    for (int j = threadIdx.x; j < s; j += 256) {
        const double dj = d[j];
        int before = 0;
        for (int l = 0; l < s; ++l) before += d[l] < dj || (d[l] == dj && l < j) ? 1 : 0;
        if (dj == dj && before == k - 1) kth[blockIdx.x] = dj;      // (the ranks of non-NaN values are distinct: one writer)
    }
}

// h = the caller's, or the mean of kth in sample order; flat: h is 0, not finite, or too small for the bins to pack
__global__ void sg_bandwidth_kernel(const double* __restrict__ kth, int s, double given, SgReport* report) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double h = given;
    if (!(given > 0.0)) {
        double sum = 0.0;
        for (int j = 0; j < s; ++j) sum = sum + kth[j];
        h = sum / static_cast<double>(s);
    }
    report->bandwidth = h;
    report->flat = __builtin_isfinite(h) && h >= kSgMinBandwidth ? 0 : 1;
}

// the packed bin of every row: rint(x / h), ties to even, 21 bits a coordinate (x < 1 and h >= 2^-20)
__global__ __launch_bounds__(256) void sg_bins_kernel(const double* __restrict__ feat, int64_t n, int64_t n_pad,
                                                      const SgReport* report, unsigned long long* __restrict__ keys) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_pad) return;
    if (i >= n || report->flat != 0) {
        keys[i] = kNoKey;
        return;
    }
    const double h = report->bandwidth;
    unsigned long long key = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) key = key << kBinBits | static_cast<unsigned long long>(rint(feat[3 * i + k] / h));
    keys[i] = key;
}

// the distinct bins of the sorted keys, in key order; their number into the state
__global__ __launch_bounds__(kStepThreads) void sg_seeds_kernel(const unsigned long long* __restrict__ sorted_keys, int64_t n,
                                                                unsigned long long* __restrict__ seeds, SgState* state) {
    __shared__ int lds[kStepThreads];
    const int64_t per = (n + kStepThreads - 1) / kStepThreads;
    const int64_t lo = threadIdx.x * per < n ? threadIdx.x * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    int mine = 0;
    for (int64_t i = lo; i < hi; ++i)
        mine += sorted_keys[i] != kNoKey && (i == 0 || sorted_keys[i] != sorted_keys[i - 1]) ? 1 : 0;
    int total = 0;
    int slot = block_exclusive_scan<kStepThreads>(mine, lds, &total);
    for (int64_t i = lo; i < hi; ++i)
        if (sorted_keys[i] != kNoKey && (i == 0 || sorted_keys[i] != sorted_keys[i - 1])) seeds[slot++] = sorted_keys[i];
    if (threadIdx.x == 0) state->seeds = total;
}

// fixed order over a mean-shift workgroup: the lanes' butterfly, then the waves in wave order; every thread gets the totals
__device__ __forceinline__ void shift_totals(double (&s)[3], int& count, double (*lds)[4]) {
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    double c = static_cast<double>(count);
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = wave_sum_shfl(s[k]);
    c = wave_sum_shfl(c);
    __syncthreads();                                  // (the previous round's readers are done)
    if (lane == 0) {
        lds[wave][0] = s[0]; lds[wave][1] = s[1]; lds[wave][2] = s[2]; lds[wave][3] = c;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = lds[0][k];
        for (int w = 1; w < kShiftThreads / 64; ++w) s[k] = s[k] + lds[w][k];
    }
    c = lds[0][3];
    for (int w = 1; w < kShiftThreads / 64; ++w) c = c + lds[w][3];
    count = static_cast<int>(c);
}

// One workgroup a possible seed; those beyond the seed count return at once.  Flat kernel: the members of a centre are the rows
// with squared distance <= h^2, the new centre their mean; the stop: a move <= 1e-3 h, or kSgMaxShifts updates.
__global__ __launch_bounds__(kShiftThreads) void sg_mean_shift_kernel(const double* __restrict__ feat, int64_t n,
                                                                      const unsigned long long* __restrict__ seeds,
                                                                      const SgState* state, const SgReport* report,
                                                                      double* __restrict__ centres, int32_t* __restrict__ members) {
    __shared__ double lds[kShiftThreads / 64][4];
    const int sid = blockIdx.x;
    if (sid >= state->seeds) return;
    const double h = report->bandwidth;
    const double h2 = h * h, stop = 1e-3 * h;
    const unsigned long long key = seeds[sid];
    constexpr unsigned long long kMask = (1ull << kBinBits) - 1;
    double c[3] = {h * static_cast<double>(key >> (2 * kBinBits) & kMask), h * static_cast<double>(key >> kBinBits & kMask),
                   h * static_cast<double>(key & kMask)};
    int last = 0;
    for (int it = 0; it < kSgMaxShifts; ++it) {
        double s[3] = {0.0, 0.0, 0.0};
        int count = 0;
        for (int64_t i = threadIdx.x; i < n; i += kShiftThreads) {
            const double* x = feat + 3 * i;
            if (sqdist3(x, c[0], c[1], c[2]) <= h2) {
                s[0] = s[0] + x[0]; s[1] = s[1] + x[1]; s[2] = s[2] + x[2];
                ++count;
            }
        }
        shift_totals(s, count, lds);
        last = count;
        if (count == 0) break;
        const double m[3] = {s[0] / count, s[1] / count, s[2] / count};
        const double move = sqrt(sqdist3(m, c[0], c[1], c[2]));
        c[0] = m[0]; c[1] = m[1]; c[2] = m[2];
        if (move <= stop) break;
    }
    if (threadIdx.x == 0) {
        centres[3 * sid] = c[0]; centres[3 * sid + 1] = c[1]; centres[3 * sid + 2] = c[2];
        members[sid] = last;
    }
}

// scikit-learn's order of the centres: member count descending, then the coordinates descending lexicographically (equal
// centres: the seed's position).  order[rank] = seed; the centres with members are the first state->centres of it.
__global__ __launch_bounds__(256) void sg_rank_kernel(const double* __restrict__ centres, const int32_t* __restrict__ members,
                                                      SgState* state, int32_t* __restrict__ order) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int seeds = state->seeds;
    if (i >= seeds) return;
    const int mi = members[i];
    const double a0 = centres[3 * i], a1 = centres[3 * i + 1], a2 = centres[3 * i + 2];
    int rank = 0;
    for (int j = 0; j < seeds; ++j) {
        const int mj = members[j];
        const double b0 = centres[3 * j], b1 = centres[3 * j + 1], b2 = centres[3 * j + 2];
        bool before;
        if (mj != mi) before = mj > mi;
        else if (b0 != a0) before = b0 > a0;
        else if (b1 != a1) before = b1 > a1;
        else if (b2 != a2) before = b2 > a2;
        else before = j < i;
        rank += before ? 1 : 0;
    }
    order[rank] = static_cast<int32_t>(i);
    if (mi > 0) atomicAdd(&state->centres, 1);
}

// One workgroup.  Through the ranked centres: one still standing removes every later one within <= h.  Then the standing ones,
// in rank order, are the clusters (final: 3 doubles each); their row counts are zeroed for the labelling.
__global__ __launch_bounds__(kStepThreads) void sg_suppress_kernel(const double* __restrict__ centres, const int32_t* __restrict__ order,
                                                                   SgState* state, const SgReport* report, int32_t* standing,
                                                                   double* __restrict__ final_centres, int32_t* __restrict__ label_rows) {
    __shared__ int lds[kStepThreads];
    const int live = state->centres;
    const double h = report->bandwidth;
    const double h2 = h * h;
    for (int r = threadIdx.x; r < live; r += kStepThreads) standing[r] = 1;
    for (int r = 0; r < live; ++r) {
        __syncthreads();
        if (standing[r] == 0) continue;              // (uniform: every thread reads the same word behind the barrier)
        const double* a = centres + 3 * static_cast<int64_t>(order[r]);
        for (int t = r + 1 + threadIdx.x; t < live; t += kStepThreads) {
            const double* b = centres + 3 * static_cast<int64_t>(order[t]);
            if (standing[t] != 0 && sqdist3(a, b[0], b[1], b[2]) <= h2) standing[t] = 0;
        }
    }
    __syncthreads();
    const int per = (live + kStepThreads - 1) / kStepThreads;
    const int lo = threadIdx.x * per < live ? threadIdx.x * per : live;
    const int hi = lo + per < live ? lo + per : live;
    int mine = 0;
    for (int r = lo; r < hi; ++r) mine += standing[r];
    int total = 0;
    int slot = block_exclusive_scan<kStepThreads>(mine, lds, &total);
    for (int r = lo; r < hi; ++r)
        if (standing[r] != 0) {
            const double* a = centres + 3 * static_cast<int64_t>(order[r]);
            final_centres[3 * slot] = a[0]; final_centres[3 * slot + 1] = a[1]; final_centres[3 * slot + 2] = a[2];
            label_rows[slot] = 0;
            ++slot;
        }
    if (threadIdx.x == 0) state->clusters = total;
}

// the nearest cluster's number, the first on ties; -1 when it is farther than h; flat: 0
__global__ __launch_bounds__(256) void sg_labels_kernel(const double* __restrict__ feat, int64_t n, const double* __restrict__ final_centres,
                                                        const SgState* state, const SgReport* report, int32_t* __restrict__ labels,
                                                        int32_t* label_rows) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    if (report->flat != 0) {
        labels[i] = 0;
        return;
    }
    const double h = report->bandwidth;
    const int clusters = state->clusters;
    int best = -1;
    double best_d2 = 0.0;
    for (int l = 0; l < clusters; ++l) {
        const double d2 = sqdist3(feat + 3 * i, final_centres[3 * l], final_centres[3 * l + 1], final_centres[3 * l + 2]);
        if (best < 0 || d2 < best_d2) {
            best = l;
            best_d2 = d2;
        }
    }
    if (best >= 0 && !(best_d2 <= h * h)) best = -1;
    labels[i] = best;
    if (best >= 0) atomicAdd(label_rows + best, 1);
}

// One workgroup: the benign cluster (the most rows, the lowest number on ties), keep, w, K and the counts into the report
__global__ __launch_bounds__(kStepThreads) void sg_result_kernel(const double* __restrict__ pznq, int64_t n, const int32_t* __restrict__ norm_ok,
                                                                 const int32_t* __restrict__ labels, const int32_t* __restrict__ label_rows,
                                                                 const SgState* state, SgReport* report, int32_t* __restrict__ keep,
                                                                 double* __restrict__ w, double* mk_out) {
    __shared__ int lds[kStepThreads];
    __shared__ int lds_at[kStepThreads];
    const bool flat = report->flat != 0;
    const int clusters = flat ? 1 : state->clusters;
    int benign = flat ? 0 : -1;
    if (!flat) {
        int best_rows = -1, best_at = -1;
        for (int l = threadIdx.x; l < clusters; l += kStepThreads)        // (ascending: a later equal count does not replace)
            if (label_rows[l] > best_rows) {
                best_rows = label_rows[l];
                best_at = l;
            }
        lds[threadIdx.x] = best_rows;
        lds_at[threadIdx.x] = best_at;
        __syncthreads();
        for (int step = kStepThreads / 2; step >= 1; step >>= 1) {
            if (threadIdx.x < step) {
                const int r = lds[threadIdx.x + step], at = lds_at[threadIdx.x + step];
                if (at >= 0 && (r > lds[threadIdx.x] || (r == lds[threadIdx.x] && at < lds_at[threadIdx.x]))) {
                    lds[threadIdx.x] = r;
                    lds_at[threadIdx.x] = at;
                }
            }
            __syncthreads();
        }
        benign = lds_at[0];
        __syncthreads();
    }
    const double M = report->median;
    const int64_t per = (n + kStepThreads - 1) / kStepThreads;
    const int64_t lo = threadIdx.x * per < n ? threadIdx.x * per : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    int kept = 0, failed = 0, outside = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const bool in_cluster = benign >= 0 && labels[i] == benign;
        const bool k = norm_ok[i] != 0 && in_cluster;
        const double ratio = M / sqrt(pznq[3 * n + i]);
        keep[i] = k ? 1 : 0;
        w[i] = k ? (ratio < 1.0 ? ratio : 1.0) : 0.0;
        kept += k ? 1 : 0;
        failed += norm_ok[i] != 0 ? 0 : 1;
        outside += in_cluster ? 0 : 1;
    }
    const int n_kept = block_sum<int, kStepThreads>(kept, lds);
    const int n_failed = block_sum<int, kStepThreads>(failed, lds);
    const int n_outside = block_sum<int, kStepThreads>(outside, lds);
    if (threadIdx.x == 0) {
        report->kept = n_kept;
        report->norm_failed = n_failed;
        report->outside = n_outside;
        report->clusters = clusters;
        report->seeds = flat ? 0 : state->seeds;
        report->kept_f64 = static_cast<double>(n_kept);
        if (mk_out != nullptr) {
            mk_out[0] = M;
            mk_out[1] = static_cast<double>(n_kept);
        }
    }
}

int64_t padded_rows(int64_t n) { return std::max<int64_t>(2, next_pow2(n)); }      // segment_sort_u64 takes two keys at least

}  // namespace

// ctx->signguard for n rows: the census partials (at most 64 chunks a row), then the selection's arrays
int signguard_workspace(byz_ctx* ctx, int64_t n, int64_t n_cols, SgScratch* out) {
    int64_t chunk_cols = 0;
    const int64_t chunks = n_cols > 0 ? geomed_chunks(ctx, n, n_cols, &chunk_cols) : 0;
    const int64_t n_pad = padded_rows(n);
    Carve c;
    c.take(&out->q_part, chunks * n);
    c.take(&out->cnt_part, 3 * chunks * n);
    c.take(&out->pznq, 4 * n);
    c.take(&out->keys, n_pad);
    c.take(&out->seeds, n);
    for (double** xyz : {&out->feat, &out->centres, &out->final_centres}) c.take(xyz, 3 * n);
    c.take(&out->kth, kSgMaxSamples);
    c.take(&out->w, n);
    c.take(&out->state, 64);               // SgState (launch_signguard_select asserts that it fits)
    for (int32_t** per_row : {&out->norm_ok, &out->members, &out->order, &out->standing, &out->label_rows, &out->keep, &out->labels})
        c.take(per_row, n);
    c.take(&out->sample, kSgMaxSamples);
    return c.commit(ctx->signguard);
}

int launch_row_signs(byz_ctx* ctx, const SgScratch& t, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t win_start,
                     int64_t win_len, long long* counts, double* q, double* pznq, hipStream_t stream) {
    BYZ_REQUIRE(G && n_rows > 0 && n_rows <= kLargeMaxRows && n_cols > 0 && ld >= n_cols, "row signs: bad arguments");
    BYZ_REQUIRE(win_start >= 0 && win_len >= 0 && win_start <= n_cols && win_len <= n_cols - win_start,
                "row signs: the window [%lld, %lld + %lld) is outside the %lld columns", (long long)win_start, (long long)win_start,
                (long long)win_len, (long long)n_cols);
    int64_t chunk = 0;
    const int chunks = geomed_chunks(ctx, n_rows, n_cols, &chunk);
    // a lane counts at most chunk / 64 + 16 columns in 32 bits
    BYZ_REQUIRE(chunk / 64 + 16 < (int64_t{1} << 31), "row signs: %lld columns a chunk is beyond the lane counters", (long long)chunk);
    const bool vec4 = (ld % 4 == 0) && aligned16(G);
    const dim3 grid(static_cast<unsigned>(ceil_div(n_rows, kRowBlock)), static_cast<unsigned>(chunks));
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    if (vec4) row_signs_partial_kernel<true><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, chunk, win_start, win_start + win_len, t.q_part, t.cnt_part);
    else row_signs_partial_kernel<false><<<grid, kThreads, 0, stream>>>(G, n_rows, n_cols, ld, chunk, win_start, win_start + win_len, t.q_part, t.cnt_part);
    BYZ_TRY(check_launch("row_signs_partial_kernel"));
    row_signs_finish_kernel<<<static_cast<unsigned>(ceil_div(n_rows, 256)), 256, 0, stream>>>(t.q_part, t.cnt_part, n_rows, chunks, counts, q, pznq);
    return check_launch("row_signs_finish_kernel");
}

int launch_signguard_counts_f64(byz_ctx* ctx, const long long* counts, const double* q, int64_t n, double* pznq, hipStream_t stream) {
    (void)ctx;
    counts_to_f64_kernel<<<static_cast<unsigned>(ceil_div(n, 256)), 256, 0, stream>>>(counts, q, n, pznq);
    return check_launch("counts_to_f64_kernel");
}

// pznq (4n fp64: pos, zero, neg, q) -> keep, w, labels (n each; never null), M and K into the context's report (and mk_out,
// optional: two device doubles).  sample: n_sample device int32 row numbers, read only when bandwidth is not > 0.
int launch_signguard_select(byz_ctx* ctx, const SgScratch& t, const double* pznq, int64_t n, int64_t window_len, double lower,
                            double upper, double bandwidth, const int32_t* sample, int64_t n_sample, int32_t* keep, double* w,
                            int32_t* labels, double* mk_out, hipStream_t stream) {
    BYZ_REQUIRE(pznq && keep && w && labels && n > 0 && n <= kLargeMaxRows && window_len > 0, "signguard select: bad arguments");
    const bool estimate = !(bandwidth > 0.0);
    BYZ_REQUIRE(!estimate || (sample && n_sample >= 1 && n_sample <= kSgMaxSamples), "signguard select: bad sample");
    static_assert(sizeof(SgState) <= 64, "the state's slot");
    SgState* state = reinterpret_cast<SgState*>(t.state);
    SgReport* report = &device_scalars(ctx)->sg;
    const int64_t n_pad = padded_rows(n);
    const unsigned row_blocks = static_cast<unsigned>(ceil_div(n, 256)), pad_blocks = static_cast<unsigned>(ceil_div(n_pad, 256));
    KernelTimer timer(ctx, BYZ_K_MISC, stream);
    BYZ_HIP(hipMemsetAsync(state, 0, sizeof(SgState), stream));
    sg_norm_keys_kernel<<<pad_blocks, 256, 0, stream>>>(pznq, n, n_pad, t.keys, state);
    BYZ_TRY(check_launch("sg_norm_keys_kernel"));
    BYZ_TRY(segment_sort_u64(ctx, t.keys, 1, n_pad, stream));
    sg_features_kernel<<<row_blocks, 256, 0, stream>>>(pznq, n, t.keys, state, static_cast<double>(window_len), lower, upper, t.feat,
                                                       t.norm_ok, report);
    BYZ_TRY(check_launch("sg_features_kernel"));
    if (estimate) {
        const int s = static_cast<int>(n_sample);
        sg_kth_distance_kernel<<<static_cast<unsigned>(s), 256, 0, stream>>>(t.feat, n, sample, s, std::max(1, s / 2), t.kth);
        BYZ_TRY(check_launch("sg_kth_distance_kernel"));
    }
    sg_bandwidth_kernel<<<1, 64, 0, stream>>>(t.kth, static_cast<int>(n_sample), estimate ? 0.0 : bandwidth, report);
    BYZ_TRY(check_launch("sg_bandwidth_kernel"));
    sg_bins_kernel<<<pad_blocks, 256, 0, stream>>>(t.feat, n, n_pad, report, t.keys);
    BYZ_TRY(check_launch("sg_bins_kernel"));
    BYZ_TRY(segment_sort_u64(ctx, t.keys, 1, n_pad, stream));
    sg_seeds_kernel<<<1, kStepThreads, 0, stream>>>(t.keys, n, t.seeds, state);
    BYZ_TRY(check_launch("sg_seeds_kernel"));
    sg_mean_shift_kernel<<<static_cast<unsigned>(n), kShiftThreads, 0, stream>>>(t.feat, n, t.seeds, state, report, t.centres, t.members);
    BYZ_TRY(check_launch("sg_mean_shift_kernel"));
    sg_rank_kernel<<<row_blocks, 256, 0, stream>>>(t.centres, t.members, state, t.order);
    BYZ_TRY(check_launch("sg_rank_kernel"));
    sg_suppress_kernel<<<1, kStepThreads, 0, stream>>>(t.centres, t.order, state, report, t.standing, t.final_centres, t.label_rows);
    BYZ_TRY(check_launch("sg_suppress_kernel"));
    sg_labels_kernel<<<row_blocks, 256, 0, stream>>>(t.feat, n, t.final_centres, state, report, labels, t.label_rows);
    BYZ_TRY(check_launch("sg_labels_kernel"));
    sg_result_kernel<<<1, kStepThreads, 0, stream>>>(pznq, n, t.norm_ok, labels, t.label_rows, state, report, keep, w, mk_out);
    return check_launch("sg_result_kernel");
}

}  // namespace byz
