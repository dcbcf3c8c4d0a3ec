// The scalars a call leaves on the device: ONE typed block per context (byz_ctx::scalars), allocated and zeroed with it.  The
// leading `core` is all a hot path reads back; behind it one report per byz_*_info call, written by that defence's kernels and
// by the composites that run them ("public call -> reports it writes").  The last call that wrote a report is
// remembered per ReportKind (byz_ctx::last), and its info call reads the block back once, on that call's stream.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace byz {

// the sticky status' bits (CoreScalars::status)
constexpr int kStatusLostTicket = 1;     // a Gram chunk lost its ticket
constexpr int kStatusPairOverflow = 2;   // the near-duplicate pair list overflowed
constexpr int kStatusFalseTwin = 4;      // two rows with bitwise equal Gram entries turned out to differ
constexpr int kStatusSmallTimeout = 8;   // the row workgroups of the small-N path did not all report their scores in time
constexpr int kStatusNoTurn = 16;        // a wave of the register-resident column statistics never got its turn

// the Bulyan loop's status, the rows it re-scored: cleared together before every loop
struct BulyanStatus { int32_t status, rescored, pad; };
// three groups, each at the head of 32 bytes of its own
struct CoreScalars {
    int32_t krum_winner, pad0[7];
    BulyanStatus bulyan;
    int32_t pad1[5];
    int32_t status;                  // sticky: the kStatus* bits
    int32_t near_pairs;              // near-duplicate pairs listed by the last distance kernel
    // non-zero: the register-resident column statistics of the CURRENT call gave up a turn; the two-pass kernel queued behind
    // them recomputes the call's columns (zeroed before every such launch; kStatusNoTurn is no longer set)
    int32_t attack_redo, pad2;
};
struct GeomedReport {
    int32_t done, iterations, excluded, fallback;   // done: the launches still queued return at once; fallback: mean0 was not finite
    double objective;
};
// the rows the last call kept, the rows its last iteration found inactive
struct DncReport { int32_t kept, inactive; };
// of the last iteration: tau < d < inf, d not finite
struct CclipReport { int32_t clipped, excluded; };
struct FltrustReport {
    int32_t trusted, excluded;       // rows with a positive trust score, with a non-finite dot product or norm
    double trust_sum;                // T, the divisor of the sum
    int32_t root_ok, pad;            // the root's squared norm was finite and positive
};
// rows whose list is themselves alone although k > 1, rows whose list is shorter than k
struct NnmReport { int32_t solo, short_rows; };
// the columns the last call flipped
struct RlrReport { unsigned long long flipped; };
struct SgReport {
    int32_t kept, norm_failed, outside, clusters, seeds;
    int32_t flat;                    // the bandwidth was 0, not finite or below kSgMinBandwidth and every row got label 0
    double bandwidth, median;        // h, the median norm M
    double kept_f64;                 // K, the divisor of the sum
};
// selected, the ties at the threshold, those taken, the threshold key
struct TopkReport { unsigned long long selected, ties, taken, key; };
struct WeakDpReport {                // byz_clip_scales_dev, byz_weak_dp_dev and the composites that clip
    int32_t clipped, excluded;
    double clip;                     // the clip used
};
struct FlameInfo {
    int32_t admitted, broken_rows;   // the rows admitted; the rows without a finite off-diagonal distance
    float w_star;                    // the threshold (+inf: nobody admitted)
    int32_t pad;
    double admitted_f64;             // the divisor of the sum
    double clip;                     // byz_flame_dev: the median norm
};
struct MmInfo {
    int32_t kept, usable, degenerate, pad;   // rows chosen = min(usable, keep); rows with three finite features; the fallback ran
    double det;                              // det R of the features' correlation matrix (0 when fewer than 4 rows are usable)
};
struct LinkageInfo {
    int32_t admitted, usable;        // ClippedClustering: the rows admitted; the rows with a finite off-diagonal distance
    int32_t steps, rescans;          // the last linkage: its merges; the nearest-partner caches it rebuilt from a row of W
    int32_t max_rescans, pad;        // the most of them in one step
    double top_height, second_height;        // the last merge's height and the one before (0 where there is none)
    double admitted_f64;             // the divisor of the sum
    double clip;                     // byz_clipped_clustering_dev: the clip used
};
struct FabaReport {
    int32_t removed, kept;           // the rows removed; the rows kept (they add up to n)
    int32_t forced, pad;             // the rows removed beyond the caller's count because a bad count forced it
    double last_score;               // s of the last removed row (0 when nobody was removed)
    double kept_f64;                 // the divisor of the sum
};
struct AfaReport {
    int32_t rounds, kept;            // the rounds run (the last one removed nobody unless max_rounds cut it); the rows kept
    int32_t removed, excluded;       // the rows a round removed; the rows that were never usable (the three add up to n)
    int32_t branch, degenerate;      // the last removing round: -1 below the median, +1 above, 0 none; a round's A was not > 0
    double mean, med, sd, thr;       // the last complete round's statistics (0 before the first)
    double divisor;                  // the kept rows' weights summed: the divisor of the sum
};
struct AurorReport {                 // byz_auror_select_dev and byz_auror_dev: what the selection read and decided
    long long indicative, clustered; // counts[0] and counts[1] as the selection found them (accumulated: over the rounds)
    long long capped;                // counts[2]: the columns max_iter stopped
    int32_t removed, kept;           // the rows removed (bad rows included) and kept: they add up to n
    int32_t bad_rows, pad;           // the rows with a non-finite value
    double kept_f64;                 // the divisor of the sum
};
struct MinmaxReport {                // byz_minmax_attack_dev: what minmax_solve_kernel decided, what the fill reads
    double gamma;                    // NaN when broken, 0 when degenerate
    double bound;                    // Min-Max: T = Dmax^2; Min-Sum: S = r max a_i + A
    double c;                        // |p|^2
    int32_t row, r;                  // the binding row (-1: none); the known rows
    int32_t degenerate, broken;      // c == 0 or r == 1; a moment, c, gamma or the bound is not finite
};
struct FoolsgoldReport {             // byz_foolsgold_weights_dev and byz_foolsgold_dev
    int32_t usable, excluded;        // the rows with a finite diagonal entry >= 0; the others (they add up to n)
    int32_t at_zero, at_one;         // the usable rows whose weight is exactly 0, exactly 1
    int32_t degenerate, pad;         // two or more usable rows and top == 0: everybody's twin, every weight 0
    double top;                      // the largest raw weight v of a usable row (0 when nobody is usable)
    double divisor;                  // T, the divisor of the sum: the usable count, or the weights summed in ascending row order
};

struct DeviceScalars {
    CoreScalars core;
    GeomedReport geomed;
    DncReport dnc;
    CclipReport cclip;
    FltrustReport fltrust;
    NnmReport nnm;
    RlrReport rlr;
    SgReport sg;
    TopkReport topk;
    WeakDpReport weak_dp;
    FlameInfo flame;
    MmInfo mm;
    LinkageInfo linkage;
    FabaReport faba;
    AfaReport afa;
    AurorReport auror;
    MinmaxReport minmax;
    FoolsgoldReport foolsgold;
};

// What a read-back as bytes, and a 64-bit store or atomic of a kernel, rely on.  No member is padded by the compiler: the sizes
// add up, so every field lies where the declarations say.
static_assert(std::is_trivially_copyable<DeviceScalars>::value, "read back as bytes");
static_assert(sizeof(CoreScalars) % sizeof(int32_t) == 0 && sizeof(DeviceScalars) % sizeof(int32_t) == 0, "whole 4-byte words");
static_assert(sizeof(DeviceScalars) == sizeof(CoreScalars) + sizeof(GeomedReport) + sizeof(DncReport) + sizeof(CclipReport) +
                                           sizeof(FltrustReport) + sizeof(NnmReport) + sizeof(RlrReport) + sizeof(SgReport) +
                                           sizeof(TopkReport) + sizeof(WeakDpReport) + sizeof(FlameInfo) + sizeof(MmInfo) +
                                           sizeof(LinkageInfo) + sizeof(FabaReport) + sizeof(AfaReport) + sizeof(AurorReport) +
                                           sizeof(MinmaxReport) + sizeof(FoolsgoldReport),
              "no padding between the reports");
#define BYZ_AT(member) offsetof(DeviceScalars, member)
constexpr size_t kEightByteFields[] = {
    BYZ_AT(geomed.objective), BYZ_AT(fltrust.trust_sum), BYZ_AT(rlr.flipped), BYZ_AT(sg.bandwidth), BYZ_AT(sg.median),
    BYZ_AT(sg.kept_f64), BYZ_AT(topk.selected), BYZ_AT(topk.ties), BYZ_AT(topk.taken), BYZ_AT(topk.key), BYZ_AT(weak_dp.clip),
    BYZ_AT(flame.admitted_f64), BYZ_AT(flame.clip), BYZ_AT(mm.det), BYZ_AT(linkage.top_height), BYZ_AT(linkage.second_height),
    BYZ_AT(linkage.admitted_f64), BYZ_AT(linkage.clip), BYZ_AT(faba.last_score), BYZ_AT(faba.kept_f64),
    BYZ_AT(afa.mean), BYZ_AT(afa.med), BYZ_AT(afa.sd), BYZ_AT(afa.thr), BYZ_AT(afa.divisor),
    BYZ_AT(auror.indicative), BYZ_AT(auror.clustered), BYZ_AT(auror.capped), BYZ_AT(auror.kept_f64),
    BYZ_AT(minmax.gamma), BYZ_AT(minmax.bound), BYZ_AT(minmax.c),
    BYZ_AT(foolsgold.top), BYZ_AT(foolsgold.divisor)};
#undef BYZ_AT
constexpr bool eight_byte_fields_aligned() {
    for (size_t at : kEightByteFields)
        if (at % 8 != 0) return false;
    return true;
}
static_assert(eight_byte_fields_aligned(), "every double and 64-bit counter sits at an 8-byte offset");

// the reports an info call reads; byz_ctx::last[kind]: the stream of the last call that wrote it, and whether there was one
// (kReportFoolsgold, kReportMinmax, kReportAuror and kReportAfa stand in front of kReportFaba: tests/test_faba.py holds FABA's kind to the place in front of
// kReportCount; the kinds index byz_ctx::last and nothing else, so their numbers are free)
enum ReportKind {
    kReportGeomed, kReportDnc, kReportCclip, kReportFltrust, kReportNnm, kReportRlr, kReportSignguard, kReportTopk, kReportWeakDp,
    kReportFlame, kReportMultiMetrics, kReportLinkage, kReportClippedClustering, kReportFangKrum, kReportFoolsgold, kReportMinmax, kReportAuror, kReportAfa,
    kReportFaba, kReportCount
};
struct LastCall { hipStream_t stream = nullptr; bool ran = false; };

}  // namespace byz
