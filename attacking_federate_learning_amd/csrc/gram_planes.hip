// The Gram contraction of defences.py:16-21 on PRE-SPLIT operands (the long-K, many-tile case: N >= 2817, D > 16384).
//
// gram.hip's split arithmetic turns every fp32 operand into 16-bit planes inside the tile kernel, i.e. once per (tile,
// element): at N = 4000 every element of G is split ~32 times, and that VALU work (and its power: the kernel runs at the
// socket's power cap) is what holds the matrix pipe at a third of its rate.  Here the split runs ONCE per element:
//
//   plane_split_*_kernel   G[:, k0 : k0 + SC] (fp32, row-major)  ->  16-bit planes of that column range, stored in MFMA
//                          FRAGMENT ORDER: for every (32-row block, 16-column step, plane) the 1 KiB image that the 64
//                          lanes of a wave hold as the A/B operand of v_mfma_f32_32x32x16_{bf16,f16} (lane l: row l & 31,
//                          columns 8 (l >> 5) .. + 7).  HBM bound.
//   gram_planes_kernel     (bf16x3) one workgroup = 8 waves = a 256 x 128 tile of C = G G^T (two 128 x 128 slabs of
//                          gram.hip's slab format), each wave a 64 x 64 sub-tile.  A 16-column stage of the 12 row blocks
//                          reaches LDS by LDS-DMA as contiguous 1 KiB pieces (lane-linear on both sides: perfectly coalesced,
//                          conflict-free ds_read_b128, no swizzle), NBUF stages of LDS, the DMA NBUF stages ahead, and the
//                          MFMAs of stage s run from registers while the fragments of stage s + 1 are read.
//   gram_planes16_kernel   (f16x2) the same tile, planes and ring on v_mfma_f32_16x16x32_f16, 32 columns per step.
//
// Two arithmetics (BYZ_GRAM_MODE):
//   f16x2  (default here)  per (row, 8192-column chunk) the values are scaled by a power of two so that the chunk's
//          largest magnitude lies in [2^14, 2^15), then x = h + m + r with h = fp16(x), m = fp16(x - h) (both round to
//          nearest), |r| <= 2^-23 |x|: the operand's own fp32 rounding unit.  Three fp16 MFMAs per block form
//          m h' + h m' + h h' (each product exact in fp32); the dropped m m' is below 2^-22 |x y| with a random sign, except
//          on the diagonal where sum m^2 = ~4e-8 sum x^2.  Against fp64: 6e-8 relative on c_ii, 1e-9 on c_ij (numpy
//          emulation and GPU test) -- the reference's own np.linalg.norm (OpenBLAS sdot, fp32 accumulation) is
//          1e-6 .. 8e-5 on the same data.  Half the MFMAs and two thirds of the operand bytes of bf16x3.  The scale is
//          undone exactly (power of two, in fp64) when a chunk's sum enters the slab.
//   bf16x3 EXACTLY gram.hip's split mode, operation for operation (three truncated bf16 planes, six terms in the same
//          order per 16-column step, 256-column MFMA chains, fp32 level-1 sums, fp64 slab per chunk): the Gram is bitwise
//          the fused kernel's; tests/test_gpu_scale.py::test_plane_gram_is_bitwise_the_fused_gram holds it to that.
//
// The super-chunk SC (a multiple of the 8192-column chunk) is sized by a memory budget; per super-chunk one split launch
// and one tile launch, stream-ordered.  Inside a launch a workgroup computes one (tile, 8192-column chunk) unit, and all
// chunks of a tile add in chunk order into the tile's fp64 slabs: behind a ticket per tile inside the tile kernel, or
// (f16x2, deferred) in chunk_reduce_kernel after it.  Rounds of one workgroup per CU start together.  bf16x3 keeps
// gram.hip's schedule: a tile list in 8 x 8 super-blocks, a contiguous share of it per XCD.  f16x2 lists the tiles in bands
// of four 256-row blocks, as a table of units that says where every wave's operands and sub-tile are (build_gram_units: on
// the diagonal two unit types of their own), and the XCDs claim runs of units from one counter.
#include "common.hpp"

#include <cstring>
#include <type_traits>

namespace byz {
namespace {

constexpr int kWgRows = 256;            // rows of the workgroup tile (A side)
constexpr int kWgCols = 128;            // columns of the workgroup tile (B side) = one slab edge
constexpr int kSlab = 128;              // slab edge of gram.hip (TM)
constexpr int kThreads = 512;
constexpr int kFragBytes = 1024;        // 64 lanes x 16 bytes
constexpr int kRowBlocks = (kWgRows + kWgCols) / 32;  // 8 A + 4 B
constexpr int kChunkCols = 8192;        // must match gram.hip's chunk (the fp32 level-1 sums never spill inside one)
constexpr int kChunkSteps = kChunkCols / 16;
constexpr int kFlushSteps = 16;         // 256-column MFMA chains (the 16-bit MFMAs accumulate with truncation)
constexpr int kSpareRoundsPercent = 10;  // spare rounds per XCD of the f16x2 tile kernel (5, 12 and 30 % measured alike: G8)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// gram.hip's split8, verbatim in effect: x = h + m + l, the three 8-bit fields of the 24-bit significand (truncation)
__device__ __forceinline__ void split_bf16x3(const f32x4& lo4, const f32x4& hi4, u32x4& hp, u32x4& mp, u32x4& lp) {
    uint32_t xb[8], r1b[8], r2b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = e < 4 ? lo4[e] : hi4[e - 4];
        xb[e] = __float_as_uint(x);
        const float r1 = x - __uint_as_float(xb[e] & 0xffff0000u);
        r1b[e] = __float_as_uint(r1);
        const float r2 = r1 - __uint_as_float(r1b[e] & 0xffff0000u);
        r2b[e] = __float_as_uint(r2);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        hp[e] = __builtin_amdgcn_perm(xb[2 * e + 1], xb[2 * e], 0x07060302u);
        mp[e] = __builtin_amdgcn_perm(r1b[2 * e + 1], r1b[2 * e], 0x07060302u);
        lp[e] = __builtin_amdgcn_perm(r2b[2 * e + 1], r2b[2 * e], 0x07060302u);
    }
}

// x * scale = h + m + r, h and m fp16 (round to nearest), |r| <= 2^-23 |x * scale| (x - h is exact in fp32)
__device__ __forceinline__ void split_f16x2(const f32x4& lo4, const f32x4& hi4, float scale, u32x4& hp, u32x4& mp) {
    f16x8 h, m;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = (e < 4 ? lo4[e] : hi4[e - 4]) * scale;
        h[e] = static_cast<_Float16>(x);
        m[e] = static_cast<_Float16>(x - static_cast<float>(h[e]));
    }
    hp = __builtin_bit_cast(u32x4, h);
    mp = __builtin_bit_cast(u32x4, m);
}

__device__ __forceinline__ f32x4 load4_tail(const float* __restrict__ src, int64_t k, int64_t n_cols) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (k + 3 < n_cols) {
        v = *reinterpret_cast<const f32x4*>(src + k);
    } else {
        if (k + 0 < n_cols) v.x = src[k + 0];
        if (k + 1 < n_cols) v.y = src[k + 1];
        if (k + 2 < n_cols) v.z = src[k + 2];
    }
    return v;
}

// bf16x3: one workgroup = a 32-row block x 128 columns (8 steps).  Reads are 128-byte row segments, the transposition
// into fragment order goes through LDS, writes are whole 1 KiB fragment images.
constexpr int kSplitCols = 128;
__global__ __launch_bounds__(256) void plane_split_bf16_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols,
                                                               int64_t ld, const int32_t* __restrict__ row_index,
                                                               int64_t k0, int64_t n_steps, u32x4* __restrict__ planes) {
    __shared__ __attribute__((aligned(16))) float tile[32][kSplitCols + 4];
    const int tid = threadIdx.x;
    const int64_t rb = blockIdx.y;
    const int64_t step0 = static_cast<int64_t>(blockIdx.x) * (kSplitCols / 16);
    {
        const int r = tid >> 3, c = tid & 7;
        int64_t row = rb * 32 + r;
        if (row > n_rows - 1) row = n_rows - 1;     // rows past the matrix: clamped, they land in Gram entries nobody reads
        if (row_index != nullptr) row = row_index[row];
        const float* src = G + row * ld;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int col = 4 * c + 32 * p;
            *reinterpret_cast<f32x4*>(&tile[r][col]) = load4_tail(src, k0 + step0 * 16 + col, n_cols);
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int sl = 2 * wave + i;
        const int64_t step = step0 + sl;
        if (step >= n_steps) continue;
        const int row = lane & 31, kk = sl * 16 + 8 * (lane >> 5);
        const f32x4 lo4 = *reinterpret_cast<const f32x4*>(&tile[row][kk]);
        const f32x4 hi4 = *reinterpret_cast<const f32x4*>(&tile[row][kk + 4]);
        u32x4 h, m, l;
        split_bf16x3(lo4, hi4, h, m, l);
        u32x4* out = planes + ((rb * n_steps + step) * 3) * 64 + lane;
        out[0] = h;
        out[64] = m;
        out[128] = l;
    }
}

// f16x2: one workgroup = a 32-row block x one 8192-column chunk: first the rows' largest magnitudes over the chunk (the
// 1 MiB block then sits in L2), then the split pass over it.  unscale[chunk][row] = 2^-shift, the factor that undoes the
// row's scale (a power of two: exact).
__global__ __launch_bounds__(256) void plane_split_f16_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols,
                                                              int64_t ld, const int32_t* __restrict__ row_index, int64_t k0,
                                                              int64_t n_steps, u32x4* __restrict__ planes,
                                                              double* __restrict__ unscale, int64_t rows_pad,
                                                              const int32_t* __restrict__ redo) {
    __shared__ __attribute__((aligned(16))) float tile[32][kSplitCols + 4];
    __shared__ float row_scale[32];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    // redo != nullptr: the (chunk, row block) pairs the streaming kernel listed (redo[0] of them), dealt to the workgroups of
    // the launch in a grid-stride loop: however many were listed, they are all redone and the host never has to read the
    // count back (the read-back serialised host and device once per super-chunk at N = 10,000)
    const int listed = redo != nullptr ? redo[0] : 1;
    for (int item = redo != nullptr ? static_cast<int>(blockIdx.x) : 0; item < listed; item += static_cast<int>(gridDim.x)) {
    const int64_t rb = redo != nullptr ? redo[2 + 2 * item] : blockIdx.y;
    const int64_t chunk = redo != nullptr ? redo[1 + 2 * item] : blockIdx.x;
    const int r = tid >> 3, c = tid & 7;
    int64_t row = rb * 32 + r;
    if (row > n_rows - 1) row = n_rows - 1;
    if (row_index != nullptr) row = row_index[row];
    const float* src = G + row * ld;
    const int64_t kbeg = k0 + chunk * kChunkCols;
    {
        float mx = 0.0f;
        bool bad = false;
#pragma unroll 8
        for (int i = 0; i < kChunkCols / 32; ++i) {
            const f32x4 v = load4_tail(src, kbeg + 4 * c + 32 * i, n_cols);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = __builtin_fabsf(v[e]);
                bad = bad || !(a <= 3.0e38f);          // inf or NaN: no scaling, the poison propagates as it is
                mx = __builtin_fmaxf(mx, a);
            }
        }
#pragma unroll
        for (int msk = 1; msk < 8; msk <<= 1) {
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, msk, 64));
            bad = bad || (__shfl_xor(bad ? 1 : 0, msk, 64) != 0);
        }
        int shift = 0;
        if (!bad && mx > 0.0f) {
            shift = 14 - (static_cast<int>((__float_as_uint(mx) >> 23) & 0xffu) - 127);   // mx 2^shift in [2^14, 2^15)
            if (mx < 1.17549435e-38f) shift = 126;   // subnormal magnitudes: as far up as a float scale goes
            if (shift > 126) shift = 126;
            if (shift < -126) shift = -126;
        }
        if (c == 0) {
            row_scale[r] = __uint_as_float(static_cast<uint32_t>(shift + 127) << 23);
            unscale[chunk * rows_pad + rb * 32 + r] = __longlong_as_double(static_cast<long long>(1023 - shift) << 52);
        }
    }
    __syncthreads();
    const int64_t step_base = chunk * kChunkSteps;
    for (int sub = 0; sub < kChunkCols / kSplitCols; ++sub) {
        const int64_t step0 = step_base + sub * (kSplitCols / 16);
        if (step0 >= n_steps) break;   // uniform
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int col = 4 * c + 32 * p;
            *reinterpret_cast<f32x4*>(&tile[r][col]) = load4_tail(src, k0 + step0 * 16 + col, n_cols);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int sl = 2 * wave + i;
            const int64_t step = step0 + sl;
            if (step >= n_steps) continue;
            const int frow = lane & 31, kk = sl * 16 + 8 * (lane >> 5);
            const f32x4 lo4 = *reinterpret_cast<const f32x4*>(&tile[frow][kk]);
            const f32x4 hi4 = *reinterpret_cast<const f32x4*>(&tile[frow][kk + 4]);
            u32x4 h, m;
            split_f16x2(lo4, hi4, row_scale[frow], h, m);
            u32x4* out = planes + ((rb * n_steps + step) * 2) * 64 + lane;
            out[0] = h;
            out[64] = m;
        }
        __syncthreads();
    }
    if (redo == nullptr) break;
    __syncthreads();
    }
}

// f16x2 in ONE pass over G (round 3).  The two-pass kernel above reads every element twice -- once for the row's largest
// magnitude over the chunk, once to split -- and the second read does not come out of L2 (the resident workgroups hold far
// more than 4 MiB of 1 MiB blocks): 320 GB read + 164 GB written per 160 GB of G, at copy speed.
// The scale does not have to put the chunk's largest magnitude into [2^14, 2^15): fp16 rounding is invariant under a power
// of two as long as nothing overflows and the large elements' low plane stays normal, i.e. as long as
//     2^7 <= (largest magnitude) * 2^shift < 2^16.
// So the shift comes from a SAMPLE of the row's chunk (16 groups of 8 columns, every 512 columns: 512 of its 32,768 bytes)
// placed at [2^9, 2^10) -- six binades of head room above, two below -- the chunk is then split as it streams by, and the
// true largest magnitude, which falls out of the same pass, says whether the assumption held.  Where it did not (an outlier
// 64 times the sampled maximum, a chunk whose sampled columns are all zero, inf / NaN) the (row block, chunk) goes on a
// list and the two-pass kernel redoes exactly those.  For every other block the planes are what the exact scale would give,
// scaled by a power of two that `unscale` undoes -- bit for bit for every element whose two planes stay NORMAL fp16 numbers
// under both scales; an element below ~2^-17 of the row's largest magnitude lands on a different subnormal grid (its planes
// differ by ~2^-32 of that magnitude: harmless numerically, but the Gram under the sampled scale is NOT bitwise the two-pass
// Gram, and twin rows in row blocks of which only one was redone do not give bitwise equal Gram entries -- which is why
// rows proven identical get their zero distance from the proof, gram.hip distance_kernel, not from cancellation).
constexpr int kSampleGroups = 16;
__global__ __launch_bounds__(256) void plane_split_f16_stream_kernel(const float* __restrict__ G, int64_t n_rows, int64_t n_cols,
                                                                     int64_t ld, const int32_t* __restrict__ row_index, int64_t k0,
                                                                     int64_t n_steps, u32x4* __restrict__ planes,
                                                                     double* __restrict__ unscale, int64_t rows_pad,
                                                                     int32_t* __restrict__ redo) {
    __shared__ __attribute__((aligned(16))) float tile[2][32][kSplitCols + 4];
    __shared__ float row_scale[32];
    __shared__ int block_bad;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t rb = blockIdx.y;
    const int64_t chunk = blockIdx.x;
    const int r = tid >> 3, c = tid & 7;
    int64_t row = rb * 32 + r;
    if (row > n_rows - 1) row = n_rows - 1;
    if (row_index != nullptr) row = row_index[row];
    const float* src = G + row * ld;
    const int64_t kbeg = k0 + chunk * kChunkCols;
    if (tid == 0) block_bad = 0;
    // ---- the sample: thread c of the row's eight takes groups 2 c and 2 c + 1 (eight columns each)
    int shift = 0;
    {
        float mx = 0.0f;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int64_t k = kbeg + (2 * c + g) * (kChunkCols / kSampleGroups);
            const f32x4 a = load4_tail(src, k, n_cols), b = load4_tail(src, k + 4, n_cols);
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = __builtin_fmaxf(mx, __builtin_fmaxf(__builtin_fabsf(a[e]), __builtin_fabsf(b[e])));
        }
#pragma unroll
        for (int msk = 1; msk < 8; msk <<= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, msk, 64));
        // (NaN never wins an fmax and inf gives an out-of-range exponent: both are caught by the streaming pass)
        if (mx >= 1.17549435e-38f && mx <= 3.0e38f) {
            shift = 9 - (static_cast<int>((__float_as_uint(mx) >> 23) & 0xffu) - 127);   // mx 2^shift in [2^9, 2^10)
            if (shift > 126) shift = 126;
            if (shift < -126) shift = -126;
        }
        if (c == 0) row_scale[r] = __uint_as_float(static_cast<uint32_t>(shift + 127) << 23);
    }
    // ---- the stream: sub-block s + 1 is in flight while sub-block s is transposed through LDS and split
    const int64_t step_base = chunk * kChunkSteps;
    const float scale = __uint_as_float(static_cast<uint32_t>(shift + 127) << 23);
    float true_max = 0.0f;
    bool bad = false;
    f32x4 cur[4], nxt[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) cur[p] = load4_tail(src, k0 + step_base * 16 + 4 * c + 32 * p, n_cols);
    __syncthreads();   // row_scale
    for (int sub = 0; sub < kChunkCols / kSplitCols; ++sub) {
        const int64_t step0 = step_base + sub * (kSplitCols / 16);
        if (step0 >= n_steps) break;   // uniform
        const bool more = sub + 1 < kChunkCols / kSplitCols && step0 + kSplitCols / 16 < n_steps;
        if (more) {
#pragma unroll
            for (int p = 0; p < 4; ++p) nxt[p] = load4_tail(src, k0 + (step0 + kSplitCols / 16) * 16 + 4 * c + 32 * p, n_cols);
        }
        float (*t)[kSplitCols + 4] = tile[sub & 1];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            *reinterpret_cast<f32x4*>(&t[r][4 * c + 32 * p]) = cur[p];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = __builtin_fabsf(cur[p][e]);
                bad = bad || !(a <= 3.0e38f);
                true_max = __builtin_fmaxf(true_max, a);
            }
        }
        __syncthreads();   // one barrier per sub-block: the other tile is free again once everybody has passed this one
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int sl = 2 * wave + i;
            const int64_t step = step0 + sl;
            if (step >= n_steps) continue;
            const int frow = lane & 31, kk = sl * 16 + 8 * (lane >> 5);
            const f32x4 lo4 = *reinterpret_cast<const f32x4*>(&t[frow][kk]);
            const f32x4 hi4 = *reinterpret_cast<const f32x4*>(&t[frow][kk + 4]);
            u32x4 h, m;
            split_f16x2(lo4, hi4, row_scale[frow], h, m);
            u32x4* out = planes + ((rb * n_steps + step) * 2) * 64 + lane;
            out[0] = h;
            out[64] = m;
        }
        if (more) {
#pragma unroll
            for (int p = 0; p < 4; ++p) cur[p] = nxt[p];
        }
    }
    // ---- did the sampled scale hold?  2^7 <= max 2^shift < 2^16 (an all-zero chunk holds with any scale)
#pragma unroll
    for (int msk = 1; msk < 8; msk <<= 1) {
        true_max = __builtin_fmaxf(true_max, __shfl_xor(true_max, msk, 64));
        bad = bad || (__shfl_xor(bad ? 1 : 0, msk, 64) != 0);
    }
    const float scaled = true_max * scale;
    const bool holds = !bad && (true_max == 0.0f || (scaled >= 128.0f && scaled < 65536.0f));
    if (c == 0) {
        unscale[chunk * rows_pad + rb * 32 + r] = __longlong_as_double(static_cast<long long>(1023 - shift) << 52);
        if (!holds) block_bad = 1;
    }
    __syncthreads();
    if (tid == 0 && block_bad != 0) {
        const int at = atomicAdd(redo, 1);
        redo[1 + 2 * at] = static_cast<int32_t>(chunk);
        redo[2 + 2 * at] = static_cast<int32_t>(rb);
    }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_vmcnt_dyn(int n) {   // n is wave-uniform; only the first and last stages of a chunk
    switch (n) {
#define BYZ_W(k) case k: wait_vmcnt<k>(); break;
        BYZ_W(0) BYZ_W(3) BYZ_W(4) BYZ_W(5) BYZ_W(6) BYZ_W(8) BYZ_W(9) BYZ_W(10) BYZ_W(12) BYZ_W(15) BYZ_W(16) BYZ_W(18) BYZ_W(20) BYZ_W(24)
#undef BYZ_W
        default: wait_vmcnt<0>(); break;
    }
}

struct Frags {
    bf16x8 a[3][2], b[3][2];   // [plane h, m, l][32-row block]
};

// bf16x3 (gram.hip's arithmetic).  NBUF stages of LDS; the DMA runs NBUF stages ahead.  Eight waves of 64 x 64, two per
// SIMD: each wave's sub-tile is 2 x 2 blocks of 32 x 32.  (Four waves of 128 x 64, built in round 4, are bitwise equal and
// lost by 8.6 %: EXPERIMENTS.md G4.)
template <int NBUF>
__global__ __launch_bounds__(512, 1) void gram_planes_kernel(const u32x4* __restrict__ planes, int64_t n_steps,
                                                             double* __restrict__ partial, int n_tiles,
                                                             const int2* __restrict__ tile_order, int n_chunks,
                                                             int* __restrict__ tickets, int round_size, int t128,
                                                             int slab_live0, int n_blocks32,
                                                             int32_t* __restrict__ device_status) {
    constexpr int PLANES = 3;
    constexpr int kRbBytes = PLANES * kFragBytes;           // one 32-row block, one stage: [plane][1 KiB]
    constexpr int kStage = kRowBlocks * kRbBytes;           // 36,864
    constexpr int NW = 8;                                   // waves of the workgroup
    constexpr int kPieces = kRowBlocks * PLANES;            // 1 KiB pieces per stage
    constexpr int kPerWave = (kPieces + NW - 1) / NW;       // DMA instructions per wave and stage (the last may be idle)
    constexpr int kFullWaves = kPieces % NW == 0 ? NW : kPieces % NW;   // waves that issue all kPerWave
    constexpr int kLead = NBUF;
    typedef bf16x8 frag_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];   // [NBUF][12 row blocks][planes][1 KiB]

    // workgroup -> (tile, chunk): XCD x owns a contiguous share of the tile list and works through it chunk by chunk
    const int xcd = blockIdx.x & 7;
    const int seq = blockIdx.x >> 3;
    const int base = n_tiles >> 3, rem = n_tiles & 7;
    const int mine = base + (xcd < rem ? 1 : 0);
    const int first = xcd * base + (xcd < rem ? xcd : rem);
    const int chunk = mine > 0 ? seq / mine : n_chunks;
    int* done = tickets + n_tiles + xcd;
    {
        // rounds: a workgroup starts only when every workgroup of the earlier rounds of its XCD has finished, so that the
        // members of a round walk K in step and hit each other's operand lines in the XCD's L2 (gram.hip)
        const int round = round_size > 0 ? seq / round_size : 0;
        if (round > 0 && threadIdx.x == 0) {
            unsigned spins = 0;
            while (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < round * round_size) {
                __builtin_amdgcn_s_sleep(16);
                if (++spins > (1u << 20)) break;   // only speed depends on the gate
            }
        }
        __syncthreads();
        if (chunk >= n_chunks) {
            if (threadIdx.x == 0) __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    const int t_list = first + (seq - chunk * mine);
    const int2 tt = tile_order[t_list];
    const int bi = __builtin_amdgcn_readfirstlane(tt.x);   // 256-row block of the A side
    const int tj = __builtin_amdgcn_readfirstlane(tt.y);   // 128-row block of the B side

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int ti = 2 * bi + wr / 2;                    // this wave's slab row
    const int row_in_slab = (wr % 2) * 64;             // and where its 64 x 64 sub-tile starts inside it
    // Which of the wave's 2 x 2 output blocks (32 x 32) anybody reads: block (m, n) covers 32-row block `rblk` of the A side and
    // `cblk` of the B side.  Not needed: blocks of rows past the matrix (N = 4000 pads to 4096: three quarters of the last slab
    // row; N = 10,000 to 10,112), and blocks strictly above the diagonal (gram_reduce_kernel reads a diagonal slab's lower
    // triangle only).  Round 4 skipped at slab granularity only and issued 8 % more MFMAs than 3 N^2 D / 32768 at N = 4000
    // (VERDICT r4, weak 5).  A skipped block is never multiplied, never flushed and never touches its slab entries; the blocks
    // that are computed go through the same MFMA chain in the same order as before: the Gram is bitwise the same.
    unsigned live_blocks = 0;
    if (tj <= ti && ti < t128 && n_blocks32 < 0) {
        live_blocks = 15u;     // BYZ_GRAM_BLOCK_SKIP=0: round 4's slab-granular rule
    } else if (tj <= ti && ti < t128) {     // the upper half of a tile that straddles the diagonal is not needed
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int rblk = ti * 4 + row_in_slab / 32 + m, cblk = tj * 4 + wc * 2 + n;
                if (rblk < n_blocks32 && cblk <= rblk) live_blocks |= 1u << (m * 2 + n);
            }
    }
    // The K loop is instantiated once per mask that can occur (bit m * 2 + n): all four blocks; the row block m = 0 only (the
    // last valid row block of the matrix is the first of its wave); a diagonal 64 x 64 sub-tile without its upper block;
    // both; nothing (a dead wave still takes part in the DMA and the barriers).  A run-time test per MFMA instead cost the
    // compiler its schedule (a wait for ALL pending LDS reads in front of every MFMA).
    const bool live_wave = live_blocks != 0;

    const int step0 = chunk * kChunkSteps;
    int n_stages = static_cast<int>(n_steps) - step0;
    if (n_stages > kChunkSteps) n_stages = kChunkSteps;

    // LDS-DMA: piece q = wave + 8 i of the stage (row block q / PLANES, plane q % PLANES): a wave-uniform byte offset from
    // `planes` plus 16 bytes per lane; the LDS image of a stage is piece-linear, and so is a row block's stage in HBM
    int64_t piece_off[kPerWave];
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
        int q = wave + NW * i;
        if (q >= kPieces) q = kPieces - 1;
        const int rbl = q / PLANES, piece = q % PLANES;
        const int64_t rb = rbl < 8 ? static_cast<int64_t>(bi) * 8 + rbl : static_cast<int64_t>(tj) * 4 + (rbl - 8);
        piece_off[i] = (((rb * n_steps + step0) * PLANES + piece) * 64) * 16;
    }
    const unsigned char* lane_base = reinterpret_cast<const unsigned char*>(planes) + lane * 16;
    const int my_dmas = wave < kFullWaves ? kPerWave : kPerWave - 1;
    auto dma = [&](int s) __attribute__((always_inline)) {
        unsigned char* dst = lds + (s % NBUF) * kStage + wave * kFragBytes;
#pragma unroll
        for (int i = 0; i < kPerWave; ++i) {
            if (kFullWaves != NW && i == kPerWave - 1 && wave >= kFullWaves) break;   // wave-uniform
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(lane_base + piece_off[i] + static_cast<int64_t>(s) * (PLANES * kFragBytes)),
                (__attribute__((address_space(3))) void*)(dst + i * NW * kFragBytes), 16, 0, 0);
        }
    };

    f32x16 acc[2][2], acc2[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                acc[m][n][e] = 0.0f;
                acc2[m][n][e] = 0.0f;
            }

    auto read_frags = [&](int s, Frags& f, auto mask_c) __attribute__((always_inline)) {
        constexpr unsigned MASK = decltype(mask_c)::value;     // only the fragments a live block multiplies
        const unsigned char* A = lds + (s % NBUF) * kStage + (2 * wr) * kRbBytes + lane * 16;
        const unsigned char* B = lds + (s % NBUF) * kStage + (8 + 2 * wc) * kRbBytes + lane * 16;
#pragma unroll
        for (int p = 0; p < PLANES; ++p) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
                if (((MASK >> (m * 2)) & 3u) != 0) f.a[p][m] = *reinterpret_cast<const frag_t*>(A + m * kRbBytes + p * kFragBytes);
#pragma unroll
            for (int n = 0; n < 2; ++n)
                if (((MASK >> n) & 5u) != 0) f.b[p][n] = *reinterpret_cast<const frag_t*>(B + n * kRbBytes + p * kFragBytes);
        }
    };
    // the six terms of the split product, smallest first, term-major over the accumulators (the order of gram.hip's split
    // mode): h h' + h m' + m h' + m m' + h l' + l h'
    auto multiply = [&](const Frags& f, auto mask_c) __attribute__((always_inline)) {
        constexpr unsigned MASK = decltype(mask_c)::value;
        constexpr int pa[6] = {2, 0, 1, 1, 0, 0};
        constexpr int pb[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n)
                    if (((MASK >> (m * 2 + n)) & 1u) != 0)   // folds: the loops are unrolled
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[pa[t]][m], f.b[pb[t]][n], acc[m][n], 0, 0, 0);
    };
    auto flush = [&](int s) __attribute__((always_inline)) {
        if ((s + 1) % kFlushSteps == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        acc2[m][n][e] += acc[m][n][e];
                        acc[m][n][e] = 0.0f;
                    }
        }
    };
    // one stage: multiply `cur` (stage s, in registers), read stage s + 1 into `next`, keep the DMA kLead stages ahead
    auto steady = [&](int s, const Frags& cur, Frags& next, auto mask_c) __attribute__((always_inline)) {
        constexpr bool kLive = decltype(mask_c)::value != 0;
        dma(s + kLead);                       // into the buffer of stage s, whose last readers passed the previous barrier
        if (kLive) {
            read_frags(s + 1, next, mask_c);
            multiply(cur, mask_c);
        }
        // before anyone reads stage s + 2 it must have landed: of my requests only stages s + 3 .. s + kLead may be
        // outstanding (memory reads return in order, so that is a vmcnt bound)
        if (kFullWaves == NW || wave < kFullWaves) wait_vmcnt<(kLead - 2) * kPerWave>();
        else wait_vmcnt<(kLead - 2) * (kPerWave - 1)>();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kLive) flush(s);
    };
    auto drain = [&](int s, const Frags& cur, Frags& next, auto mask_c) __attribute__((always_inline)) {
        constexpr bool kLive = decltype(mask_c)::value != 0;
        if (s + kLead < n_stages) dma(s + kLead);
        if (kLive) {
            if (s + 1 < n_stages) read_frags(s + 1, next, mask_c);
            multiply(cur, mask_c);
        }
        const int last = s + kLead < n_stages ? s + kLead : n_stages - 1;
        const int ahead = last - (s + 2);
        wait_vmcnt_dyn((ahead > 0 ? ahead : 0) * my_dmas);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kLive) flush(s);
    };

    for (int a = 0; a < kLead && a < n_stages; ++a) dma(a);
    {
        const int issued = n_stages < kLead ? n_stages : kLead;
        wait_vmcnt_dyn((issued > 2 ? issued - 2 : 0) * my_dmas);   // stages 0 and 1 have landed
    }
    asm volatile("s_barrier" ::: "memory");
    auto k_loop = [&](auto mask_c) __attribute__((always_inline)) {
        constexpr bool kLive = decltype(mask_c)::value != 0;
        Frags x, y;
        if (kLive && n_stages > 0) read_frags(0, x, mask_c);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");    // everybody has read stage 0: its buffer may be refilled
        int s = 0;
        for (; s + 1 + kLead < n_stages; s += 2) {
            steady(s, x, y, mask_c);
            steady(s + 1, y, x, mask_c);
        }
        for (; s < n_stages; s += 2) {
            drain(s, x, y, mask_c);
            if (s + 1 < n_stages) drain(s + 1, y, x, mask_c);
        }
    };
    // wave-uniform; every instantiation passes the same barriers.  A mask outside the set (there is none) computes all four.
    switch (live_blocks) {
        case 0u: k_loop(std::integral_constant<unsigned, 0u>{}); break;
        case 1u: k_loop(std::integral_constant<unsigned, 1u>{}); break;
        case 3u: k_loop(std::integral_constant<unsigned, 3u>{}); break;
        case 13u: k_loop(std::integral_constant<unsigned, 13u>{}); break;
        default: live_blocks = 15u; k_loop(std::integral_constant<unsigned, 15u>{}); break;
    }
    auto block_live = [&](int m, int n) __attribute__((always_inline)) { return ((live_blocks >> (m * 2 + n)) & 1u) != 0; };

    // epilogue: chunks of a tile add into its slabs in chunk order (gram.hip's ticket protocol)
    bool lost = false;
    if (chunk > 0) {
        if (tid == 0) {
            unsigned spins = 0;
            while (__hip_atomic_load(tickets + t_list, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != chunk) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > (1u << 26)) {   // bounded: a lost ticket must not hang the device ...
                    lost = true;
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        lost = __syncthreads_or(lost ? 1 : 0) != 0;
    }
    if (lost) {
        // ... and must not be papered over: without the ticket the slab is not ours to update (the host turns the
        // status word into BYZ_E_HIP)
        if (tid == 0) atomicOr(device_status, kStatusLostTicket);
    } else if (live_wave) {
        const bool slab_live = chunk > 0 || slab_live0 != 0;
        double* out = partial + (static_cast<int64_t>(ti) * (ti + 1) / 2 + tj) * (kSlab * kSlab);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                if (!block_live(m, n)) continue;     // nobody reads this block of the slab
                const int j = wc * 64 + n * 32 + (lane & 31);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int i = row_in_slab + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    double v = static_cast<double>(acc2[m][n][e]);
                    v += static_cast<double>(acc[m][n][e]);
                    if (slab_live) v += out[i * kSlab + j];
                    out[i * kSlab + j] = v;
                }
            }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(tickets + t_list, chunk + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the f16x2 tile kernel on v_mfma_f32_16x16x32_f16 (round 6) ------------------------------------------------------------
// Same workgroup tile (256 x 128), same wave tile (64 x 64), same plane images, same LDS-DMA ring and the same fp32 level-1 /
// fp64 slab hierarchy as gram_planes_kernel above -- but on fp16 planes, and the matrix instruction is the 16 x 16 x 32 one:
// per MAC it reads and writes HALF the accumulator registers and twice the operand registers of the 32 x 32 x 16 form
// (round 5's f16x2 kernel, 6.6 % slower at N = 4000: EXPERIMENTS.md G7), and at the socket's power cap (which is what bounds this kernel: EXPERIMENTS.md G6) that is worth 12-14 % of
// MFMA throughput on random fp16 data (scripts/ubench/mfma_shapes.hip: 1430 -> 1610 TF with the operands re-read from LDS every
// step, 1580 -> 1800 TF with them in registers; on all-zero data, where nothing is power-bound, the two shapes tie).
//
// A K = 32 step is a SUPER-STAGE: two consecutive 16-column stages of the ring.  The planes are stored as 1 KiB images of
// (32 rows x 16 columns) per plane: lane l' of an image holds row l' & 31, columns 8 (l' >> 5) .. + 7.  The A / B operand of
// the 16 x 16 x 32 MFMA wants lane l: row l & 15, k = 8 (l >> 4) .. + 7 of 32.  So lane l reads 16 bytes at
//       stage (l >> 5) of the pair,  image lane (l & 15) + 16 h + 32 ((l >> 4) & 1)        (h = which half of the 32-row block)
// -- lanes 0-31 from the first stage's buffer, lanes 32-63 from the second's, one ds_read_b128 -- and the sixteen lanes of
// every service group of ds_read_b128 land on sixteen different 16-byte slots: conflict-free, no change to the split kernels.
//
// Registers: accumulators 64 + level-1 sums 64 + fragments 96 (A of this super-stage 32, A of the next 32, the two halves of B
// 16 + 16).  The B side is walked in two halves of 32 columns: the first half's 24 MFMAs cover the reads of the second half's
// B fragments, the second half's 24 MFMAs cover the reads of the NEXT super-stage's A and first-half B fragments.  One
// workgroup barrier per super-stage (half as many as the 16-column form).
//
// DEFER (round 5): a chunk does not read-modify-write its tile's fp64 slabs (512 KB through the fabric per workgroup and
// chunk, behind a ticket, with the matrix pipe idle: 8 % of the kernel, EXPERIMENTS.md G3) but WRITES its level-1 sums as they
// are -- fp32, 128 KB, no read, no ticket -- into `chunk_sums`; chunk_reduce_kernel adds them into the slabs afterwards, in
// chunk order, in the same fp64 operations: the Gram is bitwise the same.  DEFER = false is the fallback where the sums do
// not fit beside the matrix.
template <int NBUF, bool DEFER>
__global__ __launch_bounds__(512, 1) void gram_planes16_kernel(const u32x4* __restrict__ planes, int64_t n_steps,
                                                            const double* __restrict__ unscale, int64_t rows_pad,
                                                            double* __restrict__ partial, int n_tiles,
                                                            const GramUnit* __restrict__ units, int n_chunks,
                                                            int* __restrict__ tickets, int round_size, int run,
                                                            int slab_live0, int n_sum_slots,
                                                            int32_t* __restrict__ device_status,
                                                            float* __restrict__ chunk_sums,
                                                            float* __restrict__ ragged_sums) {
    constexpr int PLANES = 2;
    constexpr int kRbBytes = PLANES * kFragBytes;           // one 32-row block, one stage: [plane][1 KiB]
    constexpr int kStage = kRowBlocks * kRbBytes;           // 24,576
    constexpr int NW = 8;
    constexpr int kPerWave = kRowBlocks * PLANES / NW;      // 3 DMA instructions per wave and stage
    constexpr int kSuperFlush = kFlushSteps / 2;            // super-stages per 256-column MFMA chain
    static_assert(kRowBlocks * PLANES % NW == 0 && NBUF == 6, "ring arithmetic below");
    typedef f16x8 frag_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];   // [NBUF][12 row blocks][2 planes][1 KiB]

    // workgroup -> (chunk, tile) unit: the units of the launch form ONE sequence, chunk-major, cut into runs of `run` units, and
    // every round of an XCD CLAIMS the next run from one counter as it gets there -- `run` CONSECUTIVE tiles of the list on (but
    // for one round in n_tiles / run) ONE chunk, so with the list in bands of four 256-row blocks a round touches 16 row blocks
    // of 128: the fewest 32 tiles of 256 x 128 can.  The XCDs of one chip do not run at one speed: an XCD whose rounds held the
    // cheaper diagonal tiles takes more runs, and the launch ends with every XCD busy (EXPERIMENTS.md G8).
    const int xcd = blockIdx.x & 7;
    const int seq = blockIdx.x >> 3;
    int* done = tickets + n_tiles + xcd;
    __shared__ int claimed_round;
    {
        // rounds: a workgroup starts only when every workgroup of the earlier rounds of its XCD has finished (gram.hip)
        const int round = round_size > 0 ? seq / round_size : 0;
        if (round > 0 && threadIdx.x == 0) {
            unsigned spins = 0;
            while (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < round * round_size) {
                __builtin_amdgcn_s_sleep(16);
                if (++spins > (1u << 20)) break;   // only speed depends on the gate
            }
        }
        if (threadIdx.x == 0) {
            // the first workgroup of this XCD's round `seq / run` to get here claims the next run of units for all of them
            int* slot = tickets + n_tiles + 9 + xcd * static_cast<int>(gridDim.x / (8u * static_cast<unsigned>(run))) + seq / run;
            int v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v == 0) {
                int expected = 0;
                if (__hip_atomic_compare_exchange_strong(slot, &expected, -1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    v = __hip_atomic_fetch_add(tickets + n_tiles + 8, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
                    __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    v = expected;
                }
            }
            while (v <= 0) {   // (the claimer is between its exchange and its store: a fetch-add away)
                __builtin_amdgcn_s_sleep(1);
                v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            claimed_round = v - 1;
        }
        __syncthreads();
    }
    // (integer division runs on the vector ALU: readfirstlane keeps the unit's numbers in scalar registers -- left in vector
    // registers they live through the K loop and push it from 251 / 254 VGPRs to 256 and a spill)
    const int unit = __builtin_amdgcn_readfirstlane(claimed_round * run + seq % run);
    const int chunk = __builtin_amdgcn_readfirstlane(unit / n_tiles);
    if (chunk >= n_chunks) {   // a spare round: every unit was claimed before it got here
        if (threadIdx.x == 0) __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int t_list = unit - chunk * n_tiles;
    const GramUnit* __restrict__ my_unit = units + t_list;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // this wave's entry of the unit table (build_gram_units): where its operands sit in a stage of LDS, which 32 x 32 blocks of
    // its 64 x 64 sub-tile are live (bit m32 * 2 + n32) and where the sub-tile goes
    const unsigned where = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(my_unit->wave[wave].where));
    const int a_slot = static_cast<int>(where & 0xffu);           // LDS slot of its first A row block (two, consecutive)
    const int b_slot = static_cast<int>((where >> 8) & 0xffu);    // ... of its first B row block (two, consecutive)
    unsigned live_blocks = (where >> 16) & 0xffu;
    const int row_in_slab = static_cast<int>((where >> 24) & 1u) * 64;   // where the sub-tile starts inside its slab
    const int col_in_slab = static_cast<int>((where >> 25) & 1u) * 64;
    const int sum_slot = __builtin_amdgcn_readfirstlane(my_unit->wave[wave].sum_slot);
    const bool live_wave = live_blocks != 0;

    const int step0 = chunk * kChunkSteps;
    int n_stages = static_cast<int>(n_steps) - step0;       // even: n_steps counts whole 32-column pairs, chunks are even
    if (n_stages > kChunkSteps) n_stages = kChunkSteps;
    const int n_super = n_stages / 2;

    // LDS-DMA: piece q = wave + 8 i of a stage (row block q / 2, plane q % 2)
    int64_t piece_off[kPerWave];
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
        const int q = wave + NW * i;
        const int rbl = q / PLANES, piece = q % PLANES;
        const int64_t rb = __builtin_amdgcn_readfirstlane(my_unit->rb[rbl]);   // the global 32-row block of LDS slot rbl
        piece_off[i] = (((rb * n_steps + step0) * PLANES + piece) * 64) * 16;
    }
    const unsigned char* lane_base = reinterpret_cast<const unsigned char*>(planes) + lane * 16;
    auto dma_piece = [&](int s, int i) __attribute__((always_inline)) {   // (i: a compile-time piece number after unrolling)
        unsigned char* dst = lds + (s % NBUF) * kStage + wave * kFragBytes;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(lane_base + piece_off[i] + static_cast<int64_t>(s) * (PLANES * kFragBytes)),
            (__attribute__((address_space(3))) void*)(dst + i * NW * kFragBytes), 16, 0, 0);
    };
    auto dma = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPerWave; ++i) dma_piece(s, i);
    };

    f32x4 acc[4][4], acc2[4][4];     // [16-row block][16-column block]
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[m][n][e] = 0.0f;
                acc2[m][n][e] = 0.0f;
            }

    // this lane's byte offset inside a 32-row block's stage image pair: which stage of the pair, which image lane
    const int lane_in_image = (lane & 15) + 32 * ((lane >> 4) & 1);
    const int pair_half = lane >> 5;                         // 0: the first stage of the super-stage, 1: the second
    // fragment (row block rb32 of the stage image, half h of it, plane p) of super-stage sp
    auto frag_at = [&](int sp, int rb32, int h, int p) __attribute__((always_inline)) -> frag_t {
        // (NBUF = 6 is even: the two stages of a super-stage sit in buffers 2 (sp % 3) and 2 (sp % 3) + 1)
        const unsigned char* at = lds + (2 * (sp % (NBUF / 2)) + pair_half) * kStage + rb32 * kRbBytes + p * kFragBytes +
                                  (lane_in_image + 16 * h) * 16;
        return *reinterpret_cast<const frag_t*>(at);
    };
    struct AFrags { frag_t v[2][4]; };     // [plane h, m][16-row block of the wave's 64 rows]
    struct BFrags { frag_t v[2][2]; };     // [plane][16-column block of one 32-column half]
    auto read_a = [&](int sp, AFrags& a, auto mask_c) __attribute__((always_inline)) {
        constexpr unsigned MASK = decltype(mask_c)::value;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (((MASK >> ((m / 2) * 2)) & 3u) != 0) a.v[p][m] = frag_at(sp, a_slot + m / 2, m % 2, p);
    };
    auto read_b = [&](int sp, int half, BFrags& b, auto mask_c) __attribute__((always_inline)) {
        constexpr unsigned MASK = decltype(mask_c)::value;
        // (the caller passes a compile-time `half`)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int n = 0; n < 2; ++n) b.v[p][n] = frag_at(sp, b_slot + half, n, p);
        (void)MASK;
    };
    // the 24 MFMAs of one 32-column half: m h' + h m' + h h' per 16 x 16 block, term-major as written; this generic and masked
    // path (ragged and diagonal waves) leaves their order to the compiler
    auto multiply_half = [&](const AFrags& a, const BFrags& b, auto half_c, auto mask_c) __attribute__((always_inline)) {
        constexpr unsigned MASK = decltype(mask_c)::value;
        constexpr int HALF = decltype(half_c)::value;
        constexpr int pa[3] = {1, 0, 0};
        constexpr int pb[3] = {0, 1, 0};
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n)
                    if (((MASK >> ((m / 2) * 2 + HALF)) & 1u) != 0)
                        acc[m][2 * HALF + n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v[pa[t]][m], b.v[pb[t]][n], acc[m][2 * HALF + n], 0, 0, 0);
    };
    auto flush = [&](int sp) __attribute__((always_inline)) {
        if ((sp + 1) % kSuperFlush == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc2[m][n][e] += acc[m][n][e];
                        acc[m][n][e] = 0.0f;
                    }
        }
    };

    // ---- the ring: six stages = three super-stages; the DMA runs two super-stages ahead of the one being multiplied
    for (int a = 0; a < NBUF && a < n_stages; ++a) dma(a);
    {
        const int issued = n_stages < NBUF ? n_stages : NBUF;
        wait_vmcnt_dyn((issued > 2 ? issued - 2 : 0) * kPerWave);   // stages 0 and 1 have landed
    }
    asm volatile("s_barrier" ::: "memory");
    auto k_loop = [&](auto mask_c) __attribute__((always_inline)) {
        constexpr unsigned MASK = decltype(mask_c)::value;
        constexpr bool kLive = MASK != 0;
        constexpr std::integral_constant<int, 0> h0{};
        constexpr std::integral_constant<int, 1> h1{};
        AFrags a0, a1;
        BFrags b0, b1;
        if (kLive && n_super > 0) {
            read_a(0, a0, mask_c);
            if ((MASK & 5u) != 0) read_b(0, 0, b0, mask_c);
        }
        // one super-stage: cur A in `a`, next A goes to `an`
        auto super = [&](int sp, AFrags& a, AFrags& an) __attribute__((always_inline)) {
            if (kLive) {
                if ((MASK & 10u) != 0) read_b(sp, 1, b1, mask_c);            // the second half's B: under the first half's MFMAs
                if ((MASK & 5u) != 0) multiply_half(a, b0, h0, mask_c);
            }
            // stages 2 sp + 2, 2 sp + 3 must have landed before anybody reads them; of my requests only the stages behind them
            // may still be outstanding (returns are in issue order)
            {
                const int last = 2 * sp + 5 < n_stages - 1 ? 2 * sp + 5 : n_stages - 1;   // the last stage requested so far
                const int ahead = last - (2 * sp + 3);
                if (2 * sp + 7 < n_stages) wait_vmcnt<2 * kPerWave>();                   // steady state: two stages may be in flight
                else wait_vmcnt_dyn((ahead > 0 ? ahead : 0) * kPerWave);
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // everybody has read super-stage sp; sp + 1 has landed
            if (2 * sp + NBUF < n_stages) dma(2 * sp + NBUF);
            if (2 * sp + NBUF + 1 < n_stages) dma(2 * sp + NBUF + 1);
            if (kLive) {
                if (sp + 1 < n_super) {
                    read_a(sp + 1, an, mask_c);                               // under the second half's MFMAs
                    if ((MASK & 5u) != 0) read_b(sp + 1, 0, b0, mask_c);
                }
                if ((MASK & 10u) != 0) multiply_half(a, b1, h1, mask_c);
                flush(sp);
            }
        };
        // The steady state of a FULL wave (all sixteen blocks live, both stages of super-stage sp + 3 still to be requested) with its
        // instructions in a PINNED order.  Left to itself hipcc issues the six DMA pieces and the twelve reads first -- both
        // waves of every SIMD at once, right behind the barrier, with the matrix pipe idle -- and the 24 MFMAs behind them
        // (45.6 -> 42.3 ms per launch at N = 4000, bitwise: EXPERIMENTS.md G7; four pinned orders of the memory instructions
        // tied at 41.3 .. 41.8 ms, profiles/r06o_gram_pin_orders_ab.txt: what pays is that they are spread AT ALL).
        // The MFMAs of a half are issued BLOCK-MAJOR and CHAINED: the three products m h', h m', h h' of one 16 x 16 block back to
        // back into its accumulator (SrcC = the vDst just written; the second and third share A = h), the eight blocks in a
        // serpentine walk m0n0 m0n1 m1n1 m1n0 m2n0 ... so that a change of row keeps B.  Every accumulator receives the same
        // products in the same order as in a term-major walk -- the Gram's bits do not move -- but the accumulator and operand
        // registers toggle less, and at the socket's power cap energy is time: +4.7 % MFMA throughput on random data in
        // scripts/ubench/mfma_orders.hip, a tie on zeros (EXPERIMENTS.md G10).  A sched_barrier behind every MFMA keeps the
        // order; the memory instructions sit BETWEEN blocks, never inside a chain:
        //   * first half: one read of the second half's B in front of every other block;
        //   * second half, behind the barrier: {one DMA piece, two fragment reads of super-stage sp + 1} in front of each of the
        //     first six blocks.  They write `an`, b0 and LDS, none of which this half's MFMAs read.
        // The steady state runs in TRIPS OF EIGHT super-stages = one 256-column MFMA chain, every position of the chain its own
        // straight-line code:
        //   * position 0 starts every block's chain from C = 0 (an inline constant of the block's first product), so the flush at
        //     position 7 does not have to zero the accumulators: 64 of its 128 vector instructions gone;
        //   * position 7 adds the first half's eight blocks to the level-1 sums one per block of the second half (their last
        //     MFMAs were issued before the barrier) and only the second half's eight behind them.  (Adding a block of the second
        //     half two blocks after its third product as well takes the kernel to 256 registers and the in-kernel form to a spill.)
        auto super8 = [&](int sp, AFrags& a, AFrags& an, auto pos_c) __attribute__((always_inline)) {
            constexpr int POS = decltype(pos_c)::value;
            constexpr bool FRESH = POS == 0, FLUSHING = POS == 7;
            constexpr int pa[3] = {1, 0, 0};
            constexpr int pb[3] = {0, 1, 0};
            const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
            // block k = 0 .. 7 of a half in the serpentine walk: row k / 2, column walk_n(k)
            auto walk_n = [](int k) __attribute__((always_inline)) { return ((k / 2) & 1) ? 1 - k % 2 : k % 2; };
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int m = k / 2, n = walk_n(k);
                if (k % 2 == 0) b1.v[k / 4][m % 2] = frag_at(sp, b_slot + 1, m % 2, k / 4);
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v[pa[t]][m], b0.v[pb[t]][n], (FRESH && t == 0) ? zero4 : acc[m][n], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            wait_vmcnt<2 * kPerWave>();
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int m = k / 2, n = walk_n(k);
                if (k < 6) {
                    dma_piece(2 * sp + NBUF + k / 3, k % 3);
#pragma unroll
                    for (int r = 2 * k; r < 2 * k + 2; ++r) {
                        if (r < 8) an.v[r / 4][r % 4] = frag_at(sp + 1, a_slot + (r % 4) / 2, (r % 4) % 2, r / 4);
                        else b0.v[(r - 8) / 2][(r - 8) % 2] = frag_at(sp + 1, b_slot, (r - 8) % 2, (r - 8) / 2);
                    }
                }
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    acc[m][2 + n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v[pa[t]][m], b1.v[pb[t]][n], (FRESH && t == 0) ? zero4 : acc[m][2 + n], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (FLUSHING) {
                    // block k of the first half: all of its products were issued in front of the barrier
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc2[m][k % 2][e] += acc[m][k % 2][e];
                }
            }
            if constexpr (FLUSHING) {
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 2; n < 4; ++n)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc2[m][n][e] += acc[m][n][e];
            }
        };
        int sp = 0;
        if constexpr (MASK == 15u) {
            bool any = false;
            for (; 2 * (sp + 7) + NBUF + 1 < n_stages && sp + 8 < n_super; sp += 8) {
                super8(sp + 0, a0, a1, std::integral_constant<int, 0>{});
                super8(sp + 1, a1, a0, std::integral_constant<int, 1>{});
                super8(sp + 2, a0, a1, std::integral_constant<int, 2>{});
                super8(sp + 3, a1, a0, std::integral_constant<int, 3>{});
                super8(sp + 4, a0, a1, std::integral_constant<int, 4>{});
                super8(sp + 5, a1, a0, std::integral_constant<int, 5>{});
                super8(sp + 6, a0, a1, std::integral_constant<int, 6>{});
                super8(sp + 7, a1, a0, std::integral_constant<int, 7>{});
                any = true;
            }
            if (any) {     // the trips leave the accumulators as the last chain left them: what follows starts from zero
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[m][n][e] = 0.0f;
            }
        }
        for (; sp + 1 < n_super; sp += 2) {
            super(sp, a0, a1);
            super(sp + 1, a1, a0);
        }
        if (sp < n_super) super(sp, a0, a1);
    };
    switch (live_blocks) {
        case 0u: k_loop(std::integral_constant<unsigned, 0u>{}); break;
        case 1u: k_loop(std::integral_constant<unsigned, 1u>{}); break;
        case 3u: k_loop(std::integral_constant<unsigned, 3u>{}); break;
        case 13u: k_loop(std::integral_constant<unsigned, 13u>{}); break;
        default: live_blocks = 15u; k_loop(std::integral_constant<unsigned, 15u>{}); break;
    }
    auto block_live = [&](int m, int n) __attribute__((always_inline)) { return ((live_blocks >> ((m / 2) * 2 + n / 2)) & 1u) != 0; };

    if constexpr (DEFER) {
        // this chunk's level-1 sums, as they are: slot `sum_slot` of the chunk (the table says which slab that is); element
        // (i, j) where the fp64 slab has it.  A chunk whose last MFMA chain has not been flushed (n_super not a multiple of kSuperFlush: only the ragged last
        // chunk of the matrix) leaves that chain's sums in `ragged_sums`, for chunk_reduce_kernel to add as the in-kernel
        // update does: (double) level-1 + (double) chain.
        if (live_wave) {
            const bool unflushed = (n_super % kSuperFlush) != 0;
            float* out = chunk_sums + (static_cast<int64_t>(chunk) * n_sum_slots + sum_slot) * (kSlab * kSlab);
            float* rag = ragged_sums + static_cast<int64_t>(sum_slot) * (kSlab * kSlab);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    if (!block_live(m, n)) continue;
                    const int j = col_in_slab + 16 * n + (lane & 15);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = row_in_slab + 16 * m + 4 * (lane >> 4) + e;
                        out[i * kSlab + j] = acc2[m][n][e];
                        if (unflushed) rag[i * kSlab + j] = acc[m][n][e];
                    }
                }
        }
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    // epilogue of the in-kernel form: chunks of a tile add into its slabs in chunk order (gram.hip's ticket protocol)
    bool lost = false;
    if (chunk > 0) {
        if (tid == 0) {
            unsigned spins = 0;
            while (__hip_atomic_load(tickets + t_list, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != chunk) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > (1u << 26)) {
                    lost = true;
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        lost = __syncthreads_or(lost ? 1 : 0) != 0;
    }
    if (lost) {
        if (tid == 0) atomicOr(device_status, kStatusLostTicket);
    } else if (live_wave) {
        const bool slab_live = chunk > 0 || slab_live0 != 0;
        const int slab = __builtin_amdgcn_readfirstlane(my_unit->wave[wave].slab);
        const int ti = slab & 0xffff, tj = slab >> 16;
        double* out = partial + (static_cast<int64_t>(ti) * (ti + 1) / 2 + tj) * (kSlab * kSlab);
        const double* un = unscale + static_cast<int64_t>(chunk) * rows_pad;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                if (!block_live(m, n)) continue;
                const int j = col_in_slab + 16 * n + (lane & 15);
                const double uj = un[static_cast<int64_t>(tj) * kSlab + j];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = row_in_slab + 16 * m + 4 * (lane >> 4) + e;
                    double v = static_cast<double>(acc2[m][n][e]);
                    v += static_cast<double>(acc[m][n][e]);
                    v *= un[static_cast<int64_t>(ti) * kSlab + i] * uj;   // powers of two: exact
                    if (slab_live) v += out[i * kSlab + j];
                    out[i * kSlab + j] = v;
                }
            }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(tickets + t_list, chunk + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The deferred slab update: slab entry (i, j) of every tile of the launch += its chunks' sums in chunk order -- per chunk
// v = (double)level-1 sum (+ (double)unflushed chain), v *= 2^-shift_i 2^-shift_j, slab = v + slab: the fp64 operations of
// the in-kernel update, in its order.  One workgroup per (tile, slab, quarter of its rows); a thread owns four consecutive
// columns of a row and keeps kReduceRun chunks' loads in flight (the additions then run in chunk order: a first version with
// one dependent load per addition ran at 0.7 TB/s, 6 ms per launch).  Entries of blocks nobody computed are left alone.
constexpr int kReduceRun = 8;
__global__ __launch_bounds__(256) void chunk_reduce_kernel(const float* __restrict__ chunk_sums, const float* __restrict__ ragged_sums,
                                                           int n_sum_slots, int n_chunks, int ragged_chunk,
                                                           const int2* __restrict__ slot_slab, const double* __restrict__ unscale,
                                                           int64_t rows_pad, double* __restrict__ partial, int slab_live0,
                                                           int n_blocks32) {
    typedef double f64x4 __attribute__((ext_vector_type(4)));
    const int slot = blockIdx.x;
    const int2 tt = slot_slab[slot];
    const int ti = tt.x, tj = tt.y;
    if (ti < 0) return;     // (a slot of the (bi, tj) list whose slab lies above the diagonal or past the matrix)
    double* out = partial + (static_cast<int64_t>(ti) * (ti + 1) / 2 + tj) * (kSlab * kSlab);
    const int64_t slab_stride = static_cast<int64_t>(n_sum_slots) * (kSlab * kSlab);
    const float* in = chunk_sums + static_cast<int64_t>(slot) * (kSlab * kSlab);
    const float* rag = ragged_sums + static_cast<int64_t>(slot) * (kSlab * kSlab);
    // blockIdx.y: a quarter of the slab's rows; a thread: row i, columns j .. j + 3 (all in one 32 x 32 block)
    const int i = static_cast<int>(blockIdx.y) * 32 + (threadIdx.x >> 3), j = (threadIdx.x & 7) * 4;
    for (int jb = 0; jb < kSlab; jb += 32) {
        const int jj = jb + j;
        if (n_blocks32 >= 0) {       // the tile kernel's rule: block (i / 32, jj / 32) was computed iff ...
            const int rblk = ti * 4 + (i >> 5), cblk = tj * 4 + (jj >> 5);
            if (!(rblk < n_blocks32 && cblk <= rblk)) continue;
        }
        const int idx = i * kSlab + jj;
        f64x4 v = {0.0, 0.0, 0.0, 0.0};
        bool live = slab_live0 != 0;
        if (live) v = *reinterpret_cast<const f64x4*>(out + idx);
        for (int c0 = 0; c0 < n_chunks; c0 += kReduceRun) {
            f32x4 p[kReduceRun];
            double ui[kReduceRun];
            f64x4 uj[kReduceRun];
#pragma unroll
            for (int k = 0; k < kReduceRun; ++k) {
                const int c = c0 + k < n_chunks ? c0 + k : n_chunks - 1;
                p[k] = *reinterpret_cast<const f32x4*>(in + c * slab_stride + idx);
                const double* un = unscale + static_cast<int64_t>(c) * rows_pad;
                ui[k] = un[static_cast<int64_t>(ti) * kSlab + i];
                uj[k] = *reinterpret_cast<const f64x4*>(un + static_cast<int64_t>(tj) * kSlab + jj);
            }
#pragma unroll
            for (int k = 0; k < kReduceRun; ++k) {
                if (c0 + k >= n_chunks) break;
                f64x4 q = {static_cast<double>(p[k][0]), static_cast<double>(p[k][1]), static_cast<double>(p[k][2]),
                           static_cast<double>(p[k][3])};
                if (c0 + k == ragged_chunk) {
                    const f32x4 r = *reinterpret_cast<const f32x4*>(rag + idx);
                    q[0] += static_cast<double>(r[0]); q[1] += static_cast<double>(r[1]);
                    q[2] += static_cast<double>(r[2]); q[3] += static_cast<double>(r[3]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    q[e] *= ui[k] * uj[k][e];
                    v[e] = live ? q[e] + v[e] : q[e];
                }
                live = true;
            }
        }
        *reinterpret_cast<f64x4*>(out + idx) = v;
    }
}

}  // namespace

bool gram_planes_enabled() { return env_int("BYZ_GRAM_PLANES", 1) != 0; }

// The units of the f16x2 tile kernel.  A 256-row block bi is a 4 x 4 grid of 64 x 64 sub-tiles (r, c) on the diagonal, ten of
// them on or below it; a workgroup is eight waves (wr = wave / 2, wc = wave % 2) of one sub-tile each.
//   plain  (bi, tj):  LDS slots 0..7 = the block's eight 32-row blocks, 8..11 = slab tj's four; wave (wr, wc) reads A from
//                     slots 2 wr, 2 wr + 1 and B from 8 + 2 wc, 9 + 2 wc: sub-tile (wr % 2, wc) of slab (2 bi + wr / 2, tj).
//   D1     (bi, 2 bi): the plain unit, whose wave (0, 1) -- strictly above the diagonal -- takes sub-tile (2, 2) instead: A AND B
//                     from slots 4, 5 (A and B operands are one image layout), the top left of slab (2 bi + 1, 2 bi + 1).
//   D2     (three consecutive bi):  slots 4 k .. 4 k + 3 = row blocks 4..7 of the k-th block; per block one full wave on
//                     sub-tile (3, 2) (A slots 4 k + 2, B slots 4 k) and one mask-13 wave on (3, 3) (A and B slots 4 k + 2).
//                     The full waves are waves 0, 1, 2: three SIMDs; the mask-13 ones 3, 7, 5.
// D1 and D2 replace the plain units (bi, 2 bi) and (bi, 2 bi + 1), of which the second had five idle waves, three of them
// beside a full one.  A D2 stands in the list where the (bi, 2 bi + 1) of its last block stood.  A last block with one slab
// only (odd t128) has no (3, *) sub-tiles and joins no D2.
void build_gram_units(int64_t t128, int64_t n_blocks32, bool diagonal_units, int share_count, int share_index,
                      std::vector<GramUnit>& units, std::vector<int32_t>& slot_slab) {
    units.clear();
    slot_slab.clear();
    const int64_t t256 = ceil_div(t128, 2);
    // live 32 x 32 blocks (bit m32 * 2 + n32) of the sub-tile at (64 row64, 64 col64) of slab (ti, tj)
    auto live_mask = [&](int64_t ti, int64_t tj, int row64, int col64) -> uint32_t {
        if (!(tj <= ti && ti < t128)) return 0u;
        if (n_blocks32 < 0) return 15u;      // the slab-granular rule
        uint32_t mask = 0;
        for (int m = 0; m < 2; ++m)
            for (int n = 0; n < 2; ++n) {
                const int64_t rblk = ti * 4 + row64 * 2 + m, cblk = tj * 4 + col64 * 2 + n;
                if (rblk < n_blocks32 && cblk <= rblk) mask |= 1u << (m * 2 + n);
            }
        return mask;
    };
    auto set_wave = [&](GramUnit& u, int wave, int a_slot, int b_slot, int64_t ti, int64_t tj, int row64, int col64,
                        int64_t sum_slot) {
        const uint32_t mask = live_mask(ti, tj, row64, col64);
        GramUnitWave& w = u.wave[wave];
        w.where = static_cast<uint32_t>(a_slot) | static_cast<uint32_t>(b_slot) << 8 | mask << 16 |
                  static_cast<uint32_t>(row64) << 24 | static_cast<uint32_t>(col64) << 25;
        w.sum_slot = mask != 0 ? static_cast<int32_t>(sum_slot) : 0;
        w.slab = mask != 0 ? static_cast<int32_t>(ti | tj << 16) : 0;
    };
    auto slab_slot = [](int64_t ti, int64_t tj) { return ti * (ti + 1) / 2 + tj; };
    int64_t position = 0;
    auto plain = [&](int64_t bi, int64_t tj, bool d1) {
        if (position++ % share_count != share_index) return;
        const int64_t t_list = static_cast<int64_t>(units.size());
        GramUnit u{};
        for (int s = 0; s < 12; ++s) u.rb[s] = static_cast<int32_t>(s < 8 ? bi * 8 + s : tj * 4 + (s - 8));
        for (int wave = 0; wave < 8; ++wave) {
            const int wr = wave / 2, wc = wave % 2;
            const int64_t ti = 2 * bi + wr / 2;
            set_wave(u, wave, 2 * wr, 8 + 2 * wc, ti, tj, wr % 2, wc, diagonal_units ? slab_slot(ti, tj) : 2 * t_list + wr / 2);
        }
        if (d1) set_wave(u, 1, 4, 4, 2 * bi + 1, 2 * bi + 1, 0, 0, slab_slot(2 * bi + 1, 2 * bi + 1));
        units.push_back(u);
        if (!diagonal_units)
            for (int sel = 0; sel < 2; ++sel) {
                const int64_t ti = 2 * bi + sel;
                const bool live = tj <= ti && ti < t128;
                slot_slab.push_back(static_cast<int32_t>(live ? ti : -1));
                slot_slab.push_back(static_cast<int32_t>(live ? tj : -1));
            }
    };
    auto d2 = [&](int64_t first, int64_t count) {
        static const int partial_wave[3] = {3, 7, 5};
        GramUnit u{};
        for (int s = 0; s < 12; ++s) u.rb[s] = static_cast<int32_t>(first * 8 + 4);   // (a slot nobody reads still gets its DMA)
        for (int64_t k = 0; k < count; ++k) {
            const int64_t bi = first + k, t = 2 * bi + 1;
            for (int s = 0; s < 4; ++s) u.rb[4 * k + s] = static_cast<int32_t>(bi * 8 + 4 + s);
            set_wave(u, static_cast<int>(k), static_cast<int>(4 * k + 2), static_cast<int>(4 * k), t, t, 1, 0, slab_slot(t, t));
            set_wave(u, partial_wave[k], static_cast<int>(4 * k + 2), static_cast<int>(4 * k + 2), t, t, 1, 1, slab_slot(t, t));
        }
        units.push_back(u);
    };
    const int64_t full_blocks = t128 / 2;     // 256-row blocks with both slabs
    for (int64_t b0 = 0; b0 < t256; b0 += 4)
        for (int64_t tj = 0; tj < t128 && tj <= 2 * (b0 + 3) + 1; ++tj)
            for (int64_t bi = b0; bi < b0 + 4 && bi < t256; ++bi) {
                if (tj > 2 * bi + 1) continue;
                if (!diagonal_units) {
                    plain(bi, tj, false);
                } else if (tj == 2 * bi + 1) {
                    if (bi % 3 == 2 || bi == full_blocks - 1) d2(bi - bi % 3, bi % 3 + 1);
                } else {
                    plain(bi, tj, tj == 2 * bi);
                }
            }
    if (diagonal_units)
        for (int64_t ti = 0; ti < t128; ++ti)
            for (int64_t tj = 0; tj <= ti; ++tj) {
                slot_slab.push_back(static_cast<int32_t>(ti));
                slot_slab.push_back(static_cast<int32_t>(tj));
            }
}

// Fills `slabs` (gram.hip's fp64 slab format: one 128 x 128 slab per lower-triangle tile ti (ti + 1) / 2 + tj) with the
// Gram of the n_rows logical rows G[row_index[r]]; with share_count > 1 only this share's tiles (owned[] says which).
// f16 = true: the f16x2 arithmetic, false: bf16x3 (bitwise gram.hip's split mode).
int launch_gram_planes(byz_ctx* ctx, const float* G, int64_t n_rows, int64_t n_cols, int64_t ld, const int32_t* row_index,
                       double* slabs, int share_count, int share_index, uint8_t* owned_host, bool f16, hipStream_t stream) {
    const int64_t t128 = ceil_div(n_rows, kSlab);
    const int64_t t256 = ceil_div(t128, 2);
    const int64_t rows_pad = t256 * kWgRows;
    // The tile list.  f16x2: bands of four 256-row blocks, inside a band column block by column block -- ANY 32 consecutive
    // tiles are (4 or 5) x (8 or 9) tiles on at most ~17 row blocks of 128, and the kernel hands out runs of consecutive
    // (chunk, tile) units to the XCDs.  bf16x3: 8 x 8 super-blocks of slabs = 4 x 8 workgroup tiles, a contiguous share of the
    // list per XCD (the rounds of an XCD then straddle two chunks and two or three super-blocks: 106 GB through the fabric per
    // 1M-column launch at N = 4000 if every line were shared perfectly inside a round, against 70 GB for the bands;
    // scripts/gram_order_footprint.py, EXPERIMENTS.md G8).  The key tells the lists apart: one engine may alternate.
    // BYZ_GRAM_DEFER=0: round 4's in-kernel slab update (the bitwise comparison of the tests)
    bool defer = f16 && env_int("BYZ_GRAM_DEFER", 1) != 0;
    const int n_blocks32 = env_int("BYZ_GRAM_BLOCK_SKIP", 1) != 0 ? static_cast<int>(ceil_div(n_rows, 32)) : -1;
    // f16x2 keeps the list as a table of units (build_gram_units).  The diagonal units need the deferred update (the ticket of
    // the in-kernel update orders the chunks of a (bi, tj) tile), the whole triangle (a share owns (bi, tj) tiles) and the
    // block-granular rule (under the slab-granular one no wave of a diagonal tile is idle).
    auto ensure_list = [&](bool diagonal_units) -> int {
        const int64_t order_key = static_cast<int64_t>((f16 ? 1 : 0) + (diagonal_units ? 2 : 0)) * (1ll << 40) + share_count * 65536 + share_index;
        const int64_t blocks_key = f16 ? n_blocks32 : -2;
        if (ctx->plane_order_T != t128 || ctx->plane_order_share != order_key || ctx->plane_order_blocks != blocks_key) {
            ctx->plane_order_host.clear();
            if (f16) {
                if (t128 > 0x7fff) {
                    set_error("gram: more than 32767 slabs per side");
                    return BYZ_E_UNSUPPORTED;
                }
                std::vector<GramUnit> units;
                std::vector<int32_t> slot_slab;
                build_gram_units(t128, n_blocks32, diagonal_units, share_count, share_index, units, slot_slab);
                ctx->plane_units = static_cast<int64_t>(units.size());
                ctx->plane_sum_slots = static_cast<int64_t>(slot_slab.size() / 2);
                ctx->plane_order_host.resize(units.size() * kGramUnitWords);
                if (!units.empty()) std::memcpy(ctx->plane_order_host.data(), units.data(), units.size() * sizeof(GramUnit));
                ctx->plane_order_host.insert(ctx->plane_order_host.end(), slot_slab.begin(), slot_slab.end());
            } else {
                int64_t position = 0;
                auto push = [&](int64_t bi, int64_t tj) {
                    if (position++ % share_count != share_index) return;
                    ctx->plane_order_host.push_back(static_cast<int32_t>(bi));
                    ctx->plane_order_host.push_back(static_cast<int32_t>(tj));
                };
                const int64_t S = ceil_div(t128, 8);
                for (int64_t I = 0; I < S; ++I)
                    for (int64_t J = 0; J <= I; ++J)
                        for (int64_t bi = I * 4; bi < I * 4 + 4 && bi < t256; ++bi)
                            for (int64_t tj = J * 8; tj < J * 8 + 8 && tj <= 2 * bi + 1 && tj < t128; ++tj) push(bi, tj);
                ctx->plane_units = static_cast<int64_t>(ctx->plane_order_host.size() / 2);
                ctx->plane_sum_slots = 0;
            }
            BYZ_TRY(ctx->plane_order.ensure(ctx->plane_order_host.size() * sizeof(int32_t) + 16));
            BYZ_HIP(hipMemcpyAsync(ctx->plane_order.ptr, ctx->plane_order_host.data(),
                                   ctx->plane_order_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
            BYZ_HIP(hipStreamSynchronize(stream));
            ctx->plane_order_T = t128;
            ctx->plane_order_share = order_key;
            ctx->plane_order_blocks = blocks_key;
        }
        return BYZ_OK;
    };
    const bool diagonal_units = defer && share_count == 1 && n_blocks32 >= 0;
    BYZ_TRY(ensure_list(diagonal_units));
    int64_t n_tiles = ctx->plane_units;
    int64_t n_sum_slots = ctx->plane_sum_slots;
    const int32_t* slot_slab_host = ctx->plane_order_host.data() + n_tiles * kGramUnitWords;   // (f16x2)
    if (owned_host != nullptr) {
        if (f16) {
            for (int64_t s = 0; s < n_sum_slots; ++s) {
                const int64_t ti = slot_slab_host[2 * s], tj = slot_slab_host[2 * s + 1];
                if (ti >= 0) owned_host[ti * (ti + 1) / 2 + tj] = 1;
            }
        } else {
            for (int64_t t = 0; t < n_tiles; ++t) {
                const int64_t bi = ctx->plane_order_host[2 * t], tj = ctx->plane_order_host[2 * t + 1];
                for (int64_t ti = 2 * bi; ti < 2 * bi + 2 && ti < t128; ++ti)
                    if (tj <= ti) owned_host[ti * (ti + 1) / 2 + tj] = 1;
            }
        }
    }
    if (n_tiles == 0) return BYZ_OK;

    // super-chunk: as many 8192-column chunks as the plane budget holds
    const int n_planes = f16 ? 2 : 3;
    size_t free_b = 0, total_b = 0;
    BYZ_HIP(hipMemGetInfo(&free_b, &total_b));
    int64_t budget = static_cast<int64_t>(env_int("BYZ_GRAM_PLANE_MB", 16384)) << 20;
    const int64_t have = static_cast<int64_t>(ctx->gram_planes.bytes);
    if (budget > have + static_cast<int64_t>(free_b / 2)) budget = have + static_cast<int64_t>(free_b / 2);
    int64_t chunks_per_sc = budget / (rows_pad * 2 * n_planes * kChunkCols);
    const int64_t chunks_total = ceil_div(n_cols, kChunkCols);
    if (chunks_per_sc > chunks_total) chunks_per_sc = chunks_total;
    if (chunks_per_sc < 1) {
        set_error("gram: no room for one 8192-column chunk of 16-bit planes (%lld rows)", (long long)rows_pad);
        return BYZ_E_HIP;
    }
    // even super-chunks: the same number of launches, the last one not a stub
    const int64_t n_sc = ceil_div(chunks_total, chunks_per_sc);
    chunks_per_sc = ceil_div(chunks_total, n_sc);
    const int64_t sc_cols = chunks_per_sc * kChunkCols;
    BYZ_TRY(ctx->gram_planes.ensure(static_cast<size_t>(rows_pad) * 2 * n_planes * sc_cols));
    double* unscale = nullptr;
    if (f16) {
        BYZ_TRY(ctx->plane_unscale.ensure(static_cast<size_t>(rows_pad) * chunks_per_sc * sizeof(double)));
        unscale = ctx->plane_unscale.as<double>();
    }
    u32x4* planes = ctx->gram_planes.as<u32x4>();
    float* chunk_sums = nullptr;
    float* ragged_sums = nullptr;
    if (defer) {
        // fp32 level-1 sums of every (chunk, sum slot) of a launch + one more slab per slot for an unflushed chain
        // (4.3 GB at configs[3], 10 GB at configs[4]'s slice).  Where that does not fit beside the matrix the update stays
        // inside the tile kernel: slower, the same bits.
        const size_t per_chunk = static_cast<size_t>(n_sum_slots) * kSlab * kSlab * sizeof(float);
        const size_t want = per_chunk * static_cast<size_t>(chunks_per_sc + 1);
        size_t free_now = 0, total_now = 0;
        BYZ_HIP(hipMemGetInfo(&free_now, &total_now));
        if (want > ctx->gram_chunk_sums.bytes && want - ctx->gram_chunk_sums.bytes > free_now / 2) defer = false;
        if (!defer && diagonal_units) {   // the in-kernel update runs on the (bi, tj) list
            BYZ_TRY(ensure_list(false));
            n_tiles = ctx->plane_units;
            n_sum_slots = ctx->plane_sum_slots;
        }
    }
    if (defer) {
        const size_t per_chunk = static_cast<size_t>(n_sum_slots) * kSlab * kSlab * sizeof(float);
        BYZ_TRY(ctx->gram_chunk_sums.ensure(per_chunk * static_cast<size_t>(chunks_per_sc + 1)));
        chunk_sums = ctx->gram_chunk_sums.as<float>();
        ragged_sums = chunk_sums + (per_chunk / sizeof(float)) * static_cast<size_t>(chunks_per_sc);
    }
    auto kernel16 = defer ? &gram_planes16_kernel<6, true> : &gram_planes16_kernel<6, false>;
    const void* kernel = f16 ? reinterpret_cast<const void*>(kernel16) : reinterpret_cast<const void*>(&gram_planes_kernel<4>);
    const size_t lds_bytes = static_cast<size_t>(f16 ? 6 : 4) * kRowBlocks * n_planes * kFragBytes;
    BYZ_HIP(allow_dynamic_lds(ctx, kernel, static_cast<int>(lds_bytes)));
    const int round_size = env_int("BYZ_GRAM_ROUND", ctx->num_cus / 8);   // one workgroup per CU
    // f16x2: runs of whole rounds (one workgroup per CU of an XCD), claimed by the XCDs as they get to them
    const int run = round_size > 0 ? round_size : ctx->num_cus / 8;
    const int64_t per_xcd = ceil_div(n_tiles, 8);
    for (int64_t sc = 0; sc < n_sc; ++sc) {
        const int64_t k0 = sc * sc_cols;
        const int64_t cols = n_cols - k0 < sc_cols ? n_cols - k0 : sc_cols;
        const int64_t n_steps = ceil_div(cols, 32) * 2;   // whole 32-column stages, as gram.hip counts them (zero-filled)
        const int64_t n_chunks = ceil_div(n_steps, kChunkSteps);
        {
            KernelTimer t(ctx, BYZ_K_PLANE_SPLIT, stream);
            if (f16) {
                const dim3 grid(static_cast<unsigned>(n_chunks), static_cast<unsigned>(rows_pad / 32));
                if (env_int("BYZ_GRAM_SPLIT_TWO_PASS", 0) != 0) {   // round 2's kernel for everything (the comparison)
                    plane_split_f16_kernel<<<grid, 256, 0, stream>>>(G, n_rows, n_cols, ld, row_index, k0, n_steps, planes,
                                                                     unscale, rows_pad, nullptr);
                } else {
                    // one pass with a sampled scale; the blocks where it did not hold are listed and redone exactly
                    const int64_t pairs = n_chunks * (rows_pad / 32);
                    BYZ_TRY(ctx->split_redo.ensure(static_cast<size_t>(1 + 2 * pairs) * sizeof(int32_t)));
                    int32_t* redo = ctx->split_redo.as<int32_t>();
                    BYZ_HIP(hipMemsetAsync(redo, 0, sizeof(int32_t), stream));
                    // (non-temporal loads of G here: measured in round 6, 6.38 ms per launch either way -- EXPERIMENTS.md G6)
                    plane_split_f16_stream_kernel<<<grid, 256, 0, stream>>>(G, n_rows, n_cols, ld, row_index, k0, n_steps, planes,
                                                                            unscale, rows_pad, redo);
                    BYZ_TRY(check_launch("plane_split_f16_stream_kernel"));
                    // (sized for a few thousand listed blocks; the surplus workgroups leave at once, and a longer list --
                    // pathological data -- is walked in a grid-stride loop: no host read-back of the count.)
                    const int64_t fix = pairs < 4096 ? pairs : 4096;
                    plane_split_f16_kernel<<<static_cast<unsigned>(fix), 256, 0, stream>>>(G, n_rows, n_cols, ld, row_index, k0,
                                                                                           n_steps, planes, unscale, rows_pad, redo);
                }
            } else {
                const dim3 grid(static_cast<unsigned>(ceil_div(n_steps, kSplitCols / 16)), static_cast<unsigned>(rows_pad / 32));
                plane_split_bf16_kernel<<<grid, 256, 0, stream>>>(G, n_rows, n_cols, ld, row_index, k0, n_steps, planes);
            }
            BYZ_TRY(check_launch("plane_split_kernel"));
        }
        {
            // f16x2: every XCD is launched the same number of rounds, kSpareRoundsPercent more than its share; a faster XCD
            // claims more runs and the surplus rounds of the others find nothing left and leave at once
            int64_t rounds_per_xcd = 0;
            if (f16) {
                rounds_per_xcd = ceil_div(ceil_div(n_tiles * n_chunks, run), 8);
                rounds_per_xcd += rounds_per_xcd * kSpareRoundsPercent / 100;
            }
            const int64_t grid = f16 ? 8 * run * rounds_per_xcd : 8 * per_xcd * n_chunks;
            // tickets: [n_tiles] chunk order of a tile (in-kernel update), [8] workgroups done per XCD, [1] runs claimed,
            // [8][rounds_per_xcd] the run each round of an XCD claimed (+ 1; 0: not yet)
            const size_t ticket_ints = static_cast<size_t>(n_tiles + 9 + 8 * rounds_per_xcd);
            BYZ_TRY(ctx->gram_tickets.ensure(ticket_ints * sizeof(int)));
            int* tickets = ctx->gram_tickets.as<int>();
            BYZ_HIP(hipMemsetAsync(tickets, 0, ticket_ints * sizeof(int), stream));
            KernelTimer t(ctx, BYZ_K_GRAM, stream);
            if (grid > 0x7fffffff) {
                set_error("gram: grid too large");
                return BYZ_E_UNSUPPORTED;
            }
            const int slab_live0 = sc > 0 ? 1 : 0;
            if (!f16) {
                gram_planes_kernel<4><<<static_cast<unsigned>(grid), kThreads, lds_bytes, stream>>>(
                    planes, n_steps, slabs, static_cast<int>(n_tiles), ctx->plane_order.as<int2>(), static_cast<int>(n_chunks), tickets,
                    round_size, static_cast<int>(t128), slab_live0, n_blocks32, device_status_word(ctx));
            } else {
                kernel16<<<static_cast<unsigned>(grid), kThreads, lds_bytes, stream>>>(
                    planes, n_steps, unscale, rows_pad, slabs, static_cast<int>(n_tiles), ctx->plane_order.as<GramUnit>(),
                    static_cast<int>(n_chunks), tickets, round_size, run, slab_live0, static_cast<int>(n_sum_slots),
                    device_status_word(ctx), chunk_sums, ragged_sums);
            }
            BYZ_TRY(check_launch("gram_planes_kernel"));
        }
        if (defer) {
            KernelTimer t(ctx, BYZ_K_GRAM_REDUCE, stream);
            const int ragged_chunk = (n_steps % kChunkSteps) % kFlushSteps != 0 ? static_cast<int>(n_chunks) - 1 : -1;
            const int2* slot_slab = reinterpret_cast<const int2*>(ctx->plane_order.as<GramUnit>() + n_tiles);
            chunk_reduce_kernel<<<dim3(static_cast<unsigned>(n_sum_slots), 4), 256, 0, stream>>>(
                chunk_sums, ragged_sums, static_cast<int>(n_sum_slots), static_cast<int>(n_chunks), ragged_chunk, slot_slab,
                unscale, rows_pad, slabs, sc > 0 ? 1 : 0, n_blocks32);
            BYZ_TRY(check_launch("chunk_reduce_kernel"));
        }
    }
    return BYZ_OK;
}

}  // namespace byz
