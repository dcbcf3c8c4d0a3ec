// Microbenchmark (EXPERIMENTS.md G10): does the ISSUE ORDER of the fp16 MFMAs matter at the socket's power cap?  The inner body is
// one 32-column half of gram_planes16_kernel's super-stage: 4 A blocks x 2 planes (h, m), 2 B blocks x 2 planes, 8 accumulator
// blocks of 16 x 16, 24 v_mfma_f32_16x16x32_f16 (m h' + h m' + h h' per block, each accumulator in that order).  The fragments
// of the NEXT iteration are read from LDS by ds_read_b128 (12 per iteration, a moving offset in a 64 KiB pool) in front of the
// 24 MFMAs, as the kernel reads them under its MFMAs; level-1 flush every 8 iterations (256 columns).  Whole chip, 256 lanes
// per workgroup, two workgroups per CU (two waves per SIMD, as in the kernel).  Every MFMA is fenced by a sched_barrier, so the
// order in the ISA is the order written here.
//   ORDER 0  (a) term-major, n fastest                 q -> t = q / 8, m = (q % 8) / 2, n = q % 2    (the kernel's super8 today)
//   ORDER 1  (b) term-major, serpentine                m0n0 m0n1 m1n1 m1n0 m2n0 ..., walked backwards in the middle term
//   ORDER 2  (c) block-major, chained, m-major         the three products of a block back to back into its accumulator
//   ORDER 3  (d) block-major, chained, serpentine
// All four give every accumulator the same products in the same order: the sums are bitwise equal (the checksum printed).
// Build: hipcc --offload-arch=gfx950 -O3 -mllvm -pragma-unroll-threshold=1000000 mfma_orders.hip -o mfma_orders
// Run:   mfma_orders ORDER [iters] [random|zeros]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct Step { int t, m, n; };
struct Order { Step s[24]; };

constexpr int serp_n(int m, int n) { return (m & 1) ? 1 - n : n; }

template <int ORDER>
constexpr Order make_order() {
    Order o{};
    for (int q = 0; q < 24; ++q) {
        if (ORDER == 0) {
            o.s[q] = {q / 8, (q % 8) / 2, q % 2};
        } else if (ORDER == 1) {
            const int t = q / 8;
            const int w = (t == 1) ? 7 - q % 8 : q % 8;     // the middle term backwards: its last block is the last term's first
            o.s[q] = {t, w / 2, serp_n(w / 2, w % 2)};
        } else if (ORDER == 2) {
            o.s[q] = {q % 3, q / 6, (q / 3) % 2};
        } else {
            o.s[q] = {q % 3, q / 6, serp_n(q / 6, (q / 3) % 2)};
        }
    }
    return o;
}

struct Frags { f16x8 a[2][4], b[2][2]; };     // [plane: 0 = h, 1 = m][block]

template <int ORDER>
__global__ __launch_bounds__(256) void kern(const f16x8* __restrict__ in, float* __restrict__ out, int iters, long long* __restrict__ clk) {
    __shared__ f16x8 pool[4096];     // 64 KiB
    const int tid = threadIdx.x;
    for (int i = tid; i < 4096; i += 256) pool[i] = in[i];
    __syncthreads();
    const int lane = tid & 63;
    constexpr Order order = make_order<ORDER>();
    constexpr int pa[3] = {1, 0, 0};
    constexpr int pb[3] = {0, 1, 0};
    auto read = [&](Frags& f, int step) __attribute__((always_inline)) {
        const int base = step * 12 * 64;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int m = 0; m < 4; ++m) f.a[p][m] = pool[(base + (p * 4 + m) * 64 + lane) & 4095];
#pragma unroll
            for (int n = 0; n < 2; ++n) f.b[p][n] = pool[(base + (8 + p * 2 + n) * 64 + lane) & 4095];
        }
    };
    f32x4 acc[4][2], acc2[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[m][n][e] = acc2[m][n][e] = 0.0f;
    Frags f[2];
    read(f[0], tid >> 6);
    const long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {              // 8 x 32 = 256 columns, then the flush
            read(f[(s + 1) & 1], it * 8 + s + 1 + (tid >> 6));
            __builtin_amdgcn_sched_barrier(0);
            const Frags& c = f[s & 1];
#pragma unroll
            for (int q = 0; q < 24; ++q) {
                const int t = order.s[q].t, m = order.s[q].m, n = order.s[q].n;
                acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(c.a[pa[t]][m], c.b[pb[t]][n], acc[m][n], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc2[m][n][e] += acc[m][n][e];
                    acc[m][n][e] = 0.0f;
                }
    }
    const long long t1 = __builtin_readcyclecounter();
    float total = 0.0f;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 4; ++e) total += acc2[m][n][e];
    out[blockIdx.x * blockDim.x + tid] = total;
    if (tid == 0) clk[blockIdx.x] = t1 - t0;
}

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main(int argc, char** argv) {
    const int which = argc > 1 ? std::atoi(argv[1]) : 0;
    const int iters = argc > 2 ? std::atoi(argv[2]) : 20000;
    const char* fill = argc > 3 ? argv[3] : "random";
    if (which < 0 || which > 3 || iters < 1) {
        std::fprintf(stderr, "usage: mfma_orders ORDER(0..3) [iters] [random|zeros]\n");
        return 2;
    }
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int wgs = 2 * prop.multiProcessorCount;
    std::vector<_Float16> host(4096 * 8);
    unsigned s = 12345u;
    for (auto& v : host) {
        s = s * 1664525u + 1013904223u;
        const float x = (static_cast<int>(s >> 8) % 65536 - 32768) / 32768.0f * 8.0f;     // full-range mantissas; |sum| stays finite in fp32
        v = static_cast<_Float16>(fill[0] == 'z' ? 0.0f : x);
    }
    f16x8* in;
    float* out;
    long long* clk;
    CHECK(hipMalloc(&in, host.size() * sizeof(_Float16)));
    CHECK(hipMalloc(&out, static_cast<size_t>(wgs) * 256 * sizeof(float)));
    CHECK(hipMalloc(&clk, static_cast<size_t>(wgs) * sizeof(long long)));
    CHECK(hipMemcpy(in, host.data(), host.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    static const char* names[4] = {"(a) term-major, n fastest", "(b) term-major, serpentine", "(c) block-major chained, m-major", "(d) block-major chained, serpentine"};
    for (int rep = 0; rep < 3; ++rep) {
        for (int warm = 0; warm < 2; ++warm) {     // the first launch brings the socket to its steady clock, the second is timed
            switch (which) {
                case 0: kern<0><<<wgs, 256>>>(in, out, iters, clk); break;
                case 1: kern<1><<<wgs, 256>>>(in, out, iters, clk); break;
                case 2: kern<2><<<wgs, 256>>>(in, out, iters, clk); break;
                default: kern<3><<<wgs, 256>>>(in, out, iters, clk); break;
            }
            if (warm == 0) { CHECK(hipDeviceSynchronize()); CHECK(hipEventRecord(a)); }
        }
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms = 0.0f;
        CHECK(hipEventElapsedTime(&ms, a, b));
        std::vector<long long> c(wgs);
        CHECK(hipMemcpy(c.data(), clk, wgs * sizeof(long long), hipMemcpyDeviceToHost));
        std::vector<float> o(static_cast<size_t>(wgs) * 256);
        CHECK(hipMemcpy(o.data(), out, o.size() * sizeof(float), hipMemcpyDeviceToHost));
        unsigned check = 0;
        for (size_t i = 0; i < 1024; ++i) {     // workgroups 0 .. 3: every workgroup computes the same sums
            unsigned bits;
            std::memcpy(&bits, &o[i], 4);
            check = check * 31u + bits;
        }
        double cyc = 0;
        for (long long v : c) cyc += static_cast<double>(v);
        cyc /= wgs;
        const double flops = 2.0 * 16 * 16 * 32 * 24 * 8.0 * iters * 4 * wgs;     // per launch
        std::printf("%s data, %s: %.3f ms, %.0f TF of fp16 MFMA (%.3f of 2.5 PF), %.0f cycles per workgroup = %.3f GHz, checksum %08x\n", fill, names[which], ms,
                    flops / (ms * 1e-3) / 1e12, flops / (ms * 1e-3) / 2.5e15, cyc, cyc / (ms * 1e-3) / 1e9, check);
    }
    return 0;
}
