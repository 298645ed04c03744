// mfma_gap_probe.hip -- how many single-issue vector instructions hide in the gap between two v_mfma_f32_32x32x16_bf16 of ONE wave?
// (measurement helper, not product code; the table it prints is profiles/mfma_gap_probe.txt, its device assembly profiles/mfma_gap_probe.s)
// One workgroup per CU (96 KiB of LDS keeps a second one off it), 256 threads = one wave per SIMD or 512 threads = two (wave w sits on
// SIMD w & 3).  Every wave runs a loop of dependent MFMAs on one accumulator with exactly F vector instructions after each MFMA, F = 0..8,
// in the instruction mix of the operand split of mfma_split.h (v_and_b32, v_sub_f32, v_perm_b32, v_max_f32), on eight registers that have
// nothing to do with the accumulator or the operands.  The whole loop body is ONE asm volatile string, so the placement is what is written
// here and not what a scheduler makes of it; the loop is timed in shader cycles (s_memtime), the clock is read off s_memrealtime (100 MHz).
// Build: tools/peak/build.sh (the library's flags, -fno-slp-vectorize -fno-vectorize among them: no packed-fp32 instruction).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int GROUPS = 16;       // MFMA + F fillers, written out this many times per loop iteration
constexpr int LDS_BYTES = 96 * 1024;

#define MF "v_mfma_f32_32x32x16_bf16 %[acc], %[a], %[b], %[acc]\n\t"
#define FI0 "v_and_b32 %[x0], %[msk], %[x0]\n\t"
#define FI1 "v_sub_f32 %[x1], %[x1], %[c]\n\t"
#define FI2 "v_perm_b32 %[x2], %[x2], %[x6], %[sel]\n\t"
#define FI3 "v_max_f32 %[x3], %[x3], %[c]\n\t"
#define FI4 "v_and_b32 %[x4], %[msk], %[x4]\n\t"
#define FI5 "v_sub_f32 %[x5], %[x5], %[c]\n\t"
#define FI6 "v_perm_b32 %[x6], %[x6], %[x2], %[sel]\n\t"
#define FI7 "v_max_f32 %[x7], %[x7], %[c]\n\t"
#define FILL_0 ""
#define FILL_1 FI0
#define FILL_2 FILL_1 FI1
#define FILL_3 FILL_2 FI2
#define FILL_4 FILL_3 FI3
#define FILL_5 FILL_4 FI4
#define FILL_6 FILL_5 FI5
#define FILL_7 FILL_6 FI6
#define FILL_8 FILL_7 FI7
#define G1(F) MF FILL_##F
#define G4(F) G1(F) G1(F) G1(F) G1(F)
#define G16(F) G4(F) G4(F) G4(F) G4(F)

// out[2 * wave_global] = shader cycles of the loop, out[2 * wave_global + 1] = 100 MHz ticks of the same interval
#define PROBE_KERNEL(F)                                                                                                              \
    __global__ __launch_bounds__(512) void gap_probe_##F(int iters, unsigned long long *out, float *sink, float seed) {              \
        extern __shared__ float lds_pad[];                                                                                           \
        f32x16 acc;                                                                                                                  \
        for (int r = 0; r < 16; ++r) acc[r] = seed * r;                                                                              \
        bf16x8 a, b;                                                                                                                 \
        for (int i = 0; i < 8; ++i) { a[i] = (__bf16)(seed * 0.01f + (threadIdx.x & 63) * 0.001f); b[i] = (__bf16)(seed * 0.01f - i * 0.005f); } \
        float x0 = seed + threadIdx.x, x1 = x0 + 1.f, x2 = x0 + 2.f, x3 = x0 + 3.f, x4 = x0 + 4.f, x5 = x0 + 5.f, x6 = x0 + 6.f, x7 = x0 + 7.f; \
        const float c = 0.5f * seed;                                                                                                 \
        const unsigned msk = 0xFFFF0000u, sel = 0x07060302u;                                                                         \
        asm volatile("s_nop 4" ::: "memory");                                                                                        \
        const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();                                                              \
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();                                                                  \
        _Pragma("unroll 1") for (int it = 0; it < iters; ++it)                                                                       \
            asm volatile(G16(F)                                                                                                      \
                         : [acc] "+v"(acc), [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2), [x3] "+v"(x3), [x4] "+v"(x4), [x5] "+v"(x5), \
                           [x6] "+v"(x6), [x7] "+v"(x7)                                                                              \
                         : [a] "v"(a), [b] "v"(b), [c] "v"(c), [msk] "v"(msk), [sel] "v"(sel));                                      \
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();                                                                  \
        const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();                                                              \
        asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc)); /* compiler code below reads the last MFMA's result: its wait states */      \
        float s = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;                                                                             \
        for (int r = 0; r < 16; ++r) s += acc[r];                                                                                    \
        if (iters < 0) s += lds_pad[threadIdx.x];                                                                                    \
        sink[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;                                                                     \
        if ((threadIdx.x & 63) == 0) {                                                                                               \
            const size_t w = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                                            \
            out[2 * w] = t1 - t0;                                                                                                    \
            out[2 * w + 1] = r1 - r0;                                                                                                \
        }                                                                                                                            \
    }
PROBE_KERNEL(0) PROBE_KERNEL(1) PROBE_KERNEL(2) PROBE_KERNEL(3) PROBE_KERNEL(4) PROBE_KERNEL(5) PROBE_KERNEL(6) PROBE_KERNEL(7) PROBE_KERNEL(8)

typedef void (*probe_fn)(int, unsigned long long *, float *, float);
static const probe_fn PROBES[9] = {gap_probe_0, gap_probe_1, gap_probe_2, gap_probe_3, gap_probe_4, gap_probe_5, gap_probe_6, gap_probe_7, gap_probe_8};

#define CHECK(e) do { const hipError_t e_ = (e); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_)); exit(1); } } while (0)

int main() {
    const int blocks = 256, iters = 4000;
    unsigned long long *d_out;
    float *d_sink;
    CHECK(hipMalloc(&d_out, (size_t)blocks * 8 * 2 * sizeof(unsigned long long)));
    CHECK(hipMalloc(&d_sink, (size_t)blocks * 512 * sizeof(float)));
    std::vector<unsigned long long> h((size_t)blocks * 8 * 2);
    for (int f = 0; f <= 8; ++f)
        CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(PROBES[f]), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    printf("# v_mfma_f32_32x32x16_bf16 chain on one accumulator, F vector instructions (and/sub/perm/max) pinned after every MFMA\n");
    printf("# %d workgroups (one per CU), %d MFMAs per wave; median over waves; slot = wave cycles / (MFMAs of the wave x waves per SIMD)\n", blocks,
           iters * GROUPS);
    printf("# waves/SIMD  F  cycles/MFMA(wave)  cycles/MFMA-slot(SIMD)  vs F=0  clock GHz  min..max slot\n");
    for (int wps = 1; wps <= 2; ++wps) {
        double base = 0;
        for (int f = 0; f <= 8; ++f) {
            const int waves = blocks * 4 * wps;
            for (int rep = 0; rep < 2; ++rep) {  // the first launch warms code and clock, the second is read
                hipLaunchKernelGGL(PROBES[f], dim3(blocks), dim3(256 * wps), LDS_BYTES, 0, iters, d_out, d_sink, 1.0f);
                CHECK(hipGetLastError());
                CHECK(hipDeviceSynchronize());
            }
            CHECK(hipMemcpy(h.data(), d_out, (size_t)waves * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            std::vector<double> cyc(waves), ghz(waves);
            for (int w = 0; w < waves; ++w) {
                cyc[w] = (double)h[2 * w] / ((double)iters * GROUPS);
                ghz[w] = (double)h[2 * w] / (double)h[2 * w + 1] * 0.1;
            }
            std::sort(cyc.begin(), cyc.end());
            std::sort(ghz.begin(), ghz.end());
            const double med = cyc[waves / 2], slot = med / wps;
            if (f == 0) base = slot;
            printf("%10d  %d  %17.2f  %22.2f  %+5.1f%%  %9.2f  %.2f..%.2f\n", wps, f, med, slot, 100.0 * (slot / base - 1.0), ghz[waves / 2],
                   cyc.front() / wps, cyc.back() / wps);
        }
    }
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_sink));
    return 0;
}
