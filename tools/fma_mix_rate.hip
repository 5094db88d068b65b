// Issue rates of the instruction mixes the wide-node visit can form its slot bounds with.
//
// Each stream is a kernel of its own: every lane runs ITER trips of an unrolled block of 16 independent
// accumulator chains, so no instruction waits for the one before it, and nothing is loaded or stored
// inside the loop.  The instructions are written as inline assembly so that the stream timed is the
// stream named:
//   fma        v_fma_f32 alone                                              (1 VALU per bound)
//   cvt_fma    v_cvt_f32_ubyteN + v_fma_f32                                 (2 VALU per bound)
//   mix_sub    v_perm_b32 + two v_fma_mix_f32, f16 operand subnormal        (3 VALU per 2 bounds)
//              (halves 0x00qq: the byte q read as q * 2^-24)
//   mix_norm   the same with the byte in the half's high byte (0xqq00, q in 0x3c..0x43: normal f16)
// It runs WAVES waves on every SIMD (1 and 4) and prints one JSON line per stream and occupancy: the
// time, VALU instructions per nanosecond and per SIMD, and cycles per wave64 instruction at the
// device's reported clock.  Usage: fma_mix_rate [iterations]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int CHAINS = 16;
enum Stream : int { FMA = 0, CVT_FMA, MIX_SUB, MIX_NORM, NSTREAM };
static const char *NAME[NSTREAM] = {"fma", "cvt_fma", "mix_sub", "mix_norm"};
static const int VALU_PER_BLOCK[NSTREAM] = {CHAINS, 2 * CHAINS, CHAINS + CHAINS / 2, CHAINS + CHAINS / 2};

template <int S>
__global__ __launch_bounds__(256) void stream(const uint32_t *__restrict__ in, float *__restrict__ out, uint32_t iters) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t w = in[tid & 255u];
    const float sc = 0x1p-3f;
    float acc[CHAINS];
#pragma unroll
    for (int j = 0; j < CHAINS; j++) acc[j] = (float)j;
    for (uint32_t i = 0; i < iters; i++) {
        if constexpr (S == FMA) {
            float t = __uint_as_float(w);
#pragma unroll
            for (int j = 0; j < CHAINS; j++) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(acc[j]) : "v"(t), "v"(sc));
        } else if constexpr (S == CVT_FMA) {
#pragma unroll
            for (int j = 0; j < CHAINS; j += 4) {
                float t0, t1, t2, t3;
                asm volatile("v_cvt_f32_ubyte0 %0, %1" : "=v"(t0) : "v"(w));
                asm volatile("v_cvt_f32_ubyte1 %0, %1" : "=v"(t1) : "v"(w));
                asm volatile("v_cvt_f32_ubyte2 %0, %1" : "=v"(t2) : "v"(w));
                asm volatile("v_cvt_f32_ubyte3 %0, %1" : "=v"(t3) : "v"(w));
                asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(acc[j + 0]) : "v"(t0), "v"(sc));
                asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(acc[j + 1]) : "v"(t1), "v"(sc));
                asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(acc[j + 2]) : "v"(t2), "v"(sc));
                asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(acc[j + 3]) : "v"(t3), "v"(sc));
            }
        } else {
            // v_perm_b32: selector bytes 0..3 take a byte of the second source, 0x0c gives 0x00
            constexpr uint32_t sel_lo = S == MIX_SUB ? 0x0c010c00u : 0x010c000cu;
            constexpr uint32_t sel_hi = S == MIX_SUB ? 0x0c030c02u : 0x030c020cu;
#pragma unroll
            for (int j = 0; j < CHAINS; j += 4) {
                uint32_t p0, p1;
                asm volatile("v_perm_b32 %0, 0, %1, %2" : "=v"(p0) : "v"(w), "s"(sel_lo));
                asm volatile("v_perm_b32 %0, 0, %1, %2" : "=v"(p1) : "v"(w), "s"(sel_hi));
                asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,0,0]" : "+v"(acc[j + 0]) : "v"(p0), "v"(sc));
                asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc[j + 1]) : "v"(p0), "v"(sc));
                asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,0,0]" : "+v"(acc[j + 2]) : "v"(p1), "v"(sc));
                asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc[j + 3]) : "v"(p1), "v"(sc));
            }
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < CHAINS; j++) s += acc[j];
    out[tid] = s;
}

template <int S>
static float run(const uint32_t *in, float *out, uint32_t grid, uint32_t iters, hipEvent_t a, hipEvent_t b) {
    stream<S><<<grid, 256>>>(in, out, 16);  // warm: code object loaded, clocks up
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(a));
    stream<S><<<grid, 256>>>(in, out, iters);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(b));
    CHECK(hipEventSynchronize(b));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, a, b));
    return ms;
}

int main(int argc, char **argv) {
    const uint32_t iters = argc > 1 ? (uint32_t)atoi(argv[1]) : 20000u;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const double ghz = prop.clockRate * 1e-6;
    uint32_t h_in[256];
    // bytes 0x3c..0x43: subnormal as 0x00qq, normal (1.0 .. 3.5) as 0xqq00
    for (int i = 0; i < 256; i++) h_in[i] = 0x3c3d3e3fu + 0x01010101u * (uint32_t)(i & 3);
    uint32_t *in;
    float *out;
    const uint32_t max_grid = (uint32_t)cus * 4u;  // 4 waves per SIMD: 16 waves = 4 blocks of 256 per CU
    CHECK(hipMalloc(&in, sizeof(h_in)));
    CHECK(hipMalloc(&out, (size_t)max_grid * 256 * sizeof(float)));
    CHECK(hipMemcpy(in, h_in, sizeof(h_in), hipMemcpyHostToDevice));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    for (int waves = 1; waves <= 4; waves *= 4) {
        const uint32_t grid = (uint32_t)cus * (uint32_t)waves;  // one block of 4 waves per CU and wave per SIMD
        for (int s = 0; s < NSTREAM; s++) {
            float ms = 0;
            switch (s) {
            case FMA: ms = run<FMA>(in, out, grid, iters, a, b); break;
            case CVT_FMA: ms = run<CVT_FMA>(in, out, grid, iters, a, b); break;
            case MIX_SUB: ms = run<MIX_SUB>(in, out, grid, iters, a, b); break;
            case MIX_NORM: ms = run<MIX_NORM>(in, out, grid, iters, a, b); break;
            }
            const double per_wave = (double)iters * VALU_PER_BLOCK[s];
            const double per_simd = per_wave * waves;
            const double cyc = ms * 1e6 * ghz / per_simd;  // SIMD cycles per wave64 VALU instruction
            printf("{\"stream\": \"%s\", \"waves_per_simd\": %d, \"cus\": %d, \"clock_ghz\": %.3f, \"iters\": %u, "
                   "\"valu_per_wave\": %.0f, \"ms\": %.4f, \"valu_per_ns_per_simd\": %.4f, \"cycles_per_valu\": %.3f, "
                   "\"ns_per_bound\": %.5f}\n",
                   NAME[s], waves, cus, ghz, iters, per_wave, ms, per_simd / (ms * 1e6), cyc,
                   ms * 1e6 / ((double)iters * CHAINS * waves));
            fflush(stdout);
        }
    }
    CHECK(hipFree(in));
    CHECK(hipFree(out));
    return 0;
}
