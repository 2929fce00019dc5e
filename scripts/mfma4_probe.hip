// Diagnostic microbenchmark (not part of the product), beside mfma_probe.hip: v_mfma_f32_4x4x1_16B_f32, sixteen independent
// 4x4 outer products per instruction (block b = lane / 4: D_b[i][j] += A_b[i] * B_b[j], A_b[i] in lane 4 b + i, B_b[j] in lane
// 4 b + j, D_b[i][j] in register i of lane 4 b + j).
//  1. the operand / result lane map, checked with exact integers;
//  2. cycles per instruction, back to back on one SIMD: one and two waves per SIMD, one and two accumulators, A operand from a
//     register or from a ds_read_b32 between the instructions (what the apply pass's last layer does);
//  3. the same loop on v_mfma_f32_32x32x2_f32 for the scale, and a 4x4x1 loop with one lane-half swap per instruction pair
//     (what a canonical, k-ordered last layer would add).
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ void k_map(float* out)
{
    const int lane = threadIdx.x;
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    d = __builtin_amdgcn_mfma_f32_4x4x1f32((float)(1 + lane), (float)(100 + 3 * lane), d, 0, 0, 0);
    for (int r = 0; r < 4; ++r) out[lane * 4 + r] = d[r];
}

#define T0() asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory")
#define T1() asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory")

// VARIANT 0: A in a register; 1: A read from LDS before each instruction; 2: A from LDS and one lane-half swap of B per CHAINS
// instructions
template <int CHAINS, int VARIANT>
__global__ void k4(float* out, unsigned long long* cyc, int iters)
{
    __shared__ float w[64 * 64];
    for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) w[e] = 1e-3f * (float)(e % 97);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    f32x4 acc[CHAINS];
    for (int c = 0; c < CHAINS; ++c) acc[c] = {0.f, 0.f, 0.f, 0.f};
    float a = threadIdx.x * 1e-3f, b = 1.0f + threadIdx.x * 1e-4f, b2 = 2.0f - threadIdx.x * 1e-4f;
    unsigned long long t0, t1;
    T0();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (VARIANT == 2) {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(b), __float_as_uint(b2), false, false);
                const unsigned s0 = sw[0], s1 = sw[1];
                b = __uint_as_float(s0);
                b2 = __uint_as_float(s1);
            }
#pragma unroll
            for (int c = 0; c < CHAINS; ++c) {
                if (VARIANT >= 1) a = w[(((it & 3) * 8 + u) * CHAINS + c) * 64 + lane];
                acc[c] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, acc[c], 0, 0, 0);
            }
        }
    }
    T1();
    float s = b2;
    for (int c = 0; c < CHAINS; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

template <int CHAINS, int VARIANT>
__global__ void k32(float* out, unsigned long long* cyc, int iters)
{
    __shared__ float w[64 * 64];
    for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) w[e] = 1e-3f * (float)(e % 97);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    f32x16 acc[CHAINS];
    for (int c = 0; c < CHAINS; ++c) for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    float a = threadIdx.x * 1e-3f, b = 1.0f + threadIdx.x * 1e-4f;
    unsigned long long t0, t1;
    T0();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int c = 0; c < CHAINS; ++c) {
                if (VARIANT >= 1) a = w[(((it & 3) * 8 + u) * CHAINS + c) * 64 + lane];
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[c], 0, 0, 0);
            }
    }
    T1();
    float s = 0;
    for (int c = 0; c < CHAINS; ++c) for (int r = 0; r < 16; ++r) s += acc[c][r];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

template <class K>
static void run(const char* name, K kern, int threads, int chains, int nblk)
{
    float* out; unsigned long long* cyc;
    if (hipMalloc(&out, sizeof(float) * threads * nblk) != hipSuccess || hipMalloc(&cyc, 8 * nblk) != hipSuccess) { printf("hipMalloc failed\n"); exit(1); }
    const int iters = 2000;
    kern<<<nblk, threads>>>(out, cyc, iters);
    kern<<<nblk, threads>>>(out, cyc, iters);
    if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); exit(1); }
    unsigned long long h[256]; hipMemcpy(h, cyc, 8 * nblk, hipMemcpyDeviceToHost);
    double m = 0; for (int i = 0; i < nblk; ++i) m += h[i]; m /= nblk;
    const int wps = threads / 256;
    printf("%-34s waves/SIMD=%d accumulators=%d blocks=%3d : %6.1f cycles per MFMA per wave, %6.1f per MFMA per SIMD\n", name, wps, chains,
           nblk, m / (iters * 8.0 * chains), m / (iters * 8.0 * chains) / wps);
    hipFree(out); hipFree(cyc);
}

int main()
{
    // ---- 1. lane map
    float* d; float h[256];
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) { printf("no device\n"); return 1; }
    k_map<<<1, 64>>>(d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { printf("k_map failed\n"); return 1; }
    int bad = 0;
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) bad += h[l * 4 + r] != (float)(1 + 4 * (l / 4) + r) * (float)(100 + 3 * l);
    printf("lane map D[reg r][lane l] = A[lane 4 (l / 4) + r] * B[lane l]: %s (%d of 256 differ)\n", bad ? "WRONG" : "confirmed", bad);
    hipFree(d);
    // ---- 2., 3. cycles
    for (int nblk : {1, 256}) {
        run("4x4x1  A in register", k4<1, 0>, 256, 1, nblk);
        run("4x4x1  A in register", k4<2, 0>, 256, 2, nblk);
        run("4x4x1  A in register", k4<1, 0>, 512, 1, nblk);
        run("4x4x1  A in register", k4<2, 0>, 512, 2, nblk);
        run("4x4x1  A by ds_read_b32", k4<1, 1>, 256, 1, nblk);
        run("4x4x1  A by ds_read_b32", k4<2, 1>, 256, 2, nblk);
        run("4x4x1  A by ds_read_b32", k4<1, 1>, 512, 1, nblk);
        run("4x4x1  A by ds_read_b32", k4<2, 1>, 512, 2, nblk);
        run("4x4x1  ds_read + half swap per 2", k4<2, 2>, 256, 2, nblk);
        run("4x4x1  ds_read + half swap per 2", k4<2, 2>, 512, 2, nblk);
        run("32x32x2 A in register", k32<1, 0>, 256, 1, nblk);
        run("32x32x2 A in register", k32<1, 0>, 512, 1, nblk);
        run("32x32x2 A by ds_read_b32", k32<1, 1>, 256, 1, nblk);
        run("32x32x2 A by ds_read_b32", k32<1, 1>, 512, 1, nblk);
    }
    return 0;
}
