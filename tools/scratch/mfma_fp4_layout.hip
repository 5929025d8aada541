// Operand probe of v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 (e2m1) operands on gfx950, for the matcher (match_kernels.hip).
//   hipcc --offload-arch=gfx950 -O3 mfma_fp4_layout.hip -o mfma_fp4_layout
// (a) layout: assumed lane l (r = l & 31, h = l >> 5) holds A[row r][k = 32 h + e] and B[k = 32 h + e][col r], element e = 0 .. 31 in nibble e of its
//     16 operand bytes (low nibble of byte 0 first); D lane l register v = D[8 (v / 4) + v % 4 + 4 h][r].  Checked with all sixteen e2m1 codes.
// (b) scale bytes of 127 (E8M0 1.0) on both sides leave the products unscaled (part of (a)); 128 on one side doubles them; constant zero scale
//     operands make the compiler emit the form without block scales, v_mfma_f32_32x32x64_f8f6f4, whose products are unscaled too.
// (c) the matcher's use: +-1 operands (0x2 / 0xA) expanded from descriptor bits exactly as the kernel does, four chained instructions (K = 256), the
//     first with C = n * 2^-12: D == dot + n / 4096 bit for bit for every Hamming distance 0 .. 256 and every n in 0 .. 4095.
// (d) cycles per instruction back to back (four independent accumulators per wave, one / two / four waves per SIMD), next to v_mfma_i32_32x32x32_i8.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

__device__ inline v8i wide(v4i x) { return v8i{x[0], x[1], x[2], x[3], 0, 0, 0, 0}; }
__device__ inline v16f mma(v4i a, v4i b, v16f c, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wide(a), wide(b), c, 4, 4, 0, sa, 0, sb);
}
__device__ inline v16f mma_unscaled(v4i a, v4i b, v16f c) { // constant 0 scales: v_mfma_f32_32x32x64_f8f6f4
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wide(a), wide(b), c, 4, 4, 0, 0, 0, 0);
}
// the matcher's expansion: 32 descriptor bits -> 32 e2m1 nibbles (clear -> 0x2 = +1, set -> 0xA = -1); operand dword i, nibble n holds bit 4 n + i
__device__ inline v4i expand32(uint32_t x) {
    return v4i{(int)(((x << 3) & 0x88888888u) | 0x22222222u), (int)(((x << 2) & 0x88888888u) | 0x22222222u),
               (int)(((x << 1) & 0x88888888u) | 0x22222222u), (int)((x & 0x88888888u) | 0x22222222u)};
}

// (a), (b): A, Bt are 32 x 64 e2m1 codes, one per byte, row-major [row or col][k]
__global__ void layout_kernel(const uint8_t* A, const uint8_t* Bt, float* D, int sa, int sb) {
    const int l = threadIdx.x, r = l & 31, h = l >> 5;
    v4i a, b;
    for (int w = 0; w < 4; ++w) {
        uint32_t ua = 0, ub = 0;
        for (int e = 0; e < 8; ++e) {
            ua |= (uint32_t)(A[r * 64 + 32 * h + 8 * w + e] & 15) << (4 * e);
            ub |= (uint32_t)(Bt[r * 64 + 32 * h + 8 * w + e] & 15) << (4 * e);
        }
        a[w] = (int)ua; b[w] = (int)ub;
    }
    v16f c;
    for (int v = 0; v < 16; ++v) c[v] = 0.f;
    c = sa == 0 ? mma_unscaled(a, b, c) : mma(a, b, c, sa, sb);
    for (int v = 0; v < 16; ++v) D[l * 16 + v] = c[v];
}

// (c): block (nb, hb): rows i carry n = 32 nb + i, columns j carry the descriptor U ^ mask[32 hb + j] (mask index = its popcount, clamped to 256)
template <bool kUnscaled>
__global__ void key_kernel(const uint32_t* U /* 8 dwords */, const uint32_t* masks /* [288][8] */, int* bad, float* worst) {
    const int l = threadIdx.x, r = l & 31, h = l >> 5, nb = blockIdx.x, hb = blockIdx.y;
    const int ham = min(32 * hb + r, 256);
    v16f c;
    for (int v = 0; v < 16; ++v) c[v] = (float)(32 * nb + 8 * (v / 4) + v % 4 + 4 * h) * (1.f / 4096.f);
    for (int s = 0; s < 4; ++s) { // half h of step s takes descriptor dword 4 h + s, as the kernel does
        const v4i a = expand32(U[4 * h + s]), b = expand32(U[4 * h + s] ^ masks[ham * 8 + 4 * h + s]);
        c = kUnscaled ? mma_unscaled(a, b, c) : mma(a, b, c, 0x7F7F7F7F, 0x7F7F7F7F);
    }
    const float dot = (float)(256 - 2 * ham);
    for (int v = 0; v < 16; ++v) {
        const float want = dot + (float)(32 * nb + 8 * (v / 4) + v % 4 + 4 * h) * (1.f / 4096.f); // exact: 21 significant bits
        if (c[v] != want) { atomicAdd(bad, 1); worst[0] = c[v]; worst[1] = want; }
    }
}

// (d)
template <bool kFp4>
__global__ __launch_bounds__(256) void rate_kernel(int iters, float* sink) {
    const int l = threadIdx.x;
    v4i a = {0x22222222 + (l & 1) * 0x80, 0x2A2A2A2A, 0x22222222, 0x2222A222}, b = {0x2A222222, 0x22222222, 0x222A2222, 0x22222222};
    float tot = 0.f;
    if (kFp4) {
        v16f c[4];
        for (int t = 0; t < 4; ++t) for (int v = 0; v < 16; ++v) c[t][v] = 0.f;
        for (int i = 0; i < iters; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t) c[t] = mma_unscaled(a, b, c[t]);
        for (int t = 0; t < 4; ++t) for (int v = 0; v < 16; ++v) tot += c[t][v];
    } else {
        v16i c[4];
        for (int t = 0; t < 4; ++t) for (int v = 0; v < 16; ++v) c[t][v] = 0;
        for (int i = 0; i < iters; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c[t], 0, 0, 0);
        for (int t = 0; t < 4; ++t) for (int v = 0; v < 16; ++v) tot += (float)c[t][v];
    }
    if (tot == 12345.678f) sink[0] = tot;
}

static float e2m1(int code) {
    static const float t[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    return (code & 8) ? -t[code & 7] : t[code & 7];
}

int main() {
    int rc = 0;
    // (a), (b)
    uint8_t hA[32 * 64], hB[32 * 64];
    for (int i = 0; i < 32; ++i) for (int k = 0; k < 64; ++k) { hA[i * 64 + k] = (uint8_t)((i * 7 + k * 3 + (i * k) % 5) & 15); hB[i * 64 + k] = (uint8_t)((i * 5 + k * 11 + 1 + (i + k) % 3) & 15); }
    uint8_t *dA, *dB; float* dD; float hD[64 * 16];
    CK(hipMalloc(&dA, sizeof hA)); CK(hipMalloc(&dB, sizeof hB)); CK(hipMalloc(&dD, sizeof hD));
    CK(hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice));
    for (int pass = 0; pass < 3; ++pass) {
        const int sa = pass == 2 ? 0 : pass ? 0x7F7F7F80 : 0x7F7F7F7F; // byte 0 (opsel 0) is the scale: 127 = 1.0, 128 = 2.0; 0: the form without scales
        hipLaunchKernelGGL(layout_kernel, dim3(1), dim3(64), 0, 0, dA, dB, dD, sa, 0x7F7F7F7F);
        CK(hipDeviceSynchronize()); CK(hipMemcpy(hD, dD, sizeof hD, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int l = 0; l < 64; ++l) for (int v = 0; v < 16; ++v) {
            const int j = l & 31, i = 8 * (v / 4) + v % 4 + 4 * (l >> 5);
            float ref = 0.f;
            for (int k = 0; k < 64; ++k) ref += e2m1(hA[i * 64 + k]) * e2m1(hB[j * 64 + k]);
            bad += hD[l * 16 + v] != (pass == 1 ? 2.f : 1.f) * ref;
        }
        if (pass == 2) printf("(b) FP4 32x32x64 without block scales: mismatches with the assumed layout: %d of 1024\n", bad);
        else printf("(%s) FP4 32x32x64, scale A %d, scale B 127: mismatches with the assumed layout: %d of 1024\n", pass ? "b" : "a", pass ? 128 : 127, bad);
        rc |= bad != 0;
    }
    // (c)
    for (int unscaled = 0; unscaled < 2; ++unscaled) {
        uint32_t hU[8], state = 12345u; std::vector<uint32_t> hM(288 * 8, 0u);
        auto rnd = [&]() { state = state * 1664525u + 1013904223u; return state >> 8; };
        for (int w = 0; w < 8; ++w) hU[w] = rnd() * 2654435761u;
        for (int m = 0; m <= 256; ++m) { // m distinct random bit positions
            int perm[256];
            for (int i = 0; i < 256; ++i) perm[i] = i;
            for (int i = 0; i < m; ++i) { const int j = i + (int)(rnd() % (uint32_t)(256 - i)); const int t = perm[i]; perm[i] = perm[j]; perm[j] = t; hM[m * 8 + perm[i] / 32] |= 1u << (perm[i] % 32); }
        }
        uint32_t *dU, *dM; int* dBad; float* dW; int hBad = -1; float hW[2] = {0.f, 0.f};
        CK(hipMalloc(&dU, sizeof hU)); CK(hipMalloc(&dM, hM.size() * 4)); CK(hipMalloc(&dBad, 4)); CK(hipMalloc(&dW, 8));
        CK(hipMemcpy(dU, hU, sizeof hU, hipMemcpyHostToDevice)); CK(hipMemcpy(dM, hM.data(), hM.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemset(dBad, 0, 4)); CK(hipMemset(dW, 0, 8));
        if (unscaled) hipLaunchKernelGGL(key_kernel<true>, dim3(128, 9), dim3(64), 0, 0, dU, dM, dBad, dW);
        else hipLaunchKernelGGL(key_kernel<false>, dim3(128, 9), dim3(64), 0, 0, dU, dM, dBad, dW);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(&hBad, dBad, 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hW, dW, 8, hipMemcpyDeviceToHost));
        printf("(c) %s: C = n / 4096 + sum of 256 +-1 products over four chained instructions, n = 0 .. 4095, Hamming 0 .. 256: %d inexact of %d",
               unscaled ? "without block scales" : "scales 127", hBad, 128 * 9 * 1024);
        if (hBad) printf(" (one of them: got %.9g, want %.9g)", hW[0], hW[1]);
        printf("\n");
        rc |= hBad != 0;
    }
    // (d)
    {
        hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
        const int cus = prop.multiProcessorCount, iters = 20000;
        float* sink; CK(hipMalloc(&sink, 4));
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        for (int fp4 = 0; fp4 < 2; ++fp4)
            for (int wps = 1; wps <= 4; wps *= 2) { // waves per SIMD: one workgroup of 256 threads = one wave on each SIMD of a CU
                const dim3 grid(cus * wps);
                for (int rep = 0; rep < 2; ++rep) {
                    CK(hipEventRecord(e0));
                    if (fp4) hipLaunchKernelGGL(rate_kernel<true>, grid, dim3(256), 0, 0, iters, sink);
                    else hipLaunchKernelGGL(rate_kernel<false>, grid, dim3(256), 0, 0, iters, sink);
                    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
                }
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                printf("(d) %s, %d wave(s) per SIMD: %.1f ns per instruction and SIMD = %.1f cycles at 2.4 GHz\n", fp4 ? "v_mfma_f32_32x32x64_f8f6f4 (FP4)" : "v_mfma_i32_32x32x32_i8",
                       wps, ms * 1e6 / ((double)iters * 4 * wps), ms * 1e6 / ((double)iters * 4 * wps) * 2.4);
            }
    }
    printf(rc ? "FAILED\n" : "ok\n");
    return rc;
}
