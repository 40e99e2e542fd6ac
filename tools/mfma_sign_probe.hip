// Is v_mfma_f32_32x32x16_bf16 odd in its operands?  For random bf16 A [32][K] and B [K][32] one wave computes C = A B and Cn = (-A) B as chains of
// K / 16 instructions from a zero accumulator (the k order of the library's tile GEMM) and counts the outputs with Cn != -C.  Negating a bf16
// operand is exact (a sign bit), so with an accumulation rounded symmetrically about zero (round to nearest, or truncation of the magnitude) the
// two chains mirror each other bit for bit.  Two controls beside it on the same data: the same product as an fp32 fmaf chain in k order on the
// vector pipe (IEEE round to nearest: must mirror), and the exact product in fp64 on the host, which says on which side of the exact value the
// two matrix-pipe results lie.  The tangent pass of the library (csrc/k_jvp.hip.h) pairs every tangent product because of what this prints.
//   build: hipcc -O3 --offload-arch=gfx950 -std=c++17 tools/mfma_sign_probe.hip -o tools/_exp/mfma_sign_probe
//   run:   tools/_exp/mfma_sign_probe [seed]          (profiles/jvp_parity.txt keeps one run)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../lam_slide_amd/csrc/common.hip.h"
#include "../lam_slide_amd/csrc/k_gemm.hip.h"  // the library's tile GEMM and its plain epilogue

// A, An: [32][K] bf16 row-major; Bt: [32][K] bf16 (column c of B as a row); out: [32][32] (row, col).  One wave.
__global__ void __launch_bounds__(64) k_probe(const u16 *A, const u16 *An, const u16 *Bt, int K, float *C, float *Cn, float *Cv, float *Cvn) {
    const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
    f32x16 c, cn;
#pragma unroll
    for (int e = 0; e < 16; ++e) c[e] = cn[e] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const bf16x8 a = as_bf16x8(*reinterpret_cast<const u32x4 *>(A + (size_t)r * K + k0 + 8 * hf));
        const bf16x8 an = as_bf16x8(*reinterpret_cast<const u32x4 *>(An + (size_t)r * K + k0 + 8 * hf));
        const bf16x8 b = as_bf16x8(*reinterpret_cast<const u32x4 *>(Bt + (size_t)r * K + k0 + 8 * hf));
        c = mfma32(a, b, c);
        cn = mfma32(an, b, cn);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        C[acc_row(e, hf) * 32 + r] = c[e];
        Cn[acc_row(e, hf) * 32 + r] = cn[e];
    }
    for (int i = lane; i < 1024; i += 64) {  // the vector-pipe control: one fmaf per k, in k order
        const int row = i >> 5, col = i & 31;
        float s = 0.0f, sn = 0.0f;
        for (int k = 0; k < K; ++k) {
            s = fmaf(bf2f(A[(size_t)row * K + k]), bf2f(Bt[(size_t)col * K + k]), s);
            sn = fmaf(bf2f(An[(size_t)row * K + k]), bf2f(Bt[(size_t)col * K + k]), sn);
        }
        Cv[i] = s;
        Cvn[i] = sn;
    }
}

static u16 to_bf16(float f) {  // round to nearest even
    unsigned u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (u16)(u >> 16);
}
static float from_bf16(u16 v) {
    const unsigned u = (unsigned)v << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// operand distributions: 0 uniform in (-1, 1); 1 the same times 2^e, e uniform in -8 .. 8 (a wide spread of exponents inside one dot product)
static float draw(int dist) {
    const float u = 2.0f * rand() / (float)RAND_MAX - 1.0f;
    return dist == 0 ? u : ldexpf(u, rand() % 17 - 8);
}

// The library's tile GEMM (k_gemm_glds, 128 x 128 tiles, the plain fp32 epilogue) on W [F][K] and X [N][K] against the same on -X
static int gemm_probe(int dist, int F, int N, int K) {
    std::vector<u16> W((size_t)F * K), X((size_t)N * K), Xn((size_t)N * K);
    for (auto &w : W) w = to_bf16(draw(dist) / sqrtf((float)K));
    for (size_t i = 0; i < X.size(); ++i) X[i] = to_bf16(draw(dist)), Xn[i] = X[i] ^ 0x8000u;
    u16 *dW, *dX, *dXn;
    float *dO, *dOn;
    hipMalloc(&dW, W.size() * 2), hipMalloc(&dX, X.size() * 2), hipMalloc(&dXn, X.size() * 2), hipMalloc(&dO, (size_t)N * F * 4), hipMalloc(&dOn, (size_t)N * F * 4);
    hipMemcpy(dW, W.data(), W.size() * 2, hipMemcpyHostToDevice);
    hipMemcpy(dX, X.data(), X.size() * 2, hipMemcpyHostToDevice);
    hipMemcpy(dXn, Xn.data(), X.size() * 2, hipMemcpyHostToDevice);
    auto kern = k_gemm_glds<128, 128, 2, 2, 64, 2, false, EpiPlain>;
    const size_t lds = GemmCfg<128, 128, 2, 2, 64, 2, false, EpiPlain>::lds_bytes;
    hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const int tiles = (N / 128) * (F / 128);
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(256), lds, 0, GemmArgs{dW, dX, F, N, K, 0, 0}, EpiPlain{nullptr, dO, F, 0});
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(256), lds, 0, GemmArgs{dW, dXn, F, N, K, 0, 0}, EpiPlain{nullptr, dOn, F, 0});
    std::vector<float> o((size_t)N * F), on((size_t)N * F);
    if (hipMemcpy(o.data(), dO, o.size() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(on.data(), dOn, o.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return printf("HIP error in the tile GEMM\n"), 1;
    long bad = 0, nonzero = 0;
    float worst = 0.0f;
    for (size_t i = 0; i < o.size(); ++i) {
        nonzero += o[i] != 0.0f;
        if (on[i] != -o[i]) ++bad, worst = fmaxf(worst, fabsf(on[i] + o[i]));
    }
    printf("tile GEMM k_gemm_glds<128, 128, 2, 2, 64, 2, EpiPlain>, distribution %d, F = %d, N = %d, K = %d: G(-X) != -G(X) at %ld of %zu outputs (%ld nonzero; largest "
           "|G(-X) + G(X)| %.3e)\n", dist, F, N, K, bad, o.size(), nonzero, worst);
    hipFree(dW), hipFree(dX), hipFree(dXn), hipFree(dO), hipFree(dOn);
    return 0;
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return printf("no GPU\n"), 1;
    printf("v_mfma_f32_32x32x16_bf16 on %s (%s), seed %u: C = A B against Cn = (-A) B, 1024 outputs per K; operand distribution 0: uniform in (-1, 1), "
           "1: the same times 2^e with e uniform in -8 .. 8; rounded to bf16\n", prop.name, prop.gcnArchName, seed);
    srand(seed);
    for (int dist = 0; dist < 2; ++dist)
    for (int K : {16, 64, 256, 512, 2048}) {
        std::vector<u16> A(32 * K), An(32 * K), Bt(32 * K);
        for (int i = 0; i < 32 * K; ++i) {
            A[i] = to_bf16(draw(dist));
            An[i] = A[i] ^ 0x8000u;
            Bt[i] = to_bf16(draw(dist));
        }
        u16 *dA, *dAn, *dB;
        float *dC;
        hipMalloc(&dA, 64 * K), hipMalloc(&dAn, 64 * K), hipMalloc(&dB, 64 * K), hipMalloc(&dC, 4 * 4096);
        hipMemcpy(dA, A.data(), 64 * K, hipMemcpyHostToDevice);
        hipMemcpy(dAn, An.data(), 64 * K, hipMemcpyHostToDevice);
        hipMemcpy(dB, Bt.data(), 64 * K, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_probe, dim3(1), dim3(64), 0, 0, dA, dAn, dB, K, dC, dC + 1024, dC + 2048, dC + 3072);
        std::vector<float> out(4096);
        if (hipMemcpy(out.data(), dC, 4 * 4096, hipMemcpyDeviceToHost) != hipSuccess) return printf("HIP error\n"), 1;
        int odd_fail = 0, ctl_fail = 0, both_above = 0, both_below = 0, straddle = 0;
        float worst = 0.0f;
        for (int i = 0; i < 1024; ++i) {
            const float c = out[i], cn = out[1024 + i];
            if (out[3072 + i] != -out[2048 + i]) ++ctl_fail;
            if (cn == -c) continue;
            ++odd_fail;
            worst = fmaxf(worst, fabsf(cn + c));
            double exact = 0.0;
            for (int k = 0; k < K; ++k) exact += (double)from_bf16(A[(size_t)(i >> 5) * K + k]) * (double)from_bf16(Bt[(size_t)(i & 31) * K + k]);
            // the signed errors of the two chains: symmetric rounding gives err(C) = -err(Cn); a rounding towards one side gives the same sign
            const double e1 = (double)c - exact, e2 = (double)cn + exact;
            if (e1 > 0 && e2 > 0) ++both_above;
            else if (e1 < 0 && e2 < 0) ++both_below;
            else ++straddle;
        }
        printf("distribution %d, K = %4d: Cn != -C at %4d of 1024 outputs (largest |Cn + C| %.3e); of those, both chains above the exact value %d, both below %d, "
               "on opposite sides %d; fp32 fmaf-chain control Cn != -C at %d\n", dist, K, odd_fail, worst, both_above, both_below, straddle, ctl_fail);
        hipFree(dA), hipFree(dAn), hipFree(dB), hipFree(dC);
    }
    for (int dist = 0; dist < 2; ++dist)
        for (int K : {64, 512, 1536})
            if (gemm_probe(dist, 256, 512, K)) return 1;
    return 0;
}
