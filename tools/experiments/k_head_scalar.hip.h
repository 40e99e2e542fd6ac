// The scalar-FMA output head, measured and rejected (LSL_HEAD_MFMA=0 of -DLSL_EXPERIMENTS builds: A/B measurements against
// k_head_step_mfma, lam_slide_amd/csrc/k_small.hip.h).  Included by lsl_api.hip under LSL_EXPERIMENTS only; never in the product library.
//
// Same contract as k_head_step_mfma, through the same fragments (k_small_frag.hip.h: ln_mod, step_apply):
//   m = Linear_{D->C}(LayerNorm_{1e-6}(h) * (1 + scale) + shift)          (fp32 FMA chain, exact fp32 weights)
//   do_step: the record's update of x with m                              else: out <- m
// Persistent workgroups walk 32-token tiles.  Phase 1: each wave normalises + modulates 8 token rows into LDS (fp32).
// Phase 2: thread (token, cg) accumulates 4 consecutive output channels over D, reading the token row and the
// transposed weight slab W_s[cg][d] (float4 = 4 channels) from LDS; slabs of 32 channels are cycled for C > 32.
// LDS rows are padded (+4 floats / +1 float4) so the 8 tokens / 8 channel groups of a wave hit distinct banks.
// LDS-bandwidth bound: 5 ds_read_b128 per 16 FMAs, 82 KB of LDS reads per token.
#pragma once
#include "k_small.hip.h"

template <int NE>
constexpr size_t head_lds_bytes() { return (size_t)8 * (NE * 64 + 1) * 16 + (size_t)HEAD_TOK * (NE * 64 + 4) * 4; }

template <int NE, int VEC>
__global__ void __launch_bounds__(256) k_head_step(float *x, float *out, const float *h, const float *shift, const float *scale, int mod_stride,
                                                   const float *Wo, const float *bo, int N, int C, int tokens_per_traj, int do_step, StepUpdate u) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int D = NE * 64, AS = D + 4, WS = D + 1, RPW = HEAD_TOK / 4;  // rows per wave
    float4 *Ws = reinterpret_cast<float4 *>(smem);                    // [8][WS]
    float *As = reinterpret_cast<float *>(smem + (size_t)8 * WS * 16);  // [HEAD_TOK][AS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tk = tid >> 3, cg = tid & 7;
    const int n_tiles = (N + HEAD_TOK - 1) / HEAD_TOK;
    const bool w_resident = C <= 32;  // one 32-channel slab: fill it once per workgroup, then walk token tiles

    auto fill_w = [&](int c0) {
#pragma unroll 8
        for (int i = tid; i < 32 * D; i += 256) {
            const int cl = i / D, d = i - cl * D, c = c0 + cl;
            reinterpret_cast<float *>(&Ws[(cl >> 2) * WS + d])[cl & 3] = c < C ? Wo[(size_t)c * D + d] : 0.0f;
        }
    };
    if (w_resident) fill_w(0);

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int n0 = tile * HEAD_TOK;
        // phase 1: all of this wave's rows are requested before any reduction, so their latencies overlap
        float v[RPW][NE];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const int n = min(n0 + wave + 4 * i, N - 1);
            row_load<NE, VEC>(h + (size_t)n * D, lane, v[i]);
        }
        __syncthreads();  // previous tile's phase 2 has finished reading As (and Ws when not resident)
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const int n = min(n0 + wave + 4 * i, N - 1);
            float mean, rstd;
            row_stats<NE>(v[i], 1e-6f, mean, rstd);
            const size_t mo = (size_t)(n / tokens_per_traj) * mod_stride;
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                const int d = row_col<NE, VEC>(lane, k);
                As[(wave + 4 * i) * AS + d] = ln_mod_scale(v[i][k], mean, rstd, scale[mo + d], shift[mo + d]);
            }
        }
        const int n = n0 + tk;
        for (int c0 = 0; c0 < C; c0 += 32) {
            if (!w_resident) {
                if (c0) __syncthreads();  // previous slab fully consumed
                fill_w(c0);
            }
            __syncthreads();  // As (and Ws) visible
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            const float *ar = As + tk * AS;
            const float4 *wr = Ws + cg * WS;
#pragma unroll 2
            for (int d = 0; d < D; d += 4) {
                const float4 av = *reinterpret_cast<const float4 *>(ar + d);
                const float4 w0 = wr[d], w1 = wr[d + 1], w2 = wr[d + 2], w3 = wr[d + 3];
                a0 = fmaf(av.x, w0.x, a0); a1 = fmaf(av.x, w0.y, a1); a2 = fmaf(av.x, w0.z, a2); a3 = fmaf(av.x, w0.w, a3);
                a0 = fmaf(av.y, w1.x, a0); a1 = fmaf(av.y, w1.y, a1); a2 = fmaf(av.y, w1.z, a2); a3 = fmaf(av.y, w1.w, a3);
                a0 = fmaf(av.z, w2.x, a0); a1 = fmaf(av.z, w2.y, a1); a2 = fmaf(av.z, w2.z, a2); a3 = fmaf(av.z, w2.w, a3);
                a0 = fmaf(av.w, w3.x, a0); a1 = fmaf(av.w, w3.y, a1); a2 = fmaf(av.w, w3.z, a2); a3 = fmaf(av.w, w3.w, a3);
            }
            if (n < N) {
                const float acc[4] = {a0, a1, a2, a3};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + 4 * cg + j;
                    if (c < C) {
                        const float m = acc[j] + bo[c];
                        const size_t e = (size_t)n * C + c;
                        if (do_step) step_apply<true>(u, x, e, x[e], m);
                        else out[e] = m;
                    }
                }
            }
        }
    }
}
