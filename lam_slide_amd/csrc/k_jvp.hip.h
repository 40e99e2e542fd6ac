// The tangent pass of the network (lsl_forward_jvp, host_jvp.hip.h): out' = (d network / d x)(x) . x', forward mode, one pass beside the primal
// evaluation and reading its buffers.  DESIGN.md 6.2 has the formulas.  The tangent stream is linear operation by operation - products with
// primal values, sums in a fixed order, round-to-nearest roundings - so jvp(0) = 0, jvp(-v) = -jvp(v) and jvp(2 v) = 2 jvp(v) hold bit for
// bit; no bias enters it, and a token's (a sequence's) tangent depends on nothing outside its trajectory.  The operands of the four large
// products (linear1, linear2, the two attention products) are bf16 like their primal twins; everything else is fp32.
// The bf16 matrix instruction is the one operation here that is NOT odd in its operands: v_mfma_f32_32x32x16_bf16 does not round its
// accumulation symmetrically about zero (tools/mfma_sign_probe.hip, one run in profiles/jvp_parity.txt: (-A) B differs from -(A B) at one output in
// a few thousand for operands of similar size, at 8-27 % of them with a wide spread of exponents, and where they differ both results lie below the
// exact value or on opposite sides of it, never both above; the same product as an fp32 fmaf chain mirrors bit for bit).
// Each tangent product on it is therefore computed as (G(x') - G(-x')) / 2, G the tile GEMM: odd in x' by construction, exactly homogeneous in
// powers of two, and free of the instruction's rounding bias.  The kernels below write the negated bf16 operand beside the operand (a sign
// bit) and combine the two fp32 products where they consume them.
//   k_ln_jvp              LayerNorm JVP (+ the 1 + scale of a modulation): linear1's tangent operand, or in place (normalize models)
//   k_lin1_epilogue_jvp   raw linear1 rows of both streams -> q' | k' | v' (QK-norm JVP, RoPE, q' with the softmax pre-multiplier) and Phi'(m) m'
//   k_attention_jvp_mfma  softmax attention JVP on the matrix cores, one pass over the keys per query tile behind the row maximum
//   k_attention_jvp       the same for axes of at most 8 positions: one lane per (query, head), fp32 FMA chains
//   k_head_jvp            LayerNorm JVP . (1 + scale_f), projected by the output head's weights
//   k_dot_rows_*          lsl_dot_rows: per-trajectory fp64 dot products in a fixed order
#pragma once
#include "../../include/lsl_api.h"  // LSL_SI_SLAB
#include "common.hip.h"
#include "k_attn.hip.h"
#include "k_small.hip.h"

// ---- LayerNorm JVP of one row: with xh = (h - mean) rstd,  u' = sc1 rstd (h' - mean(h') - xh mean(xh h')),  sc1 = 1 + scale (or 1).  One wave
// per row, the row's statistics as the primal kernels compute them (row_stats).  A lane's NE values: v (primal), t (tangent, replaced by u').
template <int NE>
__device__ __forceinline__ void ln_jvp_row(const float (&v)[NE], float (&t)[NE], float eps) {
    constexpr float invD = 1.0f / (float)(NE * 64);
    float mean, rstd;
    row_stats<NE>(v, eps, mean, rstd);
    float xh[NE], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        xh[k] = (v[k] - mean) * rstd;
        s1 += t[k];
        s2 = fmaf(xh[k], t[k], s2);
    }
    const float m1 = wave_sum(s1) * invD, m2 = wave_sum(s2) * invD;
#pragma unroll
    for (int k = 0; k < NE; ++k) t[k] = rstd * ((t[k] - m1) - xh[k] * m2);
}

// TO_BF16: out = bf16 [N][D], the tangent operand of linear1 (scale: the sub-block's modulation rows).  Otherwise out = fp32 [N][D], which may
// be ht itself (the in-place LayerNorm of normalize models: scale == nullptr, eps 1e-5; h still holds the rows in front of the LayerNorm).
// (TO_BF16: out_neg receives the negated operand)
template <int NE, int VEC, bool TO_BF16>
__global__ void __launch_bounds__(256) k_ln_jvp(void *out, u16 *out_neg, const float *h, const float *ht, const float *scale, int mod_stride, int N,
                                                int tokens_per_traj, float eps) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    constexpr int D = NE * 64;
    float v[NE], t[NE];
    row_load<NE, VEC>(h + (size_t)n * D, lane, v);
    row_load<NE, VEC>(ht + (size_t)n * D, lane, t);
    ln_jvp_row<NE>(v, t, eps);
    const size_t mo = (size_t)(n / tokens_per_traj) * mod_stride;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int d = row_col<NE, VEC>(lane, k);
        const float u = scale ? t[k] * (1.0f + scale[mo + d]) : t[k];
        if (TO_BF16) {
            const u16 b = f2bf(u);
            reinterpret_cast<u16 *>(out)[(size_t)n * D + d] = b;
            out_neg[(size_t)n * D + d] = b ^ 0x8000u;
        } else
            reinterpret_cast<float *>(out)[(size_t)n * D + d] = u;
    }
}

// ---- the output head's tangent: out'[n][c] = sum_d Wo[c][d] (LayerNorm-JVP(h, h')[d] (1 + scale_f[d])), fp32; one wave per token, a channel's
// products added lane-locally in k order, then across the wave (wave_sum).
template <int NE, int VEC>
__global__ void __launch_bounds__(256) k_head_jvp(float *out_t, const float *h, const float *ht, const float *scale, int mod_stride,
                                                  const float *Wo, int N, int C, int tokens_per_traj) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    constexpr int D = NE * 64;
    float v[NE], t[NE];
    row_load<NE, VEC>(h + (size_t)n * D, lane, v);
    row_load<NE, VEC>(ht + (size_t)n * D, lane, t);
    ln_jvp_row<NE>(v, t, 1e-6f);
    const size_t mo = (size_t)(n / tokens_per_traj) * mod_stride;
#pragma unroll
    for (int k = 0; k < NE; ++k) t[k] *= 1.0f + scale[mo + row_col<NE, VEC>(lane, k)];
    for (int c = 0; c < C; ++c) {
        const float *w = Wo + (size_t)c * D;
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < NE; ++k) s = fmaf(w[row_col<NE, VEC>(lane, k)], t[k], s);
        s = wave_sum(s);
        if (lane == 0) out_t[(size_t)n * C + c] = s;
    }
}

// ---- behind the raw linear1 products (EpiPlain, k_gemm.hip.h): raw = W1 a + b1 (primal), rawt = G(a'), rawn = G(-a') (the tangent product is
// (rawt - rawn) / 2, see the top of the file), fp32 [N][F1], features
// (q heads | k heads | v heads | mlp), heads padded to HDP.  One thread per (token, unit): a q or k head -
//      r = rsqrt(mean(x^2) + 1e-6), xh = x r,  y' = s (.) r (x' - xh mean(xh x'))       (means over the true head_dim; the padding is zero)
//      rotated by the position's RoPE pair rotations, q' times hd^-1/2 log2 e like q
// - or 8 features of v' (taken as they are) | Phi'(m) m', Phi'(m) = (1 + erf(m / sqrt 2)) / 2 + m exp(-m^2 / 2) / sqrt(2 pi).
// Out: qkvt bf16 [N][3 HHD] in the layout of the primal q | k | v rows, and the mlp half of zt bf16 [N][K2] with its negation in ztn.
struct Lin1JvpArgs {
    const float *raw, *rawt, *rawn;
    const float *qs, *ks;  // [HDP]
    const float2 *rope;    // [n_pos][HDP / 2] (cos, sin)
    u16 *qkvt, *zt, *ztn;
    int N, H, HHD, M;
    int pos_div, pos_mod;  // position of token n inside its sequence: (n / pos_div) % pos_mod
    float inv_hd, premul;
};
template <int HDP>
__global__ void __launch_bounds__(256) k_lin1_epilogue_jvp(Lin1JvpArgs a) {
    const int units = 2 * a.H + (a.HHD + a.M) / 8, F1 = 3 * a.HHD + a.M, K2 = a.HHD + a.M;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.N * units) return;
    const int n = (int)(idx / units), u = (int)(idx % units);
    const float *xr = a.raw + (size_t)n * F1, *tr = a.rawt + (size_t)n * F1, *nr = a.rawn + (size_t)n * F1;
    if (u < 2 * a.H) {
        const int sec = u / a.H, head = u % a.H, f0 = sec * a.HHD + head * HDP;
        float x[HDP], t[HDP];
#pragma unroll
        for (int c = 0; c < HDP / 4; ++c) {
            const float4 xv = *reinterpret_cast<const float4 *>(xr + f0 + 4 * c), tv = *reinterpret_cast<const float4 *>(tr + f0 + 4 * c);
            const float4 nv = *reinterpret_cast<const float4 *>(nr + f0 + 4 * c);
            x[4 * c] = xv.x; x[4 * c + 1] = xv.y; x[4 * c + 2] = xv.z; x[4 * c + 3] = xv.w;
            t[4 * c] = 0.5f * (tv.x - nv.x); t[4 * c + 1] = 0.5f * (tv.y - nv.y); t[4 * c + 2] = 0.5f * (tv.z - nv.z); t[4 * c + 3] = 0.5f * (tv.w - nv.w);
        }
        float ss = 0.0f;
#pragma unroll
        for (int d = 0; d < HDP; ++d) ss = fmaf(x[d], x[d], ss);
        const float r = rsqrtf(fmaf(ss, a.inv_hd, 1e-6f));
        float dot = 0.0f;
#pragma unroll
        for (int d = 0; d < HDP; ++d) {
            x[d] *= r;
            dot = fmaf(x[d], t[d], dot);
        }
        const float mean = dot * a.inv_hd, post = sec == 0 ? a.premul : 1.0f;
        const float *sc = sec == 0 ? a.qs : a.ks;
        const float2 *rope = a.rope + (size_t)((n / a.pos_div) % a.pos_mod) * (HDP / 2);
        u16 *dst = a.qkvt + (size_t)n * (3 * a.HHD) + f0;
#pragma unroll
        for (int c = 0; c < HDP / 8; ++c) {
            float o[8];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int d = 8 * c + 2 * p;
                const float y0 = sc[d] * (r * (t[d] - x[d] * mean)), y1 = sc[d + 1] * (r * (t[d + 1] - x[d + 1] * mean));
                const float2 cs = rope[d >> 1];
                o[2 * p] = post * fmaf(cs.x, y0, -(cs.y * y1));
                o[2 * p + 1] = post * fmaf(cs.y, y0, cs.x * y1);
            }
            const u32x4 w = {pack2(o[0], o[1]), pack2(o[2], o[3]), pack2(o[4], o[5]), pack2(o[6], o[7])};
            *reinterpret_cast<u32x4 *>(dst + 8 * c) = w;
        }
        return;
    }
    const int f = (u - 2 * a.H) * 8;  // of v | mlp
    float o[8];
    if (f < a.HHD) {
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = 0.5f * (tr[2 * a.HHD + f + k] - nr[2 * a.HHD + f + k]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float m = xr[2 * a.HHD + f + k], mt = 0.5f * (tr[2 * a.HHD + f + k] - nr[2 * a.HHD + f + k]);
            const float dphi = fmaf(m * 0.3989422804014327f, __expf(-0.5f * m * m), 0.5f * (1.0f + erff(m * 0.70710678118654752440f)));
            o[k] = dphi * mt;
        }
    }
    const u32x4 w = {pack2(o[0], o[1]), pack2(o[2], o[3]), pack2(o[4], o[5]), pack2(o[6], o[7])};
    u16 *dst = f < a.HHD ? a.qkvt + (size_t)n * (3 * a.HHD) + 2 * a.HHD + f : a.zt + (size_t)n * K2 + f;
    *reinterpret_cast<u32x4 *>(dst) = w;
    if (f >= a.HHD) *reinterpret_cast<u32x4 *>(a.ztn + (size_t)n * K2 + f) = w ^ 0x80008000u;
}

// ---- softmax attention JVP.  The primal q | k | v are the very bf16 rows the primal attention read (q pre-multiplied by hd^-1/2 log2 e, so a
// score in base-2 units is s_j = q . k_j); q' carries the same factor, so s'_j = ln 2 (q' . k_j + q . k'_j).  Per query row, behind the row
// maximum m (a first pass over the keys):
//      e_j = exp2(s_j - m),  l = sum e,  O = sum e v,  AB = sum e (v' + s' v),  c = sum e s',      o' = AB / l - (c / l) (O / l)
// This kernel: axes of at most 8 positions (the host's rule; it is correct at any length), where a 32 x 32 tile would be mostly padding.
// Keys in position order, every sum an fp32 fma chain, the probabilities kept in fp32.  One lane per (query token, head), lanes ordered
// (token, head): a wave reads whole token rows, and the rows of a sequence's keys come from L1 / L2.  An axis of one position gives o' = v'.
struct AttnJvpArgs {
    const u16 *qkv, *qkvt;  // [N][3 HHD] bf16
    u16 *zt, *ztn;          // [N][zw] bf16, columns [0, HHD): o' and its negation
    int HHD, zw, H, S, n_seq;
    int inner, outer_stride, pos_stride;  // token of (seq, pos) = (seq / inner) * outer_stride + (seq % inner) + pos * pos_stride
};
template <int HDP>
__device__ __forceinline__ float dot_row(const float (&q)[HDP], const u16 *row) {
    float d = 0.0f;
#pragma unroll
    for (int c = 0; c < HDP / 8; ++c) {
        const u32x4 w = *reinterpret_cast<const u32x4 *>(row + 8 * c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d = fmaf(q[8 * c + 2 * k], bf_lo(w[k]), d);
            d = fmaf(q[8 * c + 2 * k + 1], bf_hi(w[k]), d);
        }
    }
    return d;
}
template <int HDP>
__global__ void __launch_bounds__(256) k_attention_jvp(AttnJvpArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int S = a.S;
    if (idx >= (long)a.n_seq * S * a.H) return;
    const int head = (int)(idx % a.H);
    const long qi = idx / a.H;
    const int seq = (int)(qi / S), pos = (int)(qi % S);
    const size_t tok0 = (size_t)(seq / a.inner) * a.outer_stride + (seq % a.inner);
    const size_t rs = (size_t)3 * a.HHD, ps = (size_t)a.pos_stride * rs;
    const u16 *base = a.qkv + tok0 * rs + head * HDP, *baset = a.qkvt + tok0 * rs + head * HDP;
    float q[HDP], qt[HDP];
    row_unpack<HDP>(base + (size_t)pos * ps, q);
    row_unpack<HDP>(baset + (size_t)pos * ps, qt);
    float mx = -INFINITY;
    for (int j = 0; j < S; ++j) mx = fmaxf(mx, dot_row<HDP>(q, base + a.HHD + (size_t)j * ps));
    float o[HDP], ab[HDP], l = 0.0f, cs = 0.0f;
#pragma unroll
    for (int d = 0; d < HDP; ++d) o[d] = ab[d] = 0.0f;
    for (int j = 0; j < S; ++j) {
        const u16 *krow = base + a.HHD + (size_t)j * ps, *ktrow = baset + a.HHD + (size_t)j * ps;
        const float e = __builtin_amdgcn_exp2f(dot_row<HDP>(q, krow) - mx);
        const float st = 0.6931471805599453f * (dot_row<HDP>(qt, krow) + dot_row<HDP>(q, ktrow));
        l += e;
        cs = fmaf(e, st, cs);
#pragma unroll
        for (int c = 0; c < HDP / 8; ++c) {
            float vf[8], vt[8];
            unpack8(*reinterpret_cast<const u32x4 *>(krow + a.HHD + 8 * c), vf);
            unpack8(*reinterpret_cast<const u32x4 *>(ktrow + a.HHD + 8 * c), vt);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                o[8 * c + k] = fmaf(e, vf[k], o[8 * c + k]);
                ab[8 * c + k] = fmaf(e, fmaf(st, vf[k], vt[k]), ab[8 * c + k]);
            }
        }
    }
    const float inv = 1.0f / l, cl = cs * inv;
#pragma unroll
    for (int d = 0; d < HDP; ++d) ab[d] = ab[d] * inv - cl * (o[d] * inv);
    const size_t zo = (tok0 + (size_t)pos * a.pos_stride) * a.zw + head * HDP;
    row_pack<HDP>(a.zt + zo, ab, 1.0f);
    row_pack<HDP>(a.ztn + zo, ab, -1.0f);
}

// ---- the same on the matrix cores, for axes of more than 8 positions: one wave per (sequence, head, tile of 32 queries), 32 keys per step.
//      St = K Q^T (A = K rows, B = Q rows: 16-byte row reads straight from global memory, no staging) leaves lane (q = l & 31, hf) with the
//      scores of query q against keys acc_row(e, hf); Ot = V^T P^T takes P from those registers in place (p_frag's key order) and V^T by eight
//      2-byte reads per k-step (lanes = channels: 64 contiguous bytes per key).  Two passes over the keys: the row maximum, then the sums.
// Every tangent product is paired (top of the file): S' from (K Q'^T + K' Q^T) and (K (-Q')^T + (-K') Q^T), AB from (V'^T P^T + V^T (P S')^T) and
// ((-V')^T P^T + V^T (-(P S'))^T); P and P S' are rounded to bf16 as the primal kernels round P.  16-wide heads use rows 0 .. 15 of the output tile.
__device__ __forceinline__ bf16x8 neg_bf16x8(bf16x8 v) { return as_bf16x8(as_u32x4(v) ^ 0x80008000u); }
__device__ __forceinline__ bf16x8 pack_bf16x8(const float *a, const float *b) {
    return as_bf16x8(u32x4{pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(b[0], b[1]), pack2(b[2], b[3])});
}
template <int HDP>
__global__ void __launch_bounds__(256) k_attention_jvp_mfma(AttnJvpArgs a) {
    constexpr int KS = HDP / 16;
    const int lane = threadIdx.x & 63, r = lane & 31, hf = lane >> 5;
    const int S = a.S, nqt = (S + 31) >> 5;
    const long unit = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= (long)a.n_seq * a.H * nqt) return;  // (wave-uniform)
    const int qt = (int)(unit % nqt), head = (int)((unit / nqt) % a.H), seq = (int)(unit / ((long)nqt * a.H));
    const size_t tok0 = (size_t)(seq / a.inner) * a.outer_stride + (seq % a.inner);
    const size_t rs = (size_t)3 * a.HHD, ps = (size_t)a.pos_stride * rs;
    const u16 *base = a.qkv + tok0 * rs + head * HDP, *baset = a.qkvt + tok0 * rs + head * HDP;
    const int qpos = min(qt * 32 + r, S - 1);
    bf16x8 qf[KS], qtf[KS], qtn[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = as_bf16x8(*reinterpret_cast<const u32x4 *>(base + (size_t)qpos * ps + 16 * ks + 8 * hf));
        qtf[ks] = as_bf16x8(*reinterpret_cast<const u32x4 *>(baset + (size_t)qpos * ps + 16 * ks + 8 * hf));
        qtn[ks] = neg_bf16x8(qtf[ks]);
    }
    const int nkt = nqt;
    float mx = -INFINITY;
    for (int kt = 0; kt < nkt; ++kt) {
        const size_t krow = (size_t)min(kt * 32 + r, S - 1) * ps + a.HHD;
        f32x16 sc = f32x16_zero();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) sc = mfma32(as_bf16x8(*reinterpret_cast<const u32x4 *>(base + krow + 16 * ks + 8 * hf)), qf[ks], sc);
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (kt * 32 + acc_row(e, hf) < S) mx = fmaxf(mx, sc[e]);
    }
    mx = fmaxf(mx, xhalf(mx));
    f32x16 o = f32x16_zero(), abp = f32x16_zero(), abn = f32x16_zero();
    float l = 0.0f, cs = 0.0f;
    const bool chan = r < HDP;  // (16-wide heads: lanes r >= 16 supply zero rows of V^T)
    for (int kt = 0; kt < nkt; ++kt) {
        const size_t krow = (size_t)min(kt * 32 + r, S - 1) * ps + a.HHD;
        f32x16 sc = f32x16_zero(), sp = f32x16_zero(), sn = f32x16_zero();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 kf = as_bf16x8(*reinterpret_cast<const u32x4 *>(base + krow + 16 * ks + 8 * hf));
            const bf16x8 ktf = as_bf16x8(*reinterpret_cast<const u32x4 *>(baset + krow + 16 * ks + 8 * hf));
            sc = mfma32(kf, qf[ks], sc);
            sp = mfma32(kf, qtf[ks], sp);
            sp = mfma32(ktf, qf[ks], sp);
            sn = mfma32(kf, qtn[ks], sn);
            sn = mfma32(neg_bf16x8(ktf), qf[ks], sn);
        }
        float p[16], pst[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const bool valid = kt * 32 + acc_row(e, hf) < S;
            p[e] = valid ? __builtin_amdgcn_exp2f(sc[e] - mx) : 0.0f;
            const float st = 0.6931471805599453f * (0.5f * (sp[e] - sn[e]));
            pst[e] = p[e] * st;
            l += p[e];
            cs = fmaf(p[e], st, cs);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 pf = pack_bf16x8(p + 8 * s, p + 8 * s + 4), psf = pack_bf16x8(pst + 8 * s, pst + 8 * s + 4);
            u16 vv[8], vt[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const size_t vrow = (size_t)min(kt * 32 + 16 * s + 8 * (j >> 2) + 4 * hf + (j & 3), S - 1) * ps + 2 * a.HHD + (chan ? r : 0);
                vv[j] = chan ? base[vrow] : (u16)0;
                vt[j] = chan ? baset[vrow] : (u16)0;
            }
            const bf16x8 vf = as_bf16x8(u32x4{vv[0] | ((unsigned)vv[1] << 16), vv[2] | ((unsigned)vv[3] << 16), vv[4] | ((unsigned)vv[5] << 16), vv[6] | ((unsigned)vv[7] << 16)});
            const bf16x8 vtf = as_bf16x8(u32x4{vt[0] | ((unsigned)vt[1] << 16), vt[2] | ((unsigned)vt[3] << 16), vt[4] | ((unsigned)vt[5] << 16), vt[6] | ((unsigned)vt[7] << 16)});
            o = mfma32(vf, pf, o);
            abp = mfma32(vtf, pf, abp);
            abp = mfma32(vf, psf, abp);
            abn = mfma32(neg_bf16x8(vtf), pf, abn);
            abn = mfma32(vf, neg_bf16x8(psf), abn);
        }
    }
    l += xhalf(l);
    cs += xhalf(cs);
    if (qt * 32 + r >= S) return;
    const float inv = 1.0f / l, cl = cs * inv;
    const size_t zo = (tok0 + (size_t)qpos * a.pos_stride) * a.zw + head * HDP;
#pragma unroll
    for (int g = 0; g < HDP / 8; ++g) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (0.5f * (abp[4 * g + k] - abn[4 * g + k])) * inv - cl * (o[4 * g + k] * inv);
        const u32x2 w = {pack2(v[0], v[1]), pack2(v[2], v[3])};
        *reinterpret_cast<u32x2 *>(a.zt + zo + 8 * g + 4 * hf) = w;
        *reinterpret_cast<u32x2 *>(a.ztn + zo + 8 * g + 4 * hf) = w ^ 0x80008000u;
    }
}

// ---- behind the two raw linear2 products up = G(z'), un = G(-z') (fp32 [N][D]): h' += gate (.) (up - un) / 2, gate rows by trajectory
__global__ void __launch_bounds__(256) k_gate_update_jvp(float *ht, const float *up, const float *un, const float *gate, int mod_stride, int N, int D,
                                                         int tokens_per_traj) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;  // one float4 each
    const int q = D / 4;
    if (i >= (long)N * q) return;
    const int n = (int)(i / q), f = (int)(i % q) * 4;
    const float4 a = *reinterpret_cast<const float4 *>(up + (size_t)n * D + f), b = *reinterpret_cast<const float4 *>(un + (size_t)n * D + f);
    const float4 g = *reinterpret_cast<const float4 *>(gate + (size_t)(n / tokens_per_traj) * mod_stride + f);
    float4 h = *reinterpret_cast<float4 *>(ht + (size_t)n * D + f);
    h.x = fmaf(g.x, 0.5f * (a.x - b.x), h.x);
    h.y = fmaf(g.y, 0.5f * (a.y - b.y), h.y);
    h.z = fmaf(g.z, 0.5f * (a.z - b.z), h.z);
    h.w = fmaf(g.w, 0.5f * (a.w - b.w), h.w);
    *reinterpret_cast<float4 *>(ht + (size_t)n * D + f) = h;
}

// ---- lsl_dot_rows: out[b] = sum_e a[b][e] b[b][e] in fp64 from the exact products of the fp32 values.  A trajectory is cut into slabs of
// LSL_SI_SLAB elements (4096, a constant of the header); inside a slab thread i adds elements i + 256 j in j order and the 256 threads' sums go through the
// halving tree; a trajectory's slabs are added in slab order.  No atomics: a trajectory's bits are the same in any batch.
// The two fragments (k_dopri5.hip.h's k_dp_dot / k_dp_klogp run the same ones): slab blockIdx.x of trajectory blockIdx.y by a 256-thread
// workgroup, and a trajectory's slab partials in slab order
__device__ __forceinline__ void dot_rows_slab(double *red, double *partial, const float *a, const float *b, unsigned long long per) {
    const unsigned long long base = (unsigned long long)blockIdx.y * per, e0 = (unsigned long long)blockIdx.x * LSL_SI_SLAB;
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < LSL_SI_SLAB / 256; ++j) {
        const unsigned long long e = e0 + threadIdx.x + 256u * j;
        if (e < per) s += (double)a[base + e] * (double)b[base + e];
    }
    s = block_tree_sum(red, s);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}
__device__ __forceinline__ double dot_rows_total(const double *partial, int b, int slabs) {
    double s = 0.0;
    for (int k = 0; k < slabs; ++k) s += partial[(size_t)b * slabs + k];
    return s;
}
__global__ void __launch_bounds__(256) k_dot_rows_partial(double *partial, const float *a, const float *b, unsigned long long per) {
    __shared__ double red[256];
    dot_rows_slab(red, partial, a, b, per);
}
// (one thread per trajectory adds its slab partials serially - the documented order.  A likelihood state has a few hundred slabs at most
// (peptide: 375); the 2^19 slabs of the largest trajectory the entry point admits would be a long serial chain.)
__global__ void k_dot_rows_final(double *out, const double *partial, int B, int slabs) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double s = dot_rows_total(partial, b, slabs);
    out[b] = s;
}
