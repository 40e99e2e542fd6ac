// The tangent pass of the network (lsl_forward_jvp; kernels: k_jvp.hip.h): out' = (d network / d x)(x) . x' beside one primal
// evaluation.  The primal half IS the evaluation (run_eval of host_eval.hip.h, launch for launch, on the default decomposition of the general
// path); the tangent launches ride on it through EvalTangent and read its buffers before the primal overwrites them.  The scratch of the tangent
// stream lies behind the forward's scratch in the caller's workspace; a tangent pass holds half as many tokens as a forward pass.
#pragma once
#include "host_eval.hip.h"

namespace {

// Scratch of the tangent stream for a pass over `bc` trajectories
struct JvpWorkspace {
    float *ht;          // [npad][D]    tangent of the residual stream
    // (a tangent product on the bf16 matrix instruction is (G(x') - G(-x')) / 2 - k_jvp.hip.h says why - hence the pairs)
    u16 *at, *atn;      // [npad][D]    linear1's tangent operand a', and -a'
    float *raw, *rawt, *rawn;  // [n][F1]  raw linear1 rows: primal (with the bias), G(a'), G(-a')
    u16 *qkvt;          // [npad][3 HHD] q' | k' | v' in the layout of the primal rows
    u16 *zt, *ztn;      // [npad][K2]   linear2's tangent operand z', and -z'
    float *up, *un;     // [n][D]       raw linear2 rows G(z'), G(-z')
    u16 *qkv_rows;      // [npad][3 HHD] the primal q | k | v as token-major rows, where the plan left them as head-major planes
    size_t bytes;
};
JvpWorkspace carve_jvp(const lsl_model *m, char *base, int bc, int T, int L) {
    const size_t n = (size_t)bc * T * L, n_pad = align_up(n, 256), D = m->d.hidden;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align_up(bytes, 256);
        return p;
    };
    JvpWorkspace w;
    w.ht = (float *)take(n_pad * D * 4);
    w.at = (u16 *)take(n_pad * D * 2);  // (GEMM operand rows: whole 256-token tiles are read without clamping)
    w.atn = (u16 *)take(n_pad * D * 2);
    w.raw = (float *)take(n * m->F1 * 4);
    w.rawt = (float *)take(n * m->F1 * 4);
    w.rawn = (float *)take(n * m->F1 * 4);
    w.qkvt = (u16 *)take(n_pad * 3 * m->HHD * 2);
    w.zt = (u16 *)take(n_pad * m->K2 * 2);
    w.ztn = (u16 *)take(n_pad * m->K2 * 2);
    w.up = (float *)take(n * D * 4);
    w.un = (float *)take(n * D * 4);
    w.qkv_rows = (u16 *)take(n_pad * 3 * m->HHD * 2);
    w.bytes = off;
    return w;
}

// Trajectories per tangent pass: the handle's pass size (lsl_model_set_chunk), then LSL_CHUNK_TRAJ - as default_chunk -, else at most 128 Ki tokens in equal passes - half a forward
// pass, for about three times its scratch per token.  A trajectory's bits do not depend on it.
int jvp_chunk(const lsl_model *m, int B, int T, int L) {
    if (m->chunk > 0) return m->chunk < B ? m->chunk : B;
    if (const char *e = getenv("LSL_CHUNK_TRAJ")) {
        const int v = atoi(e);
        if (v > 0) return v < B ? v : B;
    }
    size_t c = (size_t)131072 / ((size_t)T * L);
    if (c < 1) c = 1;
    if (c > (size_t)B) c = B;
    const size_t passes = ((size_t)B + c - 1) / c;
    return (int)(((size_t)B + passes - 1) / passes);
}
size_t jvp_workspace_need(const lsl_model *m, int B, int T, int L, int *chunk_out = nullptr) {
    const int chunk = jvp_chunk(m, B, T, L);
    if (chunk_out) *chunk_out = chunk;
    return align_up(carve(m, nullptr, chunk, T, L).bytes, 256) + carve_jvp(m, nullptr, chunk, T, L).bytes;
}

template <int NE, int VEC>
void launch_ln_jvp_bf16(u16 *out, u16 *out_neg, const float *h, const float *ht, const float *scale, int stride, int n, int tpt, hipStream_t st) {
    hipLaunchKernelGGL((k_ln_jvp<NE, VEC, true>), dim3((n + 3) / 4), dim3(256), 0, st, (void *)out, out_neg, h, ht, scale, stride, n, tpt, 1e-6f);
}
template <int NE, int VEC>
void launch_ln_jvp_f32(float *out, const float *h, const float *ht, int n, float eps, hipStream_t st) {
    hipLaunchKernelGGL((k_ln_jvp<NE, VEC, false>), dim3((n + 3) / 4), dim3(256), 0, st, (void *)out, (u16 *)nullptr, h, ht, (const float *)nullptr, 0, n, 1, eps);
}
template <int NE, int VEC>
void launch_head_jvp(float *out_t, const float *h, const float *ht, const float *scale, int stride, const float *Wo, int n, int C, int tpt, hipStream_t st) {
    hipLaunchKernelGGL((k_head_jvp<NE, VEC>), dim3((n + 3) / 4), dim3(256), 0, st, out_t, h, ht, scale, stride, Wo, n, C, tpt);
}

// The tile GEMM with the plain epilogue, on a tiling gemm_variant names for linear1 (every tiling sums k in the same order)
void launch_gemm_plain(int variant, const u16 *W, const u16 *X, int F, int N, int K, const EpiPlain &e, hipStream_t st) {
    const GemmArgs g{W, X, F, N, K, 0, 0};
    if (variant == 12 && K % 128 == 0) return launch_gemm_glds<256, 256, 2, 4, 64, 2, true>(g, e, st);
    switch (variant) {
        case 10: return launch_gemm_glds<128, 128, 2, 2, 32, 3, false>(g, e, st);
        case 11: return launch_gemm_glds<128, 128, 2, 2, 64, 2, false>(g, e, st);
        default: return launch_gemm_glds<256, 256, 2, 4, 64, 2, false>(g, e, st);
    }
}

// The tangent launches of one evaluation for a pass (EvalTangent: where they stand between the primal launches)
struct JvpPass : EvalTangent {
    lsl_model *m;
    const Workspace &ws;
    const JvpWorkspace &jw;
    const PassPlan &p;
    const float *xt;  // [n][C] tangent of the state
    float *out_t;     // [n][C]
    hipStream_t st;
    JvpPass(lsl_model *m, const Workspace &ws, const JvpWorkspace &jw, const PassPlan &p, const float *xt, float *out_t, hipStream_t st)
        : m(m), ws(ws), jw(jw), p(p), xt(xt), out_t(out_t), st(st) {}

    // h' = W_x x' (no bias, no conditioning rows: their tangents are zero); normalize models: the LayerNorm JVP from the rows in front of it
    int embedded() override {
        const lsl_model_desc &d = m->d;
        hipMemsetAsync(jw.ht, 0, (size_t)p.n * d.hidden * 4, st);  // (the embedding kernels add a base row: zeros)
        launch_embed<1>(jw.ht, xt, m->w.x_in_w, nullptr, nullptr, nullptr, nullptr, jw.ht, p.n, d.in_dim, d.hidden, st);
        if (d.normalize) { DISPATCH_D(d.hidden, launch_ln_jvp_f32, jw.ht, ws.h, jw.ht, p.n, 1e-5f, st); }
        LSL_CHECK_LAUNCH("embed (tangent)");
        return 0;
    }
    // a' (must read h before this sub-block's linear2 updates it), then the raw linear1 rows of both streams
    int normed(int bi, const float *mbase) override {
        const lsl_model_desc &d = m->d;
        const lsl_block_weights &bw = m->blocks[bi];
        const int D = d.hidden;
        DISPATCH_D(D, launch_ln_jvp_bf16, jw.at, jw.atn, ws.h, jw.ht, mbase + D, p.mod_stride, p.n, p.T * p.L, st);
        const int variant = gemm_variant(false, m->F1, D, p.n);
        launch_gemm_plain(variant, (const u16 *)bw.w1, ws.a, m->F1, p.n, D, EpiPlain{bw.b1, jw.raw, m->F1, 0}, st);
        launch_gemm_plain(variant, (const u16 *)bw.w1, jw.at, m->F1, p.n, D, EpiPlain{nullptr, jw.rawt, m->F1, 0}, st);
        launch_gemm_plain(variant, (const u16 *)bw.w1, jw.atn, m->F1, p.n, D, EpiPlain{nullptr, jw.rawn, m->F1, 0}, st);
        LSL_CHECK_LAUNCH("linear1 (tangent)");
        return 0;
    }
    // q' | k' | v' and the mlp half of z', the attention half of z', then h' += gate (.) (W2 z')
    int attended(int bi, const float *mbase, float premul, int pdiv, int pmod) override {
        const lsl_model_desc &d = m->d;
        const lsl_block_weights &bw = m->blocks[bi];
        const int D = d.hidden, n = p.n, temporal = bi & 1, H = d.heads;
        const Lin1JvpArgs la{jw.raw, jw.rawt, jw.rawn, bw.qs, bw.ks, temporal ? ws.rope_t : ws.rope_l, jw.qkvt, jw.zt, jw.ztn, n, H, m->HHD, d.mlp_dim,
                             pdiv, pmod, 1.0f / d.head_dim, premul};
        const long units = (long)n * (2 * H + m->K2 / 8);
        const dim3 eg((unsigned)((units + 255) / 256));
        if (d.head_dim_pad == 32) hipLaunchKernelGGL(k_lin1_epilogue_jvp<32>, eg, dim3(256), 0, st, la);
        else hipLaunchKernelGGL(k_lin1_epilogue_jvp<16>, eg, dim3(256), 0, st, la);
        const u16 *qkv = ws.qkv;
        if (p.planes[temporal]) {  // the primal attention read head-major planes: the same values as token-major rows
            const long chunks = (long)n * 3 * H * (d.head_dim_pad / 8);
            hipLaunchKernelGGL(k_planes_to_rows, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, jw.qkv_rows, (const u16 *)ws.qkv, n, p.npad, 3 * H,
                               d.head_dim_pad);
            qkv = jw.qkv_rows;
        }
        AttnJvpArgs aa{qkv, jw.qkvt, jw.zt, jw.ztn, m->HHD, m->K2, H, 0, 0, 0, 0, 0};
        if (!temporal) {  // sequences (b, t), positions l
            aa.S = p.L; aa.n_seq = p.bc * p.T; aa.inner = 1; aa.outer_stride = p.L; aa.pos_stride = 1;
        } else {          // sequences (b, l), positions t
            aa.S = p.T; aa.n_seq = p.bc * p.L; aa.inner = p.L; aa.outer_stride = p.T * p.L; aa.pos_stride = p.L;
        }
        if (aa.S > 8) {  // the matrix-core form: a wave per (sequence, head, 32 queries).  The choice depends on the axis alone, never on the batch
            const long units = (long)aa.n_seq * H * ((aa.S + 31) / 32);
            const dim3 mg((unsigned)((units + 3) / 4));
            if (d.head_dim_pad == 32) hipLaunchKernelGGL(k_attention_jvp_mfma<32>, mg, dim3(256), 0, st, aa);
            else hipLaunchKernelGGL(k_attention_jvp_mfma<16>, mg, dim3(256), 0, st, aa);
        } else {  // tiny axes (a 32 x 32 tile would be >= 75 % padding): one lane per (query, head)
            const dim3 ag((unsigned)(((long)n * H + 255) / 256));
            if (d.head_dim_pad == 32) hipLaunchKernelGGL(k_attention_jvp<32>, ag, dim3(256), 0, st, aa);
            else hipLaunchKernelGGL(k_attention_jvp<16>, ag, dim3(256), 0, st, aa);
        }
        const int variant = gemm_variant(false, D, m->K2, n);
        launch_gemm_plain(variant, (const u16 *)bw.w2, jw.zt, D, n, m->K2, EpiPlain{nullptr, jw.up, D, 0}, st);
        launch_gemm_plain(variant, (const u16 *)bw.w2, jw.ztn, D, n, m->K2, EpiPlain{nullptr, jw.un, D, 0}, st);
        hipLaunchKernelGGL(k_gate_update_jvp, dim3((unsigned)(((long)n * (D / 4) + 255) / 256)), dim3(256), 0, st, jw.ht, (const float *)jw.up, (const float *)jw.un,
                           mbase + 2 * D, p.mod_stride, n, D, p.T * p.L);
        LSL_CHECK_LAUNCH("block (tangent)");
        return 0;
    }
    int head(const float *fm) override {
        const lsl_model_desc &d = m->d;
        DISPATCH_D(d.hidden, launch_head_jvp, out_t, ws.h, jw.ht, fm + d.hidden, p.mod_stride, m->w.out_w, p.n, d.in_dim, p.T * p.L, st);
        LSL_CHECK_LAUNCH("head (tangent)");
        return 0;
    }
};

// Argument checks of lsl_forward_jvp in the order the header documents; no device call in front of the first refusal
int check_jvp(const lsl_model *m, const lsl_io *io, const float *x_tangent, const float *out_tangent, const void *ws, size_t ws_bytes, int *chunk_out) {
    if (!m || !io || !x_tangent || !out_tangent) return fail(-1, "null model, io or tangent");
    if (io->B <= 0 || io->T <= 0 || io->L <= 0) return fail(-3, "B, T, L must be positive");
    if ((size_t)io->T * io->L > (1u << 24)) return fail(-3, "T*L too large");
    if (m->attention_linear) return fail(-21, "lsl_forward_jvp differentiates softmax attention only: call lsl_model_set_attention_mode(m, 0)");
    if (m->tail) return fail(-21, "lsl_forward_jvp runs the default decomposition: call lsl_model_set_tail(m, 0)");
    if (m->ln_fuse) return fail(-21, "lsl_forward_jvp runs the default decomposition: call lsl_model_set_ln_fuse(m, 0)");
    const size_t need = jvp_workspace_need(m, io->B, io->T, io->L, chunk_out);
    if (!ws || ws_bytes < need) return fail(-3, "workspace too small: need %zu bytes, got %zu", need, ws_bytes);
    if (!m->has_weights) return fail(-2, "weights not set");
    if (!io->x || !io->x_cond || !io->mask || !io->t || !io->out) return fail(-3, "x, x_cond, mask, t and out are required");
    if (io->y != nullptr && m->d.vec_in_dim <= 0) return fail(-3, "y given but the model has no vec_in");
    return 0;
}

// The passes of one tangent evaluation (lsl_forward_jvp, every evaluation of lsl_dopri_logp_*): io->out = network(io->x, io->t, ...),
// out_tangent = its Jacobian in x applied to x_tangent
int jvp_passes(lsl_model *m, const lsl_io *io, const Workspace &ws, const JvpWorkspace &jw, const CallPlans &plans, int chunk, const float *x_tangent,
               float *out_tangent, hipStream_t st) {
    run_tables(m, ws, io->T, io->L, st);
    return for_each_pass(m, ws, io, chunk, st, [&](const Pass &ps) {
        EvalArgs e;
        e.x = io->x + ps.elem;
        e.out = io->out + ps.elem;
        e.t = io->t + ps.b0;
        e.have_y = ps.y != nullptr;
        const PassPlan &plan = plans.of(ps.bc);
        JvpPass tangent(m, ws, jw, plan, x_tangent + ps.elem, out_tangent + ps.elem, st);
        return run_eval(m, ws, plan, e, st, &tangent);
    });
}

}  // namespace
