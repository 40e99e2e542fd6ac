// The sampling path's plan and kernel sequences: the plan of a pass (which kernel and instance every launch of its sub-blocks runs, decided
// and checked before the first launch; the profiler's labels are read off it); the kernel sequence of one network evaluation, of a pass, of
// a call's passes, and of the trajectory-resident sampler; argument checks of a call.
#pragma once
#include "host_launch.hip.h"

namespace {

// ---- pieces of one evaluation ----------------------------------------------------------------------

// conditioning vector -> all modulation tables for `rows` trajectories (latent_si_v31.py:176-178,
// mmdit.py:184-197).  t_dev == nullptr: scalar t.  yemb == nullptr: no class conditioning.
int run_mods(lsl_model *m, const Workspace &ws, const float *t_dev, float t_scalar, const float *yemb, int rows,
             float *vec_out, float *mods_out, hipStream_t st) {
    const lsl_weights &w = m->w;
    const int D = m->d.hidden;
    m->prof.begin(6, st);
    hipLaunchKernelGGL(k_time_features, dim3((rows * 128 + 255) / 256), dim3(256), 0, st, ws.tfeat, t_dev, t_scalar, w.time_freqs, rows);
    const bool single = !t_dev && !yemb;  // shared scalar time, no class vector: one row whatever the batch
    char k1[32], k2[32], k3[32];  // (the label of class 6: what each launch_dense chose)
    const bool lab = m->prof.kernel == 6;
    launch_dense<false, true>(ws.hid, ws.tfeat, w.time_w1, w.time_b1, nullptr, rows, 256, D, 0, st, single, 0, lab ? k1 : nullptr);
    launch_dense<false, false>(vec_out, ws.hid, w.time_w2, w.time_b2, yemb, rows, D, D, D, st, single, 0, lab ? k2 : nullptr);
    launch_dense<true, false>(mods_out, vec_out, w.mod_w, w.mod_b, nullptr, rows, D, m->MODW, 0, st, single, 0, lab ? k3 : nullptr);
    if (lab) m->prof.label(6, "k_time_features > %s > %s > %s", k1, k2, k3);
    m->prof.end(6, st);
    LSL_CHECK_LAUNCH("modulation");
    return 0;
}

// The same tables for `count` sampler records at once (shared scalar time, no class vector: one row per record).  Every row goes
// through the kernels run_mods uses for its single row (k_dense_rows: a row's sum does not depend on the other rows of the launch),
// so a record's table has the same bits as the one run_mods computes in front of a single evaluation.
int run_mods_steps(lsl_model *m, const Workspace &ws, const float *times, int count, hipStream_t st) {
    const lsl_weights &w = m->w;
    const int D = m->d.hidden;
    m->prof.begin(6, st);
    for (int c0 = 0; c0 < count; c0 += 48) {
        StepTimes tt;
        const int nc = std::min(48, count - c0);
        for (int s = 0; s < nc; ++s) tt.t[s] = times[c0 + s];
        hipLaunchKernelGGL(k_time_features_steps, dim3((nc * 128 + 255) / 256), dim3(256), 0, st, ws.tf_all + (size_t)c0 * 256, tt, nc, 1, w.time_freqs);
    }
    const unsigned gy = (unsigned)((count + 7) / 8);  // 8 rows per workgroup
    hipLaunchKernelGGL((k_dense_rows<false, true>), dim3((D + 3) / 4, gy), dim3(256), 0, st, ws.hid_all, ws.tf_all, w.time_w1, w.time_b1, nullptr, count, 256, D, 0, 0);
    hipLaunchKernelGGL((k_dense_rows<false, false>), dim3((D + 3) / 4, gy), dim3(256), 0, st, ws.vec_all, ws.hid_all, w.time_w2, w.time_b2, nullptr, count, D, D, D, 0);
    // (the wide last layer: a workgroup's four weight rows are its HBM traffic, re-read once per row range - 16 rows per workgroup)
    hipLaunchKernelGGL((k_dense_rows<true, false>), dim3((m->MODW + 3) / 4, (unsigned)((count + 15) / 16)), dim3(256), 0, st, ws.mods_all, ws.vec_all, w.mod_w, w.mod_b, nullptr, count, D, m->MODW, 0, 0);
    m->prof.label(6, "k_time_features_steps > k_dense_rows<0, 1> > k_dense_rows<0, 0> > k_dense_rows<1, 0> (row ranges of 8, 8, 16)");
    m->prof.end(6, st);
    LSL_CHECK_LAUNCH("modulation (group of records)");
    return 0;
}

// vec_in(y) (mmdit.py:118-126), constant over a sample
int run_yemb(lsl_model *m, const Workspace &ws, const float *y, int rows, hipStream_t st, float *yhid_tap = nullptr) {
    const lsl_weights &w = m->w;
    const int D = m->d.hidden, V = m->d.vec_in_dim;
    char k1[32], k2[32];
    const bool lab = m->prof.kernel == 6;  // (not timed with class 6 - once per sample; lsl_debug_mods_ex reports the label in front of run_mods')
    launch_dense<false, true>(ws.hid, y, w.vec_w1, w.vec_b1, nullptr, rows, V, D, 0, st, false, 0, lab ? k1 : nullptr);
    if (yhid_tap) hipMemcpyAsync(yhid_tap, ws.hid, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, st);  // (run_mods reuses ws.hid)
    launch_dense<false, false>(ws.yemb, ws.hid, w.vec_w2, w.vec_b2, nullptr, rows, D, D, 0, st, false, 0, lab ? k2 : nullptr);
    if (lab) m->prof.label(6, "%s > %s", k1, k2);
    LSL_CHECK_LAUNCH("vec_in");
    return 0;
}

void run_tables(const lsl_model *m, const Workspace &ws, int T, int L, hipStream_t st) {
    const int half = m->d.head_dim_pad / 2;
    if (ws.w2p) {  // linear2 weights in MFMA-fragment order (k_linear2_ws keeps them in registers for a whole launch: every load 1 KiB contiguous)
        const size_t per = (size_t)m->d.hidden * m->K2;
        for (int bi = 0; bi < 2 * m->d.depth; ++bi)
            hipLaunchKernelGGL(k_lin2_pack, dim3(128), dim3(256), 0, st, ws.w2p + (size_t)bi * per, (const u16 *)m->blocks[bi].w2, m->d.hidden, m->K2);
    }
    if (ws.wtail) {  // tail models: the weight stream of every sub-block in the order k_tail consumes it
        for (int bi = 0; bi < 2 * m->d.depth; ++bi)
            hipLaunchKernelGGL(k_tail_pack, dim3(256), dim3(256), 0, st, ws.wtail + (size_t)bi * ws.wtail_stride, (const u16 *)m->blocks[bi].w1,
                               (const u16 *)m->blocks[bi].w2, m->d.hidden, m->HHD, m->d.mlp_dim);
    }
    hipLaunchKernelGGL(k_rope_table, dim3((L * half + 255) / 256), dim3(256), 0, st, ws.rope_l, L, m->d.head_dim, m->d.head_dim_pad, m->d.theta);
    hipLaunchKernelGGL(k_rope_table, dim3((T * half + 255) / 256), dim3(256), 0, st, ws.rope_t, T, m->d.head_dim, m->d.head_dim_pad, m->d.theta);
    // the same tables with each attention block's query / key norm scales folded in (spatial blocks: L positions, temporal: T)
    const int nb = 2 * m->d.depth;
    for (int b0 = 0; b0 < 2 * nb; b0 += 16) {
        RopeScaledJobs jobs{};
        jobs.n_jobs = std::min(16, 2 * nb - b0);
        int max_pos = 0;
        for (int k = 0; k < jobs.n_jobs; ++k) {
            const int t = b0 + k, bi = t >> 1;
            jobs.out[k] = ws.rope_qk + (size_t)t * ws.rope_qk_stride;
            jobs.scale[k] = (t & 1) ? m->blocks[bi].ks : m->blocks[bi].qs;
            jobs.n_pos[k] = (bi & 1) ? T : L;
            jobs.sq_bound[k] = ws.kmax2 + ((t & 1) ? 0 : nb) + bi;
            max_pos = std::max(max_pos, jobs.n_pos[k]);
        }
        hipLaunchKernelGGL(k_rope_scaled, dim3((max_pos * half + 255) / 256, jobs.n_jobs), dim3(256), 0, st, jobs, m->d.head_dim, m->d.head_dim_pad, m->d.theta);
    }
}

// ---- the plan of a pass: which kernels every sub-block runs -----------------------------------------

// A network evaluation (lsl_forward, lsl_sample*), lsl_debug_block (one sub-block) or lsl_debug_taps (one sub-block up to its attention)
enum class PlanMode { eval, debug_block, debug_taps };
enum class Lin2Kind { none, tail, ws, gemm };  // k_tail (the whole back half), k_linear2_ws, the tile GEMM (EpiLinear2)

// Decided once per pass size, before the call's first launch; run_eval / run_block only read it.  Every choice depends on the model, the
// handle's forms (tail, ln_fuse), T, L, the pass size and the mode - the forms whose rounding differs (tail, ln_fuse) never on the batch.
struct PassPlan {
    PlanMode mode;
    int bc, n, npad, T, L, mod_stride, blocks;  // (npad: n rounded up to whole 256-token tiles; blocks: 2 * depth)
    bool tail;  // k_tail runs the back half of every sub-block and writes the next one's LayerNorm + modulate; linear1 computes q | k | v only
    int F1;     // linear1's output features
    bool lin1_ts;    // token-stationary linear1 (k_linear1_ts), else the tile GEMM (EpiLinear1)
    int lin1_waves;  // its waves per workgroup (linear1_ts_waves)
    bool ln_stats;   // ln_fuse handles: k_linear2_ws leaves the rows' statistics for the next sub-block, whose linear1 normalises on load
    bool emb_stats;  // ... and the embedding leaves them for the first sub-block
    int gemm1;       // !lin1_ts: the tiling of the tile GEMM (gemm_variant)
    bool planes[2];  // q / k / v as head-major planes: [spatial, temporal] sub-blocks
    AttnPlan attn[2];  // the attention form of the [spatial, temporal] sub-blocks
    Lin2Kind lin2;
    Lin2Grid l2grid;  // lin2 == ws
    int gemm2;        // lin2 == gemm: its tiling

    bool a_from_tail(int bi) const { return mode == PlanMode::eval && tail && bi > 0; }  // ws.a written by the previous sub-block's k_tail
    bool lin1_lnf(int bi) const { return mode == PlanMode::eval && ln_stats && (bi > 0 || emb_stats); }  // no LayerNorm launch, ws.a unused
    bool lin2_stats(int bi) const { return ln_stats && bi + 1 < blocks; }
};

// The plan of a pass of bc trajectories through sub-blocks [0, 2 depth) (eval) or sub-block `block` (the debug modes).  Refuses (-3) a pass
// too large for the kernels' 32-bit arithmetic or an attention axis no kernel takes, with the message of the first check a sub-block's launches would meet.
int plan_pass(const lsl_model *m, const Workspace &ws, int bc, int T, int L, int mod_stride, PlanMode mode, int block, PassPlan &p) {
    const lsl_model_desc &d = m->d;
    const int D = d.hidden, n = bc * T * L;
    p = PassPlan{};
    p.mode = mode;
    p.bc = bc;
    p.n = n;
    p.npad = (n + 255) & ~255;
    p.T = T;
    p.L = L;
    p.mod_stride = mod_stride;
    p.blocks = 2 * d.depth;
    p.tail = m->tail && mode != PlanMode::debug_taps;  // (the taps hand out the GELU'd mlp half of z)
    p.F1 = p.tail ? 3 * m->HHD : m->F1;
    p.lin1_ts = linear1_ts_ok(d.head_dim_pad, D, p.F1, m->HHD, n);
    p.lin1_waves = linear1_ts_waves(D, n);
    // (never with tail: k_tail reads `a` itself; the statistics come from k_linear2_ws)
    p.ln_stats = m->ln_fuse && !m->tail && ws.w2p && mode != PlanMode::debug_taps &&
                 linear1_lnf_ok(d.head_dim_pad, D, m->F1, m->HHD, n, T * L, mod_stride);
    // (models without the in-place LayerNorm behind the embedding)
    p.emb_stats = p.ln_stats && mode == PlanMode::eval && !d.normalize && embed_stats_ok(d.in_dim, D);
    if (!p.lin1_ts) p.gemm1 = gemm_variant(false, p.F1, D, n);
    for (int t = 0; t < 2; ++t) {
        p.attn[t] = plan_attention(m->attention_linear, d.head_dim_pad, d.heads, d.head_dim, bc, T, L, t != 0);
        p.planes[t] = qkv_planes_ok(d.head_dim_pad, d.heads, t ? T : L, t != 0, p.lin1_ts, p.attn[t]);
    }
    const bool ws_reach = ws.w2p && (unsigned long long)n * (unsigned)(4 * D) < (1ull << 32);  // (k_linear2_ws: 32-bit byte offsets into h)
    if (ws_reach) p.l2grid = linear2_ws_grid(D, n, T * L, mod_stride == 0);
    const bool on_ws = ws_reach && p.l2grid.gate_rows <= linear2_ws_max_gate_rows(m->K2);
    p.lin2 = mode == PlanMode::debug_taps ? Lin2Kind::none : p.tail ? Lin2Kind::tail : on_ws ? Lin2Kind::ws : Lin2Kind::gemm;
    if (p.lin2 == Lin2Kind::gemm) p.gemm2 = gemm_variant(true, D, m->K2, n);

    const int b0 = mode == PlanMode::eval ? 0 : block, b1 = mode == PlanMode::eval ? p.blocks : block + 1;  // the sub-blocks the call runs
    for (int bi = b0; bi < b1; ++bi) {
        const int temporal = bi & 1, pdiv = temporal ? L : 1, pmod = temporal ? T : L;
        // position of token n along the attended axis = (n / pdiv) % pmod, done with multiply-high in the epilogue: exact while n * d < 2^32
        if ((unsigned long long)n * (unsigned)std::max(pdiv, pmod) >= (1ull << 32)) return fail(-3, "pass too large for the position arithmetic");
        // head-major planes are addressed with 32-bit per-lane byte offsets over the whole q | k | v buffer (k_lin1.hip.h flush, k_attn.hip.h
        // stream requests): a pass set larger than that through lsl_model_set_chunk / LSL_CHUNK_TRAJ is refused, never wrapped
        if (p.planes[temporal] && (unsigned long long)p.npad * 3ull * (unsigned)m->HHD * 2ull >= (1ull << 32))
            return fail(-3, "pass too large for the q/k/v plane offsets (%d tokens: at most %llu with this model)", n, (unsigned long long)((1ull << 32) / (6ull * (unsigned)m->HHD)) - 256);
        // an axis that is not on the stream kernel (LSL_ATTN_STREAM=0, or a pass of 2^31 stream units) needs K | V of a whole (sequence, head) in LDS
        if (p.attn[temporal].form == AttnForm::none)
            return fail(-3, "attention axis of %d positions is not on the stream kernel and too long for k_attention_rows (at most %d positions at %d-wide heads)",
                        pmod, attention_rows_max_s(d.head_dim_pad), d.head_dim_pad);
        if (p.lin2 == Lin2Kind::none) continue;
        if ((unsigned long long)n * (unsigned)(T * L) >= (1ull << 32)) return fail(-3, "pass too large for the trajectory arithmetic");
        if (p.tail && (unsigned long long)p.npad * (unsigned)(4 * D) >= (1ull << 32)) return fail(-3, "pass too large for the residual-stream offsets");
        // (which LayerNorm form the next sub-block runs must not depend on the launch: a pass the weight-stationary kernel cannot take - more
        // trajectories per token range than its gate table holds - is refused on ln_fuse handles, never served by the other form)
        if (p.lin2_stats(bi) && !on_ws) {
            if (ws_reach) return fail(-3, "ln_fuse: a pass of %d tokens has too many trajectories per token range for k_linear2_ws; use smaller passes (lsl_model_set_chunk)", n);
            return fail(-3, "ln_fuse: pass too large for the residual-stream offsets (%d tokens)", n);
        }
    }
    return 0;
}

// The plans of a call's passes: `chunk` trajectories, and the rest of the batch when B is not a multiple of it
struct CallPlans {
    PassPlan full, rest;
    const PassPlan &of(int bc) const { return bc == full.bc ? full : rest; }
};
int plan_call(const lsl_model *m, const Workspace &ws, const lsl_io *io, int chunk, int mod_stride, CallPlans &cp) {
    if (int rc = plan_pass(m, ws, chunk, io->T, io->L, mod_stride, PlanMode::eval, 0, cp.full)) return rc;
    if (io->B % chunk) return plan_pass(m, ws, io->B % chunk, io->T, io->L, mod_stride, PlanMode::eval, 0, cp.rest);
    return 0;
}

// What sub-block bi's launch of the profiled class (0 linear1, 1 linear2 / tail, 2 attention) runs, for lsl_profile_kernel_name: read off the plan
void label_block(lsl_model *m, const PassPlan &p, int bi) {
    const lsl_model_desc &d = m->d;
    Profiler &pr = m->prof;
    switch (pr.kernel) {
        case 0:
            if (!p.lin1_ts) pr.label(0, "k_gemm_glds<EpiLinear1<%d>> (tiling %d)", d.head_dim_pad, p.gemm1);
            else if (p.lin1_lnf(bi)) pr.label(0, "k_linear1_ts<%d, %d, 8, true> (LayerNorm fused)", d.head_dim_pad, d.hidden);
            else pr.label(0, "k_linear1_ts<%d, %d, %d>%s", d.head_dim_pad, d.hidden, p.lin1_waves, p.tail ? " (q | k | v)" : "");
            break;
        case 1:
            if (p.lin2 == Lin2Kind::tail) pr.label(1, "k_tail<%d, %d>", d.hidden, m->HHD);
            else if (p.lin2 == Lin2Kind::ws) pr.label(1, p.lin2_stats(bi) ? "k_linear2_ws<%d> (+ row statistics)" : "k_linear2_ws<%d>", m->K2);
            else if (p.lin2 == Lin2Kind::gemm) pr.label(1, "k_gemm_glds<EpiLinear2> (tiling %d)", p.gemm2);
            break;
        case 2: {
            const AttnPlan &a = p.attn[bi & 1];
            pr.label(2, "%s", a.form == AttnForm::linear ? "k_attention_linear" : a.stream() ? "k_attention_stream" : "k_attention_rows / k_attention_tiny");
            break;
        }
        default: break;
    }
}

unsigned magic_of(int dv) { return dv == 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)dv + 1); }  // floor(2^32 / dv) + 1: division by multiply-high

template <int HDP>
void launch_linear1_gemm(const lsl_model *m, const Workspace &ws, const PassPlan &p, int bi, int pdiv, int pmod, float premul, hipStream_t st) {
    const lsl_block_weights &bw = m->blocks[bi];
    const EpiLinear1<HDP> e{bw.b1, bw.qs, bw.ks, (bi & 1) ? ws.rope_t : ws.rope_l, ws.rope_qk + (size_t)(2 * bi) * ws.rope_qk_stride,
                            ws.rope_qk + (size_t)(2 * bi + 1) * ws.rope_qk_stride, ws.qkv, ws.z, m->HHD, m->d.mlp_dim,
                            pdiv, pmod, magic_of(pdiv), magic_of(pmod), 1.0f / m->d.head_dim, premul, 0};
    launch_gemm(p.gemm1, (const u16 *)bw.w1, ws.a, p.F1, p.n, m->d.hidden, e, st, m->HHD);
}

AttnArgs attention_args(const lsl_model *m, const Workspace &ws, const PassPlan &p, int bi, float premul) {
    const lsl_model_desc &d = m->d;
    const AttnPlan &ap = p.attn[bi & 1];
    static const int nt_mask = tune_int("LSL_NT", 3);
    static const int attn_bound = tune_int("LSL_ATTN_BOUND", 1);
    AttnArgs aa{};
    aa.nt = (nt_mask >> 2) & 1;
    aa.qkv = ws.qkv; aa.z = ws.z; aa.HHD = m->HHD; aa.zw = m->K2; aa.H = d.heads; aa.hd = d.head_dim; aa.premul = premul;
    aa.kmax2 = ws.kmax2 + bi;
    aa.qmax2 = ws.kmax2 + 2 * d.depth + bi;
    aa.planes = p.planes[bi & 1] ? 1 : 0;
    aa.npad = p.npad;
    aa.bound = attn_bound == 2 || (attn_bound == 1 && ((bi & 1) ? p.T : p.L) > 96);  // short axes: the max pass is one or two tiles, cheaper than the norms
    aa.S = ap.S; aa.n_seq = ap.n_seq; aa.inner = ap.inner; aa.outer_stride = ap.outer_stride; aa.pos_stride = ap.pos_stride;
    aa.blk = ap.blk; aa.n_tok = ap.n_tok;
    return aa;
}

// The tangent pass (lsl_forward_jvp, host_jvp.hip.h) rides on the primal launches of an evaluation: run_embed / run_block / run_eval call these
// between their own launches, which stay what they are - the primal half of a tangent pass is the evaluation itself, launch for launch.
struct EvalTangent {
    virtual int embedded() = 0;  // ws.h holds the state embedding, in front of the LayerNorm of normalize models
    virtual int normed(int bi, const float *mbase) = 0;  // ws.a holds sub-block bi's linear1 operand (mbase: its shift | scale | gate rows)
    virtual int attended(int bi, const float *mbase, float premul, int pdiv, int pmod) = 0;  // ws.qkv and ws.z are written, ws.h is not yet updated
    virtual int head(const float *fm) = 0;  // the output head has read ws.h (fm: the final shift | scale rows)
    virtual ~EvalTangent() = default;
};

// one ParallelMLPAttentionV2 sub-block on ws.h (in place): LN+modulate -> linear1 -> attention -> linear2; which kernels: the plan.
// a_tap (lsl_debug_block_ex; debug plans only, where the LayerNorm launch always runs): receives ws.a, linear1's operand, right behind the
// LayerNorm launch - on a tail handle k_tail overwrites ws.a with the NEXT sub-block's operand (TailArgs::a_next aliases A)
int run_block(lsl_model *m, const Workspace &ws, const PassPlan &p, int bi, const float *mods, hipStream_t st, void *a_tap = nullptr,
              EvalTangent *tg = nullptr) {
    const lsl_model_desc &d = m->d;
    const lsl_block_weights &bw = m->blocks[bi];
    const int D = d.hidden, n = p.n, tpt = p.T * p.L, mod_stride = p.mod_stride, temporal = bi & 1;
    const float *mbase = mods + (size_t)(bi / 2) * 6 * D + (temporal ? 3 * D : 0);  // shift, scale, gate
    const bool lnf = p.lin1_lnf(bi);  // (ws.lnstat holds the statistics of h)
    // softmax attention: log2(e) / sqrt(head_dim) rides on q (the kernels use exp2); attention_linear takes the plain normalised, rotated q
    const float premul = m->attention_linear ? 1.0f : (float)(1.4426950408889634 / std::sqrt((double)d.head_dim));
    const int pdiv = temporal ? p.L : 1, pmod = temporal ? p.T : p.L;  // position of token n = (n / pdiv) % pmod (plan_pass: the range check)
    label_block(m, p, bi);
    if (!p.a_from_tail(bi) && !lnf) {
        m->prof.begin(3, st);
        DISPATCH_D(D, launch_ln_mod_t, ws.a, ws.h, mbase, mbase + D, mod_stride, n, tpt, st);
        m->prof.end(3, st);
        if (a_tap) hipMemcpyAsync(a_tap, ws.a, (size_t)n * D * 2, hipMemcpyDeviceToDevice, st);
    }
    if (tg)
        if (int rc = tg->normed(bi, mbase)) return rc;
    m->prof.begin(0, st);
    if (p.lin1_ts) {
        const Lin1Args la{(const u16 *)bw.w1, lnf ? (const u16 *)ws.h : ws.a, bw.b1, ws.rope_qk + (size_t)(2 * bi) * ws.rope_qk_stride,
                          ws.rope_qk + (size_t)(2 * bi + 1) * ws.rope_qk_stride, ws.qkv, ws.z, p.F1, n, m->HHD, d.mlp_dim,
                          pdiv, pmod, magic_of(pdiv), magic_of(pmod), 1.0f / d.head_dim, premul, 1, 0, p.planes[temporal] ? 1 : 0, p.npad,
                          ws.lnstat, mbase, mbase + D, mod_stride, tpt, magic_of(tpt)};
        launch_linear1_ts(d.head_dim_pad, D, p.lin1_waves, lnf, la, st);
    } else if (d.head_dim_pad == 32) launch_linear1_gemm<32>(m, ws, p, bi, pdiv, pmod, premul, st);
    else launch_linear1_gemm<16>(m, ws, p, bi, pdiv, pmod, premul, st);
    m->prof.end(0, st);

    const AttnArgs aa = attention_args(m, ws, p, bi, premul);
    m->prof.begin(2, st);
    if (d.head_dim_pad == 32) launch_attention_t<32>(p.attn[temporal], aa, st);
    else launch_attention_t<16>(p.attn[temporal], aa, st);
    m->prof.end(2, st);
    if (p.lin2 == Lin2Kind::none) {  // (lsl_debug_taps)
        LSL_CHECK_LAUNCH("block");
        return 0;
    }
    if (tg)
        if (int rc = tg->attended(bi, mbase, premul, pdiv, pmod)) return rc;
    m->prof.begin(1, st);
    if (p.lin2 == Lin2Kind::tail) {  // up-projection -> GELU -> down-projection + out-projection + gated residual + the next sub-block's LayerNorm + modulate
        const bool next = bi + 1 < 2 * d.depth;
        const float *nb = mods + (size_t)((bi + 1) / 2) * 6 * D + (((bi + 1) & 1) ? 3 * D : 0);  // next sub-block: shift, scale
        const TailArgs ta{ws.wtail + (size_t)bi * ws.wtail_stride, ws.a, ws.z, bw.b1 + 3 * m->HHD, bw.b2, mbase + 2 * D, ws.h, next ? ws.a : nullptr,
                          nb, nb + D, n, d.mlp_dim, m->K2, mod_stride, tpt, magic_of(tpt)};
        launch_tail(ta, st);
    } else if (p.lin2 == Lin2Kind::ws) {
        // ln_fuse handles: the rows' statistics for the NEXT sub-block's LayerNorm (inside its linear1) leave with the update
        const bool stats = p.lin2_stats(bi);
        const Lin2Args l2{ws.w2p + (size_t)bi * D * m->K2, ws.z, bw.b2, mbase + 2 * D, ws.h, D, n, mod_stride, tpt, magic_of(tpt),
                          p.l2grid.slices, p.l2grid.rpx, p.l2grid.gate_rows, stats ? ws.lnparts : nullptr, p.npad};
        launch_linear2_ws(m->K2, l2, st);
        if (stats) hipLaunchKernelGGL(k_ln_finalize, dim3((n + 255) / 256), dim3(256), 0, st, ws.lnstat, ws.lnparts, D / 32, p.npad, n, 32.0f);
    } else {
        const EpiLinear2 e2{bw.b2, mbase + 2 * D, ws.h, D, mod_stride, tpt, 0, magic_of(tpt)};
        launch_gemm(p.gemm2, (const u16 *)bw.w2, ws.z, D, n, m->K2, e2, st);
    }
    m->prof.end(1, st);
    LSL_CHECK_LAUNCH(p.lin2 == Lin2Kind::tail ? "block (tail)" : "block");
    return 0;
}

// What one evaluation reads besides its pass: lsl_forward's per-trajectory times and output buffer, or a sampler record (lsl_sample_ex)
// whose state update the head applies, with the slices of noise / trace / saved state it uses
struct EvalArgs {
    float *x = nullptr;
    float *out = nullptr;              // network output (lsl_forward)
    const float *t = nullptr;          // per-trajectory times (lsl_forward); nullptr: the record's scalar time
    bool have_y = false;
    const lsl_step_ex *rec = nullptr;  // nullptr: no state update
    const float *noise = nullptr;
    uint64_t seed = 0, elem_off = 0;
    float *trace = nullptr;
    const float *saved = nullptr;
    float *save_out = nullptr;
    const float *mods_ready = nullptr;  // this record's row of the group table (run_mods_steps), or nullptr
};
// THE place where a record becomes the update the kernels apply (k_small_frag.hip.h: StepUpdate) - for the head and for k_state_affine
StepUpdate step_update(const EvalArgs &e) {
    const lsl_step_ex r = e.rec ? *e.rec : lsl_step_ex{};
    return StepUpdate{e.noise, e.trace, e.saved, e.save_out, (unsigned long long)e.seed, (unsigned long long)e.elem_off, r.ax, r.am, r.aw, r.as, (unsigned)r.noise_index};
}

// The state embedding of an evaluation: ws.h = x_in(x) + ws.cond_emb, with what the pass plan attaches to it (ln_fuse handles: the rows'
// statistics for the first sub-block's linear1; normalize models: the in-place LayerNorm).  h_tap (lsl_debug_embed): ws.h in front of the LayerNorm.
int run_embed(lsl_model *m, const Workspace &ws, const PassPlan &p, const float *x, hipStream_t st, float *h_tap = nullptr, EvalTangent *tg = nullptr) {
    const lsl_model_desc &d = m->d;
    const int D = d.hidden, n = p.n;
    m->prof.begin(5, st);
    // ln_fuse handles: the embedding leaves the rows' statistics, so that the FIRST sub-block's LayerNorm runs inside its linear1 too
    launch_embed<1>(ws.h, x, m->w.x_in_w, nullptr, nullptr, nullptr, nullptr, ws.cond_emb, n, d.in_dim, D, st, p.emb_stats ? ws.lnparts : nullptr, p.npad,
                    &m->prof);
    if (p.emb_stats) hipLaunchKernelGGL(k_ln_finalize, dim3((n + 255) / 256), dim3(256), 0, st, ws.lnstat, ws.lnparts, D / 256, p.npad, n, 256.0f);
    if (h_tap) hipMemcpyAsync(h_tap, ws.h, (size_t)n * D * 4, hipMemcpyDeviceToDevice, st);
    if (tg)
        if (int rc = tg->embedded()) return rc;
    if (d.normalize) { DISPATCH_D(D, launch_ln_inplace_t, ws.h, n, 1e-5f, st); }
    m->prof.end(5, st);
    LSL_CHECK_LAUNCH("embed");
    return 0;
}

// The output head on the rows h [n, D] with the final modulation rows fm = (shift | scale): e.out <- the network output, or the record's
// update of e.x fused into it
int run_head(lsl_model *m, const float *h, const float *fm, int mod_stride, int n, int tpt, const EvalArgs &e, hipStream_t st) {
    const int D = m->d.hidden;
    const HeadArgs a{e.x, e.out, h, fm, fm + D, mod_stride, m->w.out_w, m->w.out_b, n, m->d.in_dim, tpt, e.rec ? 1 : 0, step_update(e)};
    m->prof.begin(4, st);
    DISPATCH_D(D, launch_head_mfma, a, st, &m->prof);
    m->prof.end(4, st);
    LSL_CHECK_LAUNCH("head");
    return 0;
}

// One evaluation for a pass: embeds x, runs the sub-blocks and the head (write the network output, or fuse the record's update into it)
int run_eval(lsl_model *m, const Workspace &ws, const PassPlan &p, const EvalArgs &e, hipStream_t st, EvalTangent *tg = nullptr) {
    const lsl_model_desc &d = m->d;
    const int D = d.hidden, n = p.n;
    const lsl_step_ex r = e.rec ? *e.rec : lsl_step_ex{};
    // modulation rows: one per trajectory, or a single shared row when t is a scalar and there is no y (plan: mod_stride 0)
    const bool shared = p.mod_stride == 0;
    int rc = 0;
    const float *mods = ws.mods;
    if (e.mods_ready && shared) mods = e.mods_ready;
    else rc = run_mods(m, ws, e.t, r.t, e.have_y ? ws.yemb : nullptr, shared ? 1 : p.bc, ws.vec, ws.mods, st);
    if (rc) return rc;
    if ((rc = run_embed(m, ws, p, e.x, st, nullptr, tg))) return rc;
    for (int bi = 0; bi < 2 * d.depth; ++bi)
        if ((rc = run_block(m, ws, p, bi, mods, st, nullptr, tg))) return rc;
    const float *fm = mods + (size_t)d.depth * 6 * D;  // adaLN: shift, scale
    if ((rc = run_head(m, ws.h, fm, p.mod_stride, n, p.T * p.L, e, st))) return rc;
    return tg ? tg->head(fm) : 0;
}

int prepare_pass(lsl_model *m, const Workspace &ws, const float *x_cond, const int64_t *mask, const float *y, int bc, int T,
                 int L, hipStream_t st) {
    const lsl_model_desc &d = m->d;
    const int n = bc * T * L;
    launch_embed<0>(ws.cond_emb, x_cond, m->w.cond_w, m->w.cond_b, m->w.x_in_b, m->w.mask_emb, mask, nullptr, n, d.in_dim, d.hidden, st, nullptr, 0, &m->prof);
    LSL_CHECK_LAUNCH("cond_embed");
    if (y) return run_yemb(m, ws, y, bc, st);
    return 0;
}

// ---- trajectory-resident path (k_resident.hip.h): models whose whole trajectory fits one workgroup's LDS ----------------------
// The choice depends on the MODEL and on T*L only, never on the batch: a trajectory's bits are the same in any batch / shard / pass.
bool resident_ok(const lsl_model *m, int T, int L) {
    static const int off = env_int("LSL_RESIDENT", 1) == 0;  // documented runtime switch: 0 = always the general path
    const lsl_model_desc &d = m->d;
    return !off && !m->attention_linear && d.hidden == RES_D && d.heads == RES_H && d.head_dim == RES_HD && d.head_dim_pad == RES_HD && d.mlp_dim == RES_M &&
           d.in_dim <= RES_MAX_C && d.in_dim % 4 == 0 && 2 * d.depth <= RES_MAX_BLOCKS && (long)T * L <= 48 && T <= 32 && L <= 32;
}

struct ResWorkspace {
    float *cond_emb, *yemb, *tfeat, *hid, *vec, *mods, *blkpar;
    u16 *blkw;
    int steps_per_launch;
    size_t bytes;
};
ResWorkspace carve_resident(const lsl_model *m, char *base, int B, int T, int L, bool have_y) {
    const size_t n = (size_t)B * T * L, D = m->d.hidden;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align_up(bytes, 256);
        return p;
    };
    ResWorkspace ws;
    const size_t rows = have_y ? (size_t)B : 1;
    // modulation tables of a whole group of state updates are computed before the group's single launch: bound them to 256 MiB
    size_t spl = ((size_t)256 << 20) / (rows * m->MODW * 4);
    ws.steps_per_launch = (int)std::max<size_t>(1, std::min<size_t>(spl, RES_MAX_STEPS));
    const size_t rt = rows * ws.steps_per_launch;
    ws.cond_emb = (float *)take(n * D * 4);
    ws.yemb = (float *)take((size_t)B * D * 4);
    ws.tfeat = (float *)take(rt * 256 * 4);
    ws.hid = (float *)take(std::max(rt, (size_t)B) * D * 4);
    ws.vec = (float *)take(rt * D * 4);
    ws.mods = (float *)take(rt * m->MODW * 4);
    ws.blkpar = (float *)take((size_t)2 * m->d.depth * RES_P_SHIFT * 4);
    ws.blkw = (u16 *)take((size_t)2 * m->d.depth * (RES_W1_ELEMS + RES_W2_ELEMS) * 2);
    ws.bytes = off;
    return ws;
}

template <int NNT>
void launch_resident(const ResArgs &a, int B, int T, int L, hipStream_t st) {
    auto kern = k_resident<NNT>;
    const size_t lds = ResLds<NNT>::bytes(T, L);
    LSL_ALLOW_LDS(kern, (size_t)163840);
    hipLaunchKernelGGL(kern, dim3(B), dim3(RES_NTHR), lds, st, a);
}

int resident_sample(lsl_model *m, const lsl_io *io, const lsl_step *steps, int n_steps, const float *noise, uint64_t seed, uint64_t elem_offset,
                    float *trace, void *workspace, hipStream_t st) {
    const lsl_model_desc &d = m->d;
    const lsl_weights &w = m->w;
    const int B = io->B, T = io->T, L = io->L, n_t = T * L, D = d.hidden;
    const bool have_y = io->y != nullptr;
    const ResWorkspace ws = carve_resident(m, (char *)workspace, B, T, L, have_y);
    const int rows = have_y ? B : 1;
    if (have_y) {
        launch_dense<false, true>(ws.hid, io->y, w.vec_w1, w.vec_b1, nullptr, B, d.vec_in_dim, D, 0, st);
        launch_dense<false, false>(ws.yemb, ws.hid, w.vec_w2, w.vec_b2, nullptr, B, D, D, 0, st);
        LSL_CHECK_LAUNCH("vec_in");
    }
    ResArgs a;
    a.cond_emb = ws.cond_emb;
    a.x_cond = io->x_cond;
    a.mask = (const int64_t *)io->mask;
    a.cond_w = w.cond_w; a.cond_b = w.cond_b; a.x_in_b = w.x_in_b; a.mask_emb = w.mask_emb;
    a.x = io->x;
    a.mods = ws.mods;
    a.mods_step_stride = (long)rows * m->MODW;
    a.mods_traj_stride = have_y ? m->MODW : 0;
    a.x_in_w = w.x_in_w;
    a.out_w = w.out_w;
    a.out_b = w.out_b;
    a.noise = noise;
    a.noise_step_stride = (long)B * n_t * d.in_dim;
    a.seed = seed;
    a.elem_offset = elem_offset;
    a.trace = trace;
    a.trace_step_stride = (long)B * n_t * d.in_dim;
    a.n_t = n_t; a.T = T; a.L = L; a.C = d.in_dim; a.depth = d.depth; a.normalize = d.normalize;
    a.theta = d.theta;
    a.skip = tune_int("LSL_RES_SKIP", 0);
    a.q_premul = (float)(1.4426950408889634 / std::sqrt((double)d.head_dim));
    ResPack pack;
    for (int bi = 0; bi < 2 * d.depth; ++bi) {
        const lsl_block_weights &bw = m->blocks[bi];
        const u16 *wb = ws.blkw + (size_t)bi * (RES_W1_ELEMS + RES_W2_ELEMS);
        a.blk[bi] = ResBlock{wb, wb + RES_W1_ELEMS};
        pack.w1[bi] = (const u16 *)bw.w1; pack.w2[bi] = (const u16 *)bw.w2;
        pack.b1[bi] = bw.b1; pack.qs[bi] = bw.qs; pack.ks[bi] = bw.ks; pack.b2[bi] = bw.b2;
    }
    hipLaunchKernelGGL(k_res_pack, dim3(2 * d.depth, 49), dim3(256), 0, st, ws.blkw, ws.blkpar, pack);
    LSL_CHECK_LAUNCH("k_res_pack");
    a.blkpar = ws.blkpar;
    for (int s0 = 0; s0 < n_steps; s0 += ws.steps_per_launch) {
        const int ns = std::min(ws.steps_per_launch, n_steps - s0);
        StepTimes tt;
        for (int s = 0; s < ns; ++s) {
            tt.t[s] = steps[s0 + s].t;
            a.step[s] = make_float4(steps[s0 + s].t, steps[s0 + s].ax, steps[s0 + s].am, steps[s0 + s].aw);
        }
        const int rt = ns * rows;
        // conditioning vector -> modulation tables of the group's steps (latent_si_v31.py:176-178, mmdit.py:184-197); the tiled kernel
        // is used for any row count, so a trajectory's tables do not depend on the batch it is sampled in
        hipLaunchKernelGGL(k_time_features_steps, dim3((rt * 128 + 255) / 256), dim3(256), 0, st, ws.tfeat, tt, ns, rows, w.time_freqs);
        launch_dense<false, true>(ws.hid, ws.tfeat, w.time_w1, w.time_b1, nullptr, rt, 256, D, 0, st);
        launch_dense<false, false>(ws.vec, ws.hid, w.time_w2, w.time_b2, have_y ? ws.yemb : nullptr, rt, D, D, D, st, false, have_y ? B : 0);
        launch_dense<true, false>(ws.mods, ws.vec, w.mod_w, w.mod_b, nullptr, rt, D, m->MODW, 0, st);
        LSL_CHECK_LAUNCH("modulation");
        a.step0 = (unsigned)s0;
        a.n_steps = ns;
        if (n_t <= 32) launch_resident<2>(a, B, T, L, st);
        else launch_resident<3>(a, B, T, L, st);
        LSL_CHECK_LAUNCH("k_resident");
    }
    return 0;
}

// The workspace a call on B trajectories needs: the general path's pass, and the resident path's whole batch where it can take the call
size_t workspace_need(const lsl_model *m, int B, int T, int L, int *chunk_out = nullptr) {
    const int chunk = default_chunk(m, B, T, L);
    size_t need = carve(m, nullptr, chunk, T, L).bytes;
    if (resident_ok(m, T, L)) need = std::max(need, carve_resident(m, nullptr, B, T, L, m->d.vec_in_dim > 0).bytes);
    if (chunk_out) *chunk_out = chunk;
    return need;
}

int check_call(const lsl_model *m, const lsl_io *io, size_t ws_bytes, void *ws, int *chunk_out) {
    if (!m || !io) return fail(-1, "null model or io");
    if (!m->has_weights) return fail(-2, "weights not set");
    if (io->B <= 0 || io->T <= 0 || io->L <= 0) return fail(-3, "B, T, L must be positive");
    if (!io->x || !io->x_cond || !io->mask) return fail(-3, "x, x_cond and mask are required");
    if ((io->y != nullptr) != (m->d.vec_in_dim > 0) && io->y != nullptr) return fail(-3, "y given but the model has no vec_in");
    if ((size_t)io->T * io->L > (1u << 24)) return fail(-3, "T*L too large");
    const size_t need = workspace_need(m, io->B, io->T, io->L, chunk_out);
    if (!ws || ws_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, ws_bytes);
    return 0;
}

// The lsl_debug_* calls: a handle with weights, a sub-block index, the call's own pointers and sizes (args_ok), a workspace for one pass of B
int check_debug(const lsl_model *m, int bi, bool args_ok, int B, int T, int L, const void *ws, size_t ws_bytes) {
    if (!m || !m->has_weights) return fail(-2, "weights not set");
    if (bi < 0 || bi >= 2 * m->d.depth) return fail(-3, "block index out of range");
    if (!args_ok) return fail(-3, "invalid arguments");
    const size_t need = carve(m, nullptr, B, T, L).bytes;
    if (!ws || ws_bytes < need) return fail(-4, "workspace too small: need %zu bytes", need);
    return 0;
}

// The passes of a call: `chunk` trajectories each (the last one the rest), as offsets into the call's arrays.  Per pass: the conditioning
// embedding (prepare_pass), then body(pass).
struct Pass {
    int b0, bc;
    size_t elem;  // b0 trajectories of x / x_cond / out / noise / trace, in elements
    const float *y;
};
template <class Body>
int for_each_pass(lsl_model *m, const Workspace &ws, const lsl_io *io, int chunk, hipStream_t st, Body &&body) {
    const size_t per = (size_t)io->T * io->L * m->d.in_dim;
    for (int b0 = 0; b0 < io->B; b0 += chunk) {
        const Pass ps{b0, std::min(chunk, io->B - b0), b0 * per, io->y ? io->y + (size_t)b0 * m->d.vec_in_dim : nullptr};
        if (int rc = prepare_pass(m, ws, io->x_cond + ps.elem, io->mask + (size_t)b0 * io->T * io->L, ps.y, ps.bc, io->T, io->L, st)) return rc;
        if (int rc = body(ps)) return rc;
    }
    return 0;
}

// the passes of one network evaluation at per-trajectory times: io->out = network(io->x, io->t, ...) (lsl_forward, the middle of lsl_si_loss,
// every evaluation of lsl_dopri_*)
int forward_passes(lsl_model *m, const lsl_io *io, const Workspace &ws, const CallPlans &plans, int chunk, hipStream_t st) {
    run_tables(m, ws, io->T, io->L, st);
    return for_each_pass(m, ws, io, chunk, st, [&](const Pass &ps) {
        EvalArgs e;
        e.x = io->x + ps.elem;
        e.out = io->out + ps.elem;
        e.t = io->t + ps.b0;
        e.have_y = ps.y != nullptr;
        return run_eval(m, ws, plans.of(ps.bc), e, st);
    });
}

// Whether a unit of n_evals network evaluations per trajectory goes through the handle's GraphCache (host_graph.hip.h; the rule is described
// in lsl_sample_ex)
bool graph_gate(const lsl_model *m, const lsl_io *io, int chunk, int n_evals) {
    static const int use_graph = env_int("LSL_GRAPH", 1);
    const int passes = (io->B + chunk - 1) / chunk;
    const long est_launches = (long)passes * n_evals * (8L * m->d.depth + 6);
    const bool launch_bound = (size_t)chunk * io->T * io->L <= 65536;
    return use_graph && (launch_bound || use_graph >= 2) && m->prof.kernel < 0 && est_launches <= 4096;
}

}  // namespace
