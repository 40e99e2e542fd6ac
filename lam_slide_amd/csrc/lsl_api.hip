// Host side of liblamslide_hip.so: the C ABI of include/lsl_api.h.  Enqueues the kernel sequence of one
// network evaluation (latent_si_v31.py:168-188) and of the sampler loops (integrators.py:67-78,103-120)
// on the caller's stream.  No allocation, no synchronisation, no host<->device copies.
// The main translation unit (the token-stationary linear1 kernel and its launcher are unit_lin1.hip): this file = the entry points of the sampling path (model handle, forward, fused sampler + opt-in hipGraph replay,
// noise, Runge-Kutta state arithmetic, the stochastic-interpolant objective around one evaluation, the geometry losses of the decoded positions, the peptide frame and torsion losses, the displacement errors (ADE / FDE, best-of-K), the torsion statistics (dihedrals, histograms, lagged products, JS distance), the TICA and state statistics (lagged second moments, projection, nearest centre, transition counts), the reversible Markov state models (active set, row-sum iteration, transition matrix), debug taps); host_common / host_launch / host_eval.hip.h = what they enqueue (host_graph.hip.h: the replay cache); decode_host.hip.h +
// stage1_api.hip.h = the frozen stage-1 encode / decode beside the path (every decoder head from one trunk) and the class losses of those heads.
#include "../../include/lsl_api.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include <atomic>
#include <new>

#include "k_attn.hip.h"
#include "k_gemm.hip.h"
#define LSL_LIN1_HOST_SIDE  // the kernel body is compiled in unit_lin1.hip
#include "k_lin1.hip.h"
#include "k_lin2.hip.h"
#include "k_tail.hip.h"
#include "k_small.hip.h"
#include "k_resident.hip.h"
#include "k_siloss.hip.h"
#include "k_geomloss.hip.h"
#include "k_peptloss.hip.h"
#include "k_disperr.hip.h"
#include "k_torsstat.hip.h"
#include "k_structstat.hip.h"
#include "k_tica.hip.h"
#include "k_wtica.hip.h"
#include "k_kmeans.hip.h"
#include "k_msm.hip.h"
#include "k_classloss.hip.h"
#ifdef LSL_EXPERIMENTS  // measured-and-rejected structures, built only by tools/build_experiments.sh (never in the product library)
#include "k_gemm_pp.hip.h"        // tools/experiments/ (on the include path of tools/build_experiments.sh only)
#include "k_gemm_drain.hip.h"
#include "k_head_scalar.hip.h"    // the scalar-FMA output head
#endif

#ifndef LSL_UNIT_OPTIONS
#define LSL_UNIT_OPTIONS ""  // (the options this unit was compiled with: lam_slide_amd/_lib.py passes them)
#endif

#include "host_common.hip.h"
#include "host_launch.hip.h"
#include "host_eval.hip.h"

}  // namespace (opened in host_common.hip.h)

#include "decode_host.hip.h"

extern "C" {

int lsl_version(void) { return LSL_VERSION; }
const char *lsl_build_info(void) {  // compiler, target, and the compile options of each translation unit (lam_slide_amd/_lib.py UNITS)
    static const std::string info = std::string("clang " __clang_version__ " gfx950; lsl_api.hip: " LSL_UNIT_OPTIONS "; unit_lin1.hip: ") + lsl_lin1_unit_options();
    return info.c_str();
}
const char *lsl_last_error(void) { return g_err; }

int lsl_model_create(const lsl_model_desc *desc, lsl_model **out) try {
    if (!desc || !out) return fail(-1, "null argument");
    const lsl_model_desc &d = *desc;
    if (d.heads <= 0 || d.hidden % d.heads != 0)
        return fail(-20, "Hidden size %d must be divisible by num_heads %d", d.hidden, d.heads);  // latent_si_v31.py:92-95
    if (d.head_dim != d.hidden / d.heads) return fail(-21, "head_dim must equal hidden / heads");
    if (d.hidden % 64 != 0 || d.hidden < 64 || d.hidden > 512) return fail(-21, "hidden_size %d unsupported (multiple of 64, 64..512)", d.hidden);
    if (d.head_dim % 2 != 0 || d.head_dim > 32) return fail(-21, "head_dim %d unsupported (even, <= 32)", d.head_dim);
    if (d.head_dim_pad != (d.head_dim <= 16 ? 16 : 32)) return fail(-21, "head_dim_pad must be 16 (head_dim <= 16) or 32");
    if ((d.heads * d.head_dim_pad) % 32 != 0) return fail(-21, "heads * head_dim_pad must be a multiple of 32");
    if (d.mlp_dim <= 0 || d.mlp_dim % 32 != 0) return fail(-21, "mlp_dim %d must be a positive multiple of 32", d.mlp_dim);
    if ((d.heads * d.head_dim_pad + d.mlp_dim) % 64 != 0) return fail(-21, "heads*head_dim_pad + mlp_dim must be a multiple of 64");
    if (3 * d.heads * d.head_dim_pad + d.mlp_dim > 7936) return fail(-21, "3 * heads * head_dim_pad + mlp_dim = %d too wide (the linear1 bias lives in LDS beside a 128 KiB operand ring: <= 7936)", 3 * d.heads * d.head_dim_pad + d.mlp_dim);
    if (d.in_dim <= 0 || d.in_dim > 128) return fail(-21, "in_dim %d unsupported (1..128)", d.in_dim);
    if (d.depth <= 0 || d.depth > 64) return fail(-21, "depth %d unsupported", d.depth);
    if (d.vec_in_dim < 0 || d.vec_in_dim > 512) return fail(-21, "vec_in_dim %d unsupported (<= 512)", d.vec_in_dim);
    lsl_model *m = new (std::nothrow) lsl_model();
    if (!m) return fail(-5, "out of host memory");
    m->d = d;
    m->HHD = d.heads * d.head_dim_pad;
    m->F1 = 3 * m->HHD + d.mlp_dim;
    m->K2 = m->HHD + d.mlp_dim;
    m->MODW = (6 * d.depth + 2) * d.hidden;
    m->tail = tail_env() == 1 && tail_shape_ok(d.hidden, m->HHD, d.mlp_dim);
    m->ln_fuse = ln_fuse_env() == 1;
    *out = m;
    return 0;
} LSL_API_CATCH

int lsl_model_set_weights(lsl_model *m, const lsl_weights *w) try {
    if (!m || !w || !w->blocks) return fail(-1, "null argument");
    const void *req[] = {w->x_in_w, w->x_in_b, w->cond_w, w->cond_b, w->mask_emb, w->time_freqs, w->time_w1, w->time_b1,
                         w->time_w2, w->time_b2, w->mod_w, w->mod_b, w->out_w, w->out_b};
    for (const void *p : req)
        if (!p) return fail(-2, "missing weight pointer");
    if (m->d.vec_in_dim > 0 && (!w->vec_w1 || !w->vec_b1 || !w->vec_w2 || !w->vec_b2)) return fail(-2, "missing vec_in weights");
    m->blocks.assign(w->blocks, w->blocks + 2 * m->d.depth);
    for (const auto &b : m->blocks)
        if (!b.w1 || !b.b1 || !b.qs || !b.ks || !b.w2 || !b.b2) return fail(-2, "missing block weight pointer");
    m->w = *w;
    m->w.blocks = m->blocks.data();
    m->has_weights = true;
    m->graphs.clear();  // (captured launches hold the old weight pointers)
    return 0;
} LSL_API_CATCH

void lsl_model_destroy(lsl_model *m) {
    if (m) m->prof.clear();
    delete m;  // (~GraphCache: the captured graphs and the capture stream)
}

int lsl_profile_enable(lsl_model *m, int32_t kernel, int32_t max_launches) try {
    if (!m) return fail(-1, "null model");
    m->prof.clear();
    if (kernel < 0 || max_launches <= 0) return 0;
    m->prof.ev.resize(2 * (size_t)max_launches);
    for (auto &e : m->prof.ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(-10, "hipEventCreate failed");
    m->prof.kernel = kernel;
    m->prof.cap = max_launches;
    return 0;
} LSL_API_CATCH

int lsl_profile_read(lsl_model *m, double *total_ms, int32_t *launches) {
    if (!m || !total_ms || !launches) return fail(-1, "null argument");
    double tot = 0.0;
    for (int i = 0; i < m->prof.used; ++i) {
        hipEventSynchronize(m->prof.ev[2 * i + 1]);
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, m->prof.ev[2 * i], m->prof.ev[2 * i + 1]) != hipSuccess) return fail(-10, "hipEventElapsedTime failed");
        tot += ms;
    }
    *total_ms = tot;
    *launches = m->prof.used;
    m->prof.used = 0;
    return 0;
}

int lsl_model_set_chunk(lsl_model *m, int32_t c) try {
    if (!m || c < 0) return fail(-1, "bad argument");
    m->chunk = c;
    m->graphs.clear();
    return 0;
} LSL_API_CATCH

int lsl_model_set_attention_mode(lsl_model *m, int32_t mode) try {
    if (!m || (mode != 0 && mode != 1)) return fail(-1, "attention mode must be 0 (scaled_dot_product) or 1 (linear)");
    m->attention_linear = mode == 1;
    m->graphs.clear();
    return 0;
} LSL_API_CATCH

int lsl_model_set_tail(lsl_model *m, int32_t on) try {
    if (!m || (on != 0 && on != 1)) return fail(-1, "tail must be 0 or 1");
    if (on && !tail_shape_ok(m->d.hidden, m->HHD, m->d.mlp_dim))
        return fail(-21, "no tail kernel for this model (hidden 256 with heads * head_dim_pad = 256, mlp_dim a multiple of 64; LSL_TAIL=0 disables it)");
    if (m->tail != (on == 1)) m->graphs.clear();
    m->tail = on == 1;
    return 0;
} LSL_API_CATCH
int32_t lsl_model_tail(const lsl_model *m) { return m && m->tail ? 1 : 0; }
int lsl_model_set_ln_fuse(lsl_model *m, int32_t on) try {
    if (!m || (on != 0 && on != 1)) return fail(-1, "ln_fuse must be 0 or 1");
    if (on && ln_fuse_env() == 0) return fail(-21, "LayerNorm fusion is disabled (LSL_LN_FUSE=0)");
    if (m->ln_fuse != (on == 1)) m->graphs.clear();
    m->ln_fuse = on == 1;
    return 0;
} LSL_API_CATCH
int32_t lsl_model_ln_fuse(const lsl_model *m) { return m && m->ln_fuse ? 1 : 0; }
const char *lsl_profile_kernel_name(const lsl_model *m) { return m ? m->prof.name : ""; }

int32_t lsl_pass_size(const lsl_model *m, int32_t B, int32_t T, int32_t L) {
    if (!m || B <= 0 || T <= 0 || L <= 0) return 0;
    return default_chunk(m, B, T, L);
}

#ifdef LSL_EXPERIMENTS
// tools only: read and clear the phase clock of k_resident (cycles of workgroup 0 / wave 0 per phase)
int lsl_debug_res_stamps(unsigned long long *out8) {
    hipDeviceSynchronize();
    unsigned long long z[8] = {0};
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_res_stamps), sizeof(z)) != hipSuccess) return fail(-10, "stamps");
    hipMemcpyToSymbol(HIP_SYMBOL(g_res_stamps), z, sizeof(z));
    return 0;
}
#endif

int32_t lsl_sampler_path(const lsl_model *m, int32_t T, int32_t L) {
    if (!m || T <= 0 || L <= 0) return -1;
    return resident_ok(m, T, L) && m->prof.kernel < 0 ? 1 : 0;  // (per-kernel profiling runs the general kernels: lsl_sample below)
}

size_t lsl_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L) {
    if (!m || B <= 0 || T <= 0 || L <= 0) return 0;
    return workspace_need(m, B, T, L);
}

// the passes of one network evaluation at per-trajectory times: io->out = network(io->x, io->t, ...) (lsl_forward, and the middle of lsl_si_loss)
static int forward_passes(lsl_model *m, const lsl_io *io, const Workspace &ws, const CallPlans &plans, int chunk, hipStream_t st) {
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

int lsl_forward(lsl_model *m, const lsl_io *io, void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    int chunk = 0;
    if (int rc = check_call(m, io, workspace_bytes, workspace, &chunk)) return rc;
    if (!io->t || !io->out) return fail(-3, "t and out are required");
    hipStream_t st = (hipStream_t)stream;
    const Workspace ws = carve(m, (char *)workspace, chunk, io->T, io->L);
    CallPlans plans;
    if (int rc = plan_call(m, ws, io, chunk, m->MODW, plans)) return rc;  // (per-trajectory times: a modulation row per trajectory)
    return forward_passes(m, io, ws, plans, chunk, st);
} LSL_API_CATCH

// ---- stochastic-interpolant objective (k_siloss.hip.h) ----
static_assert(sizeof(lsl_si_row) == sizeof(SiRow) && sizeof(SiRow) == 24 && LSL_SI_SLAB == LSL_SI_SLAB_ELEMS, "lsl_si_row layout / slab size");
static size_t si_slabs(uint64_t per) { return (size_t)((per + LSL_SI_SLAB_ELEMS - 1) / LSL_SI_SLAB_ELEMS); }
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the two reduction launches; arguments already checked
static int si_reduce_enqueue(const float *pred, const float *x1, const float *x0, const lsl_si_row *rows, int B, uint64_t per, float *loss,
                             float *partial, hipStream_t st) {
    const size_t slabs = si_slabs(per);
    const bool vec = per % 4 == 0 && aligned16(pred) && aligned16(x1) && aligned16(x0);
    for (int b0 = 0; b0 < B; b0 += 65535) {  // (a grid has at most 65535 rows)
        const dim3 grid((unsigned)slabs, (unsigned)std::min(B - b0, 65535));
        const size_t o = (size_t)b0 * per;
        if (vec)
            hipLaunchKernelGGL(k_si_loss_partial<true>, grid, dim3(256), 0, st, partial + (size_t)b0 * slabs, pred + o, x1 + o, x0 + o,
                               (const SiRow *)rows + b0, (unsigned long long)per);
        else
            hipLaunchKernelGGL(k_si_loss_partial<false>, grid, dim3(256), 0, st, partial + (size_t)b0 * slabs, pred + o, x1 + o, x0 + o,
                               (const SiRow *)rows + b0, (unsigned long long)per);
    }
    hipLaunchKernelGGL(k_si_loss_final, dim3((unsigned)B), dim3(64), 0, st, loss, (const float *)partial, (const SiRow *)rows, (int)slabs,
                       (unsigned long long)per);
    LSL_CHECK_LAUNCH("si loss reduction");
    return 0;
}

static size_t si_scratch_bytes(int32_t B, uint64_t per_trajectory) {  // one float per (trajectory, slab)
    if (B <= 0 || per_trajectory == 0 || per_trajectory > ((uint64_t)1 << 31)) return 0;
    return (size_t)B * si_slabs(per_trajectory) * sizeof(float);
}

size_t lsl_si_loss_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L) {
    const size_t fwd = lsl_workspace_bytes(m, B, T, L);
    if (!fwd) return 0;
    return align_up(fwd, 256) + align_up(si_scratch_bytes(B, (uint64_t)T * L * m->d.in_dim), 256);  // (the partial sums live behind the forward's scratch)
}

int lsl_si_reduce(const float *pred, const float *x1, const float *x0, const lsl_si_row *rows, int32_t B, uint64_t per_trajectory, float *loss,
                  void *scratch, size_t scratch_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pred || !x1 || !x0 || !rows || !loss) return fail(-1, "null argument");
    if (B <= 0 || per_trajectory == 0) return fail(-3, "B and per_trajectory must be positive");
    if (per_trajectory > ((uint64_t)1 << 31)) return fail(-3, "per_trajectory too large");
    const size_t need = si_scratch_bytes(B, per_trajectory);
    if (!scratch || scratch_bytes < need) return fail(-4, "scratch too small: need %zu bytes, got %zu", need, scratch_bytes);
    return si_reduce_enqueue(pred, x1, x0, rows, B, per_trajectory, loss, (float *)scratch, (hipStream_t)stream);
} LSL_API_CATCH

int lsl_si_loss(lsl_model *m, const lsl_io *io, const float *x1, const float *x0, const lsl_si_row *rows, float *loss, void *workspace,
                size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    int chunk = 0;
    if (int rc = check_call(m, io, workspace_bytes, workspace, &chunk)) return rc;
    if (!io->t || !io->out) return fail(-3, "t and out are required");
    if (!x1 || !x0 || !rows || !loss) return fail(-1, "null argument");
    const size_t need = lsl_si_loss_workspace_bytes(m, io->B, io->T, io->L);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const Workspace ws = carve(m, (char *)workspace, chunk, io->T, io->L);
    CallPlans plans;
    if (int rc = plan_call(m, ws, io, chunk, m->MODW, plans)) return rc;  // (before the first launch: a refused call enqueues nothing)
    const uint64_t per = (uint64_t)io->T * io->L * m->d.in_dim, total = per * (uint64_t)io->B;
    const bool vec = per % 4 == 0 && aligned16(io->x) && aligned16(x1) && aligned16(x0);
    const unsigned grid = (unsigned)std::min<uint64_t>(((vec ? total / 4 : total) + 255) / 256, (uint64_t)device_cus() * 16);
    if (vec)
        hipLaunchKernelGGL(k_si_mix<true>, dim3(grid), dim3(256), 0, st, io->x, x1, x0, (const SiRow *)rows, (unsigned long long)per, (unsigned long long)total);
    else
        hipLaunchKernelGGL(k_si_mix<false>, dim3(grid), dim3(256), 0, st, io->x, x1, x0, (const SiRow *)rows, (unsigned long long)per, (unsigned long long)total);
    LSL_CHECK_LAUNCH("k_si_mix");
    if (int rc = forward_passes(m, io, ws, plans, chunk, st)) return rc;
    float *partial = (float *)((char *)workspace + align_up(lsl_workspace_bytes(m, io->B, io->T, io->L), 256));
    return si_reduce_enqueue(io->out, x1, x0, rows, io->B, per, loss, partial, st);
} LSL_API_CATCH

// ---- geometry losses of the decoded positions (k_geomloss.hip.h) ----
int lsl_geom_loss_sums(const float *pred, const float *target, const uint8_t *mask, int32_t F, int32_t A, int32_t D, float *sums, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pred || !target || !mask || !sums) return fail(-1, "null argument");
    if (F <= 0) return fail(-3, "F must be positive");
    if (A < 1 || A > LSL_GEOM_MAX_A) return fail(-3, "A = %d outside the native form (1..%d entities)", A, LSL_GEOM_MAX_A);
    if (D < 1 || D > LSL_GEOM_MAX_D) return fail(-3, "D = %d outside the native form (1..%d coordinates)", D, LSL_GEOM_MAX_D);
    hipStream_t st = (hipStream_t)stream;
    dispatch_d(D, [&](auto d) {
        if (loss_team(A) == 64)
            launch_geom_frame<d(), 64>(sums, pred, target, mask, F, A, st);
        else
            launch_geom_frame<d(), 256>(sums, pred, target, mask, F, A, st);
    });
    LSL_CHECK_LAUNCH("lsl_geom_loss_sums");
    return 0;
} LSL_API_CATCH

int lsl_geom_loss_final(const float *sums, int32_t F, float *out, void *stream) try {
    return loss_final<5, 0, 3>("lsl_geom_loss_final", sums, nullptr, F, out, GEOM_QUOTS, stream);
} LSL_API_CATCH

// ---- frame-local and torsion losses of the decoded peptide positions (k_peptloss.hip.h) ----
int lsl_peptide_loss_sums(const float *pred, const float *target_frame, const uint8_t *atom14_mask, const float *tors_target, const uint8_t *tors_mask,
                          const int64_t *aatype, const int8_t *restab, int32_t F, int32_t R, int32_t kind, float *sums, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pred || !target_frame || !atom14_mask || !tors_target || !tors_mask || !aatype || !restab || !sums) return fail(-1, "null argument");
    if (F <= 0) return fail(-3, "F must be positive");
    if (R < 1 || R > LSL_PEPT_MAX_R) return fail(-3, "R = %d outside the native form (1..%d residues)", R, LSL_PEPT_MAX_R);
    if (kind != 0 && kind != 1) return fail(-3, "kind = %d: 0 (MaskedCosineLoss) or 1 (MaskedCosineLossV2)", kind);
    hipStream_t st = (hipStream_t)stream;
    if (loss_team(R * 14) == 64)
        launch_peptide_frame<64>(sums, pred, target_frame, atom14_mask, tors_target, tors_mask, (const long long *)aatype, (const signed char *)restab, F, R, kind, st);
    else
        launch_peptide_frame<256>(sums, pred, target_frame, atom14_mask, tors_target, tors_mask, (const long long *)aatype, (const signed char *)restab, F, R, kind, st);
    LSL_CHECK_LAUNCH("lsl_peptide_loss_sums");
    return 0;
} LSL_API_CATCH

int lsl_peptide_loss_final(const float *geom_sums, const float *pept_sums, int32_t F, float *out, void *stream) try {
    return loss_final<5, 4, 5>("lsl_peptide_loss_final", geom_sums, pept_sums, F, out, PEPT_QUOTS, stream);
} LSL_API_CATCH

// ---- displacement errors of the decoded positions: ADE / FDE and best-of-K (k_disperr.hip.h) ----
int lsl_disp_error_rows(const float *pred, const float *target, int32_t K, int32_t B, int32_t Tp, int32_t t0p, int32_t Tt, int32_t t0t, int32_t Tf,
                        int32_t A, int32_t D, float *rows, float *traj, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pred || !target || !rows) return fail(-1, "null argument");
    if (K < 1 || B < 1) return fail(-3, "K = %d and B = %d must be positive", K, B);
    if ((long long)K * B > LSL_DISP_MAX_UNITS) return fail(-3, "K * B = %lld sample trajectories: at most %lld", (long long)K * B, LSL_DISP_MAX_UNITS);
    if (A < 1) return fail(-3, "A = %d: at least one agent", A);
    if (D < 1 || D > LSL_DISP_MAX_D) return fail(-3, "D = %d outside the native form (1..%d coordinates)", D, LSL_DISP_MAX_D);
    if (Tf < 1) return fail(-3, "Tf = %d: at least one future frame", Tf);
    if (t0p < 0 || (long long)t0p + Tf > Tp) return fail(-3, "frames %d..%d outside pred's %d frames", t0p, t0p + Tf - 1, Tp);
    if (t0t < 0 || (long long)t0t + Tf > Tt) return fail(-3, "frames %d..%d outside target's %d frames", t0t, t0t + Tf - 1, Tt);
    hipStream_t st = (hipStream_t)stream;
    const long long units = (long long)K * B;
    dispatch_d(D, [&](auto d) {
        if (loss_team(A) == 64)
            launch_disp_rows<d(), 64>(rows, traj, pred, target, units, B, Tp, t0p, Tt, t0t, Tf, A, st);
        else
            launch_disp_rows<d(), 256>(rows, traj, pred, target, units, B, Tp, t0p, Tt, t0t, Tf, A, st);
    });
    LSL_CHECK_LAUNCH("lsl_disp_error_rows");
    return 0;
} LSL_API_CATCH

int lsl_disp_error_final(const float *rows, const float *traj, const uint8_t *mask, int32_t K, int32_t num_runs, int32_t B, int32_t A, float *agents,
                         double *totals, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!rows || !agents || !totals) return fail(-1, "null argument");
    if (K < 1 || B < 1 || A < 1) return fail(-3, "K = %d, B = %d and A = %d must be positive", K, B, A);
    if (num_runs < 1 || num_runs > K) return fail(-3, "num_runs = %d outside 1..K = %d", num_runs, K);
    hipLaunchKernelGGL(k_disp_final, dim3(1), dim3(256), 0, (hipStream_t)stream, agents, totals, rows, traj, mask, (int)num_runs, (int)B, (int)A);
    LSL_CHECK_LAUNCH("lsl_disp_error_final");
    return 0;
} LSL_API_CATCH

// ---- torsion statistics of a sampled peptide trajectory: dihedrals, histograms, lagged products, JS distance (k_torsstat.hip.h) ----
int lsl_dihedral_angles(const float *pos, const int32_t *quads, const int32_t *quads_host, int64_t F, int32_t A, int32_t Q, float *angles,
                        void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pos || !quads || !quads_host || !angles) return fail(-1, "null argument");
    if (A < 1 || A > LSL_TORS_MAX_A) return fail(-3, "A = %d outside the native form (1..%d atoms of a frame)", A, LSL_TORS_MAX_A);
    if (Q < 1 || Q > LSL_TORS_MAX_Q) return fail(-3, "Q = %d outside 1..%d quadruples", Q, LSL_TORS_MAX_Q);
    const int fpb = LSL_TORS_LDS_ATOMS / A;
    if (F < 1 || (F + fpb - 1) / fpb > 0x7fffffffLL) return fail(-3, "F = %lld frames: 1 .. %lld at A = %d", (long long)F, 0x7fffffffLL * fpb, A);
    for (int i = 0; i < 4 * Q; ++i)
        if (quads_host[i] < 0 || quads_host[i] >= A)
            return fail(-3, "quads[%d][%d] = %d outside the frame's atoms 0..%d", i / 4, i % 4, quads_host[i], A - 1);
    hipLaunchKernelGGL(k_dihedral, dim3((unsigned)((F + fpb - 1) / fpb)), dim3(256), 0, (hipStream_t)stream, angles, pos, (const int *)quads,
                       (long long)F, (int)A, (int)Q, fpb);
    LSL_CHECK_LAUNCH("lsl_dihedral_angles");
    return 0;
} LSL_API_CATCH

int lsl_histogram(const float *x, int32_t S, int32_t n, int32_t Q, const double *edges, int32_t bins, int64_t *counts, const int32_t *pairs,
                  const int32_t *pairs_host, int32_t P, const double *edges2a, const double *edges2b, int32_t bins2, int64_t *counts2,
                  void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !edges || !counts) return fail(-1, "null argument");
    if (S < 1 || S > 65535) return fail(-3, "S = %d outside 1..65535 series", S);
    if (n < 1 || Q < 1) return fail(-3, "n = %d and Q = %d must be positive", n, Q);
    if (bins < 1 || bins > LSL_HIST_MAX_BINS) return fail(-3, "bins = %d outside 1..%d", bins, LSL_HIST_MAX_BINS);
    const int qt = std::min<int>(Q, LSL_HIST_CELLS / bins);
    if ((Q + qt - 1) / qt > 65535) return fail(-3, "Q = %d columns of %d bins: at most %d", Q, bins, 65535 * qt);
    if (P < 0 || P > 65535) return fail(-3, "P = %d outside 0..65535 pairs", P);
    if (P > 0) {
        if (!pairs || !pairs_host || !edges2a || !edges2b || !counts2) return fail(-1, "null argument (P > 0 needs pairs, their host copy, both edge tables and counts2)");
        if (bins2 < 1 || bins2 > LSL_HIST2_MAX_BINS) return fail(-3, "bins2 = %d outside 1..%d", bins2, LSL_HIST2_MAX_BINS);
        for (int i = 0; i < 2 * P; ++i)
            if (pairs_host[i] < 0 || pairs_host[i] >= Q) return fail(-3, "pairs[%d][%d] = %d outside the columns 0..%d", i / 2, i % 2, pairs_host[i], Q - 1);
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned tb = (unsigned)(((long long)n + LSL_HIST_ROWS - 1) / LSL_HIST_ROWS);
    hipLaunchKernelGGL(k_hist1, dim3(tb, (unsigned)((Q + qt - 1) / qt), (unsigned)S), dim3(256), 0, st, (unsigned long long *)counts, x, edges, (int)n,
                       (int)Q, (int)bins, qt);
    LSL_CHECK_LAUNCH("lsl_histogram");
    if (P > 0) {
        hipLaunchKernelGGL(k_hist2, dim3(tb, (unsigned)P, (unsigned)S), dim3(256), 0, st, (unsigned long long *)counts2, x, (const int *)pairs, edges2a,
                           edges2b, (int)n, (int)Q, (int)P, (int)bins2);
        LSL_CHECK_LAUNCH("lsl_histogram (pairs)");
    }
    return 0;
} LSL_API_CATCH

static const char *lag_shape_error(int32_t S, int32_t n, int32_t C, int32_t nlag) {
    if (S < 1 || C < 1 || (long long)S * C > LSL_LAG_MAX_ROWS) return "S and C must be positive and S * C at most 65535 (series x channels of one call)";
    if (n < 1) return "n must be positive";
    if (nlag < 0 || nlag >= n) return "nlag outside 0..n-1 (lag k has n - k terms)";
    if ((long long)nlag + 1 > LSL_LAG_MAX_PART) return "nlag + 1 above 2^21 lags";
    return nullptr;
}

size_t lsl_lag_products_workspace_bytes(int32_t S, int32_t n, int32_t C, int32_t nlag) {
    if (lag_shape_error(S, n, C, nlag)) return 0;
    return (size_t)S * C * lag_segments(n, nlag).nseg * ((size_t)nlag + 1) * sizeof(double);
}

int lsl_lag_products(const float *x, int32_t S, int32_t n, int32_t C, int32_t nlag, float *ac, void *workspace, size_t workspace_bytes,
                     void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !ac || !workspace) return fail(-1, "null argument");
    if (const char *why = lag_shape_error(S, n, C, nlag)) return fail(-3, "S = %d, n = %d, C = %d, nlag = %d: %s", S, n, C, nlag, why);
    const size_t need = lsl_lag_products_workspace_bytes(S, n, C, nlag);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    const LagSplit sp = lag_segments(n, nlag);
    hipStream_t st = (hipStream_t)stream;
    const unsigned tiles = (unsigned)((nlag + LSL_LAG_TILE) / LSL_LAG_TILE);  // ceil((nlag + 1) / tile)
    hipLaunchKernelGGL(k_lag_partial, dim3(tiles, (unsigned)sp.nseg, (unsigned)(S * C)), dim3(LSL_LAG_TILE), 0, st, (double *)workspace, x, (int)n, (int)C,
                       (int)nlag, sp.cps);
    LSL_CHECK_LAUNCH("lsl_lag_products");
    hipLaunchKernelGGL(k_lag_final, dim3((unsigned)((nlag + 256) / 256), (unsigned)(S * C)), dim3(256), 0, st, ac, (const double *)workspace, (int)n,
                       (int)nlag, sp.nseg);
    LSL_CHECK_LAUNCH("lsl_lag_products (final)");
    return 0;
} LSL_API_CATCH

int lsl_js_distance(const int64_t *counts_a, const int64_t *counts_b, int32_t rows, int32_t bins, double *out, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts_a || !counts_b || !out) return fail(-1, "null argument");
    if (rows < 1 || bins < 1) return fail(-3, "rows = %d and bins = %d must be positive", rows, bins);
    hipLaunchKernelGGL(k_js, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, out, (const long long *)counts_a, (const long long *)counts_b, (int)bins);
    LSL_CHECK_LAUNCH("lsl_js_distance");
    return 0;
} LSL_API_CATCH

// ---- structure statistics of a sampled peptide trajectory: pair distances, per-frame statistics, column histograms, density JS (k_structstat.hip.h) ----
int lsl_pair_distances(const float *pos, const int32_t *pairs, const int32_t *pairs_host, int64_t F, int32_t A, int32_t P, float *dist,
                       void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pos || !pairs || !pairs_host || !dist) return fail(-1, "null argument");
    if (A < 1 || A > LSL_TORS_MAX_A) return fail(-3, "A = %d outside the native form (1..%d atoms of a frame)", A, LSL_TORS_MAX_A);
    if (P < 1 || P > LSL_PAIR_MAX_P) return fail(-3, "P = %d outside 1..%d pairs", P, LSL_PAIR_MAX_P);
    const int fpb = LSL_TORS_LDS_ATOMS / A;
    if (F < 1 || (F + fpb - 1) / fpb > 0x7fffffffLL) return fail(-3, "F = %lld frames: 1 .. %lld at A = %d", (long long)F, 0x7fffffffLL * fpb, A);
    for (int i = 0; i < 2 * P; ++i)
        if (pairs_host[i] < 0 || pairs_host[i] >= A)
            return fail(-3, "pairs[%d][%d] = %d outside the frame's atoms 0..%d", i / 2, i % 2, pairs_host[i], A - 1);
    hipLaunchKernelGGL(k_pair_dist, dim3((unsigned)((F + fpb - 1) / fpb)), dim3(256), 0, (hipStream_t)stream, dist, pos, (const int *)pairs,
                       (long long)F, (int)A, (int)P, fpb);
    LSL_CHECK_LAUNCH("lsl_pair_distances");
    return 0;
} LSL_API_CATCH

int lsl_ca_frame_stats(const float *pos, const int32_t *sel, const int32_t *sel_host, int64_t F, int32_t A, int32_t R, float clash_thr,
                       float break_thr, float contact_thr, float *rg, int32_t *flags, int64_t *tally, int64_t *contacts, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pos || !sel || !sel_host) return fail(-1, "null argument");
    if (A < 1) return fail(-3, "A = %d must be positive", A);
    if (R < 1 || R > LSL_CA_MAX_R) return fail(-3, "R = %d outside 1..%d selected atoms", R, LSL_CA_MAX_R);
    const int tf = std::min<int>(LSL_CA_TILE, LSL_CA_LDS_ATOMS / R);
    if (F < 1 || (F + tf - 1) / tf > 0x7fffffffLL) return fail(-3, "F = %lld frames: 1 .. %lld at R = %d", (long long)F, 0x7fffffffLL * tf, R);
    for (int i = 0; i < R; ++i)
        if (sel_host[i] < 0 || sel_host[i] >= A) return fail(-3, "sel[%d] = %d outside the frame's atoms 0..%d", i, sel_host[i], A - 1);
    if (!rg && !flags && !tally && !contacts) return 0;  // (nothing asked for)
    hipLaunchKernelGGL(k_ca_stats, dim3((unsigned)((F + tf - 1) / tf)), dim3(256), 0, (hipStream_t)stream, rg, (int *)flags, (unsigned long long *)tally,
                       (unsigned long long *)contacts, pos, (const int *)sel, (long long)F, (int)A, (int)R, tf, clash_thr, break_thr, contact_thr);
    LSL_CHECK_LAUNCH("lsl_ca_frame_stats");
    return 0;
} LSL_API_CATCH

int lsl_histogram_columns(const float *x, int32_t n, int32_t Q, const double *edges, int32_t bins, int64_t *counts, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !edges || !counts) return fail(-1, "null argument");
    if (n < 1 || Q < 1) return fail(-3, "n = %d and Q = %d must be positive", n, Q);
    if (bins < 1 || bins > LSL_HIST_MAX_BINS) return fail(-3, "bins = %d outside 1..%d", bins, LSL_HIST_MAX_BINS);
    const int qt = std::min<int>(Q, LSL_HCOL_CELLS / (bins + 1));
    if ((Q + qt - 1) / qt > 65535) return fail(-3, "Q = %d columns of %d bins: at most %d", Q, bins, 65535 * qt);
    const unsigned tb = (unsigned)(((long long)n + LSL_HIST_ROWS - 1) / LSL_HIST_ROWS);
    hipLaunchKernelGGL(k_hist_cols, dim3(tb, (unsigned)((Q + qt - 1) / qt)), dim3(256), 0, (hipStream_t)stream, (unsigned long long *)counts, x, edges,
                       (int)n, (int)Q, (int)bins, qt);
    LSL_CHECK_LAUNCH("lsl_histogram_columns");
    return 0;
} LSL_API_CATCH

int lsl_js_distance_density(const int64_t *counts_a, const int64_t *counts_b, const double *measure, int32_t rows, int32_t bins, double pseudo,
                            double *out, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts_a || !counts_b || !measure || !out) return fail(-1, "null argument");
    if (rows < 1 || bins < 1) return fail(-3, "rows = %d and bins = %d must be positive", rows, bins);
    hipLaunchKernelGGL(k_js_density, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, out, (const long long *)counts_a,
                       (const long long *)counts_b, measure, (int)bins, pseudo);
    LSL_CHECK_LAUNCH("lsl_js_distance_density");
    return 0;
} LSL_API_CATCH

// ---- TICA and state statistics of the peptide evaluation: lagged second moments, projection, nearest centre, transition counts (k_tica.hip.h) ----
static const char *moments_shape_error(int32_t S, int32_t n, int32_t F, int32_t lag) {
    if (S < 1 || S > 65535) return "S outside 1..65535 series";
    if (F < 1 || F > LSL_MOM_MAX_F) return "F outside the native form (1..128 features)";
    if (n < 2) return "n must be at least 2";
    if (lag < 1 || lag >= n) return "lag outside 1..n-1 (the window has n - lag rows)";
    return nullptr;
}

size_t lsl_lagged_moments_workspace_bytes(int32_t S, int32_t n, int32_t F, int32_t lag) {
    if (moments_shape_error(S, n, F, lag)) return 0;
    return (size_t)S * mom_segments(n, lag) * mom_entries(F) * sizeof(double);
}

int lsl_lagged_moments(const float *x, int32_t S, int32_t n, int32_t F, int32_t lag, double *moments, void *workspace, size_t workspace_bytes,
                       void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !moments || !workspace) return fail(-1, "null argument");
    if (const char *why = moments_shape_error(S, n, F, lag)) return fail(-3, "S = %d, n = %d, F = %d, lag = %d: %s", S, n, F, lag, why);
    const size_t need = lsl_lagged_moments_workspace_bytes(S, n, F, lag);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int nseg = mom_segments(n, lag), T = mom_block(F), nb = (F + T - 1) / T;
    const dim3 grid((unsigned)nseg, (unsigned)((nb * nb + 255) / 256), (unsigned)S);
    if (T == 2)
        hipLaunchKernelGGL(k_moments_partial<2>, grid, dim3(256), 0, st, (double *)workspace, x, (int)n, (int)F, (int)lag);
    else
        hipLaunchKernelGGL(k_moments_partial<4>, grid, dim3(256), 0, st, (double *)workspace, x, (int)n, (int)F, (int)lag);
    LSL_CHECK_LAUNCH("lsl_lagged_moments");
    const long long E = (long long)mom_entries(F);
    hipLaunchKernelGGL(k_moments_final, dim3((unsigned)((E + 255) / 256), (unsigned)S), dim3(256), 0, st, moments, (const double *)workspace, E, nseg);
    LSL_CHECK_LAUNCH("lsl_lagged_moments (final)");
    return 0;
} LSL_API_CATCH

// The bracket of a projection with running limits, lsl_project's (k_project) and lsl_project_wide's (`wide`: k_project_wide): lim's floats
// to keys, the projection, the keys back to floats.  `block`: the threads of the two one-workgroup launches, each entry's own.
static int project_with_limits(const char *entry, bool wide, unsigned block, const float *x, int n, int F, const double *mean, const double *W, int d,
                               float *y, float *lim, hipStream_t st) {
    if (lim) {
        hipLaunchKernelGGL(k_lim_keys, dim3(1), dim3(block), 0, st, lim, 2 * d);
        if (hipError_t e = hipGetLastError()) return fail(-10, "%s (limits to keys): %s", entry, hipGetErrorString(e));
    }
    if (wide)
        hipLaunchKernelGGL(k_project_wide<false>, dim3((unsigned)(((long long)n + LSL_WPROJ_ROWS - 1) / LSL_WPROJ_ROWS)), dim3(256), 0, st, y, (double *)nullptr,
                           x, mean, W, 0.0, (unsigned *)lim, n, F, d);
    else
        hipLaunchKernelGGL(k_project, dim3((unsigned)(((long long)n + LSL_PROJ_ROWS - 1) / LSL_PROJ_ROWS)), dim3(256), 0, st, y, x, mean, W, (unsigned *)lim, n, F, d);
    LSL_CHECK_LAUNCH(entry);
    if (lim) {
        hipLaunchKernelGGL(k_lim_floats, dim3(1), dim3(block), 0, st, lim, 2 * d);
        if (hipError_t e = hipGetLastError()) return fail(-10, "%s (keys to limits): %s", entry, hipGetErrorString(e));
    }
    return 0;
}

int lsl_project(const float *x, int32_t n, int32_t F, const double *mean, const double *W, int32_t d, float *y, float *lim, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !mean || !W || !y) return fail(-1, "null argument");
    if (n < 1) return fail(-3, "n = %d must be positive", n);
    if (F < 1 || F > LSL_MOM_MAX_F) return fail(-3, "F = %d outside the native form (1..%d features)", F, LSL_MOM_MAX_F);
    if (d < 1 || d > LSL_PROJ_MAX_D) return fail(-3, "d = %d outside the native form (1..%d output columns)", d, LSL_PROJ_MAX_D);
    return project_with_limits("lsl_project", false, 64, x, (int)n, (int)F, mean, W, (int)d, y, lim, (hipStream_t)stream);
} LSL_API_CATCH

// The centres clause of lsl_assign_centers and of the k-means entry points - k centres of d coordinates stay in LDS: 0, or the argument
// outside the native form ('d', then 'k').
static char centres_outside(int32_t d, int32_t k) {
    if (d < 1 || d > LSL_ASG_MAX_D) return 'd';
    if (k < 1 || k > LSL_ASG_MAX_K || (long long)k * d > LSL_ASG_CELLS) return 'k';
    return 0;
}

int lsl_assign_centers(const float *y, int32_t n, int32_t d, const float *centers, int32_t k, const int32_t *map, int32_t nstates, int32_t *labels,
                       int64_t *state_counts, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!y || !centers || !labels) return fail(-1, "null argument");
    if (n < 1) return fail(-3, "n = %d must be positive", n);
    const char outside = centres_outside(d, k);
    if (outside == 'd') return fail(-3, "d = %d outside the native form (1..%d coordinates)", d, LSL_ASG_MAX_D);
    if (outside == 'k')
        return fail(-3, "k = %d centres of d = %d outside the native form (1..%d centres, k * d <= %d: the centres stay in LDS)", k, d, LSL_ASG_MAX_K, LSL_ASG_CELLS);
    if ((map || state_counts) && (nstates < 1 || nstates > LSL_ASG_MAX_STATES))
        return fail(-3, "nstates = %d outside 1..%d (a map or a count table needs the number of states)", nstates, LSL_ASG_MAX_STATES);
    const int ra = std::min<int>(256, LSL_ASG_TILE / d);
    hipLaunchKernelGGL(k_assign, dim3((unsigned)(((long long)n + ra - 1) / ra)), dim3(256), 0, (hipStream_t)stream, (int *)labels,
                       (unsigned long long *)state_counts, y, centers, (const int *)map, (int)n, (int)d, (int)k, (int)nstates, ra);
    LSL_CHECK_LAUNCH("lsl_assign_centers");
    return 0;
} LSL_API_CATCH

int lsl_transition_counts(const int32_t *dtraj, int32_t S, int32_t n, int32_t lag, int32_t nstates, int64_t *counts, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!dtraj || !counts) return fail(-1, "null argument");
    if (S < 1 || S > 65535) return fail(-3, "S = %d outside 1..65535 series", S);
    if (n < 1) return fail(-3, "n = %d must be positive", n);
    if (lag < 1) return fail(-3, "lag = %d must be positive", lag);
    if (nstates < 1 || nstates > LSL_TR_MAX_STATES)
        return fail(-3, "nstates = %d outside the native form (1..%d: the counts of a workgroup stay in LDS)", nstates, LSL_TR_MAX_STATES);
    if (lag >= n) return 0;  // (no pair: nothing to add)
    const unsigned tb = (unsigned)(((long long)n - lag + LSL_TR_ROWS - 1) / LSL_TR_ROWS);
    hipLaunchKernelGGL(k_transitions, dim3(tb, (unsigned)S), dim3(256), 0, (hipStream_t)stream, (unsigned long long *)counts, (const int *)dtraj, (int)n,
                       (int)lag, (int)nstates);
    LSL_CHECK_LAUNCH("lsl_transition_counts");
    return 0;
} LSL_API_CATCH

// ---- Koopman-reweighted TICA on wide feature tables: weighted lagged moments, affine weights, the wide projection (k_wtica.hip.h) ----
static const char *wmom_shape_error(int32_t n, int32_t F, int32_t lag) {
    if (F < LSL_WMOM_MIN_F || F > LSL_WMOM_MAX_F) return "F outside the native form (129..2048 features; 1..128 are lsl_lagged_moments')";
    if (n < 2) return "n must be at least 2";
    if (lag < 1 || lag >= n) return "lag outside 1..n-1 (the window has n - lag rows)";
    return nullptr;
}

size_t lsl_weighted_moments_workspace_bytes(int32_t n, int32_t F, int32_t lag) {
    if (wmom_shape_error(n, F, lag)) return 0;
    return (size_t)wmom_plan(n, F, lag).nsplit * wmom_part_entries(F) * sizeof(double);
}

int lsl_weighted_moments(const float *x, int32_t n, int32_t F, int32_t lag, const double *w, double *moments, void *workspace, size_t workspace_bytes,
                         void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !moments || !workspace) return fail(-1, "null argument");
    if (const char *why = wmom_shape_error(n, F, lag)) return fail(-3, "n = %d, F = %d, lag = %d: %s", n, F, lag, why);
    const size_t need = lsl_weighted_moments_workspace_bytes(n, F, lag);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const WmomPlan p = wmom_plan(n, F, lag);
    hipLaunchKernelGGL(k_wmom_tiles, dim3((unsigned)p.jobs, (unsigned)p.nsplit), dim3(256), 0, st, (double *)workspace, x, w, (int)n, (int)F, (int)lag,
                       p.Te, p.T, p.q);
    LSL_CHECK_LAUNCH("lsl_weighted_moments");
    const long long E = 1 + 2LL * F + 3LL * F * F;
    hipLaunchKernelGGL(k_wmom_final, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, moments, (const double *)workspace, (int)F, p.nsplit);
    LSL_CHECK_LAUNCH("lsl_weighted_moments (final)");
    return 0;
} LSL_API_CATCH

int lsl_affine_weights(const float *x, int32_t m, int32_t F, const double *u, double c, double *w, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !u || !w) return fail(-1, "null argument");
    if (m < 1) return fail(-3, "m = %d must be positive", m);
    if (F < 1 || F > LSL_WMOM_MAX_F) return fail(-3, "F = %d outside the native form (1..%d features)", F, LSL_WMOM_MAX_F);
    hipLaunchKernelGGL(k_project_wide<true>, dim3((unsigned)(((long long)m + LSL_WPROJ_ROWS - 1) / LSL_WPROJ_ROWS)), dim3(256), 0, (hipStream_t)stream,
                       (float *)nullptr, w, x, (const double *)nullptr, u, c, (unsigned *)nullptr, (int)m, (int)F, 1);
    LSL_CHECK_LAUNCH("lsl_affine_weights");
    return 0;
} LSL_API_CATCH

int lsl_project_wide(const float *x, int32_t n, int32_t F, const double *mean, const double *W, int32_t d, float *y, float *lim, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !mean || !W || !y) return fail(-1, "null argument");
    if (n < 1) return fail(-3, "n = %d must be positive", n);
    if (F < LSL_WMOM_MIN_F || F > LSL_WMOM_MAX_F)
        return fail(-3, "F = %d outside the native form (%d..%d features; 1..128 are lsl_project's)", F, LSL_WMOM_MIN_F, LSL_WMOM_MAX_F);
    if (d < 1 || d > LSL_WPROJ_MAX_D) return fail(-3, "d = %d outside the native form (1..%d output columns)", d, LSL_WPROJ_MAX_D);
    return project_with_limits("lsl_project_wide", true, 128, x, (int)n, (int)F, mean, W, (int)d, y, lim, (hipStream_t)stream);
} LSL_API_CATCH

// ---- k-means fitting: one Lloyd step of S independent problems, the reverse lookup of post_process (k_kmeans.hip.h) ----
static const char *kmeans_shape_error(int32_t S, int32_t n, int32_t d, int32_t k) {
    if (S < 1 || S > LSL_KM_MAX_S) return "S outside 1..65535 series";
    if (n < 1) return "n must be positive";
    const char outside = centres_outside(d, k);
    if (outside == 'd') return "d outside the native form (1..64 coordinates)";
    if (outside == 'k') return "k outside the native form (1..1024 centres, k * d <= 8192: the centres stay in LDS)";
    return nullptr;
}

size_t lsl_kmeans_workspace_bytes(int32_t S, int32_t n, int32_t d, int32_t k) {
    if (kmeans_shape_error(S, n, d, k)) return 0;
    const size_t units = (size_t)S * km_segments(n);
    return units * ((size_t)k * d + 1) * sizeof(double) + units * ((size_t)k + 1) * sizeof(int32_t);
}

int lsl_kmeans_step(const float *y, int32_t S, int32_t n, int32_t d, float *centers, int32_t k, int32_t *labels, int64_t *counts, double *state,
                    int32_t *done, int32_t update, double rel_tol, double center_tol, void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!y || !centers || !labels || !counts || !state || !done || !workspace) return fail(-1, "null argument");
    if (const char *why = kmeans_shape_error(S, n, d, k)) return fail(-3, "S = %d, n = %d, d = %d, k = %d: %s", S, n, d, k, why);
    if (!(rel_tol >= 0.0) || !(center_tol >= 0.0)) return fail(-3, "rel_tol = %g and center_tol = %g must not be negative (0 switches a rule off)", rel_tol, center_tol);
    const size_t need = lsl_kmeans_workspace_bytes(S, n, d, k);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int nseg = km_segments(n), G = km_group(n, d, k), per = 256 / G;
    const size_t units = (size_t)S * nseg;
    double *wsum = (double *)workspace, *winert = wsum + units * k * d;
    int *wcnt = (int *)(winert + units), *wchg = wcnt + units * k;
    const dim3 grid = (G == 256) ? dim3((unsigned)nseg, (unsigned)S) : dim3((unsigned)((S + per - 1) / per));
    const int q = (k * d + G - 1) / G;  // items (c, j) per thread, at most LSL_KM_MAX_Q: the next power of two is compiled
#define LSL_KM_LAUNCH(NQ) launch_kmeans_step<NQ>(grid, st, y, centers, (int *)labels, (const int *)done, wsum, winert, wcnt, wchg, (int)S, (int)n, (int)d, (int)k, nseg, G, (int)update)
    if (q <= 1) LSL_KM_LAUNCH(1);
    else if (q <= 2) LSL_KM_LAUNCH(2);
    else if (q <= 4) LSL_KM_LAUNCH(4);
    else if (q <= 8) LSL_KM_LAUNCH(8);
    else if (q <= 16) LSL_KM_LAUNCH(16);
    else LSL_KM_LAUNCH(32);
#undef LSL_KM_LAUNCH
    LSL_CHECK_LAUNCH("lsl_kmeans_step");
    hipLaunchKernelGGL(k_kmeans_final, dim3((unsigned)S), dim3(256), 0, st, centers, (long long *)counts, state, (int *)done, (const double *)wsum,
                       (const double *)winert, (const int *)wcnt, (const int *)wchg, (int)d, (int)k, nseg, (int)update, rel_tol, center_tol);
    LSL_CHECK_LAUNCH("lsl_kmeans_step (final)");
    return 0;
} LSL_API_CATCH

int lsl_kmeans_nearest_rows(const float *y, int32_t S, int32_t n, int32_t d, const float *centers, int32_t k, int32_t *rows, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!y || !centers || !rows) return fail(-1, "null argument");
    if (const char *why = kmeans_shape_error(S, n, d, k)) return fail(-3, "S = %d, n = %d, d = %d, k = %d: %s", S, n, d, k, why);
    const int P = n <= 64 ? 1 : 64;
    const long long items = (long long)S * k;
    if ((items * P + 255) / 256 > 2147483647LL) return fail(-3, "S = %d series of k = %d centres: more than 2^31 - 1 workgroups; split the batch", S, k);
    hipLaunchKernelGGL(k_nearest_rows, dim3((unsigned)((items * P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int *)rows, y, centers, items, (int)n,
                       (int)d, (int)k, P);
    LSL_CHECK_LAUNCH("lsl_kmeans_nearest_rows");
    return 0;
} LSL_API_CATCH

// ---- reversible maximum-likelihood Markov state models: active set, the row-sum iteration, the embedded transition matrix (k_msm.hip.h) ----
static const char *msm_shape_error(int32_t S, int32_t ns) {
    if (S < 1 || S > LSL_MSM_MAX_S) return "S outside 1..65535 series";
    if (ns < 1 || ns > LSL_MSM_MAX_STATES) return "ns outside the native form (1..128 states: fp64 K of a series stays in LDS)";
    return nullptr;
}

int lsl_msm_active_set(const int64_t *counts, int32_t S, int32_t ns, int32_t *active, int32_t *n_active, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts || !active || !n_active) return fail(-1, "null argument");
    if (const char *why = msm_shape_error(S, ns)) return fail(-3, "S = %d, ns = %d: %s", S, ns, why);
    hipLaunchKernelGGL(k_msm_active, dim3((unsigned)S), dim3(128), 0, (hipStream_t)stream, (const long long *)counts, (int)ns, (int *)active, (int *)n_active);
    LSL_CHECK_LAUNCH("lsl_msm_active_set");
    return 0;
} LSL_API_CATCH

int lsl_msm_reversible_step(const int64_t *counts, const int32_t *active, int32_t S, int32_t ns, int32_t iters, int32_t maxiter, double maxerr,
                            int32_t restart, double *x, int32_t *n_iter, double *err, int32_t *done, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts || !active || !x || !n_iter || !err || !done) return fail(-1, "null argument");
    if (const char *why = msm_shape_error(S, ns)) return fail(-3, "S = %d, ns = %d: %s", S, ns, why);
    if (iters < 0 || maxiter < 0) return fail(-3, "iters = %d and maxiter = %d must not be negative", iters, maxiter);
    if (maxerr != maxerr) return fail(-3, "maxerr is NaN (a negative maxerr never stops early)");
    hipStream_t st = (hipStream_t)stream;
#define LSL_MSM_LAUNCH(NSP) hipLaunchKernelGGL(k_msm_step<NSP>, dim3((unsigned)S), dim3(LSL_MSM_PARTS * NSP), 0, st, (const long long *)counts, (const int *)active, (int)ns, (int)iters, (int)maxiter, maxerr, (int)restart, x, (int *)n_iter, err, (int *)done)
    const int pad = msm_pad(ns);
    if (pad == 32) LSL_MSM_LAUNCH(32);
    else if (pad == 64) LSL_MSM_LAUNCH(64);
    else LSL_MSM_LAUNCH(128);
#undef LSL_MSM_LAUNCH
    LSL_CHECK_LAUNCH("lsl_msm_reversible_step");
    return 0;
} LSL_API_CATCH

int lsl_msm_transition_matrix(const int64_t *counts, const int32_t *active, const double *x, int32_t S, int32_t ns, double *T, double *pi, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts || !active || !x || !T || !pi) return fail(-1, "null argument");
    if (const char *why = msm_shape_error(S, ns)) return fail(-3, "S = %d, ns = %d: %s", S, ns, why);
    hipStream_t st = (hipStream_t)stream;
#define LSL_MSM_LAUNCH(NSP) hipLaunchKernelGGL(k_msm_tmatrix<NSP>, dim3((unsigned)S), dim3(256), 0, st, (const long long *)counts, (const int *)active, x, (int)ns, T, pi)
    const int pad = msm_pad(ns);
    if (pad == 32) LSL_MSM_LAUNCH(32);
    else if (pad == 64) LSL_MSM_LAUNCH(64);
    else LSL_MSM_LAUNCH(128);
#undef LSL_MSM_LAUNCH
    LSL_CHECK_LAUNCH("lsl_msm_transition_matrix");
    return 0;
} LSL_API_CATCH

static int sample_enqueue(lsl_model *m, const lsl_io *io, const lsl_step_ex *steps, int32_t n_steps, const float *noise, uint64_t seed,
                          uint64_t elem_offset, float *trace, void *workspace, int chunk, hipStream_t st);

int lsl_sample(lsl_model *m, const lsl_io *io, const lsl_step *steps, int32_t n_steps, const float *noise, int32_t n_noise, uint64_t seed,
               uint64_t elem_offset, float *trace, void *workspace, size_t workspace_bytes, void *stream) try {
    if (!steps || n_steps <= 0) return fail(-3, "steps required");
    std::vector<lsl_step_ex> ex((size_t)n_steps);
    for (int s = 0; s < n_steps; ++s) ex[s] = lsl_step_ex{steps[s].t, steps[s].ax, steps[s].am, steps[s].aw, 0.0f, 0, s, s};
    return lsl_sample_ex(m, io, ex.data(), n_steps, noise, n_noise, seed, elem_offset, trace, n_steps, workspace, workspace_bytes, stream);
} LSL_API_CATCH

int lsl_sample_ex(lsl_model *m, const lsl_io *io, const lsl_step_ex *steps, int32_t n_steps, const float *noise, int32_t n_noise, uint64_t seed,
                  uint64_t elem_offset, float *trace, int32_t n_trace, void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    int chunk = 0;
    if (int rc = check_call(m, io, workspace_bytes, workspace, &chunk)) return rc;
    if (!steps || n_steps <= 0) return fail(-3, "steps required");
    bool plain = true, have_saved = false;
    for (int s = 0; s < n_steps; ++s) {
        const lsl_step_ex &sp = steps[s];
        if (sp.aw != 0.0f && (sp.noise_index < 0 || (noise && sp.noise_index >= n_noise)))
            return fail(-3, "step %d needs noise slice %d but only %d slices were given", s, sp.noise_index, n_noise);
        if (sp.trace_index < -1 || (trace && sp.trace_index >= n_trace))
            return fail(-3, "step %d: trace slice %d out of range (the trace buffer holds %d slices)", s, sp.trace_index, trace ? n_trace : 0);
        if (sp.as != 0.0f && !have_saved) return fail(-3, "step %d reads the saved state before any record saved one", s);
        have_saved |= (sp.flags & LSL_STEP_SAVE) != 0;
        plain &= sp.as == 0.0f && sp.flags == 0 && sp.noise_index == s && sp.trace_index == s;
    }
    hipStream_t st = (hipStream_t)stream;
    if (plain && resident_ok(m, io->T, io->L) && m->prof.kernel < 0) {  // small trajectories: the whole loop in one launch per group of updates
        std::vector<lsl_step> ps((size_t)n_steps);
        for (int s = 0; s < n_steps; ++s) ps[s] = lsl_step{steps[s].t, steps[s].ax, steps[s].am, steps[s].aw};
        return resident_sample(m, io, ps.data(), n_steps, noise, seed, elem_offset, trace, workspace, st);
    }
    // hipGraph replay (host_graph.hip.h).  LSL_GRAPH: 1 (default since round 6) for launch-bound calls (at most 64 Ki tokens per pass and 4096
    // launches) whose arguments repeat, 2 for every call of at most 4096 launches, 0 off.  Bit-identical to the eager path
    // (test_graph_replay_matches_eager_bits).  Measured on MI355X (tools/latency_small_batch.py, profiles/r06_small_launches.txt): a
    // 10-update pedestrian call (~600 launches) 3.38 -> 3.23 ms, md17_bench B = 1 (50 updates) 30.0 -> 29.2 ms: the floor of the small-batch
    // configs is the GPU-side cost of their dependent tiny kernels, replay removes the host-side gaps between them (0-4 %).
    static const int use_graph = env_int("LSL_GRAPH", 1);
    const int passes = (io->B + chunk - 1) / chunk;
    const long est_launches = (long)passes * n_steps * (8L * m->d.depth + 6);
    const bool launch_bound = (size_t)chunk * io->T * io->L <= 65536;
    if (use_graph && (launch_bound || use_graph >= 2) && m->prof.kernel < 0 && est_launches <= 4096) {
        GraphCache::Key key;  // everything the enqueued launches depend on
        auto put = [&](const void *p, size_t n) { key.insert(key.end(), (const unsigned char *)p, (const unsigned char *)p + n); };
        put(io, sizeof(*io));
        put(steps, sizeof(lsl_step_ex) * n_steps);
        put(&noise, sizeof(noise));
        put(&seed, sizeof(seed));
        put(&elem_offset, sizeof(elem_offset));
        put(&trace, sizeof(trace));
        put(&workspace, sizeof(workspace));
        put(&chunk, sizeof(chunk));
        put(&st, sizeof(st));
        const int rc = m->graphs.run(key, st, [&](hipStream_t cs) { return sample_enqueue(m, io, steps, n_steps, noise, seed, elem_offset, trace, workspace, chunk, cs); });
        if (rc) return rc < 0 ? rc : 0;  // (replayed, or captured and launched; 0: eagerly)
    }
    return sample_enqueue(m, io, steps, n_steps, noise, seed, elem_offset, trace, workspace, chunk, st);
} LSL_API_CATCH

static int sample_enqueue(lsl_model *m, const lsl_io *io, const lsl_step_ex *steps, int32_t n_steps, const float *noise, uint64_t seed,
                          uint64_t elem_offset, float *trace, void *workspace, int chunk, hipStream_t st) {
    const Workspace ws = carve(m, (char *)workspace, chunk, io->T, io->L);
    CallPlans plans;
    if (int rc = plan_call(m, ws, io, chunk, io->y ? m->MODW : 0, plans)) return rc;  // (a scalar time: one shared row without class conditioning)
    run_tables(m, ws, io->T, io->L, st);
    const size_t per = (size_t)io->T * io->L * m->d.in_dim;
    const size_t total = per * io->B;
    // no class conditioning: modulation tables per group of network records, one row each (run_mods_steps); recomputed only when a pass
    // crosses into another group (calls of at most mods_group records: once per pass).  LSL_MODS_GROUP=0: per evaluation.
    // (>= 2: at most that many records per group - the GPU suite crosses group boundaries with it)
    static const int group_on = env_int("LSL_MODS_GROUP", 1);
    const int G = (group_on && !io->y) ? (group_on >= 2 ? std::min(group_on, ws.mods_group) : ws.mods_group) : 0;
    std::vector<int> net_idx;
    std::vector<float> net_t;
    if (G) {
        net_idx.resize((size_t)n_steps);
        for (int s = 0; s < n_steps; ++s) {
            net_idx[s] = (int)net_t.size();
            if (!(steps[s].flags & LSL_STEP_NO_NETWORK)) net_t.push_back(steps[s].t);
        }
    }
    int cur_group = -1;
    return for_each_pass(m, ws, io, chunk, st, [&](const Pass &ps) -> int {  // one pass = all records for its trajectories
        for (int s = 0; s < n_steps; ++s) {
            const lsl_step_ex &sp = steps[s];
            EvalArgs e;
            e.x = io->x + ps.elem;
            e.have_y = io->y != nullptr;
            e.rec = &sp;
            if (sp.aw != 0.0f && noise) e.noise = noise + (size_t)sp.noise_index * total + ps.elem;
            e.seed = seed;
            e.elem_off = elem_offset + ps.elem;
            e.trace = trace && sp.trace_index >= 0 ? trace + (size_t)sp.trace_index * total + ps.elem : nullptr;
            e.saved = sp.as != 0.0f ? ws.saved : nullptr;  // (the pass's own copy: a pass runs all records for its trajectories)
            e.save_out = (sp.flags & LSL_STEP_SAVE) ? ws.saved : nullptr;
            if (sp.flags & LSL_STEP_NO_NETWORK) {
                launch_state_affine(e.x, (unsigned long long)ps.bc * per, step_update(e), st);
                LSL_CHECK_LAUNCH("state update");
                continue;
            }
            if (G) {
                const int k = net_idx[s], g = k / G;
                if (cur_group != g) {
                    if (int rc = run_mods_steps(m, ws, net_t.data() + (size_t)g * G, std::min(G, (int)net_t.size() - g * G), st)) return rc;
                    cur_group = g;
                }
                e.mods_ready = ws.mods_all + (size_t)(k - g * G) * m->MODW;
            }
            if (int rc = run_eval(m, ws, plans.of(ps.bc), e, st)) return rc;
        }
        return 0;
    });
}

// x_0 ~ N(0, 1) from the documented counter stream (k_small.hip.h: k_randn); the reference draws torch.randn_like(x_cond)
// (lightning_base.py:231), whose generator stream cannot be reproduced off an NVIDIA/torch build anyway.
int lsl_randn(float *x, uint64_t n, uint64_t seed, uint64_t elem_offset, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x && n) return fail(-1, "null argument");
    if (!n) return 0;
    const unsigned long long blocks = (n + 255) / 256;
    const unsigned grid = (unsigned)std::min<unsigned long long>(blocks, (unsigned long long)device_cus() * 16);
    hipLaunchKernelGGL(k_randn, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (unsigned long long)n, (unsigned long long)seed, LSL_INIT_STEP,
                       (unsigned long long)elem_offset);
    LSL_CHECK_LAUNCH("lsl_randn");
    return 0;
} LSL_API_CATCH

// ---- Runge-Kutta arithmetic of the adaptive sampler (k_small.hip.h: k_rk_*) ----
static int rk_terms(RkTerms &t, const float *const *x, const float *c, int32_t n_x) {
    if (!x || !c || n_x < 1 || n_x > 8) return fail(-3, "1 to 8 terms");
    t.n = n_x;
    for (int j = 0; j < 8; ++j) {
        t.x[j] = j < n_x ? x[j] : nullptr;
        t.c[j] = j < n_x ? c[j] : 0.0f;
        if (j < n_x && !x[j]) return fail(-1, "null term pointer");
    }
    return 0;
}
static unsigned rk_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)device_cus() * 8); }

int lsl_rk_lincomb(float *out, const float *const *x, const float *c, int32_t n_x, uint64_t n, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!out && n) return fail(-1, "null argument");
    RkTerms t;
    if (int rc = rk_terms(t, x, c, n_x)) return rc;
    if (!n) return 0;
    hipLaunchKernelGGL(k_rk_lincomb, dim3(rk_grid(n)), dim3(256), 0, (hipStream_t)stream, out, t, (unsigned long long)n);
    LSL_CHECK_LAUNCH("lsl_rk_lincomb");
    return 0;
} LSL_API_CATCH

int lsl_rk_dense(float *out, const float *a, const float *b, const float *c, const float *d, const float *e, float x, uint64_t n, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (n && (!out || !a || !b || !c || !d || !e)) return fail(-1, "null argument");
    if (!n) return 0;
    hipLaunchKernelGGL(k_rk_poly4, dim3(rk_grid(n)), dim3(256), 0, (hipStream_t)stream, out, a, b, c, d, e, x, (unsigned long long)n);
    LSL_CHECK_LAUNCH("lsl_rk_dense");
    return 0;
} LSL_API_CATCH

int lsl_rk_error_ratio(float *ratio, const float *y0, const float *y1, const float *const *k, const float *c, int32_t n_k, float atol, float rtol,
                       uint64_t n, void *scratch, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!ratio || !y0 || !y1 || !scratch) return fail(-1, "null argument");
    if (!n) return fail(-3, "empty state");
    RkTerms t;
    if (int rc = rk_terms(t, k, c, n_k)) return rc;
    const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, LSL_RK_SCRATCH_BYTES / 4);  // (fixed for a given n: the sum's order is part of the contract)
    hipLaunchKernelGGL(k_rk_error_partial, dim3(grid), dim3(256), 0, (hipStream_t)stream, (float *)scratch, y0, y1, t, atol, rtol, (unsigned long long)n);
    hipLaunchKernelGGL(k_rk_error_final, dim3(1), dim3(256), 0, (hipStream_t)stream, ratio, (const float *)scratch, (int)grid, (unsigned long long)n);
    LSL_CHECK_LAUNCH("lsl_rk_error_ratio");
    return 0;
} LSL_API_CATCH

int lsl_debug_block_ex(lsl_model *m, int32_t bi, const float *h_in, float *h_out, void *a_out, const float *mods, int32_t mod_rows, int32_t B,
                       int32_t T, int32_t L, void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    const bool args_ok = mod_rows == 1 || mod_rows == B;  // a row per trajectory, or one row shared by all of them (mod_stride 0)
    if (int rc = check_debug(m, bi, args_ok, B, T, L, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Workspace ws = carve(m, (char *)workspace, B, T, L);
    PassPlan plan;
    if (int rc = plan_pass(m, ws, B, T, L, mod_rows == 1 ? 0 : m->MODW, PlanMode::debug_block, bi, plan)) return rc;
    run_tables(m, ws, T, L, st);
    const size_t bytes = (size_t)B * T * L * m->d.hidden * 4;
    // (on the workspace's residual stream, like an evaluation: its rows are padded to whole tiles)
    hipMemcpyAsync(ws.h, h_in, bytes, hipMemcpyDeviceToDevice, st);
    if (int rc = run_block(m, ws, plan, bi, mods, st, a_out)) return rc;
    hipMemcpyAsync(h_out, ws.h, bytes, hipMemcpyDeviceToDevice, st);
    return 0;
} LSL_API_CATCH

int lsl_debug_block(lsl_model *m, int32_t bi, const float *h_in, float *h_out, const float *mods, int32_t B, int32_t T, int32_t L,
                    void *workspace, size_t workspace_bytes, void *stream) {
    return lsl_debug_block_ex(m, bi, h_in, h_out, nullptr, mods, B, B, T, L, workspace, workspace_bytes, stream);
}

int lsl_debug_taps(lsl_model *m, int32_t bi, const float *h_in, const float *mods, int32_t B, int32_t T, int32_t L, void *qkv_out,
                   void *z_out, void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    const bool args_ok = h_in && mods && qkv_out && z_out && B > 0 && T > 0 && L > 0;
    if (int rc = check_debug(m, bi, args_ok, B, T, L, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Workspace ws = carve(m, (char *)workspace, B, T, L);
    PassPlan plan;
    if (int rc = plan_pass(m, ws, B, T, L, m->MODW, PlanMode::debug_taps, bi, plan)) return rc;
    run_tables(m, ws, T, L, st);
    const size_t n = (size_t)B * T * L;
    hipMemcpyAsync(ws.h, h_in, n * m->d.hidden * 4, hipMemcpyDeviceToDevice, st);
    if (int rc = run_block(m, ws, plan, bi, mods, st)) return rc;
    if (plan.planes[bi & 1]) {
        const long chunks = (long)n * 3 * m->d.heads * (m->d.head_dim_pad / 8);  // the block left q / k / v as head-major planes: hand them out as token-major rows
        hipLaunchKernelGGL(k_planes_to_rows, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, (u16 *)qkv_out, ws.qkv, (int)n,
                           (int)((n + 255) & ~(size_t)255), 3 * m->d.heads, m->d.head_dim_pad);
    } else
        hipMemcpyAsync(qkv_out, ws.qkv, n * 3 * m->HHD * 2, hipMemcpyDeviceToDevice, st);
    hipMemcpyAsync(z_out, ws.z, n * m->K2 * 2, hipMemcpyDeviceToDevice, st);
    LSL_CHECK_LAUNCH("debug taps");
    return 0;
} LSL_API_CATCH

int lsl_debug_mods_ex(lsl_model *m, const float *t, float t_scalar, const float *y, int32_t B, float *vec_out, float *mods_out, float *tfeat_out,
                      float *hid_out, float *yhid_out, float *yemb_out, void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    // (t == NULL: the scalar time for every row - with one row the sampler's `single` route, which has no class vector)
    const bool args_ok = m && B > 0 && vec_out && mods_out && (t || !y) && (!y || m->d.vec_in_dim > 0) && ((!yhid_out && !yemb_out) || y);
    if (int rc = check_debug(m, 0, args_ok, B, 1, 1, workspace, workspace_bytes)) return rc;  // (no sub-block: index 0 always exists)
    hipStream_t st = (hipStream_t)stream;
    const Workspace ws = carve(m, (char *)workspace, B, 1, 1);
    const size_t D = m->d.hidden;
    char ylabel[sizeof(m->prof.name)] = "";
    if (y) {
        if (int rc = run_yemb(m, ws, y, B, st, yhid_out)) return rc;
        if (yemb_out) hipMemcpyAsync(yemb_out, ws.yemb, (size_t)B * D * 4, hipMemcpyDeviceToDevice, st);
        if (m->prof.kernel == 6) snprintf(ylabel, sizeof(ylabel), "%s", m->prof.name);
    }
    if (int rc = run_mods(m, ws, t, t_scalar, y ? ws.yemb : nullptr, B, vec_out, mods_out, st)) return rc;
    // (nothing behind their launches writes ws.tfeat or ws.hid: the copies see what the next layer read)
    if (tfeat_out) hipMemcpyAsync(tfeat_out, ws.tfeat, (size_t)B * 256 * 4, hipMemcpyDeviceToDevice, st);
    if (hid_out) hipMemcpyAsync(hid_out, ws.hid, (size_t)B * D * 4, hipMemcpyDeviceToDevice, st);
    if (ylabel[0]) {  // class 6 of this call: the vec_in chain, then the time chain
        char both[sizeof(m->prof.name)];
        snprintf(both, sizeof(both), "%s ; %s", ylabel, m->prof.name);
        m->prof.label(6, "%s", both);
    }
    LSL_CHECK_LAUNCH("debug mods");
    return 0;
} LSL_API_CATCH

int lsl_debug_mods(lsl_model *m, const float *t, const float *y, int32_t B, float *vec_out, float *mods_out, void *workspace,
                   size_t workspace_bytes, void *stream) {
    return lsl_debug_mods_ex(m, t, 0.0f, y, B, vec_out, mods_out, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int lsl_debug_mods_steps(lsl_model *m, const float *times, int32_t count, float *mods_out, float *vec_out, void *workspace, size_t workspace_bytes,
                         void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (int rc = check_debug(m, 0, m && times && count > 0 && mods_out, 1, 1, 1, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Workspace ws = carve(m, (char *)workspace, 1, 1, 1);
    if (count > ws.mods_group) return fail(-3, "%d records: a group of this model holds %d (0: class-conditioned, tables per evaluation)", count, ws.mods_group);
    if (int rc = run_mods_steps(m, ws, times, count, st)) return rc;
    hipMemcpyAsync(mods_out, ws.mods_all, (size_t)count * m->MODW * 4, hipMemcpyDeviceToDevice, st);
    if (vec_out) hipMemcpyAsync(vec_out, ws.vec_all, (size_t)count * m->d.hidden * 4, hipMemcpyDeviceToDevice, st);
    LSL_CHECK_LAUNCH("debug mods (group of records)");
    return 0;
} LSL_API_CATCH

int lsl_debug_embed(lsl_model *m, const float *x, const float *x_cond, const int64_t *mask, int32_t B, int32_t T, int32_t L, float *cond_emb_out,
                    float *h_out, float *hn_out, void *stats_out, void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (int rc = check_debug(m, 0, x && x_cond && mask && B > 0 && T > 0 && L > 0, B, T, L, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Workspace ws = carve(m, (char *)workspace, B, T, L);
    PassPlan plan;  // of an evaluation with one shared modulation row, as a sampler's
    if (int rc = plan_pass(m, ws, B, T, L, 0, PlanMode::eval, 0, plan)) return rc;
    if (stats_out && !plan.emb_stats) return fail(-3, "stats_out: this handle's embedding leaves no row statistics (ln_fuse, no normalize, in_dim <= 32, hidden 256 / 512)");
    const size_t n = (size_t)plan.n, D = m->d.hidden;
    if (int rc = prepare_pass(m, ws, x_cond, mask, nullptr, B, T, L, st)) return rc;
    char clabel[sizeof(m->prof.name)];
    snprintf(clabel, sizeof(clabel), "%s", m->prof.name);
    if (cond_emb_out) hipMemcpyAsync(cond_emb_out, ws.cond_emb, n * D * 4, hipMemcpyDeviceToDevice, st);
    if (int rc = run_embed(m, ws, plan, x, st, h_out)) return rc;
    if (hn_out) hipMemcpyAsync(hn_out, ws.h, n * D * 4, hipMemcpyDeviceToDevice, st);
    if (stats_out) hipMemcpyAsync(stats_out, ws.lnstat, n * sizeof(float2), hipMemcpyDeviceToDevice, st);
    if (m->prof.kernel == 5) {  // class 5 of this call: the cond embedding, then the state embedding
        char both[sizeof(m->prof.name)];
        snprintf(both, sizeof(both), "%s ; %s", clabel, m->prof.name);
        m->prof.label(5, "%s", both);
    }
    LSL_CHECK_LAUNCH("debug embed");
    return 0;
} LSL_API_CATCH

int lsl_debug_head(lsl_model *m, const float *h, const float *mods, int32_t mod_rows, float *x, float *out, const lsl_step_ex *rec, const float *noise,
                   uint64_t seed, uint64_t elem_offset, float *trace, const float *saved, float *save_out, int32_t B, int32_t T, int32_t L,
                   void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!m || !m->has_weights) return fail(-2, "weights not set");
    const bool shape_ok = B > 0 && T > 0 && L > 0 && (unsigned long long)B * T * L * (unsigned)std::max(m->d.in_dim, m->d.hidden) < (1ull << 31);
    if (!shape_ok || !h || !mods || (mod_rows != 1 && mod_rows != B) || (rec ? !x : !out)) return fail(-3, "invalid arguments");
    if (rec && ((rec->flags & LSL_STEP_NO_NETWORK) || (rec->aw != 0.0f && rec->noise_index < 0) || (rec->as != 0.0f && !saved)))
        return fail(-3, "invalid record");
    EvalArgs e;
    e.x = x;
    e.out = out;
    e.rec = rec;
    if (rec) {
        e.noise = rec->aw != 0.0f ? noise : nullptr;
        e.seed = seed;
        e.elem_off = elem_offset;
        e.trace = trace;
        e.saved = rec->as != 0.0f ? saved : nullptr;
        e.save_out = save_out;
    }
    const float *fm = mods + (size_t)m->d.depth * 6 * m->d.hidden;  // adaLN: shift, scale
    return run_head(m, h, fm, mod_rows == 1 ? 0 : m->MODW, B * T * L, T * L, e, (hipStream_t)stream);
} LSL_API_CATCH

#include "stage1_api.hip.h"

}  // extern "C"
