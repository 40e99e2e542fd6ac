// The sampling path's translation unit of liblamslide_hip.so (include/lsl_api.h): version and error report, the model handle, forward, the
// stochastic-interpolant objective around one evaluation, the samplers with their hipGraph replay, noise, Runge-Kutta state arithmetic and
// the debug taps.  Enqueues on the caller's stream: no allocation, no synchronisation, no host<->device copies.
#include "../../include/lsl_api.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "k_attn.hip.h"
#include "k_gemm.hip.h"
#define LSL_LIN1_HOST_SIDE  // the kernel body is compiled in unit_lin1.hip
#include "k_lin1.hip.h"
#include "k_lin2.hip.h"
#include "k_tail.hip.h"
#include "k_small.hip.h"
#include "k_dopri5.hip.h"
#include "k_resident.hip.h"
#include "k_jvp.hip.h"
#ifdef LSL_EXPERIMENTS  // measured-and-rejected structures, built only by tools/build_experiments.sh (never in the product library)
#include "k_gemm_pp.hip.h"        // tools/experiments/ (on the include path of tools/build_experiments.sh only)
#include "k_gemm_drain.hip.h"
#include "k_head_scalar.hip.h"    // the scalar-FMA output head
#endif

#include "host_eval.hip.h"  // (on top of host_launch.hip.h and host_common.hip.h)
#include "host_jvp.hip.h"
#include "host_dopri.hip.h"

LSL_UNIT_INFO;

// ---- what every unit reaches through host_api.hip.h: the one error buffer of the library, the units' lines of lsl_build_info() ----
namespace {
thread_local char g_err[512] = "";
std::string &unit_info() {  // (built while the units' static objects are, whichever comes first)
    static std::string lines;
    return lines;
}
}  // namespace

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

void lsl_add_unit_info(const char *line) { unit_info().append("; ").append(line); }

// ---- the kernels of the stochastic-interpolant objective (k_siloss.hip.h) are launched in unit_loss.hip ----
// k_si_loss_final calls the fragments k_loss_final calls (k_loss_frag.hip.h), and hipcc orders its instructions by whether an instance of
// k_loss_final is compiled beside it: the objective's kernels stay beside the other loss kernels, behind these two launchers.
// x = alpha_b x1 + sigma_b x0 on at most 16 workgroups per compute unit of `cus`
LSL_HIDDEN void lsl_si_mix_launch(float *x, const float *x1, const float *x0, const lsl_si_row *rows, uint64_t per, uint64_t total, int cus, hipStream_t st);
// the two reduction launches (partial: one float per trajectory and slab); arguments already checked
LSL_HIDDEN int lsl_si_reduce_launch(const float *pred, const float *x1, const float *x0, const lsl_si_row *rows, int B, uint64_t per, float *loss,
                                    float *partial, hipStream_t st);

extern "C" {

int lsl_version(void) { return LSL_VERSION; }
const char *lsl_build_info(void) {  // compiler, target, and "<unit>: <options>" of each translation unit (lam_slide_amd/_lib.py UNITS)
    static const std::string info = "clang " __clang_version__ " gfx950" + unit_info();
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

// ---- the tangent pass (host_jvp.hip.h, k_jvp.hip.h): the general path, eagerly - no trajectory-resident kernel, no hipGraph replay ----
size_t lsl_forward_jvp_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L) {
    if (!m || B <= 0 || T <= 0 || L <= 0) return 0;
    return jvp_workspace_need(m, B, T, L);
}

int lsl_forward_jvp(lsl_model *m, const lsl_io *io, const float *x_tangent, float *out_tangent, void *workspace, size_t workspace_bytes,
                    void *stream) try {
    int chunk = 0;
    if (int rc = check_jvp(m, io, x_tangent, out_tangent, workspace, workspace_bytes, &chunk)) return rc;
    DeviceGuard dev_guard_((hipStream_t)stream);
    hipStream_t st = (hipStream_t)stream;
    const Workspace ws = carve(m, (char *)workspace, chunk, io->T, io->L);
    const JvpWorkspace jw = carve_jvp(m, (char *)workspace + align_up(ws.bytes, 256), chunk, io->T, io->L);
    CallPlans plans;
    if (int rc = plan_call(m, ws, io, chunk, m->MODW, plans)) return rc;  // (before the first launch: a refused call enqueues nothing)
    return jvp_passes(m, io, ws, jw, plans, chunk, x_tangent, out_tangent, st);
} LSL_API_CATCH

int lsl_dot_rows(const float *a, const float *b, int32_t B, uint64_t per_trajectory, double *out, void *scratch, size_t scratch_bytes,
                 void *stream) try {
    static_assert(LSL_SI_SLAB % 256 == 0, "k_dot_rows_partial: whole rounds of 256 threads per slab");
    if (!a || !b || !out) return fail(-1, "null argument");
    if (B <= 0 || per_trajectory == 0) return fail(-3, "B and per_trajectory must be positive");
    if (B > 65535 || per_trajectory > ((uint64_t)1 << 31)) return fail(-3, "at most 65535 trajectories of at most 2^31 elements");
    const size_t slabs = (size_t)((per_trajectory + LSL_SI_SLAB - 1) / LSL_SI_SLAB), need = (size_t)B * slabs * sizeof(double);
    if (!scratch || scratch_bytes < need) return fail(-4, "scratch too small: need %zu bytes, got %zu", need, scratch_bytes);
    DeviceGuard dev_guard_((hipStream_t)stream);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dot_rows_partial, dim3((unsigned)slabs, (unsigned)B), dim3(256), 0, st, (double *)scratch, a, b, (unsigned long long)per_trajectory);
    hipLaunchKernelGGL(k_dot_rows_final, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, out, (const double *)scratch, (int)B, (int)slabs);
    LSL_CHECK_LAUNCH("lsl_dot_rows");
    return 0;
} LSL_API_CATCH

// ---- stochastic-interpolant objective (kernels: k_siloss.hip.h, through lsl_si_mix_launch / lsl_si_reduce_launch above) ----
static size_t si_slabs(uint64_t per) { return (size_t)((per + LSL_SI_SLAB - 1) / LSL_SI_SLAB); }

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
    return lsl_si_reduce_launch(pred, x1, x0, rows, B, per_trajectory, loss, (float *)scratch, (hipStream_t)stream);
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
    lsl_si_mix_launch(io->x, x1, x0, rows, per, total, device_cus(), st);
    LSL_CHECK_LAUNCH("k_si_mix");
    if (int rc = forward_passes(m, io, ws, plans, chunk, st)) return rc;
    float *partial = (float *)((char *)workspace + align_up(lsl_workspace_bytes(m, io->B, io->T, io->L), 256));
    return lsl_si_reduce_launch(io->out, x1, x0, rows, io->B, per, loss, partial, st);
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
    if (graph_gate(m, io, chunk, n_steps)) {
        GraphCache::Key key;  // everything the enqueued launches depend on
        key.put(*io);
        key.put(steps, sizeof(lsl_step_ex) * n_steps);
        key.put(noise);
        key.put(seed);
        key.put(elem_offset);
        key.put(trace);
        key.put(workspace);
        key.put(chunk);
        key.put(st);
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

// ---- Runge-Kutta arithmetic and the adaptive Dormand-Prince solver with its controller on the device (host_dopri.hip.h) ----
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
    const unsigned grid = rk_error_blocks(n);
    static_assert(LSL_RK_SCRATCH_BYTES / 4 == 2048, "rk_error_blocks: one partial sum per workgroup");
    hipLaunchKernelGGL(k_rk_error_partial, dim3(grid), dim3(256), 0, (hipStream_t)stream, (float *)scratch, y0, y1, t, atol, rtol, (unsigned long long)n);
    hipLaunchKernelGGL(k_rk_error_final, dim3(1), dim3(256), 0, (hipStream_t)stream, ratio, (const float *)scratch, (int)grid, (unsigned long long)n);
    LSL_CHECK_LAUNCH("lsl_rk_error_ratio");
    return 0;
} LSL_API_CATCH

size_t lsl_dopri_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L, int32_t n_out) {
    if (!m || B <= 0 || T <= 0 || L <= 0 || n_out <= 0) return 0;
    return dopri_carve(m, nullptr, B, T, L, n_out).bytes;
}
size_t lsl_dopri_each_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L, int32_t n_out, int32_t log_rows) {
    if (!m || B <= 0 || B > DOPRI_EACH_MAX_B || T <= 0 || L <= 0 || n_out <= 0 || log_rows < 0 || log_rows > LSL_DOPRI_MAX_ATTEMPTS) return 0;
    return dopri_carve(m, nullptr, B, T, L, n_out, true, log_rows).bytes;
}

int lsl_dopri_begin(lsl_model *m, const lsl_io *io, const lsl_dopri_desc *desc, const double *grid, int32_t n_out, float *out, void *workspace,
                    size_t workspace_bytes, void *stream) try {
    return dopri_begin(m, io, desc, grid, n_out, out, false, LSL_DOPRI_MAX_ATTEMPTS, workspace, workspace_bytes, stream);
} LSL_API_CATCH

int lsl_dopri_each_begin(lsl_model *m, const lsl_io *io, const lsl_dopri_desc *desc, const double *grid, int32_t n_out, float *out, int32_t log_rows,
                         void *workspace, size_t workspace_bytes, void *stream) try {
    return dopri_begin(m, io, desc, grid, n_out, out, true, log_rows, workspace, workspace_bytes, stream);
} LSL_API_CATCH

int lsl_dopri_advance(lsl_model *m, const lsl_io *io, int32_t n_attempts, void *workspace, size_t workspace_bytes, void *stream) try {
    // (n_out = 1: lsl_dopri_begin checked the room of the output times)
    return dopri_advance(m, io, n_attempts, false, 1, LSL_DOPRI_MAX_ATTEMPTS, workspace, workspace_bytes, stream);
} LSL_API_CATCH

int lsl_dopri_each_advance(lsl_model *m, const lsl_io *io, int32_t n_attempts, void *workspace, size_t workspace_bytes, void *stream) try {
    if (!m || !io) return fail(-1, "null model or io");
    const auto call = m->dopri_each.find(workspace);
    if (call == m->dopri_each.end() || call->second.B != io->B || call->second.T != io->T || call->second.L != io->L)
        return fail(-3, "no lsl_dopri_each_begin on this handle laid this workspace out for B, T, L = %d, %d, %d", io->B, io->T, io->L);
    return dopri_advance(m, io, n_attempts, true, call->second.n_out, call->second.log_rows, workspace, workspace_bytes, stream);
} LSL_API_CATCH

// ---- the augmented solve of sample_ode_likelihood: the vector [x | logp], an evaluation = a tangent pass (host_dopri.hip.h) ----
size_t lsl_dopri_logp_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L, int32_t n_out, int32_t each, int32_t log_rows) {
    if (!m || B <= 0 || B > DOPRI_EACH_MAX_B || T <= 0 || L <= 0 || n_out <= 0 || log_rows < 0 || log_rows > LSL_DOPRI_MAX_ATTEMPTS) return 0;
    return dopri_carve(m, nullptr, B, T, L, n_out, each != 0, each ? log_rows : LSL_DOPRI_MAX_ATTEMPTS, true).bytes;
}

int lsl_dopri_logp_begin(lsl_model *m, const lsl_io *io, const lsl_dopri_desc *desc, const double *grid, int32_t n_out, float *out, float *out_logp,
                         int32_t each, int32_t log_rows, const float *eps, const uint64_t *probe_seeds, void *workspace, size_t workspace_bytes,
                         void *stream) try {
    const DopriLogp logp{eps, (const unsigned long long *)probe_seeds, out_logp};
    return dopri_begin(m, io, desc, grid, n_out, out, each != 0, each ? log_rows : LSL_DOPRI_MAX_ATTEMPTS, workspace, workspace_bytes, stream, &logp);
} LSL_API_CATCH

int lsl_dopri_logp_advance(lsl_model *m, const lsl_io *io, int32_t n_attempts, void *workspace, size_t workspace_bytes, void *stream) try {
    if (!m || !io) return fail(-1, "null model or io");
    const auto call = m->dopri_logp.find(workspace);
    if (call == m->dopri_logp.end() || call->second.B != io->B || call->second.T != io->T || call->second.L != io->L)
        return fail(-3, "no lsl_dopri_logp_begin on this handle laid this workspace out for B, T, L = %d, %d, %d", io->B, io->T, io->L);
    const DopriLogp logp{call->second.eps, nullptr, call->second.out_logp};
    return dopri_advance(m, io, n_attempts, call->second.each != 0, call->second.n_out, call->second.log_rows, workspace, workspace_bytes, stream, &logp);
} LSL_API_CATCH

int lsl_rademacher(float *out, uint64_t n, uint64_t seed, uint32_t eval_index, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!out && n) return fail(-1, "null argument");
    if (!n) return 0;
    hipLaunchKernelGGL(k_rademacher, dim3(rk_grid(n)), dim3(256), 0, (hipStream_t)stream, out, (unsigned long long)n, (unsigned long long)seed, (unsigned)eval_index);
    LSL_CHECK_LAUNCH("lsl_rademacher");
    return 0;
} LSL_API_CATCH

int lsl_debug_dopri_coeffs(int32_t path_type, int32_t model_type, const float *t, int32_t n, double *out, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!t || !out || n <= 0) return fail(-3, "invalid arguments");
    if (path_type < LSL_PATH_LINEAR || path_type > LSL_PATH_VP || model_type < LSL_PRED_VELOCITY || model_type > LSL_PRED_SCORE) return fail(-3, "unknown path or model type");
    hipLaunchKernelGGL(k_dp_coeffs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)path_type, (int)model_type, t, (int)n, out);
    LSL_CHECK_LAUNCH("lsl_debug_dopri_coeffs");
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

}  // extern "C"
