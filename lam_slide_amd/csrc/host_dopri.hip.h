// The host side of the Runge-Kutta entry points (lsl_rk_*, lsl_dopri_*, lsl_dopri_each_*; kernels: k_small.hip.h k_rk_*, k_dopri5.hip.h,
// DESIGN.md 6.1): the term lists, the tableau, the layout of a solve in the caller's workspace, and the adaptive solver with its controller
// on the device - begin (the initial step), one attempt as a sequence of launches, advance (attempts, replayed as a hipGraph where the gate
// allows).  A call checks, carves and plans once, ahead of its first launch; every attempt and evaluation reads that one DopriCall.
#pragma once
#include <cmath>
#include <initializer_list>

#include "host_eval.hip.h"
#include "host_jvp.hip.h"

namespace {

// ---- Runge-Kutta arithmetic (k_small.hip.h: k_rk_*) ----
int rk_terms(RkTerms &t, const float *const *x, const float *c, int32_t n_x) {
    if (!x || !c || n_x < 1 || n_x > 8) return fail(-3, "1 to 8 terms");
    t.n = n_x;
    for (int j = 0; j < 8; ++j) {
        t.x[j] = j < n_x ? x[j] : nullptr;
        t.c[j] = j < n_x ? c[j] : 0.0f;
        if (j < n_x && !x[j]) return fail(-1, "null term pointer");
    }
    return 0;
}
unsigned rk_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)device_cus() * 8); }

// ---- adaptive Dormand-Prince with the controller on the device (k_dopri5.hip.h) ----
// The tableau of lam_slide_amd/ode.py (_DP_ALPHA, _DP_BETA, _DP_C_ERR, _DP_C_MID): the same fp64 quotients
const double DP_ALPHA[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
const double DP_BETA[6][6] = {{1.0 / 5},
                              {3.0 / 40, 9.0 / 40},
                              {44.0 / 45, -56.0 / 15, 32.0 / 9},
                              {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
                              {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656},
                              {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
const double DP_C_ERR[7] = {35.0 / 384 - 1951.0 / 21600, 0.0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720,
                            -2187.0 / 6784 + 12231.0 / 42400, 11.0 / 84 - 649.0 / 6300, -1.0 / 60};
const double DP_C_MID[7] = {6025192743.0 / 30085553152.0 / 2, 0.0, 51252292925.0 / 65400821598.0 / 2, -2691868925.0 / 45128329728.0 / 2,
                            187940372067.0 / 1594534317056.0 / 2, -1776094331.0 / 19743644256.0 / 2, 11237099.0 / 235043384.0 / 2};

// The buffers of a call inside the caller's workspace (the records a caller reads first, at the offsets of the header; the output times
// last, so that nothing in front of them depends on their number).  One copy for both forms: the batch form is one solve of B T L C
// elements, the per-trajectory form (each) B solves of T L C elements with a record, a log and a row of partial sums each.
//
// The augmented solve (logp: lsl_dopri_logp_*) adds the side part of the vector [x | logp]: behind every state-sized buffer
// a side array of B floats (side_off elements from the buffer's start: y, stage, k_1..k_7 and mid, which shares the network output's
// buffer), the probe, the tangent output, the slab partials of the dot product, the seed table; the network's workspace is the tangent pass's.
struct DopriWs {
    bool each, logp;
    int solves, log_rows;  // records; rows of a record's log
    unsigned long long n;  // state elements of a solve
    unsigned long long n_side, n_tot, side_off, per;  // logp: side elements of a solve (else 0); n + n_side; see above; elements of a trajectory
    int slabs;                                        // logp: lsl_dot_rows' slabs of a trajectory
    lsl_dopri_each_summary *summary;
    lsl_dopri_ctl *ctl;
    double *log, *grid, *dot;
    float *y, *stage, *net, *k[7], *tvec, *part0, *part1, *eps, *j;
    unsigned long long *seeds;
    char *fwd;  // the network's workspace
    size_t fwd_bytes, bytes;
};
DopriWs dopri_carve(const lsl_model *m, char *base, int B, int T, int L, int n_out, bool each = false, int log_rows = LSL_DOPRI_MAX_ATTEMPTS,
                    bool logp = false) {
    static_assert(sizeof(lsl_dopri_ctl) <= LSL_DOPRI_LOG_OFFSET - LSL_DOPRI_CTL_OFFSET && LSL_DOPRI_STATE_OFFSET % 256 == 0, "the header's offsets");
    static_assert(sizeof(lsl_dopri_ctl) == 128 && sizeof(lsl_dopri_each_summary) <= LSL_DOPRI_EACH_CTL_OFFSET - LSL_DOPRI_EACH_SUMMARY_OFFSET,
                  "the header's offsets (LSL_DOPRI_EACH_LOG_OFFSET counts 128 bytes a record)");
    const size_t n_all = (size_t)B * T * L * m->d.in_dim;
    size_t off = each ? LSL_DOPRI_EACH_STATE_OFFSET(B, log_rows) : LSL_DOPRI_STATE_OFFSET;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align_up(bytes, 256);
        return p;
    };
    auto at = [&](size_t o) { return base ? base + o : nullptr; };
    static_assert(LSL_DOPRI_LOGP_SIDE_OFFSET(0, 1) == 256, "the header's side offset: the state buffer rounded up to 256 bytes");
    auto take_state = [&] {  // a state-sized buffer (logp: with its side array behind it)
        float *p = (float *)take(n_all * 4);
        if (logp) take((size_t)B * 4);
        return p;
    };
    DopriWs w = {};
    w.each = each;
    w.logp = logp;
    w.solves = each ? B : 1;
    w.log_rows = log_rows;
    w.n = n_all / w.solves;
    w.n_side = logp ? (unsigned long long)(B / w.solves) : 0;
    w.n_tot = w.n + w.n_side;
    w.side_off = logp ? align_up(n_all * 4, 256) / 4 : 0;
    w.per = n_all / B;
    w.slabs = (int)((w.per + LSL_SI_SLAB - 1) / LSL_SI_SLAB);
    w.summary = (lsl_dopri_each_summary *)(each ? at(LSL_DOPRI_EACH_SUMMARY_OFFSET) : nullptr);
    w.ctl = (lsl_dopri_ctl *)at(each ? LSL_DOPRI_EACH_CTL_OFFSET : LSL_DOPRI_CTL_OFFSET);
    w.log = (double *)at(each ? LSL_DOPRI_EACH_LOG_OFFSET(B) : LSL_DOPRI_LOG_OFFSET);
    w.y = take_state();
    w.stage = take_state();
    w.net = take_state();
    for (auto &k : w.k) k = take_state();
    w.tvec = (float *)take((size_t)B * 4);
    const size_t part_bytes = each ? (size_t)B * rk_error_blocks(w.n_tot) * 4 : LSL_RK_SCRATCH_BYTES;
    w.part0 = (float *)take(part_bytes);
    w.part1 = (float *)take(part_bytes);
    w.fwd = take(w.fwd_bytes = logp ? jvp_workspace_need(m, B, T, L) : workspace_need(m, B, T, L));
    if (logp) {
        w.eps = (float *)take(n_all * 4);
        w.j = (float *)take(n_all * 4);
        w.dot = (double *)take((size_t)B * w.slabs * 8);
        w.seeds = (unsigned long long *)take((size_t)B * 8);
    }
    w.grid = (double *)take((size_t)n_out * 8);
    w.bytes = off;
    return w;
}
constexpr int DOPRI_EACH_MAX_B = 65535;  // a trajectory per gridDim.y

// What a call hands down to its attempts and evaluations: its buffers; the network's argument block (the stage state in, the time vector,
// the network output, the caller's conditioning), pass size, workspace and plans
// (the augmented solve: the tangent stream's scratch, the probe every evaluation reads - the caller's, or the workspace's, drawn on the
// device in front of every pass -, the side part as the kernels take it)
struct DopriLogp {  // what lsl_dopri_logp_begin is given beyond lsl_dopri_each_begin's arguments
    const float *eps;               // the probe [B,T,L,C], or null: drawn from seeds
    const unsigned long long *seeds;  // device [B] (begin copies them into the workspace), or null
    float *out_logp;                // [n_out][B]
};
struct DopriCall {
    DopriWs w;
    lsl_io in;
    int chunk = 0;
    Workspace ws;
    CallPlans plans;
    JvpWorkspace jw;
    const float *eps = nullptr;
    bool draw = false;
    DpAug aug = {};
};

// The checks every lsl_dopri_* call shares, and the call's one carving and planning (a refused call enqueues nothing).  logp: the augmented
// solve - the network's passes are tangent passes, with their checks and refusals (check_jvp), planned once here
int dopri_check(const lsl_model *m, const lsl_io *io, void *workspace, size_t workspace_bytes, int n_out, bool each, int log_rows, DopriCall &c,
                const DopriLogp *logp = nullptr) {
    if (!m || !io) return fail(-1, "null model or io");
    if (io->B <= 0 || io->T <= 0 || io->L <= 0) return fail(-3, "B, T, L must be positive");
    if ((each || logp) && io->B > DOPRI_EACH_MAX_B) return fail(-3, "B = %d: at most %d trajectories with a controller each", io->B, DOPRI_EACH_MAX_B);
    if (!workspace) return fail(-4, "workspace required");
    c.w = dopri_carve(m, (char *)workspace, io->B, io->T, io->L, n_out, each, log_rows, logp != nullptr);
    if (workspace_bytes < c.w.bytes) return fail(-4, "workspace too small: need %zu bytes, got %zu", c.w.bytes, workspace_bytes);
    c.in = *io;
    c.in.x = c.w.stage;
    c.in.t = c.w.tvec;
    c.in.out = c.w.net;
    if (logp) {
        c.draw = logp->eps == nullptr;
        c.eps = c.draw ? c.w.eps : logp->eps;
        c.aug = DpAug{c.w.n_side, c.w.side_off, logp->out_logp};
        if (int rc = check_jvp(m, &c.in, c.eps, c.w.j, c.w.fwd, c.w.fwd_bytes, &c.chunk)) return rc;
        c.ws = carve(m, c.w.fwd, c.chunk, io->T, io->L);
        c.jw = carve_jvp(m, c.w.fwd + align_up(c.ws.bytes, 256), c.chunk, io->T, io->L);
        return plan_call(m, c.ws, &c.in, c.chunk, m->MODW, c.plans);
    }
    if (int rc = check_call(m, &c.in, c.w.fwd_bytes, c.w.fwd, &c.chunk)) return rc;
    c.ws = carve(m, c.w.fwd, c.chunk, io->T, io->L);
    return plan_call(m, c.ws, &c.in, c.chunk, m->MODW, c.plans);
}

struct DpTerm {  // c x, or dt c x
    double c;
    bool times_dt;
    const float *x;
};
DpTerms dp_list(std::initializer_list<DpTerm> terms) {  // in list order
    DpTerms d = {};
    for (const DpTerm &t : terms) {
        d.c[d.n] = t.c;
        if (t.times_dt) d.dt_mask |= 1u << d.n;
        d.x[d.n++] = t.x;
    }
    return d;
}
// [y +] sum_j dt c[j] k[j], zero coefficients skipped (as the host loop skips them); y == nullptr: the sum alone
DpTerms dp_step_terms(const float *y, float *const *k, const double *c, int n_c) {
    DpTerms d = y ? dp_list({{1.0, false, y}}) : DpTerms{};
    for (int j = 0; j < n_c; ++j)
        if (c[j] != 0.0) {
            d.c[d.n] = c[j];
            d.dt_mask |= 1u << d.n;
            d.x[d.n++] = k[j];
        }
    return d;
}

// A kernel of k_dopri5.hip.h in the call's form: `blocks` workgroups per solve in x, the solves in y
#define DP_LAUNCH(w, kern, blocks, st, ...)                                                                                     \
    do {                                                                                                                          \
        if ((w).each) hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<true>), dim3(blocks, (w).solves), dim3(256), 0, st, __VA_ARGS__); \
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(kern<false>), dim3(blocks), dim3(256), 0, st, __VA_ARGS__);                       \
    } while (0)
// The same for a kernel with an augmented entry point (kern_aug, the side part as its last argument) where the call is an augmented solve
#define DP_LAUNCH_X(c, kern, blocks, st, ...)                                            \
    do {                                                                                 \
        if ((c).w.logp) DP_LAUNCH((c).w, kern##_aug, blocks, st, __VA_ARGS__, (c).aug); \
        else DP_LAUNCH((c).w, kern, blocks, st, __VA_ARGS__);                            \
    } while (0)
#define DP_FIRST_STEP(w, first, pg, st)                                                                                                     \
    do {                                                                                                                                  \
        if ((w).each)                                                                                                                     \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dp_first_step<first, true>), dim3(1, (w).solves), dim3(256), 0, st, (w).ctl, (const float *)(w).part0, \
                               (const float *)(w).part1, (int)(pg), (const double *)(w).grid, (w).n_tot);                                \
        else                                                                                                                              \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dp_first_step<first, false>), dim3(1), dim3(256), 0, st, (w).ctl, (const float *)(w).part0,        \
                               (const float *)(w).part1, (int)(pg), (const double *)(w).grid, (w).n_tot);                                \
    } while (0)

// One evaluation on the stage state at the time vector.  The plain solve: net = network(stage, tvec); the drift is formed by the launch
// behind it.  The augmented solve (`stage`: the evaluation is number ctl.nfe + stage of its trajectory; k_side: the side array of the k it
// fills): the probe draw, one tangent pass (net, j), eps . j in lsl_dot_rows' order, k_logp at the time of t + alpha dt
int dopri_eval(lsl_model *m, const DopriCall &c, int stage, double alpha, float *k_side, hipStream_t st) {
    const DopriWs &w = c.w;
    if (!w.logp) return forward_passes(m, &c.in, c.ws, c.plans, c.chunk, st);
    const lsl_dopri_ctl *ctl = w.ctl;
    const unsigned B = (unsigned)c.in.B;
    if (c.draw) {
        if (w.each) hipLaunchKernelGGL(k_dp_rademacher<true>, dim3(rk_grid(w.per), B), dim3(256), 0, st, ctl, w.eps, (const unsigned long long *)w.seeds, stage, w.per);
        else hipLaunchKernelGGL(k_dp_rademacher<false>, dim3(rk_grid(w.per), B), dim3(256), 0, st, ctl, w.eps, (const unsigned long long *)w.seeds, stage, w.per);
        LSL_CHECK_LAUNCH("dopri probe");
    }
    if (int rc = jvp_passes(m, &c.in, c.ws, c.jw, c.plans, c.chunk, c.eps, w.j, st)) return rc;
    if (w.each) {
        hipLaunchKernelGGL(k_dp_dot<true>, dim3(w.slabs, B), dim3(256), 0, st, ctl, w.dot, c.eps, (const float *)w.j, w.per);
        hipLaunchKernelGGL(k_dp_klogp<true>, dim3((B + 63) / 64), dim3(64), 0, st, ctl, k_side, (const double *)w.dot, w.slabs, alpha, w.per, (int)B);
    } else {
        hipLaunchKernelGGL(k_dp_dot<false>, dim3(w.slabs, B), dim3(256), 0, st, ctl, w.dot, c.eps, (const float *)w.j, w.per);
        hipLaunchKernelGGL(k_dp_klogp<false>, dim3((B + 63) / 64), dim3(64), 0, st, ctl, k_side, (const double *)w.dot, w.slabs, alpha, w.per, (int)B);
    }
    LSL_CHECK_LAUNCH("dopri k_logp");
    return 0;
}
// k = the drift of the evaluation just made (begin), the x part negated in the augmented solve
void dopri_drift(const DopriWs &w, unsigned eg, float *k, double alpha, hipStream_t st) {
    const lsl_dopri_ctl *ctl = w.ctl;
    if (!w.logp) DP_LAUNCH(w, k_dp_drift, eg, st, ctl, k, (const float *)w.stage, (const float *)w.net, alpha, w.n);
    else if (w.each) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dp_drift<true, true>), dim3(eg, w.solves), dim3(256), 0, st, ctl, k, (const float *)w.stage, (const float *)w.net, alpha, w.n);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dp_drift<false, true>), dim3(eg), dim3(256), 0, st, ctl, k, (const float *)w.stage, (const float *)w.net, alpha, w.n);
}
// partial = the sums of the error norm of `terms` with scale atol + rtol |y| (Hairer's d0, d1, d2) over every solve's vector
void dopri_norm(const DopriCall &c, float *partial, const RkTerms &terms, const lsl_dopri_desc &d, unsigned pg, hipStream_t st) {
    const DopriWs &w = c.w;
    const dim3 norm_grid(pg, w.solves);
    if (!w.logp)
        hipLaunchKernelGGL(k_rk_error_partial, norm_grid, dim3(256), 0, st, partial, (const float *)w.y, (const float *)w.y, terms, (float)d.atol, (float)d.rtol, w.n);
    else if (w.each)
        hipLaunchKernelGGL(k_dp_norm_aug<true>, norm_grid, dim3(256), 0, st, partial, (const float *)w.y, (const float *)w.y, terms, (float)d.atol, (float)d.rtol, w.n, c.aug);
    else
        hipLaunchKernelGGL(k_dp_norm_aug<false>, norm_grid, dim3(256), 0, st, partial, (const float *)w.y, (const float *)w.y, terms, (float)d.atol, (float)d.rtol, w.n, c.aug);
}

// lsl_dopri_begin (each = false, the log's rows = LSL_DOPRI_MAX_ATTEMPTS) and lsl_dopri_each_begin
// (logp != nullptr: lsl_dopri_logp_begin)
int dopri_begin(lsl_model *m, const lsl_io *io, const lsl_dopri_desc *desc, const double *grid, int32_t n_out, float *out, bool each, int32_t log_rows,
                void *workspace, size_t workspace_bytes, void *stream, const DopriLogp *logp = nullptr) {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!desc || !grid || !out) return fail(-1, "null argument");
    if (logp) {
        if (!logp->out_logp) return fail(-1, "null argument");
        if ((logp->eps != nullptr) == (logp->seeds != nullptr)) return fail(-3, "give the probe or the seed table, not both and not neither");
        if (desc->reverse != 1) return fail(-3, "the likelihood solve evaluates the drift at 1 - t: desc->reverse must be 1");
    }
    if (n_out <= 0) return fail(-3, "n_out must be positive");
    const lsl_dopri_desc &d = *desc;
    if (d.path_type < LSL_PATH_LINEAR || d.path_type > LSL_PATH_VP || d.model_type < LSL_PRED_VELOCITY || d.model_type > LSL_PRED_SCORE || (d.reverse != 0 && d.reverse != 1))
        return fail(-3, "unknown path type, model type or reverse flag");
    if (d.max_steps < 0 || d.max_steps > LSL_DOPRI_MAX_ATTEMPTS) return fail(-3, "max_steps %d outside 0..%d", d.max_steps, LSL_DOPRI_MAX_ATTEMPTS);
    if (log_rows < 0 || log_rows > LSL_DOPRI_MAX_ATTEMPTS) return fail(-3, "log_rows %d outside 0..%d", log_rows, LSL_DOPRI_MAX_ATTEMPTS);
    if (!(d.rtol >= 0.0) || !(d.atol >= 0.0) || !std::isfinite(d.rtol) || !std::isfinite(d.atol)) return fail(-3, "rtol and atol must be finite and non-negative");
    for (int j = 0; j < n_out; ++j)
        if (!std::isfinite(grid[j]) || (j && grid[j] < grid[j - 1])) return fail(-3, "the output times must be finite and non-decreasing");
    DopriCall c;
    if (int rc = dopri_check(m, io, workspace, workspace_bytes, n_out, each, log_rows, c, logp)) return rc;
    const DopriWs &w = c.w;
    if (logp) m->dopri_logp[workspace] = {io->B, io->T, io->L, n_out, log_rows, (int32_t)each, logp->eps, logp->out_logp};
    else if (each) m->dopri_each[workspace] = {io->B, io->T, io->L, n_out, log_rows};
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long n = w.n;
    const unsigned eg = rk_grid(w.n_tot), pg = rk_error_blocks(w.n_tot);  // (the launch shapes follow the length of the vector)
    if (c.draw) hipMemcpyAsync(w.seeds, logp->seeds, (size_t)io->B * 8, hipMemcpyDeviceToDevice, st);
    int n_lead = 1;
    while (n_lead < n_out && grid[n_lead] <= grid[0]) ++n_lead;
    for (int off = 0; off < n_out; off += 32) {
        DpGridChunk g = {};
        const int count = std::min(32, n_out - off);
        std::copy(grid + off, grid + off + count, g.g);
        hipLaunchKernelGGL(k_dp_grid, dim3(1), dim3(32), 0, st, w.grid, g, off, count);
    }
    DP_LAUNCH_X(c, k_dp_init, eg, st, w.ctl, d, out, (int)n_out, n_lead, grid[0], w.y, w.stage, (const float *)io->x, w.tvec, (int)io->B, n);
    LSL_CHECK_LAUNCH("lsl_dopri_begin");
    if (int rc = dopri_eval(m, c, 0, 0.0, w.k[0] + w.side_off, st)) return rc;
    dopri_drift(w, eg, w.k[0], 0.0, st);
    // d0 = |y|, d1 = |f0| in the error norm with scale atol + rtol |y|: the host loop's error_ratio(y0, y0, [(1.0, .)])
    RkTerms one;
    const float c_one[2] = {1.0f, -1.0f};
    const float *xs[2] = {w.y, nullptr};
    rk_terms(one, xs, c_one, 1);
    dopri_norm(c, w.part0, one, d, pg, st);
    xs[0] = w.k[0];
    rk_terms(one, xs, c_one, 1);
    dopri_norm(c, w.part1, one, d, pg, st);
    DP_FIRST_STEP(w, true, pg, st);
    // f1 = f(t0 + h0, y + h0 f0), d2 = |f1 - f0| / h0
    DP_LAUNCH_X(c, k_dp_stage, eg, st, (const lsl_dopri_ctl *)w.ctl, w.stage, (const float *)w.net, (float *)nullptr,
                dp_list({{1.0, false, w.y}, {1.0, true, w.k[0]}}), 0.0, 1.0, w.tvec, (int)io->B, n);
    LSL_CHECK_LAUNCH("lsl_dopri_begin");
    if (int rc = dopri_eval(m, c, 0, 1.0, w.k[1] + w.side_off, st)) return rc;  // (the record's nfe is 1 by now)
    dopri_drift(w, eg, w.k[1], 1.0, st);
    xs[0] = w.k[1];
    xs[1] = w.k[0];
    rk_terms(one, xs, c_one, 2);
    dopri_norm(c, w.part0, one, d, pg, st);
    DP_FIRST_STEP(w, false, pg, st);
    if (each) hipLaunchKernelGGL(k_dp_apply_each<false>, dim3(1), dim3(256), 0, st, w.ctl, (const double *)w.grid, w.summary, w.solves);
    LSL_CHECK_LAUNCH("lsl_dopri_begin");
    return 0;
}

// one attempt: six stages and evaluations, the error norm, the decision, the commit of an accepted step, the controller's update
int dopri_attempt_enqueue(lsl_model *m, const DopriCall &c, hipStream_t st) {
    const DopriWs &w = c.w;
    const unsigned long long n = w.n;
    const unsigned eg = rk_grid(w.n_tot), pg = rk_error_blocks(w.n_tot);
    const lsl_dopri_ctl *ctl = w.ctl;
    const double *grid = w.grid;
    for (int s = 0; s < 6; ++s) {
        DP_LAUNCH_X(c, k_dp_stage, eg, st, ctl, w.stage, (const float *)w.net, s ? w.k[s] : (float *)nullptr, dp_step_terms(w.y, w.k, DP_BETA[s], s + 1),
                    s ? DP_ALPHA[s - 1] : 0.0, DP_ALPHA[s], w.tvec, (int)c.in.B, n);
        LSL_CHECK_LAUNCH("dopri stage");
        if (int rc = dopri_eval(m, c, s, DP_ALPHA[s], w.k[s + 1] + w.side_off, st)) return rc;
    }
    DP_LAUNCH_X(c, k_dp_error, pg, st, ctl, w.part0, (const float *)w.y, (const float *)w.stage, (const float *)w.net, w.k[6],
                dp_step_terms(nullptr, w.k, DP_C_ERR, 7), n);
    DP_LAUNCH(w, k_dp_control, 1, st, w.ctl, w.log, w.log_rows, (const float *)w.part0, (int)pg, grid, w.n_tot);
    const float *y = w.y, *y1 = w.stage, *mid = w.net, *fa = w.k[0], *fb = w.k[6];
    DP_LAUNCH_X(c, k_dp_commit, eg, st, ctl, grid, w.y, y1, w.net, w.k[0], fb, dp_step_terms(w.y, w.k, DP_C_MID, 7),
                dp_list({{2.0, true, fb}, {-2.0, true, fa}, {-8.0, false, y1}, {-8.0, false, y}, {16.0, false, mid}}),
                dp_list({{5.0, true, fa}, {-3.0, true, fb}, {18.0, false, y}, {14.0, false, y1}, {-32.0, false, mid}}),
                dp_list({{1.0, true, fb}, {-4.0, true, fa}, {-11.0, false, y}, {-5.0, false, y1}, {16.0, false, mid}}),
                dp_list({{1.0, true, fa}}), n);
    if (w.each) hipLaunchKernelGGL(k_dp_apply_each<true>, dim3(1), dim3(256), 0, st, w.ctl, grid, w.summary, w.solves);
    else hipLaunchKernelGGL(k_dp_apply, dim3(1), dim3(1), 0, st, w.ctl, grid);
    LSL_CHECK_LAUNCH("dopri attempt");
    return 0;
}

#undef DP_LAUNCH
#undef DP_LAUNCH_X
#undef DP_FIRST_STEP

// lsl_dopri_advance, lsl_dopri_each_advance and lsl_dopri_logp_advance (n_out, log_rows, logp: what the begin call laid the workspace out
// for).  The augmented solve's attempts are enqueued eagerly: the tangent pass is not replayed as a hipGraph
int dopri_advance(lsl_model *m, const lsl_io *io, int32_t n_attempts, bool each, int n_out, int log_rows, void *workspace, size_t workspace_bytes,
                  void *stream, const DopriLogp *logp = nullptr) {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (n_attempts < 0) return fail(-3, "n_attempts must not be negative");
    DopriCall c;
    if (int rc = dopri_check(m, io, workspace, workspace_bytes, n_out, each, log_rows, c, logp)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool replay = !logp && graph_gate(m, &c.in, c.chunk, 6);
    GraphCache::Key key;  // a tag, then everything the enqueued launches depend on: pointers and sizes (the rest is in the controller records)
    if (each) key.put("dopri-each", 11);
    else key.put("dopri", 6);
    for (const void *p : {(const void *)c.in.x_cond, (const void *)c.in.mask, (const void *)c.in.y}) key.put(p);
    for (int32_t v : {c.in.B, c.in.T, c.in.L}) key.put(v);
    if (each)
        for (int32_t v : {(int32_t)n_out, (int32_t)log_rows}) key.put(v);
    key.put(workspace);
    key.put(c.chunk);
    key.put(st);
    for (int a = 0; a < n_attempts; ++a) {
        if (replay) {
            const int rc = m->graphs.run(key, st, [&](hipStream_t cs) { return dopri_attempt_enqueue(m, c, cs); });
            if (rc < 0) return rc;
            if (rc) continue;  // (replayed, or captured and launched; 0: eagerly)
        }
        if (int rc = dopri_attempt_enqueue(m, c, st)) return rc;
    }
    return 0;
}

}  // namespace
