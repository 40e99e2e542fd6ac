// Adaptive Dormand-Prince 5(4) with the step controller on the device (lsl_dopri_begin / lsl_dopri_advance; the host restatement is
// lam_slide_amd/transport.py: dopri5_solve around Sampler._vel).  The controller record (include/lsl_api.h: lsl_dopri_ctl) lives in device
// memory: every kernel reads the time, the step size and the decision of the attempt there, so an attempt's launches take the same arguments
// every time.  No kernel reads a field that another workgroup of the same launch writes: the fields are written by single-workgroup
// kernels (k_dp_init's first thread, k_dp_first_step, k_dp_control, k_dp_apply) and read by the launches behind them.
//
// State arithmetic: the contract of k_rk_* (k_small.hip.h) - rounded fp32 products added to the rounded running sum in list order, the
// error norm's fixed reduction.  Coefficients that carry the step size are formed in fp64 (dt * beta) and rounded to fp32 once, as the host
// loop hands them to lsl_rk_lincomb.  Times, the drift coefficients (vx, vm) and the controller run in fp64, products rounded one by one
// (dp_mul) so that the expressions of Transport.velocity_coeffs / _Schedule are followed rounding for rounding.
//
// Two forms of every kernel, one copy of each (template parameter EACH):
//   batch (EACH = false, lsl_dopri_begin / lsl_dopri_advance): one controller record, one solve of n = B T L C elements, gridDim.y = 1.
//   per trajectory (EACH = true, lsl_dopri_each_*): B records, B solves of n = T L C elements each.  gridDim.y = B: a workgroup works on
//     the elements of trajectory blockIdx.y alone, under that trajectory's record, with the launch shape in x, the element assignment, the
//     per-element arithmetic and the reductions of a B = 1 batch call - so trajectory b has the bits of that call on [b:b+1].  A finished
//     or failed trajectory's workgroups return at once.  k_dp_apply_each, one workgroup, moves every record on and writes the summary.
//
// The augmented solve (AUG, lsl_dopri_logp_*): the vector of a solve is [x | logp] - n state elements and n_side side
// elements behind them (batch: B T L C and B; per trajectory: T L C and 1).  The x part stays in the state-sized arrays, the side part lies
// in a small array behind each of them (DpAug).  One rule: element i of the vector is element i of the state-sized array if i < n, else
// element i - n of its side array.  Launch shapes, the element assignment and the reductions are those of the n + n_side vector; the x
// drift is negated, the side elements' k comes from k_dp_klogp behind the tangent pass.  The element-wise kernels are one copy
// (dp_init ... dp_commit below) with two entry points each: k_dp_* passes no side arrays and compiles to the plain solve.
#pragma once
#include "../../include/lsl_api.h"
#include "k_jvp.hip.h"  // (dot_rows_slab / dot_rows_total: lsl_dot_rows' order)
#include "k_small.hip.h"

// a rounded fp64 product (see rk_mul)
__device__ __forceinline__ double dp_mul(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// (vx, vm) of velocity = vx x + vm net(x, t): Transport.velocity_coeffs over _Schedule.alpha / sigma / drift_terms and score_coeffs, in
// their expression order (transport.py:158-226, path.py:21-206 of the reference)
__device__ inline void dp_velocity_coeffs(int path, int pred, double t, double &vx, double &vm) {
    if (pred == LSL_PRED_VELOCITY) {
        vx = 0.0;
        vm = 1.0;
        return;
    }
    constexpr double PI = 3.141592653589793, SMIN = 0.1, SMAX = 20.0;
    double a, s, ds, k, var;  // alpha, sigma, d sigma / dt, drift_mean = k x, drift_var
    if (path == LSL_PATH_VP) {
        const double u = 1.0 - t;
        const double lm = dp_mul(dp_mul(-0.25, dp_mul(u, u)), SMAX - SMIN) - dp_mul(dp_mul(0.5, u), SMIN);
        const double dlm = dp_mul(dp_mul(0.5, u), SMAX - SMIN) + 0.5 * SMIN;
        a = exp(lm);
        const double e2 = exp(dp_mul(2.0, lm));
        s = sqrt(1.0 - e2);
        ds = dp_mul(e2, dp_mul(2.0, dlm)) / dp_mul(-2.0, s);
        const double beta = SMIN + dp_mul(u, SMAX - SMIN);
        k = dp_mul(-0.5, beta);
        var = beta / 2.0;
    } else {
        double ratio;
        if (path == LSL_PATH_LINEAR) {
            a = t;
            s = 1.0 - t;
            ds = -1.0;
            ratio = t != 0.0 ? 1.0 / t : HUGE_VAL;
        } else {
            const double h = dp_mul(t, PI) / 2.0;
            a = sin(h);
            s = cos(h);
            ds = dp_mul(-PI / 2.0, sin(h));
            ratio = PI / dp_mul(2.0, tan(h));
        }
        k = -ratio;
        var = dp_mul(dp_mul(ratio, s), s) - dp_mul(s, ds);
    }
    double sx, sm;  // score = sx x + sm net
    if (pred == LSL_PRED_SCORE) {
        sx = 0.0;
        sm = 1.0;
    } else if (pred == LSL_PRED_NOISE) {
        sx = 0.0;
        sm = -1.0 / s;
    } else {
        const double s2 = dp_mul(s, s);
        sx = -1.0 / s2;
        sm = a / s2;
    }
    vx = -k + dp_mul(var, sx);
    vm = dp_mul(var, sm);
}

// the fp32 time the network is given for the solver time t + alpha dt (reverse: 1 - that time, as Sampler rounds _f32(1 - t))
__device__ __forceinline__ float dp_net_time(double t, double dt, double alpha, int reverse) {
    const double ts = t + dp_mul(alpha, dt);
    return reverse ? (float)(1.0 - ts) : (float)ts;
}

// A linear combination whose coefficients may carry the step size: term j is (dt c[j] if bit j of dt_mask else c[j]) x[j]
struct DpTerms {
    const float *x[8];
    double c[8];
    unsigned dt_mask;
    int n;
};
__device__ __forceinline__ RkTerms dp_terms(const DpTerms &d, double dt) {
    RkTerms r;
    r.n = d.n;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        r.x[j] = d.x[j];
        r.c[j] = (float)((d.dt_mask >> j) & 1u ? dp_mul(dt, d.c[j]) : d.c[j]);
    }
    return r;
}

// the drift of an evaluation: k[i] = fp32(vx) x[i] + fp32(vm) net[i] (Sampler._vel), (vx, vm) at the fp32 time the network was given
__device__ __forceinline__ void dp_drift_coeffs(const lsl_dopri_ctl *ctl, double alpha, double &vx, double &vm) {
    dp_velocity_coeffs(ctl->path_type, ctl->model_type, (double)dp_net_time(ctl->t, ctl->dt, alpha, ctl->reverse), vx, vm);
}
struct DpDrift {
    float vx, vm;
    __device__ DpDrift(const lsl_dopri_ctl *ctl, double alpha) {
        double x, m;
        dp_drift_coeffs(ctl, alpha, x, m);
        vx = (float)x;
        vm = (float)m;
    }
    __device__ __forceinline__ float operator()(float xi, float ni) const { return rk_mul(vx, xi) + rk_mul(vm, ni); }
};

struct DpGridChunk {
    double g[32];
};
// grid[off + i] = chunk.g[i]: the output times reach the device as kernel arguments
__global__ void k_dp_grid(double *grid, DpGridChunk chunk, int off, int count) {
    if ((int)threadIdx.x < count) grid[off + threadIdx.x] = chunk.g[threadIdx.x];
}

// The solve a workgroup belongs to: the index of its record, the offset of its first element in the state arrays, and the elements of one
// output slice out[j] (n elements per solve)
template <bool EACH>
__device__ __forceinline__ unsigned dp_solve() {
    return EACH ? blockIdx.y : 0u;
}
template <bool EACH>
__device__ __forceinline__ unsigned long long dp_base(unsigned long long n) {
    return EACH ? (unsigned long long)blockIdx.y * n : 0ull;
}
template <bool EACH>
__device__ __forceinline__ unsigned long long dp_slice(unsigned long long n) {
    return EACH ? (unsigned long long)gridDim.y * n : n;
}
// the network's time of the next evaluation, written by the first workgroup of a solve: every trajectory's entry (batch), the solve's own
template <bool EACH>
__device__ __forceinline__ void dp_set_time(float *tvec, int B, float v) {
    if (blockIdx.x != 0) return;
    if (EACH) {
        if (threadIdx.x == 0) tvec[blockIdx.y] = v;
    } else
        for (int b = threadIdx.x; b < B; b += 256) tvec[b] = v;
}

// The side part of an augmented solve: n_side elements behind the n state elements of a solve; the side array of a state-sized array p
// lies at p + side_off; the side elements of output slice j at out_side + j * (side elements of the call).  AUG = false: unused.
struct DpAug {
    unsigned long long n_side, side_off;
    float *out_side;
};
// a thread's side elements behind its state elements: where its grid-stride loop over the n + n_side vector of its solve leaves the n
// state elements - the first l = blockIdx.x 256 + threadIdx.x + m gridDim.x 256 with l >= n.  Returns l - n, its index in the side part;
// the thread's further side elements follow at the loop's stride
__device__ __forceinline__ unsigned long long dp_side_first(unsigned long long n) {
    const unsigned long long l0 = (unsigned long long)blockIdx.x * 256 + threadIdx.x, stride = (unsigned long long)gridDim.x * 256;
    return l0 >= n ? l0 - n : l0 + (n - l0 + stride - 1) / stride * stride - n;
}
template <bool EACH>
__device__ __forceinline__ unsigned long long dp_side_base(DpAug aug) {
    return EACH ? (unsigned long long)blockIdx.y * aug.n_side : 0ull;
}
template <bool EACH>
__device__ __forceinline__ unsigned long long dp_side_slice(DpAug aug) {
    return EACH ? (unsigned long long)gridDim.y * aug.n_side : aug.n_side;
}
__device__ __forceinline__ RkTerms dp_side_terms(RkTerms r, DpAug aug) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < r.n) r.x[j] += aug.side_off;
    return r;
}

// Begin: y = stage = y0, out[j] = y0 for the n_lead leading output times, the network's time vector at t0, the controller's first state
// (AUG: the side elements start at 0; the record's reverse field carries LSL_DOPRI_NEGATED)
template <bool EACH, bool AUG>
__device__ __forceinline__ void dp_init(lsl_dopri_ctl *ctl, const lsl_dopri_desc &desc, float *out, int n_out, int n_lead, double t0, float *y, float *stage,
                                        const float *y0, float *tvec, int B, unsigned long long n, DpAug aug) {
    const unsigned long long base = dp_base<EACH>(n), slice = dp_slice<EACH>(n);
    for (unsigned long long i = base + (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < base + n; i += (unsigned long long)gridDim.x * 256) {
        const float v = y0[i];
        y[i] = v;
        stage[i] = v;
        for (int j = 0; j < n_lead; ++j) out[(unsigned long long)j * slice + i] = v;
    }
    if (AUG) {
        const unsigned long long sbase = dp_side_base<EACH>(aug), sslice = dp_side_slice<EACH>(aug);
        for (unsigned long long e = dp_side_first(n); e < aug.n_side; e += (unsigned long long)gridDim.x * 256) {
            y[aug.side_off + sbase + e] = 0.0f;
            stage[aug.side_off + sbase + e] = 0.0f;
            for (int j = 0; j < n_lead; ++j) aug.out_side[(unsigned long long)j * sslice + sbase + e] = 0.0f;
        }
    }
    if (blockIdx.x != 0) return;
    dp_set_time<EACH>(tvec, B, dp_net_time(t0, 0.0, 0.0, desc.reverse));
    ctl += dp_solve<EACH>();
    if (threadIdx.x == 0) {
        lsl_dopri_ctl c = {};
        c.t = c.t_lo = t0;
        c.rtol = desc.rtol;
        c.atol = desc.atol;
        c.out = out;
        c.next_out = n_lead;
        c.n_out = n_out;
        c.max_steps = desc.max_steps;
        c.path_type = desc.path_type;
        c.model_type = desc.model_type;
        c.reverse = AUG ? desc.reverse | LSL_DOPRI_NEGATED : desc.reverse;
        *ctl = c;
    }
}
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_init(lsl_dopri_ctl *ctl, lsl_dopri_desc desc, float *out, int n_out, int n_lead, double t0, float *y, float *stage,
                                                 const float *y0, float *tvec, int B, unsigned long long n) {
    dp_init<EACH, false>(ctl, desc, out, n_out, n_lead, t0, y, stage, y0, tvec, B, n, DpAug{});
}
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_init_aug(lsl_dopri_ctl *ctl, lsl_dopri_desc desc, float *out, int n_out, int n_lead, double t0, float *y, float *stage,
                                                     const float *y0, float *tvec, int B, unsigned long long n, DpAug aug) {
    dp_init<EACH, true>(ctl, desc, out, n_out, n_lead, t0, y, stage, y0, tvec, B, n, aug);
}

// k[i] = drift of the evaluation at t + alpha dt on the stage state (begin: f0 and the evaluation of Hairer's rule).  NEG (the augmented
// solve's x part): the drift negated; its side elements are k_dp_klogp's
template <bool EACH, bool NEG = false>
__global__ void __launch_bounds__(256) k_dp_drift(const lsl_dopri_ctl *ctl, float *k, const float *stage, const float *net, double alpha, unsigned long long n) {
    const DpDrift drift(ctl + dp_solve<EACH>(), alpha);
    const unsigned long long base = dp_base<EACH>(n);
    for (unsigned long long i = base + (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < base + n; i += (unsigned long long)gridDim.x * 256)
        k[i] = NEG ? -drift(stage[i], net[i]) : drift(stage[i], net[i]);
}

// Hairer's initial step (Hairer, Norsett, Wanner I, II.4), one workgroup.  FIRST: d0 = |y|, d1 = |f0| in the error norm -> dt = h0, ratio = d1.
// Second: d2 = |f1 - f0| / h0 -> dt = min(100 h0, h1); a grid that ends at t0 is done, max_steps = 0 is a failure.
template <bool FIRST, bool EACH>
__global__ void __launch_bounds__(256) k_dp_first_step(lsl_dopri_ctl *ctl, const float *part0, const float *part1, int n_partial, const double *grid,
                                                       unsigned long long n) {
    __shared__ double red[256];
    ctl += dp_solve<EACH>();
    part0 += (size_t)dp_solve<EACH>() * n_partial;
    part1 += (size_t)dp_solve<EACH>() * n_partial;
    const double r0 = (double)rk_error_root(red, part0, n_partial, n);
    __syncthreads();
    const double r1 = FIRST ? (double)rk_error_root(red, part1, n_partial, n) : 0.0;
    if (threadIdx.x != 0) return;
    if (FIRST) {
        ctl->dt = r0 < 1e-5 || r1 < 1e-5 ? 1e-6 : dp_mul(0.01, r0) / r1;
        ctl->ratio = r1;
        ctl->nfe = 1;
        return;
    }
    const double h0 = ctl->dt, d1 = ctl->ratio, d2 = r0 / h0;
    const double h1 = d1 <= 1e-15 && d2 <= 1e-15 ? fmax(1e-6, dp_mul(h0, 1e-3)) : pow(0.01 / fmax(d1, d2), 1.0 / 5.0);
    ctl->dt = fmin(dp_mul(100.0, h0), h1);
    ctl->ratio = 0.0;
    ctl->nfe = 2;
    if (!(grid[ctl->n_out - 1] > ctl->t)) ctl->done = 1;
    else if (ctl->max_steps <= 0) {
        ctl->status = LSL_DOPRI_MAX_STEPS;
        ctl->done = 1;
    }
}

// The launch between two network evaluations.  k_prev != nullptr: k_prev = drift of the evaluation at t + alpha_prev dt (stage state and
// network output still in place); then stage = the terms' combination (y + sum_j fp32(dt beta_j) k_j) and the time vector of the next
// evaluation, t + alpha dt.
// AUG: k_prev's x part negated; the side elements of k_prev are in place (k_dp_klogp), their stage elements are the same combination
template <bool EACH, bool AUG>
__device__ __forceinline__ void dp_stage(const lsl_dopri_ctl *ctl, float *stage, const float *net, float *k_prev, const DpTerms &terms, double alpha_prev,
                                         double alpha, float *tvec, int B, unsigned long long n, DpAug aug) {
    ctl += dp_solve<EACH>();
    if (ctl->done) return;
    const unsigned long long base = dp_base<EACH>(n);
    const RkTerms r = dp_terms(terms, ctl->dt);
    if (k_prev) {
        const DpDrift drift(ctl, alpha_prev);
        for (unsigned long long i = base + (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < base + n; i += (unsigned long long)gridDim.x * 256) {
            k_prev[i] = AUG ? -drift(stage[i], net[i]) : drift(stage[i], net[i]);
            stage[i] = rk_sum(r, i);
        }
    } else {
        for (unsigned long long i = base + (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < base + n; i += (unsigned long long)gridDim.x * 256)
            stage[i] = rk_sum(r, i);
    }
    if (AUG) {
        const RkTerms rs = dp_side_terms(r, aug);
        const unsigned long long sbase = dp_side_base<EACH>(aug);
        for (unsigned long long e = dp_side_first(n); e < aug.n_side; e += (unsigned long long)gridDim.x * 256)
            stage[aug.side_off + sbase + e] = rk_sum(rs, sbase + e);
    }
    dp_set_time<EACH>(tvec, B, dp_net_time(ctl->t, ctl->dt, alpha, ctl->reverse));
}
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_stage(const lsl_dopri_ctl *ctl, float *stage, const float *net, float *k_prev, DpTerms terms, double alpha_prev,
                                                  double alpha, float *tvec, int B, unsigned long long n) {
    dp_stage<EACH, false>(ctl, stage, net, k_prev, terms, alpha_prev, alpha, tvec, B, n, DpAug{});
}
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_stage_aug(const lsl_dopri_ctl *ctl, float *stage, const float *net, float *k_prev, DpTerms terms, double alpha_prev,
                                                      double alpha, float *tvec, int B, unsigned long long n, DpAug aug) {
    dp_stage<EACH, true>(ctl, stage, net, k_prev, terms, alpha_prev, alpha, tvec, B, n, aug);
}

// Behind the last evaluation: k_last = its drift (the stage state is the 5th-order solution y1), then k_rk_error_partial's sums of
// ((sum_j fp32(dt c_err_j) k_j) / (atol + rtol max(|y|, |y1|)))^2 in k_rk_error_partial's launch shape
// (per trajectory: partial[b][gridDim.x], the blocks, the element assignment and the tree of a B = 1 call)
// AUG: k_last's x part negated, its side elements in place (k_dp_klogp); a thread adds its side elements behind its state elements - the
// order of k_rk_error_partial on the n + n_side vector
template <bool EACH, bool AUG>
__device__ __forceinline__ void dp_error(float *red, const lsl_dopri_ctl *ctl, float *partial, const float *y, const float *stage, const float *net, float *k_last,
                                         const DpTerms &err, unsigned long long n, DpAug aug) {
    ctl += dp_solve<EACH>();
    if (ctl->done) return;
    const unsigned long long base = dp_base<EACH>(n);
    const RkTerms r = dp_terms(err, ctl->dt);
    const DpDrift drift(ctl, 1.0);
    const float atol = (float)ctl->atol, rtol = (float)ctl->rtol;
    float s = 0.0f;
    for (unsigned long long i = base + (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < base + n; i += (unsigned long long)gridDim.x * 256) {
        k_last[i] = AUG ? -drift(stage[i], net[i]) : drift(stage[i], net[i]);
        s = rk_error_add(s, r, y, stage, atol, rtol, i);
    }
    if (AUG) {
        const RkTerms rs = dp_side_terms(r, aug);
        const unsigned long long sbase = dp_side_base<EACH>(aug);
        for (unsigned long long e = dp_side_first(n); e < aug.n_side; e += (unsigned long long)gridDim.x * 256)
            s = rk_error_add(s, rs, y + aug.side_off, stage + aug.side_off, atol, rtol, sbase + e);
    }
    const float total = block_tree_sum(red, s);
    if (threadIdx.x == 0) partial[(size_t)dp_solve<EACH>() * gridDim.x + blockIdx.x] = total;
}
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_error(const lsl_dopri_ctl *ctl, float *partial, const float *y, const float *stage, const float *net, float *k_last,
                                                  DpTerms err, unsigned long long n) {
    __shared__ float red[256];
    dp_error<EACH, false>(red, ctl, partial, y, stage, net, k_last, err, n, DpAug{});
}
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_error_aug(const lsl_dopri_ctl *ctl, float *partial, const float *y, const float *stage, const float *net, float *k_last,
                                                      DpTerms err, unsigned long long n, DpAug aug) {
    __shared__ float red[256];
    dp_error<EACH, true>(red, ctl, partial, y, stage, net, k_last, err, n, aug);
}
// Hairer's norms of the augmented solve at begin: k_rk_error_partial's sums (k_small.hip.h) over the n + n_side vector of every solve
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_norm_aug(float *partial, const float *y0, const float *y1, RkTerms k, float atol, float rtol, unsigned long long n,
                                                     DpAug aug) {
    __shared__ float red[256];
    const unsigned long long base = dp_base<EACH>(n), sbase = dp_side_base<EACH>(aug);
    float s = 0.0f;
    for (unsigned long long i = base + (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < base + n; i += (unsigned long long)gridDim.x * 256)
        s = rk_error_add(s, k, y0, y1, atol, rtol, i);
    const RkTerms ks = dp_side_terms(k, aug);
    for (unsigned long long e = dp_side_first(n); e < aug.n_side; e += (unsigned long long)gridDim.x * 256)
        s = rk_error_add(s, ks, y0 + aug.side_off, y1 + aug.side_off, atol, rtol, sbase + e);
    const float total = block_tree_sum(red, s);
    if (threadIdx.x == 0) partial[(size_t)dp_solve<EACH>() * gridDim.x + blockIdx.x] = total;
}

// The decision of the attempt, one workgroup: ratio (k_rk_error_final's value), accept iff ratio <= 1, the step size that follows, the output
// times an accepted step covers, the attempt's row of the log (log[solve][log_rows][4]; attempts beyond log_rows are counted, not logged).
// Writes decision fields only; k_dp_apply moves the controller on.
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_control(lsl_dopri_ctl *ctl, double *log, int log_rows, const float *partial, int n_partial, const double *grid,
                                                    unsigned long long n) {
    ctl += dp_solve<EACH>();
    if (ctl->done) return;
    __shared__ double red[256];
    const double ratio = (double)rk_error_root(red, partial + (size_t)dp_solve<EACH>() * n_partial, n_partial, n);
    if (threadIdx.x != 0) return;
    const double t = ctl->t, dt = ctl->dt;
    const int accept = ratio <= 1.0;
    double factor = 10.0;
    if (ratio != 0.0) factor = fmin(10.0, fmax(0.9 / pow(ratio, 0.2), ratio < 1.0 ? 1.0 : 0.2));
    const double t_new = t + dt;
    int j = ctl->next_out;
    if (accept)
        while (j < ctl->n_out && grid[j] <= t_new) ++j;
    ctl->ratio = ratio;
    ctl->accept = accept;
    ctl->t_new = t_new;
    ctl->dt_next = dp_mul(dt, factor);
    ctl->out_end = j;
    const int a = ctl->accepted + ctl->rejected;
    if (a >= log_rows) return;
    double *row = log + 4 * ((size_t)dp_solve<EACH>() * log_rows + a);
    row[0] = t;
    row[1] = dt;
    row[2] = ratio;
    row[3] = (double)accept;
}

// An accepted step, element-wise: the mid-point and the dense-output coefficients of dopri5_solve (each sum in its list order; the mid-point
// passes through `mid`, the network output's buffer), every pending output time of the step by rk_poly4, then y <- y1, k_1 <- k_7
// (AUG: the side elements the same way on the side arrays, into the side slices of the output)
template <bool EACH, bool AUG>
__device__ __forceinline__ void dp_commit(const lsl_dopri_ctl *ctl, const double *grid, float *y, const float *y1, float *mid, float *k_first,
                                          const float *k_last, DpTerms t_mid, DpTerms t_a, DpTerms t_b, DpTerms t_c, DpTerms t_d,
                                          unsigned long long n, DpAug aug) {
    ctl += dp_solve<EACH>();
    if (ctl->done || !ctl->accept) return;
    const unsigned long long base = dp_base<EACH>(n), slice = dp_slice<EACH>(n);
    const double dt = ctl->dt, t_lo = ctl->t, t_new = ctl->t_new;
    const int j0 = ctl->next_out, j1 = ctl->out_end;
    float *out = ctl->out;
    const RkTerms rm = dp_terms(t_mid, dt), ra = dp_terms(t_a, dt), rb = dp_terms(t_b, dt), rc = dp_terms(t_c, dt), rd = dp_terms(t_d, dt);
    const bool flat = !(t_new > t_lo);  // (a step that did not move the time: the state itself, as the host loop returns it)
    for (unsigned long long i = base + (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < base + n; i += (unsigned long long)gridDim.x * 256) {
        const float yn = y1[i];
        if (j0 < j1) {
            mid[i] = rk_sum(rm, i);
            const float a = rk_sum(ra, i), b = rk_sum(rb, i), c = rk_sum(rc, i), d = rk_sum(rd, i), e = y[i];
            for (int j = j0; j < j1; ++j)
                out[(unsigned long long)j * slice + i] = flat ? yn : rk_poly4(a, b, c, d, e, (float)((grid[j] - t_lo) / (t_new - t_lo)));
        }
        y[i] = yn;
        k_first[i] = k_last[i];
    }
    if (AUG) {
        const RkTerms sm = dp_side_terms(rm, aug), sa = dp_side_terms(ra, aug), sb = dp_side_terms(rb, aug), sc = dp_side_terms(rc, aug), sd = dp_side_terms(rd, aug);
        const unsigned long long sbase = dp_side_base<EACH>(aug), sslice = dp_side_slice<EACH>(aug), so = aug.side_off;
        for (unsigned long long e = dp_side_first(n); e < aug.n_side; e += (unsigned long long)gridDim.x * 256) {
            const unsigned long long q = sbase + e;
            const float yn = y1[so + q];
            if (j0 < j1) {
                mid[so + q] = rk_sum(sm, q);
                const float a = rk_sum(sa, q), b = rk_sum(sb, q), c = rk_sum(sc, q), d = rk_sum(sd, q), e0 = y[so + q];
                for (int j = j0; j < j1; ++j)
                    aug.out_side[(unsigned long long)j * sslice + q] = flat ? yn : rk_poly4(a, b, c, d, e0, (float)((grid[j] - t_lo) / (t_new - t_lo)));
            }
            y[so + q] = yn;
            k_first[so + q] = k_last[so + q];
        }
    }
}
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_commit(const lsl_dopri_ctl *ctl, const double *grid, float *y, const float *y1, float *mid, float *k_first,
                                                   const float *k_last, DpTerms t_mid, DpTerms t_a, DpTerms t_b, DpTerms t_c, DpTerms t_d,
                                                   unsigned long long n) {
    dp_commit<EACH, false>(ctl, grid, y, y1, mid, k_first, k_last, t_mid, t_a, t_b, t_c, t_d, n, DpAug{});
}
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_commit_aug(const lsl_dopri_ctl *ctl, const double *grid, float *y, const float *y1, float *mid, float *k_first,
                                                       const float *k_last, DpTerms t_mid, DpTerms t_a, DpTerms t_b, DpTerms t_c, DpTerms t_d,
                                                       unsigned long long n, DpAug aug) {
    dp_commit<EACH, true>(ctl, grid, y, y1, mid, k_first, k_last, t_mid, t_a, t_b, t_c, t_d, n, aug);
}

// ---- the evaluation of the augmented solve (lsl_dopri_logp_*): the probe draw in front of the tangent pass, the dot product and k_logp behind it.
// A solve's record is ctl[blockIdx.y] (per trajectory) or ctl[0] (batch); a trajectory of a done solve is left alone.
// eps[b][i] = +-1 for (seeds[b], ctl.nfe + stage, i): the trajectory's own evaluation count, the index inside the trajectory.  grid (., B)
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_rademacher(const lsl_dopri_ctl *ctl, float *eps, const unsigned long long *seeds, int stage, unsigned long long per) {
    ctl += dp_solve<EACH>();
    if (ctl->done) return;
    const unsigned long long seed = seeds[blockIdx.y];
    const unsigned e = (unsigned)(ctl->nfe + stage);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < per; i += (unsigned long long)gridDim.x * 256)
        eps[(unsigned long long)blockIdx.y * per + i] = philox_sign(seed, e, i);
}
// lsl_rademacher: out[i] = +-1 for (seed, eval_index, i)
__global__ void __launch_bounds__(256) k_rademacher(float *out, unsigned long long n, unsigned long long seed, unsigned eval_index) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) out[i] = philox_sign(seed, eval_index, i);
}
// partial[b][slab] of eps[b] . j[b]: lsl_dot_rows' slabs.  grid (slabs, B)
template <bool EACH>
__global__ void __launch_bounds__(256) k_dp_dot(const lsl_dopri_ctl *ctl, double *partial, const float *eps, const float *j, unsigned long long per) {
    __shared__ double red[256];
    if (ctl[dp_solve<EACH>()].done) return;
    dot_rows_slab(red, partial, eps, j, per);
}
// k_side[b] = (float)(vx N + vm dot_b) in fp64 with rounded products, (vx, vm) at the fp32 time of the evaluation at t + alpha dt; dot_b: the slab
// partials in slab order.  A thread per trajectory
template <bool EACH>
__global__ void k_dp_klogp(const lsl_dopri_ctl *ctl, float *k_side, const double *partial, int slabs, double alpha, unsigned long long per, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    ctl += EACH ? b : 0;
    if (ctl->done) return;
    double vx, vm;
    dp_drift_coeffs(ctl, alpha, vx, vm);
    k_side[b] = (float)(dp_mul(vx, (double)per) + dp_mul(vm, dot_rows_total(partial, b, slabs)));
}

// The controller moves on, one thread: an accepted step advances the time and the output cursor; the next step size; the counters; done at
// the last output time, on a non-finite ratio, and when another attempt would exceed max_steps
__device__ inline void dp_apply(lsl_dopri_ctl *ctl, const double *grid) {
    if (ctl->done) return;
    ctl->nfe += 6;
    if (!isfinite(ctl->ratio)) {
        ctl->rejected += 1;
        ctl->status = LSL_DOPRI_NON_FINITE;
        ctl->done = 1;
        return;
    }
    if (ctl->accept) {
        ctl->t_lo = ctl->t;
        ctl->t = ctl->t_new;
        ctl->next_out = ctl->out_end;
        ctl->accepted += 1;
    } else
        ctl->rejected += 1;
    ctl->dt = ctl->dt_next;
    if (ctl->t >= grid[ctl->n_out - 1]) ctl->done = 1;
    else if (ctl->accepted + ctl->rejected >= ctl->max_steps) {
        ctl->status = LSL_DOPRI_MAX_STEPS;
        ctl->done = 1;
    }
}
__global__ void k_dp_apply(lsl_dopri_ctl *ctl, const double *grid) { dp_apply(ctl, grid); }

// The per-trajectory form's last kernel of an attempt, one workgroup: every record moves on (APPLY; a thread per record, 256 at a time), then
// the summary the host polls - how many trajectories are done, how many of them failed, the largest number of attempts.  Integer counts in
// LDS; the begin call runs it with APPLY = false for the summary of the first state.
template <bool APPLY>
__global__ void __launch_bounds__(256) k_dp_apply_each(lsl_dopri_ctl *ctl, const double *grid, lsl_dopri_each_summary *summary, int B) {
    __shared__ int n_done, n_failed, most;
    if (threadIdx.x == 0) n_done = n_failed = most = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += 256) {
        if (APPLY) dp_apply(ctl + b, grid);
        if (ctl[b].done) atomicAdd(&n_done, 1);
        if (ctl[b].status != LSL_DOPRI_OK) atomicAdd(&n_failed, 1);
        atomicMax(&most, ctl[b].accepted + ctl[b].rejected);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    lsl_dopri_each_summary s;
    s.B = B;
    s.n_done = n_done;
    s.n_failed = n_failed;
    s.max_attempts = most;
    s.done = n_done == B;
    *summary = s;
}

// lsl_debug_dopri_coeffs: out[i] = (vx, vm) at the fp32 time t[i]
__global__ void k_dp_coeffs(int path, int pred, const float *t, int n, double *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dp_velocity_coeffs(path, pred, (double)t[i], out[2 * i], out[2 * i + 1]);
}
