// Reversible maximum-likelihood Markov state models on the device (lsl_msm_active_set / lsl_msm_reversible_step / lsl_msm_transition_matrix):
// S independent count matrices C i64 [S, ns, ns] -> the largest strongly connected set A, the stationary vector x of the reversible estimate
// on A, and the transition matrix embedded in the full index space (eval_peptide.py:245-288, modules/analysis.py:47-56: three models per
// peptide - microstates, coarse states, the sampled trajectory).  The estimator as mathematics: include/lsl_api.h.
//
//      K = C~ + C~^T on A (integers, exact in fp64 below 2^53), c_i = sum_j C~_ij (an exact integer)
//      step    q_i = c_i / x_i;  y_i = sum_{j : K_ij != 0} K_ij / (q_i + q_j);  x'_i = y_i / sum_i y_i;  err = max_i |x_i - x'_i| / ((x_i + x'_i) / 2)
//
// Work split.  One workgroup per series; a series whose done flag is set leaves before it loads anything.  K stays in LDS as fp64 for the
// whole launch, padded to NSP = 32 / 64 / 128 states (a function of ns alone: 8 / 32 / 128 KiB of the 160 KiB), and in the FULL index
// space: a row or column outside A is zero, and a zero entry is skipped, never divided.  The workgroup has 8 NSP threads (256 / 512 / 1024):
// thread t owns row i = t % NSP and part h = t / NSP of LSL_MSM_PARTS = 8: the columns [h W, (h + 1) W), W = NSP / 8, walked in ascending j.
// A division is a chain of dependent fp64 instructions and the branch around a zero entry keeps the compiler from interleaving two of them,
// so the latency is hidden by waves instead: four per SIMD at NSP = 128.
// K is symmetric, so the thread reads K[j][i]: the 32 lanes of a bank group read 32 consecutive doubles (all 64 banks once, no conflict)
// and q_j is a broadcast.
// Per step three barriers: the parts of y -> (y_i = the parts in ascending h by the row's owner; sum_i y_i by a butterfly over the lanes
// of the owners' wave, one value per wave to LDS) -> (the new x_i, its error and the next q_i by the row's owner; the maximum by the same
// butterfly) -> the stop test.  An earlier form let every thread add all NSP values of y from LDS itself: with sixteen waves that was
// most of a step.  x_i lives in a register of the row's owner between steps and in the caller's fp64 buffer between launches, so a
// launch resumes exactly where the last one stopped.
// Cost.  One fp64 division per non-zero entry of K per step (IEEE, correctly rounded: a v_rcp_f64 refined by fused multiply-adds), plus
// three per row.  The hardware guides give no fp64 division rate for gfx950; the measured cost per step is in profiles/msm_cost.txt.
//
// Determinism.  No atomics at all.  y_i: W terms in ascending j from zero, then the eight parts in ascending h; sum_i y_i: the balanced tree
// over the rows of a group (i with i ^ 1, then ^ 2, .., ^ GW / 2; GW = min(NSP, 64)), the two groups of NSP = 128 in order.  Both are
// functions of (ns, A) alone - not of S, the grid or which series share a launch: a series has the same bits alone and in any batch.
#pragma once
#include "common.hip.h"

#define LSL_MSM_MAX_STATES 128  // = LSL_TR_MAX_STATES; fp64 K [128, 128] is 128 KiB of the 160 KiB of LDS
#define LSL_MSM_MAX_S 65535     // series of one call (a grid dimension)
#define LSL_MSM_PARTS 8         // threads per row of k_msm_step: each owns an eighth of the row's columns
#define LSL_MSM_DONE_CONVERGED 1  // done[s]: the stop test held
#define LSL_MSM_DONE_MAXITER 2    // done[s]: maxiter steps counted and the last one did not pass the test

inline int msm_pad(int ns) { return ns <= 32 ? 32 : ns <= 64 ? 64 : 128; }

// K (symmetric, [NSP, NSP], zero outside A), c (row sums of C~ as exact integers, zero outside A) and the 0/1 flags of one series into LDS.
// NT threads; ends with a barrier.
template <int NSP, int NT>
__device__ __forceinline__ void msm_load(double *Ks, long long *cs, int *acts, const long long *C, const int *active, int ns) {
    const int tid = (int)threadIdx.x;
    if (tid < NSP) acts[tid] = tid < ns && active[tid] != 0;
    __syncthreads();
    for (int idx = tid; idx < NSP * NSP; idx += NT) {
        const int j = idx / NSP, i = idx - j * NSP;
        double k = 0.0;
        if (i < ns && j < ns && acts[i] && acts[j]) {
            const long long a = C[(size_t)i * ns + j], b = C[(size_t)j * ns + i];
            k = (double)((a > 0 ? a : 0) + (b > 0 ? b : 0));
        }
        Ks[idx] = k;
    }
    if (tid < NSP) {
        long long c = 0;
        if (acts[tid])
            for (int j = 0; j < ns; ++j) {
                const long long a = C[(size_t)tid * ns + j];
                if (acts[j] && a > 0) c += a;
            }
        cs[tid] = c;
    }
    __syncthreads();
}

// The sum of one value per row over a group of GW = min(NSP, 64) rows, in every lane of the group: the butterfly v += v[lane ^ off], off = 1, 2,
// .., GW / 2 - a balanced tree whose shape is fixed by GW; both partners add the same two numbers, so all lanes hold the same bits.
template <int GW>
__device__ __forceinline__ double msm_group_sum(double v) {
#pragma unroll
    for (int off = 1; off < GW; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// max of a and b (both >= 0), NaN if either is one: the stop test !(err > maxerr) then holds, as with numpy's max
__device__ __forceinline__ double msm_nanmax(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

template <int GW>
__device__ __forceinline__ double msm_group_max(double v) {
#pragma unroll
    for (int off = 1; off < GW; off <<= 1) v = msm_nanmax(v, __shfl_xor(v, off));
    return v;
}

// At most `iters` further steps of every series that is not done, never past maxiter in total.  counts [S, ns, ns], active [S, ns] (0/1),
// x f64 [S, ns], n_iter [S], err [S], done [S].  restart != 0: x, n_iter, err, done are first set from the counts (x0_i = rowsum_i K / sum
// K from exact integers, 0, 0, done for |A| <= 1), whatever done held.  grid S, 8 NSP threads.
template <int NSP>
__global__ void __launch_bounds__(LSL_MSM_PARTS *NSP) k_msm_step(const long long *counts, const int *active, int ns, int iters, int maxiter, double maxerr, int restart,
                                                  double *x, int *n_iter, double *err, int *done) {
    constexpr int P = LSL_MSM_PARTS, NT = P * NSP, W = NSP / P;
    constexpr int GW = NSP < 64 ? NSP : 64, NG = NSP / GW;  // rows of a group, groups: the waves [0, NG) hold the rows' owners
    __shared__ double Ks[NSP * NSP], qs[NSP], part[NT], gsum[2], gmax[2];
    __shared__ long long cs[NSP], rk[NSP];
    __shared__ int acts[NSP];
    const size_t s = blockIdx.x;
    if (!restart && done[s]) return;  // (the whole workgroup: nothing of a finished series is read or written)
    const int tid = (int)threadIdx.x, h = tid / NSP, i = tid - h * NSP;
    msm_load<NSP, NT>(Ks, cs, acts, counts + s * ns * ns, active + s * ns, ns);
    const bool own = h == 0, live = own && acts[i], owners = tid < NG * 64;  // (owners: wave-uniform)
    const double ci = live ? (double)cs[i] : 0.0;
    double xi = 0.0, e = 0.0;
    int n = 0;
    if (restart) {
        if (own) {  // row sums of K as integers: exact, whatever the order
            long long r = 0;
            for (int j = 0; j < ns; ++j) r += (long long)Ks[j * NSP + i];
            rk[i] = r;
        }
        __syncthreads();
        long long total = 0;
        int na = 0;
        for (int j = 0; j < NSP; ++j) total += rk[j], na += acts[j];
        if (live) xi = (double)rk[i] / (double)total;
        if (own && i < ns) x[s * ns + i] = xi;
        if (tid == 0) n_iter[s] = 0, err[s] = 0.0, done[s] = na <= 1 ? LSL_MSM_DONE_CONVERGED : 0;
        if (na <= 1) return;
    } else {
        if (live) xi = x[s * ns + i];
        n = n_iter[s], e = err[s];
    }
    if (n >= maxiter) {
        if (tid == 0) done[s] = LSL_MSM_DONE_MAXITER;
        return;
    }
    if (own) qs[i] = live ? ci / xi : 0.0;
    __syncthreads();
    bool stop = false;
    for (int it = 0; it < iters && n < maxiter; ++it) {
        const double qi = qs[i];
        double acc = 0.0;
#pragma unroll 2
        for (int m = 0; m < W; ++m) {
            const int j = h * W + m;
            const double k = Ks[j * NSP + i];
            if (k != 0.0) acc += k / (qi + qs[j]);
        }
        part[tid] = acc;  // (tid = h NSP + i)
        __syncthreads();
        double y = 0.0;
        if (owners) {
            if (own) {
                y = part[i];
#pragma unroll
                for (int hh = 1; hh < P; ++hh) y += part[hh * NSP + i];
            }
            const double g = msm_group_sum<GW>(y);  // (a row outside A adds +0.0)
            if ((tid & 63) == 0) gsum[tid >> 6] = g;
        }
        __syncthreads();
        const double total = NG == 1 ? gsum[0] : gsum[0] + gsum[1];
        if (owners) {
            double ei = 0.0;
            if (own) {
                const double xn = live ? y / total : 0.0;
                ei = live ? fabs(xi - xn) / (0.5 * (xi + xn)) : 0.0;
                xi = xn;
                qs[i] = live ? ci / xn : 0.0;  // (every thread has read the old q: it is behind the first barrier of the step)
            }
            const double g = msm_group_max<GW>(ei);
            if ((tid & 63) == 0) gmax[tid >> 6] = g;
        }
        __syncthreads();
        e = NG == 1 ? gmax[0] : msm_nanmax(gmax[0], gmax[1]);
        ++n;
        if (!(e > maxerr)) {
            stop = true;
            break;
        }
    }
    if (own && i < ns) x[s * ns + i] = xi;
    if (tid == 0) {
        n_iter[s] = n, err[s] = e;
        if (stop) done[s] = LSL_MSM_DONE_CONVERGED;
        else if (n >= maxiter) done[s] = LSL_MSM_DONE_MAXITER;
    }
}

// T f64 [S, ns, ns] = the identity with T_ij = X_ij / sum_j X_ij written into the block of A, X_ij = K_ij / (q_i + q_j) (0 where K_ij = 0), the
// row sum over ascending j from zero; pi f64 [S, ns] = x on A, 0 outside.  grid S, 256 threads.
template <int NSP>
__global__ void __launch_bounds__(256) k_msm_tmatrix(const long long *counts, const int *active, const double *x, int ns, double *T, double *pi) {
    __shared__ double Ks[NSP * NSP], qs[NSP], rows[NSP];
    __shared__ long long cs[NSP];
    __shared__ int acts[NSP];
    const size_t s = blockIdx.x;
    const int tid = (int)threadIdx.x;
    msm_load<NSP, 256>(Ks, cs, acts, counts + s * ns * ns, active + s * ns, ns);
    const bool live = tid < NSP && acts[tid];
    const double xi = live ? x[s * ns + tid] : 0.0;
    if (tid < NSP) qs[tid] = live ? (double)cs[tid] / xi : 0.0;
    if (tid < ns) pi[s * ns + tid] = xi;
    __syncthreads();
    if (tid < NSP) {
        double r = 0.0;
        if (live) {
            const double qi = qs[tid];
            for (int j = 0; j < ns; ++j) {
                const double k = Ks[j * NSP + tid];
                if (k != 0.0) r += k / (qi + qs[j]);
            }
        }
        rows[tid] = r;
    }
    __syncthreads();
    double *Ts = T + s * ns * ns;
    for (int idx = tid; idx < ns * ns; idx += 256) {
        const int i = idx / ns, j = idx - i * ns;
        double v = (i == j) ? 1.0 : 0.0;
        if (acts[i]) {
            const double k = Ks[i * NSP + j];  // (= K[j][i])
            v = k != 0.0 ? (k / (qs[i] + qs[j])) / rows[i] : 0.0;
        }
        Ts[idx] = v;
    }
}

// The largest strongly connected component of the graph i -> j where C_ij > 0.  Bit rows in LDS (two 64-bit words per state); ns rounds of
// reach[i] |= reach[k] where reach[i] holds bit k (row k does not change in round k); the component of i = reach[i] & reach^T[i].  A component
// of one state counts only with C_ii > 0; the larger component wins, among equals the one with the lowest state index; none: A empty.
// active i32 [S, ns] (0/1), n_active i32 [S].  grid S, 128 threads.
__global__ void __launch_bounds__(128) k_msm_active(const long long *counts, int ns, int *active, int *n_active) {
    __shared__ unsigned long long r0[128], r1[128];
    __shared__ int key[128];
    const size_t s = blockIdx.x;
    const int i = (int)threadIdx.x;
    const long long *C = counts + s * ns * ns;
    unsigned long long w0 = 0, w1 = 0;
    bool self = false;
    if (i < ns) {
        for (int j = 0; j < ns; ++j)
            if (C[(size_t)i * ns + j] > 0) (j < 64 ? w0 : w1) |= 1ull << (j & 63);
        self = (i < 64 ? w0 >> i : w1 >> (i - 64)) & 1;
        (i < 64 ? w0 : w1) |= 1ull << (i & 63);
    }
    r0[i] = w0, r1[i] = w1;
    __syncthreads();
    for (int k = 0; k < ns; ++k) {
        if (i != k && ((k < 64 ? w0 >> k : w1 >> (k - 64)) & 1)) {
            w0 |= r0[k], w1 |= r1[k];
            r0[i] = w0, r1[i] = w1;
        }
        __syncthreads();
    }
    unsigned long long t0 = 0, t1 = 0;
    if (i < ns)
        for (int j = 0; j < ns; ++j)
            if ((i < 64 ? r0[j] >> i : r1[j] >> (i - 64)) & 1) (j < 64 ? t0 : t1) |= 1ull << (j & 63);
    const unsigned long long c0 = w0 & t0, c1 = w1 & t1;
    const int size = __popcll(c0) + __popcll(c1);
    const int low = c0 ? __ffsll((long long)c0) - 1 : 64 + __ffsll((long long)c1) - 1;
    key[i] = (i < ns && (size >= 2 || self)) ? size * 256 + (255 - low) : 0;  // (larger first, then the lower state index)
    __syncthreads();
    int best = 0;
    for (int j = 0; j < 128; ++j) best = key[j] > best ? key[j] : best;
    const int root = 255 - (best & 255);
    if (i < ns) active[s * ns + i] = best > 0 && ((root < 64 ? c0 >> root : c1 >> (root - 64)) & 1);
    if (i == 0) n_active[s] = best >> 8;
}
