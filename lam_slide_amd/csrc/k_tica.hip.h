// TICA and state statistics of the peptide evaluation (lsl_lagged_moments / lsl_project / lsl_assign_centers / lsl_transition_counts): the
// second half of analyze_trajectory (eval_peptide.py:189-288, modules/analysis.py:36-56) behind the cos / sin torsion features -
//      moments  sx = sum x_t, sy = sum x_{t+lag}, xx = sum x_t x_t^T, yy = sum x_{t+lag} x_{t+lag}^T, xy = sum x_t x_{t+lag}^T over t < m = n - lag
//               (what the TICA estimator is made of: C0, C_lag and the mean follow in a few F x F operations)
//      project  y[t, j] = fp32(sum_f (x[t, f] - mean[f]) W[f, j]), with the running minimum / maximum of every output column
//      assign   labels[t] = argmin_c sum_j (y[t, j] - centers[c, j])^2   (kmeans.transform), through an optional microstate -> state map
//      counts   C[i, j] += #{t < n - lag : d_t = i, d_{t+lag} = j}       (the sliding-window count matrix of estimate_markov_model)
//
// Work split.
//  k_moments_partial  a workgroup of 256 threads owns (series, a segment of LSL_MOM_SEG time steps, 256 blocks of T x T output entries).  It
//                     stages LSL_MOM_ROWS rows x_t and the rows x_{t+lag} in LDS as fp32 (coalesced passes over contiguous memory); thread
//                     (ia, ib) holds the T x T blocks xx, yy, xy [ia T .., ib T ..] in fp64 registers and walks t ascending: fma((double)a,
//                     (double)b, acc).  The product of two fp32 values is exact in fp64, so the fma rounds once - the addition.  T = 2 for
//                     F <= 64, T = 4 above.  The threads of block column 0 also add x_t and x_{t+lag} themselves (sx, sy).
//  k_moments_final    adds the segments' partials in segment order in fp64.
//  k_project          a workgroup stages W, mean (fp64) and 64 rows of x in LDS; a thread owns outputs (row, j): the fp64 subtraction, the
//                     fused chain over f ascending, one rounding to fp32.  Minimum / maximum: lim_init / lim_update / lim_flush of
//                     k_stat_frag.hip.h - LDS integer atomics on the order-preserving key of the fp32 value, then one integer atomic per
//                     column and workgroup on the caller's table, which k_lim_keys has turned into keys before and k_lim_floats turns
//                     back after.
//  k_assign           the centres and a tile of rows (stage_rows_transposed: conflict-free) in LDS, a thread per row: nearest_centre.
//  k_transitions      a workgroup owns LSL_TR_ROWS pairs of one series: int32 counts in LDS by LDS integer atomics, the non-zero ones added
//                     to the int64 table in memory by integer atomics (flush_counts, as every histogram).
//
// Determinism.  The only atomics are integer additions and integer minimum / maximum: no order.  No float atomics.  Every entry of the
// moments is a direct sum over its own window: the terms of a segment in t order (the longest fp64 addition chain is LSL_MOM_SEG), the
// segments in segment order.  The segments are a function of (n, lag) alone - segment g is t in [g LSL_MOM_SEG, (g + 1) LSL_MOM_SEG) below
// m - not of S, the grid or the device: a series has the same bits alone and inside any batch.  xx[a, b] and xx[b, a] add the same
// exact products in the same order: the same bits, and so yy.  Nothing below depends on contraction: every fused operation is written fma.
#pragma once
#include "common.hip.h"
#include "k_stat_frag.hip.h"

#define LSL_MOM_MAX_F 128    // features of a row: two tiles of LSL_MOM_ROWS rows in LDS are 32 KiB
#define LSL_MOM_SEG 1024     // time steps per segment = the longest fp64 addition chain of a partial (10^6 steps: ~1000 workgroups per block chunk)
#define LSL_MOM_ROWS 32      // rows of x (and of the lagged x) a workgroup holds in LDS at a time
#define LSL_PROJ_MAX_D 16    // output columns of lsl_project
#define LSL_PROJ_ROWS 64     // rows of x per workgroup of k_project
#define LSL_ASG_MAX_K 1024   // centres
#define LSL_ASG_MAX_D 64     // coordinates of a centre
#define LSL_ASG_CELLS 8192   // k * d floats of centres in LDS (32 KiB)
#define LSL_ASG_TILE 4096    // floats of the row tile in LDS: min(256, 4096 / d) rows per pass
#define LSL_ASG_MAX_STATES 1024  // states counted (int32 counts in LDS)
#define LSL_TR_MAX_STATES 128    // ns^2 <= 16384 int32 counts in LDS (64 KiB)
#define LSL_TR_ROWS 8192         // pairs per workgroup of k_transitions

// ---- a. lagged second moments ----
inline int mom_segments(int n, int lag) { return (int)(((long long)n - lag + LSL_MOM_SEG - 1) / LSL_MOM_SEG); }
inline int mom_block(int F) { return F <= 64 ? 2 : 4; }  // T: the side of a thread's block of entries
__host__ __device__ inline size_t mom_entries(int F) { return 2 * (size_t)F + 3 * (size_t)F * F; }  // E: sx, sy, xx, yy, xy of a series

// part[(s nseg + g) E + e], E = 2 F + 3 F^2, e over (sx [F], sy [F], xx [F, F], yy [F, F], xy [F, F]): the sums over segment g of series s.
// x [S, n, F]; grid (nseg, ceil(nb^2 / 256), S), nb = ceil(F / T), 256 threads.
template <int T>
__global__ void __launch_bounds__(256) k_moments_partial(double *part, const float *x, int n, int F, int lag) {
    __shared__ __attribute__((aligned(16))) float xs[LSL_MOM_ROWS * LSL_MOM_MAX_F], ys[LSL_MOM_ROWS * LSL_MOM_MAX_F];
    const int nb = (F + T - 1) / T, FP = nb * T;  // (rows are padded with zeros to whole blocks: FP <= LSL_MOM_MAX_F)
    const int item = blockIdx.y * 256 + (int)threadIdx.x;
    const bool live = item < nb * nb;
    const int ia = live ? item / nb : 0, ib = live ? item - ia * nb : 0;
    const int s = blockIdx.z, g = blockIdx.x, nseg = gridDim.x;
    const int m = n - lag;
    const int t_first = g * LSL_MOM_SEG, t_last = (m - t_first < LSL_MOM_SEG) ? m : t_first + LSL_MOM_SEG;  // [t_first, t_last)
    const float *xb = x + (size_t)s * n * F;
    double axx[T][T], ayy[T][T], axy[T][T], asx[T], asy[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        asx[i] = asy[i] = 0.0;
#pragma unroll
        for (int j = 0; j < T; ++j) axx[i][j] = ayy[i][j] = axy[i][j] = 0.0;
    }
    typedef float vecT __attribute__((ext_vector_type(T)));  // (a block's T floats of a row: one aligned LDS read)
    for (long long t0 = t_first; t0 < t_last; t0 += LSL_MOM_ROWS) {
        const int rows = (int)((t_last - t0 < LSL_MOM_ROWS) ? (t_last - t0) : LSL_MOM_ROWS);
        const float *px = xb + (size_t)t0 * F, *py = xb + ((size_t)t0 + lag) * F;  // rows t0 .. t0 + rows - 1 and their lagged rows: below n
        for (int i = threadIdx.x; i < rows * FP; i += 256) {
            const int r = i / FP, f = i - r * FP;
            xs[i] = (f < F) ? px[(size_t)r * F + f] : 0.0f;
            ys[i] = (f < F) ? py[(size_t)r * F + f] : 0.0f;
        }
        __syncthreads();
        if (live) {
            for (int r = 0; r < rows; ++r) {
                const vecT vxa = *(const vecT *)(xs + r * FP + ia * T), vxc = *(const vecT *)(xs + r * FP + ib * T);
                const vecT vya = *(const vecT *)(ys + r * FP + ia * T), vyc = *(const vecT *)(ys + r * FP + ib * T);
                double xa[T], xc[T], ya[T], yc[T];
#pragma unroll
                for (int i = 0; i < T; ++i) xa[i] = (double)vxa[i], xc[i] = (double)vxc[i], ya[i] = (double)vya[i], yc[i] = (double)vyc[i];
#pragma unroll
                for (int i = 0; i < T; ++i)
#pragma unroll
                    for (int j = 0; j < T; ++j) {
                        axx[i][j] = fma(xa[i], xc[j], axx[i][j]);
                        ayy[i][j] = fma(ya[i], yc[j], ayy[i][j]);
                        axy[i][j] = fma(xa[i], yc[j], axy[i][j]);
                    }
                if (ib == 0) {
#pragma unroll
                    for (int i = 0; i < T; ++i) asx[i] += xa[i], asy[i] += ya[i];
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    double *out = part + ((size_t)s * nseg + g) * mom_entries(F);
    const size_t FF = (size_t)F * F;
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int a = ia * T + i;
        if (a >= F) continue;
        if (ib == 0) out[a] = asx[i], out[F + a] = asy[i];
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int b = ib * T + j;
            if (b >= F) continue;
            const size_t e = 2 * (size_t)F + (size_t)a * F + b;
            out[e] = axx[i][j], out[e + FF] = ayy[i][j], out[e + 2 * FF] = axy[i][j];
        }
    }
}

// out[s E + e] = sum over g of part[(s nseg + g) E + e], g ascending, fp64.  grid (ceil(E / 256), S), 256 threads.
__global__ void __launch_bounds__(256) k_moments_final(double *out, const double *part, long long E, int nseg) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const double *p = part + (size_t)blockIdx.y * nseg * E + e;
    double s = 0.0;
    for (int g = 0; g < nseg; ++g) s += p[(size_t)g * E];
    out[(size_t)blockIdx.y * E + e] = s;
}

// ---- b. projection and running limits ----
// lim [2 d] in place: floats -> keys (lim_key of k_stat_frag.hip.h), keys -> floats (one thread per entry; the table's bytes hold keys
// between the two).
__global__ void k_lim_keys(float *lim, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) ((unsigned *)lim)[i] = lim_key(lim[i]);
}
__global__ void k_lim_floats(float *lim, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) lim[i] = lim_unkey(((const unsigned *)lim)[i]);
}

// y[t d + j] = fp32(sum_f (x[t F + f] - mean[f]) W[f d + j]), f ascending; keys (or NULL): [2 d] unsigned, keys[j] = min, keys[d + j] = max
// over the key of every y[t, j] that is not NaN.  grid ceil(n / LSL_PROJ_ROWS), 256 threads.
__global__ void __launch_bounds__(256) k_project(float *y, const float *x, const double *mean, const double *W, unsigned *keys, int n, int F, int d) {
    __shared__ double Ws[LSL_MOM_MAX_F * LSL_PROJ_MAX_D], ms[LSL_MOM_MAX_F];
    __shared__ float xs[LSL_PROJ_ROWS * (LSL_MOM_MAX_F + 1)];
    __shared__ unsigned kmin[LSL_PROJ_MAX_D], kmax[LSL_PROJ_MAX_D];
    const int FS = F | 1;  // (an odd row stride: the rows of a wave's lanes fall on different banks)
    const long long t0 = (long long)blockIdx.x * LSL_PROJ_ROWS;
    const int rows = tile_rows(n, t0, LSL_PROJ_ROWS);
    for (int i = threadIdx.x; i < F * d; i += 256) Ws[i] = W[i];
    for (int i = threadIdx.x; i < F; i += 256) ms[i] = mean[i];
    lim_init(kmin, kmax, LSL_PROJ_MAX_D);
    const float *src = x + (size_t)t0 * F;
    for (int i = threadIdx.x; i < rows * F; i += 256) {
        const int r = i / F, f = i - r * F;
        xs[r * FS + f] = src[i];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * d; i += 256) {
        const int r = i / d, j = i - r * d;
        const float *xr = xs + r * FS;
        double acc = 0.0;
        for (int f = 0; f < F; ++f) acc = fma((double)xr[f] - ms[f], Ws[f * d + j], acc);
        const float v = (float)acc;
        y[(size_t)t0 * d + i] = v;
        if (keys) lim_update(kmin, kmax, j, v);
    }
    if (!keys) return;
    __syncthreads();
    lim_flush(keys, kmin, kmax, d);
}

// ---- c. nearest centre ----
// labels[t] = the lowest c that minimises sum_j (y[t, j] - centers[c, j])^2 (fp64 differences, the fused sum over j ascending), through
// map [k] when given (a mapped value outside 0 .. nstates - 1: -1); -1 for a row that holds a NaN.  state_counts [nstates] (or NULL) +=
// the number of rows of each label in 0 .. nstates - 1.  grid ceil(n / ra), ra = min(256, LSL_ASG_TILE / d) rows, 256 threads.
__global__ void __launch_bounds__(256) k_assign(int *labels, unsigned long long *state_counts, const float *y, const float *centers, const int *map,
                                                int n, int d, int k, int nstates, int ra) {
    __shared__ float cs[LSL_ASG_CELLS], yt[LSL_ASG_TILE];
    __shared__ int cnt[LSL_ASG_MAX_STATES];
    const long long t0 = (long long)blockIdx.x * ra;
    const int rows = tile_rows(n, t0, ra);
    for (int i = threadIdx.x; i < k * d; i += 256) cs[i] = centers[i];
    if (state_counts)
        for (int i = threadIdx.x; i < nstates; i += 256) cnt[i] = 0;
    stage_rows_transposed(yt, y + (size_t)t0 * d, rows, d, ra, threadIdx.x, 256);
    __syncthreads();
    const int r = threadIdx.x;
    if (r < rows) {
        bool nan;
        double best;
        const int best_c = nearest_centre(yt, ra, r, cs, d, k, &best, &nan);
        int lab = -1;
        if (!nan) {
            lab = best_c;
            if (map) {
                lab = map[best_c];
                if ((unsigned)lab >= (unsigned)nstates) lab = -1;
            }
        }
        labels[t0 + r] = lab;
        if (state_counts && (unsigned)lab < (unsigned)nstates) atomicAdd(&cnt[lab], 1);
    }
    if (!state_counts) return;
    __syncthreads();
    flush_counts(state_counts, cnt, nstates);
}

// ---- d. transition counts ----
// counts[(s ns + i) ns + j] += #{t < n - lag : dtraj[s, t] = i, dtraj[s, t + lag] = j}; a pair with a label outside 0 .. ns - 1 is skipped.
// grid (ceil((n - lag) / LSL_TR_ROWS), S), 256 threads, ns <= LSL_TR_MAX_STATES.
__global__ void __launch_bounds__(256) k_transitions(unsigned long long *counts, const int *dtraj, int n, int lag, int ns) {
    __shared__ int cnt[LSL_TR_MAX_STATES * LSL_TR_MAX_STATES];
    const int cells = ns * ns, m = n - lag;
    const long long t0 = (long long)blockIdx.x * LSL_TR_ROWS;
    const int rows = tile_rows(m, t0, LSL_TR_ROWS);
    for (int i = threadIdx.x; i < cells; i += 256) cnt[i] = 0;
    __syncthreads();
    const int *ds = dtraj + (size_t)blockIdx.y * n + t0;
    for (int t = threadIdx.x; t < rows; t += 256) {
        const int a = ds[t], b = ds[(size_t)t + lag];
        if ((unsigned)a < (unsigned)ns && (unsigned)b < (unsigned)ns) atomicAdd(&cnt[a * ns + b], 1);
    }
    __syncthreads();
    flush_counts(counts + (size_t)blockIdx.y * cells, cnt, cells);
}
