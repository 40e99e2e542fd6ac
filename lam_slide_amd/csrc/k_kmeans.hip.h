// k-means fitting on the device (lsl_kmeans_step / lsl_kmeans_nearest_rows): S independent Lloyd problems y [S, n, d] -> centers [S, k, d].  The
// two users sit at opposite ends of the shape range: the microstates of the peptide evaluation (modules/analysis.py:42-44: S = 1, n ~ 10^6,
// k = 100) and the post_process branch of the NBA / pedestrian test_step (second_stage/nba.py:202-203, 228-238: S = 11 264 agents, n = K = 60
// final frames, k = num_runs = 20, d = 2).
//
//      assign   labels[t] = the lowest c that minimises sum_j (y[t, j] - centers[c, j])^2: nearest_centre of k_stat_frag.hip.h, the very
//               function k_assign calls; a row that holds a NaN gets -1 and takes no part in anything below
//      update   sum[c, j] = sum of y[t, j] over the rows labelled c in fp64: rows ascending in t within a segment of LSL_KM_SEG rows (segment
//               g: t in [g SEG, (g + 1) SEG), a function of n alone), the segments added in segment order; count[c] an exact integer; the new
//               centre fp32(sum / count): one fp64 division, one rounding; an empty cluster keeps its centre bit for bit
//      inertia  the fp64 sum of the winning squared distances of this assignment (against the centres before the update)
//
// Work split.
//  k_kmeans_step   a group of G threads owns (series, segment); a workgroup is 256 threads.  G = 256 in general: one group per workgroup, which
//                  leaves at once when done[s] is set.  G = 64 (one wave) when the whole series fits a wave's share of the LDS (km_group: a
//                  function of (n, d, k) alone): four series per workgroup, so S = 11 264 series of 60 rows are 2816 workgroups, not 11 264.
//                  A group keeps its series' centres in LDS and walks its segment in sub-tiles of rows (stage_rows_transposed).
//                  Phase A: a thread per row finds the argmin, writes the label to LDS and to memory, compares it with the previous label,
//                  keeps the winning distance.  Phase B: thread `lane` owns the items (c, j) = lane + q G, q < NQ <= 32, in fp64 registers
//                  that persist over the sub-tiles of the segment; it walks the sub-tile's labels in LDS (broadcast reads) in ascending t and
//                  adds y[t, j] where the label is c - the order of the contract, whatever G is - and counts the members as an integer.
//  k_kmeans_final  one workgroup per series adds the segments in segment order, divides, rounds, writes centres, counts and state, sets done.
//  k_nearest_rows  the reverse lookup of post_process: rows[s, c] = the lowest t that minimises the same distance (sq_dist_chain); P lanes per (s, c), P = 1
//                  for n <= 64 (256 items of many tiny series per workgroup), 64 above (lanes stride over t, then a (distance, t) minimum).
//
// Determinism.  No float atomics; one LDS integer atomic, for the changed-label count.  The inertia of a group: every thread adds the winning
// distances of its own rows over the sub-tiles in order, then a fixed binary tree over the G threads; the segments in segment order.  Every
// order is a function of (n, d, k) alone - not of S, the grid or the device: a series has the same bits alone, inside any batch, and whichever
// series share its workgroup.
#pragma once
#include "common.hip.h"
#include "k_stat_frag.hip.h"
#include "k_tica.hip.h"

#define LSL_KM_MAX_K LSL_ASG_MAX_K  // centres, their coordinates and the k * d floats of centres in LDS: the assignment is k_assign's
#define LSL_KM_MAX_D LSL_ASG_MAX_D  // (nearest_centre), and so are its limits
#define LSL_KM_CELLS LSL_ASG_CELLS
#define LSL_KM_TILE LSL_ASG_TILE    // floats of the row tile in LDS: min(G, LSL_KM_TILE G / (256 d)) rows per pass
#define LSL_KM_MAX_S 65535  // series of one call (a grid dimension)
#define LSL_KM_SEG 2048     // rows per segment = the longest fp64 addition chain of a partial sum (10^6 rows: 489 workgroups)
#define LSL_KM_MAX_Q (LSL_KM_CELLS / 256)  // items (c, j) per thread

inline int km_segments(int n) { return (int)(((long long)n + LSL_KM_SEG - 1) / LSL_KM_SEG); }
__host__ __device__ inline int km_rows(int G, int d) {  // rows of a sub-tile of a group of G threads
    const int fit = (LSL_KM_TILE / 256) * G / d;
    return fit < G ? fit : G;
}
// threads per series: a wave when the series is one sub-tile of a wave and its centres fit a quarter of the LDS table
inline int km_group(int n, int d, int k) { return (n <= km_rows(64, d) && k * d <= LSL_KM_CELLS / 4) ? 64 : 256; }

// One Lloyd assignment with the partial sums of the update.  y [S, n, d], centers [S, k, d], labels [S, n] (read: the previous labels, written:
// the new ones), done [S].  Per unit u = s nseg + g: wsum [u, k, d] fp64, winert [u] fp64, wcnt [u, k], wchg [u] (rows whose label changed).
// update != 0: a series with done[s] set is left alone (none of its buffers is touched).  grid (nseg, S) at G = 256, (ceil(S / 4)) at G = 64
// (then nseg = 1 and n <= km_rows(64, d)); 256 threads.
template <int NQ>
__global__ void __launch_bounds__(256) k_kmeans_step(const float *y, const float *centers, int *labels, const int *done, double *wsum, double *winert,
                                                     int *wcnt, int *wchg, int S, int n, int d, int k, int nseg, int G, int update) {
    __shared__ float cs[LSL_KM_CELLS], yt[LSL_KM_TILE];
    __shared__ int labs[256], chg[4];
    __shared__ double red[256];
    const int per = 256 / G, grp = (int)threadIdx.x / G, lane = (int)threadIdx.x - grp * G;
    const int s = (G == 256) ? (int)blockIdx.y : (int)blockIdx.x * per + grp, g = (G == 256) ? (int)blockIdx.x : 0;
    const bool live = s < S && !(update && done[s]);
    if (G == 256 && !live) return;  // (the whole workgroup: nothing of a finished series is read or written)
    const int kd = k * d, ra = km_rows(G, d);
    float *csg = cs + grp * (LSL_KM_CELLS / per), *ytg = yt + grp * (LSL_KM_TILE / per);
    int *labg = labs + grp * G;
    const size_t sl = live ? (size_t)s : 0;
    const float *yb = y + sl * n * d;
    int *lb = labels + sl * n;
    if (live)
        for (int i = lane; i < kd; i += G) csg[i] = centers[sl * kd + i];
    int cq[NQ], jq[NQ], nq[NQ];
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int item = q * G + lane;
        cq[q] = item < kd ? item / d : -3;  // (no label is -3: a thread past the last item adds nothing)
        jq[q] = item < kd ? item - cq[q] * d : 0;
        nq[q] = 0, acc[q] = 0.0;
    }
    double inert = 0.0;
    int changed = 0;
    const long long t_first = (long long)g * LSL_KM_SEG, t_last = (n - t_first < LSL_KM_SEG) ? n : t_first + LSL_KM_SEG;  // [t_first, t_last)
    for (long long t0 = t_first; t0 < t_last; t0 += ra) {  // (the same trips in every group of a workgroup: the barriers are uniform)
        const int rows = tile_rows(t_last, t0, ra);
        if (live) stage_rows_transposed(ytg, yb + (size_t)t0 * d, rows, d, ra, lane, G);
        __syncthreads();
        if (live && lane < rows) {
            const int r = lane;
            bool nan;
            double best;
            const int best_c = nearest_centre(ytg, ra, r, csg, d, k, &best, &nan);
            const int lab = nan ? -1 : best_c;
            labg[r] = lab;
            changed += lab != lb[t0 + r];
            lb[t0 + r] = lab;
            if (!nan) inert += best;
        }
        __syncthreads();
        if (live) {
            for (int r = 0; r < rows; ++r) {
                const int lab = labg[r];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (lab == cq[q]) acc[q] += (double)ytg[jq[q] * ra + r], ++nq[q];
            }
        }
        __syncthreads();
    }
    const size_t u = sl * nseg + g;
    if (live) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (cq[q] < 0) continue;
            wsum[u * kd + (size_t)(q * G + lane)] = acc[q];
            if (jq[q] == 0) wcnt[u * k + cq[q]] = nq[q];
        }
    }
    red[threadIdx.x] = inert;
    if (lane == 0) chg[grp] = 0;
    __syncthreads();
    if (changed) atomicAdd(&chg[grp], changed);
    for (int off = G >> 1; off > 0; off >>= 1) {
        if (lane < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (live && lane == 0) winert[u] = red[threadIdx.x], wchg[u] = chg[grp];
}

template <int NQ>
static void launch_kmeans_step(dim3 grid, hipStream_t st, const float *y, const float *centers, int *labels, const int *done, double *wsum, double *winert,
                               int *wcnt, int *wchg, int S, int n, int d, int k, int nseg, int G, int update) {
    hipLaunchKernelGGL(k_kmeans_step<NQ>, grid, dim3(256), 0, st, y, centers, labels, done, wsum, winert, wcnt, wchg, S, n, d, k, nseg, G, update);
}

// The segments of a series added in segment order.  counts i64 [S, k]; state f64 [S, 4] = (iterations done, J, J of the iteration before, the
// squared centre shift sum (new - old)^2).  update != 0: a finished series is left alone; otherwise the new centres fp32(sum / count) (an empty
// cluster keeps its bits), counts, state, and done[s] = 1 when no label changed, or rel_tol > 0 and |J_prev - J| <= rel_tol J_prev from the
// second iteration on, or center_tol > 0 and the shift <= center_tol^2.  update == 0: counts and J only.  grid S, 256 threads.
__global__ void __launch_bounds__(256) k_kmeans_final(float *centers, long long *counts, double *state, int *done, const double *wsum,
                                                      const double *winert, const int *wcnt, const int *wchg, int d, int k, int nseg, int update,
                                                      double rel_tol, double center_tol) {
    __shared__ double red[256];
    const size_t s = blockIdx.x;
    if (update && done[s]) return;
    const int kd = k * d;
    const size_t u0 = s * nseg;
    double shift = 0.0;
    for (int item = threadIdx.x; item < kd; item += 256) {
        const int c = item / d;
        long long cnt = 0;
        for (int g = 0; g < nseg; ++g) cnt += wcnt[(u0 + g) * k + c];
        if (item - c * d == 0) counts[s * k + c] = cnt;
        if (update && cnt > 0) {
            double sum = 0.0;
            for (int g = 0; g < nseg; ++g) sum += wsum[(u0 + g) * kd + item];
            const float nc = (float)(sum / (double)cnt);
            const double diff = (double)nc - (double)centers[s * kd + item];
            shift = fma(diff, diff, shift);
            centers[s * kd + item] = nc;
        }
    }
    red[threadIdx.x] = shift;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double J = 0.0;
    long long changed = 0;
    for (int g = 0; g < nseg; ++g) J += winert[u0 + g], changed += wchg[u0 + g];
    double *st = state + s * 4;
    if (!update) {
        st[1] = J;
        return;
    }
    const double it = st[0] + 1.0, Jprev = st[1], sh = red[0];
    st[0] = it, st[1] = J, st[2] = Jprev, st[3] = sh;
    if (changed == 0 || (rel_tol > 0.0 && it >= 2.0 && fabs(Jprev - J) <= rel_tol * Jprev) || (center_tol > 0.0 && sh <= center_tol * center_tol))
        done[s] = 1;
}

// rows[s k + c] = the lowest t that minimises sum_j (y[s, t, j] - centers[s, c, j])^2 (sq_dist_chain: the arithmetic of the assignment; rows
// that hold a NaN skipped; -1 when the series has no finite row).  P lanes (a power of two <= 64) per item (s, c): lane p walks t = p, p + P, ... ascending with
// strict <, then the lanes' (distance, t) pairs are reduced: the smaller distance, on equal distances the lower t - what one walk in ascending
// t gives.  grid ceil(items P / 256), 256 threads.
__global__ void __launch_bounds__(256) k_nearest_rows(int *rows, const float *y, const float *centers, long long items, int n, int d, int k, int P) {
    const long long item = ((long long)blockIdx.x * 256 + threadIdx.x) / P;
    const int lane = (int)threadIdx.x & (P - 1);
    const bool live = item < items;
    double best = __builtin_inf();
    int bt = -1;
    if (live) {
        const float *yb = y + (size_t)(item / k) * n * d, *cc = centers + (size_t)item * d;
        for (int t = lane; t < n; t += P) {
            const double a = sq_dist_chain(yb + (size_t)t * d, 1, cc, d);
            if (a < best) best = a, bt = t;  // (a row that holds a NaN has a NaN distance: it never wins)
        }
    }
    for (int off = P >> 1; off > 0; off >>= 1) {  // (every lane of the wave takes part: no thread has left)
        const double ob = __shfl_xor(best, off);
        const int ot = __shfl_xor(bt, off);
        if (ot >= 0 && (bt < 0 || ob < best || (ob == best && ot < bt))) best = ob, bt = ot;
    }
    if (live && lane == 0) rows[item] = bt;
}
