// Rigid superposition of a sampled trajectory (lsl_superpose / lsl_atom_rmsf): what the reference does through mdtraj between a sampled
// peptide trajectory and its numbers (eval_peptide.py:347 traj.superpose(traj); utils/traj_utils.py:54-60 create_trajectory =
// center_coordinates() then superpose(traj, 0)) -
//      cx, cy   = the centroids of the selected atoms of the frame x and of the reference y
//      S        = sum_i (x_i - cx)(y_i - cy)^T over the selection (3 x 3)
//      R        = the proper rotation (det +1) that minimises sum_i |R (x_i - cx) - (y_i - cy)|^2: Horn's quaternion form - the unit
//                 eigenvector q of the largest eigenvalue of the symmetric 4 x 4 matrix K(S), R = R(q)
//      out      = R (x_a - cx) + cy for every atom a of the frame (an atom with fixed[a] != 0 is copied through)
//      rmsd     = sqrt(sum_i |R (x_i - cx) - (y_i - cy)|^2 / n_sel), from the residuals themselves
//      rmsf[a]  = sqrt(mean_f |x_fa - mean_f x_fa|^2)
// All arithmetic is fp64 on the exact fp32 inputs; each output is rounded once.
//
// Work split.
//  k_superpose          as k_pair_dist: a workgroup of 256 threads owns fpb consecutive frames (fpb * A <= LSL_TORS_LDS_ATOMS) and copies their
//                       atoms to LDS (stage_frames).  The frames go in rounds of LSL_SUP_GROUP, three steps each with a barrier between:
//                       1. ONE WAVE owns a frame (wave w the frames w, w + 4, .. of the round): lane l adds the selected atoms l, l + 64, ..
//                       in order, the 64 lanes are combined by the butterfly msm_group_sum<64>; centroids and S go to LDS.  2. ONE THREAD
//                       owns a frame: K, its eigenvector and R.  The Jacobi sweeps are a dependent chain of fp64 divisions and square
//                       roots that costs the same for 1 lane or 64: with every lane of a wave computing the same frame (the first form of
//                       this kernel) a call took 360 us at F = 10 000, A = 56 against 81 us with a frame per lane.  3. one wave per frame again: the
//                       residuals, then the frame's A * 3 floats in memory order (lane l the floats l, l + 64, ..: coalesced).  The
//                       reference is read from memory (a shared one stays in the cache).
//  k_atom_mean_partial  thread c of a 64-thread workgroup owns column c of pos [F, A * 3] inside one segment of LSL_RMSF_SEG frames: the fp64
//                       sum over the segment's frames in order (SECOND: of (x - mean)^2, mean from the first pass's partials).
//  k_atom_rmsf_final    thread a owns atom a: the segments' partials added in segment order.
//
// Determinism.  No atomics.  A frame's sums are a function of (A, sel) alone: the lane's own chain, then the fixed butterfly; the Jacobi
// eigensolver runs a fixed number of sweeps (LSL_SUP_SWEEPS, a compile-time trip count - a frame holding NaN falls through it and gives NaN,
// it cannot spin).  A frame has the same bits alone and inside any batch, wherever it falls in a workgroup.  An atom's mean and rmsf are a
// function of its own column and F.
#pragma once
#include "common.hip.h"
#include "k_stat_frag.hip.h"
#include "k_torsstat.hip.h"
#include "k_msm.hip.h"

#define LSL_SUP_SWEEPS 8    // cyclic Jacobi sweeps over the 4 x 4 matrix K: 5 give the bits of 10 on 1817 random S with gap >= 0.007; NaN falls through
#define LSL_SUP_GROUP 64    // frames of one round of a workgroup of k_superpose: their fits stay in LDS, a thread solves one
#define LSL_RMSF_SEG 128    // frames of one segment of lsl_atom_rmsf: the longest fp64 chain of a partial sum

// ---- a. the rotation of a 3 x 3 covariance ----
// R [9] (row-major) = the proper rotation that maximises sum_i (R x_i) . y_i = sum_ab R_ab S_ba, i.e. minimises sum_i |R x_i - y_i|^2, for
// S = sum_i x_i y_i^T (S [9] row-major, S[3 a + b] = sum x_a y_b).  K is Horn's matrix (J. Opt. Soc. Am. A 4, 629 (1987), eq. for N with M = S); its top eigenvector by cyclic
// Jacobi: LSL_SUP_SWEEPS sweeps of the six rotations (p, q), p < q, each the textbook one (theta = (a_qq - a_pp) / (2 a_pq),
// t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c; skipped when a_pq == 0).  The eigenvector of the first
// largest diagonal entry, normalised, its first nonzero component made positive.  S == 0 runs no rotation: q = (1, 0, 0, 0), R = 1.
__host__ __device__ inline void sup_rotation(const double *S, double *R) {
    double a[4][4], v[4][4];
    a[0][0] = S[0] + S[4] + S[8];
    a[1][1] = S[0] - S[4] - S[8];
    a[2][2] = -S[0] + S[4] - S[8];
    a[3][3] = -S[0] - S[4] + S[8];
    a[0][1] = a[1][0] = S[5] - S[7];
    a[0][2] = a[2][0] = S[6] - S[2];
    a[0][3] = a[3][0] = S[1] - S[3];
    a[1][2] = a[2][1] = S[1] + S[3];
    a[1][3] = a[3][1] = S[6] + S[2];
    a[2][3] = a[3][2] = S[5] + S[7];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < LSL_SUP_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq != 0.0) {  // (true for NaN: the frame's numbers all become NaN)
                    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double akp = a[k][p], akq = a[k][q];
                        a[k][p] = c * akp - s * akq, a[k][q] = s * akp + c * akq;
                        const double vkp = v[k][p], vkq = v[k][q];
                        v[k][p] = c * vkp - s * vkq, v[k][q] = s * vkp + c * vkq;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double apk = a[p][k], aqk = a[q][k];
                        a[p][k] = c * apk - s * aqk, a[q][k] = s * apk + c * aqk;
                    }
                }
            }
    }
    double best = a[0][0], q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (a[j][j] > best) best = a[j][j], q0 = v[0][j], q1 = v[1][j], q2 = v[2][j], q3 = v[3][j];
    const double lead = q0 != 0.0 ? q0 : (q1 != 0.0 ? q1 : (q2 != 0.0 ? q2 : q3));
    const double inv = (lead < 0.0 ? -1.0 : 1.0) / sqrt((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
    q0 *= inv, q1 *= inv, q2 *= inv, q3 *= inv;
    R[0] = (q0 * q0 + q1 * q1) - (q2 * q2 + q3 * q3), R[1] = 2.0 * (q1 * q2 - q0 * q3), R[2] = 2.0 * (q1 * q3 + q0 * q2);
    R[3] = 2.0 * (q1 * q2 + q0 * q3), R[4] = (q0 * q0 - q1 * q1) + (q2 * q2 - q3 * q3), R[5] = 2.0 * (q2 * q3 - q0 * q1);
    R[6] = 2.0 * (q1 * q3 - q0 * q2), R[7] = 2.0 * (q2 * q3 + q0 * q1), R[8] = (q0 * q0 - q1 * q1) - (q2 * q2 - q3 * q3);
}

// ---- b. one frame per wave ----
// v0, v1 or v2 by c = 0, 1, 2 (selects: an index that differs between lanes would put the array in scratch).
__device__ __forceinline__ double sup_pick(int c, double v0, double v1, double v2) { return c == 0 ? v0 : (c == 1 ? v1 : v2); }

// Selected atom i of the wave's frame: sel[i], or i without a table; -1 for a device entry outside the frame (its coordinates are NaN).
__device__ __forceinline__ int sup_atom(const int *sel, int i, int A) {
    const int a = sel ? sel[i] : i;
    return ((unsigned)a < (unsigned)A) ? a : -1;
}

// v[0..N) summed over the wave, all lanes holding the same bits.
template <int N>
__device__ __forceinline__ void sup_wave_sums(double (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = msm_group_sum<64>(v[j]);
}

// The centroid of the n_sel selected atoms of p [A, 3] (LDS or memory): lane l adds atoms l, l + 64, .. in order, then the butterfly.
__device__ __forceinline__ void sup_centroid(const float *p, const int *sel, int n_sel, int A, int lane, double (&c)[3]) {
    const double nan = __builtin_nan("");
    c[0] = c[1] = c[2] = 0.0;
    for (int i = lane; i < n_sel; i += 64) {
        const int a = sup_atom(sel, i, A);
        c[0] += a < 0 ? nan : (double)p[a * 3], c[1] += a < 0 ? nan : (double)p[a * 3 + 1], c[2] += a < 0 ? nan : (double)p[a * 3 + 2];
    }
    sup_wave_sums(c);
    c[0] /= (double)n_sel, c[1] /= (double)n_sel, c[2] /= (double)n_sel;
}

// out [F, A, 3], rmsd [F], rot [F, 3, 3], trans [F, 3], each may be NULL; pos [F, A, 3]; ref [A, 3] (ref_per_frame == 0) or [F, A, 3];
// sel [n_sel] with entries in 0 .. A - 1 (checked by the caller of the launch) or NULL = the atoms 0 .. n_sel - 1 = all; fixed u8 [A] or NULL.
// center_only: out = x - cx, rot = 1, trans = -cx, ref is not read.  out may be pos (a workgroup's frames are in LDS before it writes and
// no other workgroup reads them); out must not overlap ref.  grid ceil(F / fpb), 256 threads, fpb * A <= LSL_TORS_LDS_ATOMS.
// The workgroup's frames go in rounds of LSL_SUP_GROUP; fit[k] of frame k of the round: cx [3], cy [3], then S [9], replaced by R [9].
__global__ void __launch_bounds__(256) k_superpose(float *out, float *rmsd, double *rot, double *trans, const float *pos, const float *ref,
                                                   const int *sel, const unsigned char *fixed, long long F, int A, int n_sel, int fpb,
                                                   int ref_per_frame, int center_only) {
    __shared__ float atoms[LSL_TORS_LDS_ATOMS * 3];
    __shared__ double fit[LSL_SUP_GROUP][15];
    long long f0;
    const int nf = stage_frames(atoms, pos, F, A, fpb, &f0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double nan = __builtin_nan("");
    for (int g0 = 0; g0 < nf; g0 += LSL_SUP_GROUP) {
        const int ng = (nf - g0 < LSL_SUP_GROUP) ? (nf - g0) : LSL_SUP_GROUP;
        // 1. a wave per frame: the centroids and S (center_only: R = 1 at once)
        for (int k = wave; k < ng; k += 4) {
            const float *x = atoms + (g0 + k) * A * 3;
            const float *y = center_only ? nullptr : ref + (ref_per_frame ? (size_t)(f0 + g0 + k) * A * 3 : (size_t)0);
            double cx[3], cy[3] = {0.0, 0.0, 0.0}, S[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
            sup_centroid(x, sel, n_sel, A, lane, cx);
            if (!center_only) {
                sup_centroid(y, sel, n_sel, A, lane, cy);
#pragma unroll
                for (int c = 0; c < 9; ++c) S[c] = 0.0;
                for (int i = lane; i < n_sel; i += 64) {
                    const int a = sup_atom(sel, i, A);
                    double dx[3], dy[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) dx[c] = a < 0 ? nan : (double)x[a * 3 + c] - cx[c], dy[c] = a < 0 ? nan : (double)y[a * 3 + c] - cy[c];
#pragma unroll
                    for (int c = 0; c < 9; ++c) S[c] = fma(dx[c / 3], dy[c % 3], S[c]);
                }
                sup_wave_sums(S);
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) fit[k][c] = cx[c], fit[k][3 + c] = cy[c];
#pragma unroll
                for (int c = 0; c < 9; ++c) fit[k][6 + c] = S[c];
            }
        }
        __syncthreads();
        // 2. a thread per frame: S -> R
        if (!center_only && (int)threadIdx.x < ng) {
            double S[9], R[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) S[c] = fit[threadIdx.x][6 + c];
            sup_rotation(S, R);
#pragma unroll
            for (int c = 0; c < 9; ++c) fit[threadIdx.x][6 + c] = R[c];
        }
        __syncthreads();
        // 3. a wave per frame: the residuals, then the frame's outputs
        for (int k = wave; k < ng; k += 4) {
            const long long f = f0 + g0 + k;
            const float *x = atoms + (g0 + k) * A * 3;
            const float *y = center_only ? nullptr : ref + (ref_per_frame ? (size_t)f * A * 3 : (size_t)0);
            double cx[3], cy[3], R[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) cx[c] = fit[k][c], cy[c] = fit[k][3 + c];
#pragma unroll
            for (int c = 0; c < 9; ++c) R[c] = fit[k][6 + c];
            if (rmsd && !center_only) {
                double sq[1] = {0.0};
                for (int i = lane; i < n_sel; i += 64) {
                    const int a = sup_atom(sel, i, A);
                    double dx[3], e = 0.0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) dx[c] = a < 0 ? nan : (double)x[a * 3 + c] - cx[c];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double r = fma(R[c * 3 + 2], dx[2], fma(R[c * 3 + 1], dx[1], R[c * 3] * dx[0])) - (a < 0 ? nan : (double)y[a * 3 + c] - cy[c]);
                        e = fma(r, r, e);
                    }
                    sq[0] += e;
                }
                sup_wave_sums(sq);
                if (lane == 0) rmsd[f] = (float)sqrt(sq[0] / (double)n_sel);
            }
            if (rot) {
#pragma unroll
                for (int c = 0; c < 9; ++c)
                    if (lane == c) rot[(size_t)f * 9 + c] = R[c];
            }
            if (trans) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (lane == c) trans[(size_t)f * 3 + c] = cy[c] - fma(R[c * 3 + 2], cx[2], fma(R[c * 3 + 1], cx[1], R[c * 3] * cx[0]));
            }
            if (out) {
                float *o = out + (size_t)f * A * 3;
                for (int i = lane; i < A * 3; i += 64) {
                    const int a = i / 3, c = i - a * 3;
                    const double d0 = (double)x[a * 3] - cx[0], d1 = (double)x[a * 3 + 1] - cx[1], d2 = (double)x[a * 3 + 2] - cx[2];
                    const double r0 = sup_pick(c, R[0], R[3], R[6]), r1 = sup_pick(c, R[1], R[4], R[7]), r2 = sup_pick(c, R[2], R[5], R[8]);
                    const double r = fma(r2, d2, fma(r1, d1, r0 * d0)) + sup_pick(c, cy[0], cy[1], cy[2]);
                    o[i] = (fixed && fixed[a]) ? x[i] : (float)r;
                }
            }
        }
        __syncthreads();  // (the next round overwrites fit)
    }
}

// ---- c. per-atom mean and fluctuation over the frames ----
// sum_t p[t stride], t = 0 .. n - 1 in order (SQUARE: of (p[t stride] - m)^2), in fp64.  The loads go eight at a time ahead of their
// additions - the values are a cache line apart, one load per addition left the chain waiting on memory - the additions stay in order.
template <bool SQUARE, typename T>
__device__ __forceinline__ double rmsf_chain(const T *p, size_t stride, int n, double m) {
    double s = 0.0;
    int t = 0;
    for (; t + 8 <= n; t += 8) {
        T v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(t + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double d = (double)v[u] - m;
            s = SQUARE ? fma(d, d, s) : s + d;
        }
    }
    for (; t < n; ++t) {
        const double d = (double)p[(size_t)t * stride] - m;
        s = SQUARE ? fma(d, d, s) : s + d;
    }
    return s;
}

// The mean of column c of pos [F, C] from the first pass's partials part [nseg, C]: segments in order, one division.
__device__ __forceinline__ double rmsf_mean(const double *part, long long C, long long c, int nseg, long long F) {
    return rmsf_chain<false>(part + c, (size_t)C, nseg, 0.0) / (double)F;
}

// part[g, c] = sum over the frames f of segment g, in order, of pos[f, c] (SECOND: of (pos[f, c] - mean_c)^2, mean_c from `first`
// [nseg, C]).  pos [F, C], C = 3 A.  grid (ceil(C / 64), nseg), 64 threads.
template <bool SECOND>
__global__ void __launch_bounds__(64) k_atom_mean_partial(double *part, const double *first, const float *pos, long long F, long long C, int nseg) {
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const long long fa = (long long)blockIdx.y * LSL_RMSF_SEG;
    const int n = tile_rows(F, fa, LSL_RMSF_SEG);
    const double m = SECOND ? rmsf_mean(first, C, c, nseg, F) : 0.0;
    part[(size_t)blockIdx.y * C + c] = rmsf_chain<SECOND>(pos + (size_t)fa * C + c, (size_t)C, n, m);
}

// mean_out f64 [A, 3] and rmsf_out f32 [A] (each may be NULL) from the two passes' partials first, second [nseg, 3 A]:
// rmsf[a] = sqrt(((sx + sy) + sz) / F), each s the segments added in order.  grid ceil(A / 256), 256 threads.
__global__ void __launch_bounds__(256) k_atom_rmsf_final(double *mean_out, float *rmsf_out, const double *first, const double *second, long long F,
                                                         int A, int nseg) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const long long C = 3LL * A;
    double s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (mean_out) mean_out[(size_t)a * 3 + c] = rmsf_mean(first, C, 3LL * a + c, nseg, F);
        s[c] = rmsf_out ? rmsf_chain<false>(second + 3LL * a + c, (size_t)C, nseg, 0.0) : 0.0;
    }
    if (rmsf_out) rmsf_out[a] = (float)sqrt(((s[0] + s[1]) + s[2]) / (double)F);
}
