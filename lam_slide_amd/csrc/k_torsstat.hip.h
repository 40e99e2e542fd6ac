// Torsion statistics of a sampled peptide trajectory (lsl_dihedral_angles / lsl_histogram / lsl_lag_products / lsl_js_distance): the
// evaluation tail of the peptide family, analyze_trajectory (eval_peptide.py:102-182) behind the torsion features -
//      angle  = atan2((b1 . c1) |b2|, c1 . c2),  b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, c1 = b2 x b3, c2 = b1 x b2      (radians, [-pi, pi])
//      counts = np.histogram(x, range=, bins=)[0] / np.histogram2d(xa, xb, range=, bins=)[0] on a caller-given fp64 edge table
//      ac[k]  = (sum_{t < n - k} x_t x_{t+k}) / (n - k)            = acovf(x, demean=False, adjusted=True, nlag=)
//      jsd    = sqrt((sum rel_entr(p, m) + sum rel_entr(q, m)) / 2),  p, q = rows over their sums, m = (p + q) / 2    = jensenshannon(p, q)
//
// Work split.
//  k_dihedral     a workgroup of 256 threads owns fpb consecutive frames (fpb * A <= 2048 atoms: one frame of up to LSL_TORS_MAX_A atoms, or
//                 several small ones), copies their atoms to LDS once (stage_frames of k_stat_frag.hip.h) and thread i computes item
//                 i, i + 256, ... of the fpb * Q (frame, quadruple) items from LDS.  The quadruple table is general: any four atom slots.
//  k_hist1        a workgroup owns (series, a tile of qt columns with qt * bins <= 8192, 1024 rows): int32 counts in LDS by LDS integer atomics, the
//                 non-zero ones added to the int64 table in memory by integer atomics (flush_counts).  k_hist2: (series, pair, 1024 rows),
//                 bins2^2 <= 8192 cells.
//  k_lag_partial  a workgroup owns (series, channel, a tile of 256 lags, a segment of chunks of 448 time steps).  Per chunk it holds
//                 x[t0 .. t0 + 448) and x[t0 + k0 .. t0 + k0 + 448 + 256) of its channel in LDS; thread j (lag k0 + j) walks t ascending:
//                 x[t] is one address for the whole wave (a broadcast), x[t + k0 + j] consecutive addresses over the lanes (no bank conflict).
//                 The chunk's fp32 sum is added to the thread's fp64 sum of the segment.  k_lag_final adds the segments in segment order
//                 in fp64 and divides by n - k once.
//  k_js           a workgroup owns a row: the two int64 totals (js_totals: integers, exact in any order), then tiles of 256 bins - the
//                 threads compute the terms of a tile into LDS, thread 0 adds them in bin order in fp64.
//
// Determinism.  The only atomics are integer additions (LDS int32, memory int64), and integer addition has no order: counts are exact.
// No float atomics.  An angle is a function of its own four atoms, computed by one thread with a fixed operation sequence (no
// contraction: the products and sums below round one by one, in the order written).  A lagged product of lag k adds its terms in t order:
// 448 fused multiply-adds in fp32 per chunk (the longest fp32 addition chain is m = LSL_LAG_CHUNK = 448 <= 504), the chunk sums in chunk
// order in fp64, the segment sums in segment order in fp64.  The chunk and segment boundaries are a function of (n, nlag) alone
// (lag_segments below), not of S, C, the grid or the device: a series' row has the same bits alone and inside any batch.  The JS terms
// of a row are added in bin order in fp64.
#pragma once
#include "common.hip.h"
#include "k_stat_frag.hip.h"

#define LSL_TORS_MAX_A 2044        // 146 residues of 14 atoms: a frame in LDS (the GEOM_MAX_A entities of lsl_geom_loss_sums hold 2048)
#define LSL_TORS_MAX_Q 65536       // quadruples of one call of lsl_dihedral_angles
#define LSL_TORS_LDS_ATOMS 2048    // atoms of the frames one workgroup of k_dihedral stages
#define LSL_HIST_MAX_BINS 2048     // 1-D: the fp64 edge table (16 KiB) beside LSL_HIST_CELLS int32 counts (32 KiB) in LDS
#define LSL_HIST_CELLS 8192        // int32 counts a workgroup holds: qt * bins (1-D), bins2 * bins2 (2-D: bins2 <= 90)
#define LSL_HIST2_MAX_BINS 90      // 2-D: 90 * 90 <= LSL_HIST_CELLS
#define LSL_HIST_ROWS 1024        // rows of x per workgroup: an LDS count stays <= 1024
#define LSL_LAG_TILE 256           // lags per workgroup (one thread each)
#define LSL_LAG_CHUNK 448          // time steps per LDS chunk = the longest fp32 addition chain m
#define LSL_LAG_MAX_ROWS 65535     // S * C of one call of lsl_lag_products: (series, channel) rows are a grid dimension
#define LSL_LAG_MAX_PART (1 << 21) // fp64 partials per (series, channel): segments * (nlag + 1) stays at or below this (16 MiB)

// ---- a. dihedral angles ----
// The same operation order as the fp32 statement of the formula component by component: every product and sum rounds on its own.
__device__ __forceinline__ float tors_dihedral(const float *p0, const float *p1, const float *p2, const float *p3) {
#pragma clang fp contract(off)
    const float b1x = p1[0] - p0[0], b1y = p1[1] - p0[1], b1z = p1[2] - p0[2];
    const float b2x = p2[0] - p1[0], b2y = p2[1] - p1[1], b2z = p2[2] - p1[2];
    const float b3x = p3[0] - p2[0], b3y = p3[1] - p2[1], b3z = p3[2] - p2[2];
    const float c1x = b2y * b3z - b2z * b3y, c1y = b2z * b3x - b2x * b3z, c1z = b2x * b3y - b2y * b3x;  // b2 x b3
    const float c2x = b1y * b2z - b1z * b2y, c2y = b1z * b2x - b1x * b2z, c2z = b1x * b2y - b1y * b2x;  // b1 x b2
    const float nb2 = sqrtf((b2x * b2x + b2y * b2y) + b2z * b2z);
    const float y = ((b1x * c1x + b1y * c1y) + b1z * c1z) * nb2;
    const float x = (c1x * c2x + c1y * c2y) + c1z * c2z;
    return (float)atan2((double)y, (double)x);  // (the fp64 arctangent rounded once: the last step adds half an ulp, not atan2f's few)
}

// angles[f * Q + q] of frames f = 0 .. F - 1; pos [F, A, 3], quads [Q, 4] with entries in 0 .. A - 1 (checked by the caller of the launch;
// an entry outside gives NaN here, nothing is read with it).  grid ceil(F / fpb), 256 threads, fpb * A <= LSL_TORS_LDS_ATOMS.
__global__ void __launch_bounds__(256) k_dihedral(float *angles, const float *pos, const int *quads, long long F, int A, int Q, int fpb) {
    __shared__ float atoms[LSL_TORS_LDS_ATOMS * 3];
    long long f0;
    const int nf = stage_frames(atoms, pos, F, A, fpb, &f0);
    const int items = nf * Q;
    for (int i = threadIdx.x; i < items; i += 256) {
        const int fl = i / Q, q = i - fl * Q;
        const int a0 = quads[q * 4], a1 = quads[q * 4 + 1], a2 = quads[q * 4 + 2], a3 = quads[q * 4 + 3];
        float ang = __builtin_nanf("");
        if ((unsigned)a0 < (unsigned)A && (unsigned)a1 < (unsigned)A && (unsigned)a2 < (unsigned)A && (unsigned)a3 < (unsigned)A) {
            const float *fr = atoms + fl * A * 3;
            ang = tors_dihedral(fr + a0 * 3, fr + a1 * 3, fr + a2 * 3, fr + a3 * 3);
        }
        angles[(size_t)(f0 + fl) * Q + q] = ang;
    }
}

// ---- b. histograms ----
// The bin of v in the ascending table e[0 .. bins]: i with e[i] <= v < e[i + 1], the last bin closed on the right; -1 outside [e[0],
// e[bins]] and for NaN.  The multiply-and-floor estimate is right for a uniform table up to a step; the walk against the table itself
// decides (np.histogram corrects its estimate the same way), and is right for any ascending table.  Every index stays in 0 .. bins - 1.
__device__ __forceinline__ int tors_bin(double v, const double *e, int bins) {
    if (!(v >= e[0] && v <= e[bins])) return -1;
    const double f = (v - e[0]) / (e[bins] - e[0]) * (double)bins;
    int i = (f >= 0.0 && f < (double)bins) ? (int)f : (f >= (double)bins ? bins - 1 : 0);  // (a NaN estimate of a degenerate table: 0)
    while (i > 0 && v < e[i]) --i;
    while (i < bins - 1 && v >= e[i + 1]) ++i;
    return i;
}

// counts[(s Q + q) bins + b] += number of rows t of x [S, n, Q] with x[s, t, q] in bin b.  grid (ceil(n / LSL_HIST_ROWS), ceil(Q / qt), S),
// 256 threads, qt * bins <= LSL_HIST_CELLS, bins <= LSL_HIST_MAX_BINS.
__global__ void __launch_bounds__(256) k_hist1(unsigned long long *counts, const float *x, const double *edges, int n, int Q, int bins, int qt) {
    __shared__ double e[LSL_HIST_MAX_BINS + 1];
    __shared__ int cnt[LSL_HIST_CELLS];
    const int s = blockIdx.z, q0 = blockIdx.y * qt, nq = (Q - q0 < qt) ? (Q - q0) : qt;
    const int t0 = blockIdx.x * LSL_HIST_ROWS, nt = tile_rows(n, t0, LSL_HIST_ROWS);
    for (int i = threadIdx.x; i <= bins; i += 256) e[i] = edges[i];
    for (int i = threadIdx.x; i < nq * bins; i += 256) cnt[i] = 0;
    __syncthreads();
    const float *xs = x + ((size_t)s * n + t0) * Q + q0;
    for (int i = threadIdx.x; i < nt * nq; i += 256) {
        const int t = i / nq, q = i - t * nq;
        const int b = tors_bin((double)xs[(size_t)t * Q + q], e, bins);
        if (b >= 0) atomicAdd(&cnt[q * bins + b], 1);
    }
    __syncthreads();
    flush_counts(counts + ((size_t)s * Q + q0) * bins, cnt, nq * bins);
}

// counts2[((s P + p) bins2 + ia) bins2 + ib] += number of rows t with x[s, t, pairs[p][0]] in bin ia of ea and x[s, t, pairs[p][1]] in bin
// ib of eb; a row is dropped when either coordinate is.  grid (ceil(n / LSL_HIST_ROWS), P, S), 256 threads, bins2^2 <= LSL_HIST_CELLS.
__global__ void __launch_bounds__(256) k_hist2(unsigned long long *counts2, const float *x, const int *pairs, const double *edges_a, const double *edges_b,
                                               int n, int Q, int P, int bins2) {
    __shared__ double ea[LSL_HIST2_MAX_BINS + 1], eb[LSL_HIST2_MAX_BINS + 1];
    __shared__ int cnt[LSL_HIST_CELLS];
    const int s = blockIdx.z, p = blockIdx.y, cells = bins2 * bins2;
    const int t0 = blockIdx.x * LSL_HIST_ROWS, nt = tile_rows(n, t0, LSL_HIST_ROWS);
    for (int i = threadIdx.x; i <= bins2; i += 256) ea[i] = edges_a[i], eb[i] = edges_b[i];
    for (int i = threadIdx.x; i < cells; i += 256) cnt[i] = 0;
    __syncthreads();
    const int qa = pairs[p * 2], qb = pairs[p * 2 + 1];
    if ((unsigned)qa < (unsigned)Q && (unsigned)qb < (unsigned)Q) {  // (uniform over the workgroup; checked by the caller of the launch)
        const float *xs = x + ((size_t)s * n + t0) * Q;
        for (int t = threadIdx.x; t < nt; t += 256) {
            const int ia = tors_bin((double)xs[(size_t)t * Q + qa], ea, bins2), ib = tors_bin((double)xs[(size_t)t * Q + qb], eb, bins2);
            if (ia >= 0 && ib >= 0) atomicAdd(&cnt[ia * bins2 + ib], 1);
        }
    }
    __syncthreads();
    flush_counts(counts2 + ((size_t)s * P + p) * cells, cnt, cells);
}

// ---- c. lagged products ----
// The split of the time axis, a function of (n, nlag) alone: chunks of LSL_LAG_CHUNK steps, cps chunks per segment, nseg segments, with
// nseg * (nlag + 1) <= LSL_LAG_MAX_PART (nlag + 1 <= LSL_LAG_MAX_PART is the caller's check) and nseg <= 65535 (a grid dimension).
struct LagSplit { int cps, nseg; };
inline LagSplit lag_segments(int n, int nlag) {
    const long long chunks = ((long long)n + LSL_LAG_CHUNK - 1) / LSL_LAG_CHUNK;
    long long cap = (long long)LSL_LAG_MAX_PART / ((long long)nlag + 1);
    if (cap < 1) cap = 1;
    if (cap > 65535) cap = 65535;  // (the segments are grid.y of k_lag_partial)
    const long long cps = (chunks + cap - 1) / cap;
    return LagSplit{(int)cps, (int)((chunks + cps - 1) / cps)};
}

// part[((sc nseg + seg) (nlag + 1)) + k] = sum over the segment's t < n - k of x[s, t, c] x[s, t + k, c]: fp32 within a chunk, t ascending,
// the chunks added in fp64 in chunk order.  x [S, n, C]; grid (ceil((nlag + 1) / 256), nseg, S * C), 256 threads.
__global__ void __launch_bounds__(LSL_LAG_TILE) k_lag_partial(double *part, const float *x, int n, int C, int nlag, int cps) {
    __shared__ float xl[LSL_LAG_CHUNK], xr[LSL_LAG_CHUNK + LSL_LAG_TILE];
    const int sc = blockIdx.z, s = sc / C, c = sc - s * C;
    const int seg = blockIdx.y, nseg = gridDim.y;
    const int k0 = blockIdx.x * LSL_LAG_TILE, k = k0 + (int)threadIdx.x;
    const float *xs = x + (size_t)s * n * C + c;
    const long long t_first = (long long)seg * cps * LSL_LAG_CHUNK;
    double acc = 0.0;
    for (int ch = 0; ch < cps; ++ch) {
        const long long t0 = t_first + (long long)ch * LSL_LAG_CHUNK;
        if (t0 + k0 >= n) break;  // (uniform: no lag of this tile has a term from here on)
        for (int i = threadIdx.x; i < LSL_LAG_CHUNK; i += LSL_LAG_TILE) xl[i] = (t0 + i < n) ? xs[(size_t)(t0 + i) * C] : 0.0f;
        for (int i = threadIdx.x; i < LSL_LAG_CHUNK + LSL_LAG_TILE; i += LSL_LAG_TILE)
            xr[i] = (t0 + k0 + i < n) ? xs[(size_t)(t0 + k0 + i) * C] : 0.0f;
        __syncthreads();
        const long long left = (long long)n - k - t0;  // terms t0 .. n - k - 1 remain for lag k
        const int tend = left < LSL_LAG_CHUNK ? (left > 0 ? (int)left : 0) : LSL_LAG_CHUNK;
        float a = 0.0f;
        const float *r = xr + threadIdx.x;
        for (int t = 0; t < tend; ++t) a = fmaf(xl[t], r[t], a);
        acc += (double)a;
        __syncthreads();
    }
    if (k <= nlag) part[((size_t)sc * nseg + seg) * ((size_t)nlag + 1) + k] = acc;
}

// ac[sc (nlag + 1) + k] = (sum over seg of part[sc, seg, k], seg ascending, fp64) / (n - k), rounded to fp32 once.
__global__ void __launch_bounds__(256) k_lag_final(float *ac, const double *part, int n, int nlag, int nseg) {
    const int k = blockIdx.x * 256 + (int)threadIdx.x, sc = blockIdx.y;
    if (k > nlag) return;
    const double *p = part + (size_t)sc * nseg * ((size_t)nlag + 1) + k;
    double s = 0.0;
    for (int g = 0; g < nseg; ++g) s += p[(size_t)g * ((size_t)nlag + 1)];
    ac[(size_t)sc * ((size_t)nlag + 1) + k] = (float)(s / (double)(n - k));
}

// ---- d. Jensen-Shannon distance ----
__device__ __forceinline__ double tors_rel_entr(double p, double m) {  // scipy.special.rel_entr
    if (p != p || m != m) return __builtin_nan("");
    if (p > 0.0 && m > 0.0) return p * log(p / m);
    if (p == 0.0 && m >= 0.0) return 0.0;
    return __builtin_inf();
}

// out[r] = jensenshannon(a[r, :], b[r, :]) of two non-negative int64 count tables [rows, bins].  grid rows, 256 threads.  A row whose
// counts are all zero on either side: 0 / 0 = NaN, as scipy.  A sum that rounding left below zero is 0 (equal rows give exactly 0).
__global__ void __launch_bounds__(256) k_js(double *out, const long long *a, const long long *b, int bins) {
    __shared__ long long tot[2][256];
    __shared__ double term[2][256];
    const long long *ra = a + (size_t)blockIdx.x * bins, *rb = b + (size_t)blockIdx.x * bins;
    js_totals(tot, ra, rb, bins);
    const double na = (double)tot[0][0], nb = (double)tot[1][0];
    double left = 0.0, right = 0.0;  // (thread 0's: sum rel_entr(p, m), sum rel_entr(q, m))
    for (int i0 = 0; i0 < bins; i0 += 256) {
        const int i = i0 + (int)threadIdx.x;
        if (i < bins) {
            const double p = (double)ra[i] / na, q = (double)rb[i] / nb, m = (p + q) / 2.0;
            term[0][threadIdx.x] = tors_rel_entr(p, m), term[1][threadIdx.x] = tors_rel_entr(q, m);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int lim = (bins - i0 < 256) ? (bins - i0) : 256;
            for (int j = 0; j < lim; ++j) left += term[0][j], right += term[1][j];
        }
        __syncthreads();
    }
    const double js = left + right;
    if (threadIdx.x == 0) out[blockIdx.x] = sqrt((js < 0.0 ? 0.0 : js) / 2.0);
}
