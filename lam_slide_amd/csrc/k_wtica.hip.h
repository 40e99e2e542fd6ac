// Koopman-reweighted TICA on wide feature tables (lsl_weighted_moments / lsl_affine_weights / lsl_project_wide): run_tica of the peptide
// validation (utils/tica_utils.py:42-48) over tica_features, 129 .. 2048 columns -
//      moments  sw = sum w_t, sx = sum w_t x_t, sy = sum w_t x_{t+lag}, xx = sum w_t x_t x_t^T, yy = sum w_t x_{t+lag} x_{t+lag}^T,
//               xy = sum w_t x_t x_{t+lag}^T over t < m = n - lag (w: the Koopman weights, or all ones)
//      weights  w[t] = sum_f x[t, f] u[f] + c
//      project  y[t, j] = fp32(sum_f (x[t, f] - mean[f]) W[f, j]), with the running minimum / maximum of every output column
//
// Work split of the moments.  A row is extended by one virtual column of ones, x~ = [x, 1] (Fe = F + 1 columns), so that the sums are
// entries of the matrices: sx[a] = xx~[a, F], sy[a] = yy~[a, F], sw = xx~[F, F].  The output is cut into tiles of LSL_WMOM_TILE^2 entries; a
// job is one tile of one matrix: the tiles A <= B of xx~ and of yy~ (the lower triangle is mirrored afterwards) and every tile of xy.  A
// workgroup of 256 threads owns (job, time split).  It streams chunks of LSL_WMOM_ROWS rows through LDS, double-buffered: the chunk after
// the current one is loaded from memory into registers before the current one is multiplied and stored to the other buffer after it, one
// barrier per chunk.  The P operand (the tile's rows a) is stored as fp64 already scaled, p = w_t * (double)x~[t, a] (one rounding; exact
// when w is NULL); the Q operand (the tile's columns b) as fp32.  Thread (ty, tx) holds the 4 x 4 block of entries a = 4 ty .., b = 4 tx ..
// in fp64 registers and walks t ascending: acc = fma(p, (double)q, acc) - plain fp64 fused multiply-adds, not the fp64 MFMA.
// Four waves per SIMD are asked for (128 VGPRs, 24 KiB of LDS): measured faster than three with 32-row chunks and level 2 in registers.
//
// Summation order of one entry (a function of (n, lag, F) alone: not of the grid, the run or the device).
//   level 0  the rows of a segment (segment g: t in [1024 g, 1024 (g + 1)) below m), t ascending, fused multiply-adds from zero
//   level 1  the segments, g ascending, added to a second accumulator; it is added to the split's sum (level 2: the thread's own entries of the
//            workspace - the first group's sum is stored, later ones are added) and cleared after every segment with (g + 1) % 1024 == 0 and
//            after the last segment of the time split
//   splits   time split s holds the segments [s q, (s + 1) q): q = ceil(segments / want), want = min(32, ceil(1024 / jobs), segments)
//            - wmom_plan below; the splits' sums are added in split order by k_wmom_final, which also mirrors xx and yy.
// Roundings on the longest path to an entry: 1 (the scaling by w_t) + 1024 (level 0) + 1024 (level 1) + 2049 (level 2: n < 2^31 has at most
// 2^21 segments = 2048 groups of 1024, one more because a split need not start on a group boundary) + 32 (splits) = LSL_WMOM_CHAIN = 4130:
// every entry within LSL_WMOM_CHAIN 2^-53 sum_t |w_t x_a x_b| of the exact sum.  No atomics at all in the moments; the projection uses
// the integer minimum / maximum of k_project (lim_init / lim_update / lim_flush of k_stat_frag.hip.h) for its limits.
#pragma once
#include "common.hip.h"
#include "k_stat_frag.hip.h"
#include "k_tica.hip.h"

#define LSL_WMOM_MIN_F 129     // below: lsl_lagged_moments / lsl_project
#define LSL_WMOM_MAX_F 2048    // features of a row
#define LSL_WMOM_TILE 64       // the side of a workgroup's output tile
#define LSL_WMOM_ROWS 16       // rows of a chunk in LDS (two buffers: 24 KiB)
#define LSL_WMOM_SEG 1024      // rows of a segment: the level-0 chain
#define LSL_WMOM_SEG1 1024     // segments of a group: the level-1 chain
#define LSL_WMOM_MAX_SPLITS 32 // time splits of one call
#define LSL_WMOM_JOBS 1024     // workgroups aimed at: want = ceil(LSL_WMOM_JOBS / jobs) splits
#define LSL_WMOM_CHAIN (1 + LSL_WMOM_SEG + LSL_WMOM_SEG1 + 2049 + LSL_WMOM_MAX_SPLITS)
#define LSL_WPROJ_MAX_D 64     // output columns of lsl_project_wide
#define LSL_WPROJ_ROWS 64      // rows of x per workgroup of k_project_wide
#define LSL_WPROJ_FC 32        // features of a chunk of W and x in LDS

struct WmomPlan {
    int Te, T, jobs, nseg, q, nsplit;  // tiles per side of xx~ / yy~ and of xy, jobs, segments, segments per split, splits
};
inline WmomPlan wmom_plan(int n, int F, int lag) {
    WmomPlan p;
    const long long m = (long long)n - lag;
    p.Te = (F + 1 + LSL_WMOM_TILE - 1) / LSL_WMOM_TILE;
    p.T = (F + LSL_WMOM_TILE - 1) / LSL_WMOM_TILE;
    p.jobs = p.Te * (p.Te + 1) + p.T * p.T;
    p.nseg = (int)((m + LSL_WMOM_SEG - 1) / LSL_WMOM_SEG);
    int want = (LSL_WMOM_JOBS + p.jobs - 1) / p.jobs;
    want = want > LSL_WMOM_MAX_SPLITS ? LSL_WMOM_MAX_SPLITS : want;
    want = want > p.nseg ? p.nseg : want;
    p.q = (p.nseg + want - 1) / want;
    p.nsplit = (p.nseg + p.q - 1) / p.q;
    return p;
}
__host__ __device__ inline size_t wmom_part_entries(int F) { return 3 * (size_t)(F + 1) * (F + 1); }  // xx~, yy~, xy~ of one split, [Fe, Fe] each

// part[((s 3 + kind) Fe + a) Fe + b]: the sum over time split s of entry (a, b) of kind 0 xx~, 1 yy~ (tiles A <= B only), 2 xy.
// grid (jobs, nsplit), 256 threads; w [m] or NULL.
__global__ void __launch_bounds__(256, 4) k_wmom_tiles(double *part, const float *x, const double *w, int n, int F, int lag, int Te, int T, int q) {
    __shared__ __attribute__((aligned(16))) double ps[2][LSL_WMOM_ROWS * LSL_WMOM_TILE];
    __shared__ __attribute__((aligned(16))) float qs[2][LSL_WMOM_ROWS * LSL_WMOM_TILE];
    const int Fe = F + 1, ntri = Te * (Te + 1) / 2;
    int kind, A, B;
    {
        int i = blockIdx.x;
        if (i < 2 * ntri) {
            kind = i >= ntri;
            i -= kind * ntri;
            A = 0;
            while (i >= Te - A) i -= Te - A, ++A;
            B = A + i;
        } else {
            kind = 2;
            i -= 2 * ntri;
            A = i / T, B = i - A * T;
        }
    }
    const long long m = (long long)n - lag;
    const long long row_first = (long long)blockIdx.y * q * LSL_WMOM_SEG;
    long long row_last = row_first + (long long)q * LSL_WMOM_SEG;  // [row_first, row_last) below m: whole segments but the last
    if (row_last > m) row_last = m;
    const int nch = (int)((row_last - row_first + LSL_WMOM_ROWS - 1) / LSL_WMOM_ROWS);
    const long long ch_first = row_first / LSL_WMOM_ROWS;  // the index of the first chunk in the window: segment and group boundaries follow it
    const float *xp = x + (kind == 1 ? (size_t)lag * F : 0), *xq = x + (kind >= 1 ? (size_t)lag * F : 0);
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int sr = tid >> 6, sc = tid & 63;  // staging: this thread moves column sc of rows sr, sr + 4, ..
    const int gp = A * LSL_WMOM_TILE + sc, gq = B * LSL_WMOM_TILE + sc;
    const float padp = gp == F ? 1.0f : 0.0f, padq = gq == F ? 1.0f : 0.0f;  // (the virtual column of ones; zeros past it)
    double acc0[4][4], acc1[4][4], pv[LSL_WMOM_ROWS / 4];
    float qv[LSL_WMOM_ROWS / 4];
    bool first_group = true;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc0[i][j] = acc1[i][j] = 0.0;

#define WMOM_FETCH(c)                                                                                    \
    {                                                                                                    \
        const long long t0_ = row_first + (long long)(c) * LSL_WMOM_ROWS;                                \
        _Pragma("unroll") for (int k = 0; k < LSL_WMOM_ROWS / 4; ++k) {                                                  \
            const long long t_ = t0_ + sr + 4 * k;                                                       \
            pv[k] = 0.0, qv[k] = 0.0f;                                                                   \
            if (t_ < row_last) { /* (rows past the split are never multiplied: nothing is loaded) */     \
                const double wt_ = w ? w[t_] : 1.0;                                                      \
                pv[k] = wt_ * (double)(gp < F ? xp[(size_t)t_ * F + gp] : padp);                         \
                qv[k] = gq < F ? xq[(size_t)t_ * F + gq] : padq;                                         \
            }                                                                                            \
        }                                                                                                \
    }
#define WMOM_STORE(buf)                                                                                  \
    _Pragma("unroll") for (int k = 0; k < LSL_WMOM_ROWS / 4; ++k) {                                                      \
        ps[buf][(sr + 4 * k) * LSL_WMOM_TILE + sc] = pv[k];                                              \
        qs[buf][(sr + 4 * k) * LSL_WMOM_TILE + sc] = qv[k];                                              \
    }

    double *out = part + ((size_t)blockIdx.y * 3 + kind) * Fe * Fe;
    if (nch > 0) {
        WMOM_FETCH(0);
        WMOM_STORE(0);
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const int cur = c & 1;
        if (c + 1 < nch) WMOM_FETCH(c + 1);
        const long long left = row_last - (row_first + (long long)c * LSL_WMOM_ROWS);
        const int rows = left < LSL_WMOM_ROWS ? (int)left : LSL_WMOM_ROWS;
        const double *pp = ps[cur] + ty * 4;
        const float *qq = qs[cur] + tx * 4;
#define WMOM_ROW(r)                                                                                                                    \
    {                                                                                                                                  \
        const double2 pa = *(const double2 *)(pp + (r) * LSL_WMOM_TILE), pb = *(const double2 *)(pp + (r) * LSL_WMOM_TILE + 2);          \
        const float4 qf = *(const float4 *)(qq + (r) * LSL_WMOM_TILE);                                                                 \
        const double p[4] = {pa.x, pa.y, pb.x, pb.y};                                                                                  \
        const double qd[4] = {(double)qf.x, (double)qf.y, (double)qf.z, (double)qf.w};                                                 \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j) acc0[i][j] = fma(p[i], qd[j], acc0[i][j]); \
    }
#pragma unroll 4  // (the kernel is sensitive to occupancy - DESIGN 6k: deeper unrolling was measured slower)
        for (int r = 0; r < rows; ++r) WMOM_ROW(r)
#undef WMOM_ROW
        if (c + 1 < nch) WMOM_STORE(cur ^ 1);
        __syncthreads();
        const long long done = ch_first + c + 1;  // chunks of the window finished
        const bool last = c + 1 == nch;
        if (last || done % (LSL_WMOM_SEG / LSL_WMOM_ROWS) == 0) {  // the end of a segment
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc1[i][j] += acc0[i][j], acc0[i][j] = 0.0;
            if (last || done % ((long long)LSL_WMOM_SEG1 * (LSL_WMOM_SEG / LSL_WMOM_ROWS)) == 0) {  // the end of a group of segments
                // level 2 lives in the split's own entries of part (this thread's alone: no race): the first group's sum is stored, later ones added
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int a = A * LSL_WMOM_TILE + ty * 4 + i;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int b = B * LSL_WMOM_TILE + tx * 4 + j;
                        if (a < Fe && b < Fe) out[(size_t)a * Fe + b] = first_group ? acc1[i][j] : out[(size_t)a * Fe + b] + acc1[i][j];
                        acc1[i][j] = 0.0;
                    }
                }
                first_group = false;
            }
        }
    }
#undef WMOM_FETCH
#undef WMOM_STORE
}

// out [1 + 2 F + 3 F^2] = (sw, sx [F], sy [F], xx [F, F], yy [F, F], xy [F, F]): entry e's partials of the splits added in split order;
// xx[a, b] and yy[a, b] with a > b read entry (b, a).  grid ceil(E / 256), 256 threads.
__global__ void __launch_bounds__(256) k_wmom_final(double *out, const double *part, int F, int nsplit) {
    const long long FF = (long long)F * F, E = 1 + 2LL * F + 3 * FF;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int Fe = F + 1;
    int kind, a, b;
    if (e == 0) kind = 0, a = F, b = F;
    else if (e <= F) kind = 0, a = (int)e - 1, b = F;
    else if (e <= 2 * F) kind = 1, a = (int)e - 1 - F, b = F;
    else {
        long long r = e - 1 - 2 * F;
        kind = (int)(r / FF);
        r -= kind * FF;
        a = (int)(r / F), b = (int)(r - (long long)a * F);
        if (kind < 2 && a > b) {
            const int t = a;
            a = b, b = t;
        }
    }
    const size_t stride = wmom_part_entries(F);
    const double *p = part + ((size_t)kind * Fe + a) * Fe + b;
    double s = p[0];
    for (int g = 1; g < nsplit; ++g) s += p[(size_t)g * stride];
    out[e] = s;
}

// The chain of lsl_project_wide and lsl_affine_weights: acc[t, j] = sum_f (x[t, f] - mean[f]) W[f, j], the subtraction and the fused chain
// over f ascending in fp64 (mean NULL: no subtraction).  A workgroup owns LSL_WPROJ_ROWS rows and every column j < d: wave v holds the
// columns [v jw, (v + 1) jw), jw = ceil(d / 4) <= 16, lane r the row.  x - mean (fp64) and W stream through LDS in chunks of LSL_WPROJ_FC
// features, f ascending - the same order for every grid.  AFFINE: wout[t] = acc[t, 0] + c in fp64.  Otherwise y[t, j] = fp32(acc) and keys
// as k_project.  grid ceil(n / LSL_WPROJ_ROWS), 256 threads.
template <bool AFFINE>
__global__ void __launch_bounds__(256) k_project_wide(float *y, double *wout, const float *x, const double *mean, const double *W, double c, unsigned *keys,
                                                      int n, int F, int d) {
    __shared__ double xd[LSL_WPROJ_ROWS * (LSL_WPROJ_FC + 1)];  // (an odd row stride: the rows of a wave's lanes fall on different banks)
    __shared__ double Ws[LSL_WPROJ_FC * LSL_WPROJ_MAX_D];
    __shared__ unsigned kmin[LSL_WPROJ_MAX_D], kmax[LSL_WPROJ_MAX_D];
    const int tid = threadIdx.x, r = tid & 63, v = tid >> 6;
    const int jw = (d + 3) / 4, j0 = v * jw;
    const long long t0 = (long long)blockIdx.x * LSL_WPROJ_ROWS;
    const int rows = tile_rows(n, t0, LSL_WPROJ_ROWS);
    lim_init(kmin, kmax, LSL_WPROJ_MAX_D);
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    const float *src = x + (size_t)t0 * F;
    for (int f0 = 0; f0 < F; f0 += LSL_WPROJ_FC) {
        const int fc = (F - f0 < LSL_WPROJ_FC) ? (F - f0) : LSL_WPROJ_FC;
        __syncthreads();  // (the chunk before has been read)
        for (int i = tid; i < rows * LSL_WPROJ_FC; i += 256) {
            const int rr = i / LSL_WPROJ_FC, ff = i - rr * LSL_WPROJ_FC;
            if (ff < fc) xd[rr * (LSL_WPROJ_FC + 1) + ff] = (double)src[(size_t)rr * F + f0 + ff] - (mean ? mean[f0 + ff] : 0.0);
        }
        for (int i = tid; i < fc * d; i += 256) Ws[i] = W[(size_t)f0 * d + i];
        __syncthreads();
        if (r < rows && j0 < d) {
            const double *xr = xd + r * (LSL_WPROJ_FC + 1);
            for (int ff = 0; ff < fc; ++ff) {
                const double dv = xr[ff];
                const double *wr = Ws + ff * d + j0;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < jw && j0 + k < d) acc[k] = fma(dv, wr[k], acc[k]);
            }
        }
    }
    if (r < rows && j0 < d) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int j = j0 + k;
            if (k >= jw || j >= d) continue;
            if (AFFINE) {
                wout[t0 + r] = acc[k] + c;
            } else {
                const float val = (float)acc[k];
                y[((size_t)t0 + r) * d + j] = val;
                if (keys) lim_update(kmin, kmax, j, val);
            }
        }
    }
    if (AFFINE || !keys) return;
    __syncthreads();
    lim_flush(keys, kmin, kmax, d);
}
