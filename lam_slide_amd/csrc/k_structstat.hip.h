// Structure statistics of a sampled peptide trajectory (lsl_pair_distances / lsl_ca_frame_stats / lsl_histogram_columns /
// lsl_js_distance_density): what SIAtom14SampleCallback logs per validation epoch through traj_analysis (utils/traj_utils.py:63-103,
// utils/backbone_utils.py, utils/tica_utils.py:12-39) -
//      dist     = sqrtf((dx dx + dy dy) + dz dz),  d = pos[pairs[p][0]] - pos[pairs[p][1]]                  = np.linalg.norm(.., axis=-1) on float32
//      rg       = sqrt(mean_i |x_i - mean_j x_j|^2) over the selected atoms                                  = mdtraj.compute_rg, unit masses
//      flags    = (some d_ij < clash_thr, i < j) | (some d_{i,i+1} > break_thr) << 1                          = compute_validity
//      contacts = #{frames : d_ij < contact_thr}, i < j                                                      = compute_contact_matrix x frames
//      counts   = np.histogram(x[:, q], bins=edges[q])[0], one edge table per column                         = discretize_features' counts
//      js       = jensenshannon(h_a, h_b),  h = counts / measure / N + pseudo                                = density=True + pseudo_count
//
// Work split.
//  k_pair_dist    as k_dihedral: a workgroup of 256 threads owns fpb consecutive frames (fpb * A <= LSL_TORS_LDS_ATOMS), copies their atoms
//                 to LDS (stage_frames of k_stat_frag.hip.h) and thread i computes item i, i + 256, ... of the fpb * P (frame, pair) items from LDS.
//  k_ca_stats     a workgroup owns a tile of tf consecutive frames (tf <= 256, tf * R <= LSL_CA_LDS_ATOMS) and holds their R selected atoms in
//                 LDS, coordinate-major with the frame innermost (at[(c R + r) tfs + frame], tfs odd: the threads of the frame pass read
//                 consecutive words, the threads of the pair pass read words an odd stride apart).  Frame pass: thread f owns frame f - rg in
//                 fp64, then all i < j distances for the two flag bits; the four tallies are LDS integer counts, added to memory by one int64
//                 atomic each.  Pair pass: thread p owns the cells p, p + 256, ... of the R x R table with i < j, walks the tile's frames
//                 with a register count and adds a non-zero count to memory by one int64 atomic.
//  k_hist_cols    a workgroup owns (a tile of qt columns, LSL_HIST_ROWS rows): the qt edge tables (fp64) and qt * bins int32 counts in LDS,
//                 qt * (bins + 1) <= LSL_HCOL_CELLS; counts by LDS integer atomics, the non-zero ones added to the int64 table by integer
//                 atomics (flush_counts).
//  k_js_density   a workgroup owns a row: the two int64 totals (js_totals), then tiles of 256 bins twice - first the sums of the two density
//                 rows, then the terms; in both the threads compute a tile into LDS and thread 0 adds it in bin order in fp64 (as k_js).
//
// Determinism.  The only atomics are integer additions of counts (LDS int32, memory int64): exact in any order.  No float atomics.  A
// distance is a function of its own two atoms, computed by one thread with a fixed operation sequence (no contraction).  rg of a frame is
// two fp64 sums over the selected atoms in sel order by one thread.  A density row's sum and its JS terms are added in bin order in fp64.
// Nothing depends on the grid, the tile or the frame's place in the batch: a frame has the same bits alone and inside any batch.
#pragma once
#include "common.hip.h"
#include "k_stat_frag.hip.h"
#include "k_torsstat.hip.h"

#define LSL_PAIR_MAX_P 65536      // pairs of one call of lsl_pair_distances
#define LSL_CA_MAX_R 146          // selected atoms of a frame in lsl_ca_frame_stats: the residues of a frame of LSL_TORS_MAX_A atoms
#define LSL_CA_LDS_ATOMS 2048     // selected atoms of the frames one workgroup of k_ca_stats stages
#define LSL_CA_TILE 256           // frames per workgroup at most: one thread each in the frame pass
#define LSL_HCOL_CELLS 4096       // fp64 edges (qt * (bins + 1), 32 KiB) and int32 counts (qt * bins, 16 KiB) a workgroup of k_hist_cols holds

// ---- a. pair distances ----
// np.linalg.norm of the float32 difference: every product and sum rounds on its own, in the order written; sqrtf is correctly rounded.
__device__ __forceinline__ float ss_dist(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// dist[f * P + p] of frames f = 0 .. F - 1; pos [F, A, 3], pairs [P, 2] with entries in 0 .. A - 1 (checked by the caller of the launch; an
// entry outside gives NaN here, nothing is read with it).  grid ceil(F / fpb), 256 threads, fpb * A <= LSL_TORS_LDS_ATOMS.
__global__ void __launch_bounds__(256) k_pair_dist(float *dist, const float *pos, const int *pairs, long long F, int A, int P, int fpb) {
    __shared__ float atoms[LSL_TORS_LDS_ATOMS * 3];
    long long f0;
    const int nf = stage_frames(atoms, pos, F, A, fpb, &f0);
    const int items = nf * P;  // (<= 2048 * 65536 = 2^27)
    for (int i = threadIdx.x; i < items; i += 256) {
        const int fl = i / P, p = i - fl * P;
        const int a = pairs[p * 2], b = pairs[p * 2 + 1];
        float d = __builtin_nanf("");
        if ((unsigned)a < (unsigned)A && (unsigned)b < (unsigned)A) {
            const float *pa = atoms + (fl * A + a) * 3, *pb = atoms + (fl * A + b) * 3;
            d = ss_dist(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2]);
        }
        dist[(size_t)(f0 + fl) * P + p] = d;
    }
}

// ---- b. per-frame statistics of the selected atoms ----
// rg [F], flags [F], tally [4] +=, contacts [R, R] += (cells i < j), each may be NULL; pos [F, A, 3], sel [R] with entries in 0 .. A - 1
// (checked by the caller of the launch; an entry outside stages NaN, nothing is read with it).  grid ceil(F / tf), 256 threads,
// tf <= LSL_CA_TILE, tf * R <= LSL_CA_LDS_ATOMS, tfs = tf | 1.
__global__ void __launch_bounds__(256) k_ca_stats(float *rg, int *flags, unsigned long long *tally, unsigned long long *contacts, const float *pos,
                                                  const int *sel, long long F, int A, int R, int tf, float clash_thr, float break_thr,
                                                  float contact_thr) {
    __shared__ float at[3 * (LSL_CA_LDS_ATOMS + LSL_CA_MAX_R)];  // (R * tfs <= R * tf + R)
    __shared__ int cnt[4];
    const int tfs = tf | 1;
    const long long f0 = (long long)blockIdx.x * tf;
    const int nf = (int)((F - f0 < tf) ? (F - f0) : tf);
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < nf * R; i += 256) {
        const int fl = i / R, r = i - fl * R, a = sel[r];
        float x = __builtin_nanf(""), y = x, z = x;
        if ((unsigned)a < (unsigned)A) {
            const float *p = pos + ((size_t)(f0 + fl) * A + a) * 3;
            x = p[0], y = p[1], z = p[2];
        }
        at[r * tfs + fl] = x, at[(R + r) * tfs + fl] = y, at[(2 * R + r) * tfs + fl] = z;
    }
    __syncthreads();
    const float *X = at, *Y = at + R * tfs, *Z = at + 2 * R * tfs;
    if ((rg || flags || tally) && (int)threadIdx.x < nf) {  // the frame pass
        const int fl = threadIdx.x;
        if (rg) {
#pragma clang fp contract(off)
            double sx = 0.0, sy = 0.0, sz = 0.0;
            for (int r = 0; r < R; ++r) sx += (double)X[r * tfs + fl], sy += (double)Y[r * tfs + fl], sz += (double)Z[r * tfs + fl];
            const double mx = sx / (double)R, my = sy / (double)R, mz = sz / (double)R;
            double s = 0.0;
            for (int r = 0; r < R; ++r) {
                const double dx = (double)X[r * tfs + fl] - mx, dy = (double)Y[r * tfs + fl] - my, dz = (double)Z[r * tfs + fl] - mz;
                s += (dx * dx + dy * dy) + dz * dz;
            }
            rg[f0 + fl] = (float)sqrt(s / (double)R);
        }
        if (flags || tally) {
            int fb = 0;
            for (int i = 0; i < R - 1; ++i) {
                const float xi = X[i * tfs + fl], yi = Y[i * tfs + fl], zi = Z[i * tfs + fl];
                const float dn = ss_dist(xi, yi, zi, X[(i + 1) * tfs + fl], Y[(i + 1) * tfs + fl], Z[(i + 1) * tfs + fl]);
                if (dn > break_thr) fb |= 2;
                if (dn < clash_thr) fb |= 1;
                if (!(fb & 1))
                    for (int j = i + 2; j < R; ++j)
                        if (ss_dist(xi, yi, zi, X[j * tfs + fl], Y[j * tfs + fl], Z[j * tfs + fl]) < clash_thr) { fb |= 1; break; }
            }
            if (flags) flags[f0 + fl] = fb;
            if (tally) {
                atomicAdd(&cnt[0], 1);
                if (fb & 1) atomicAdd(&cnt[1], 1);
                if (fb & 2) atomicAdd(&cnt[2], 1);
                if (fb == 0) atomicAdd(&cnt[3], 1);
            }
        }
    }
    if (contacts) {  // the pair pass
        for (int c = threadIdx.x; c < R * R; c += 256) {
            const int i = c / R, j = c - i * R;
            if (i >= j) continue;
            const float *xi = X + i * tfs, *yi = Y + i * tfs, *zi = Z + i * tfs, *xj = X + j * tfs, *yj = Y + j * tfs, *zj = Z + j * tfs;
            int k = 0;
            for (int fl = 0; fl < nf; ++fl) k += (ss_dist(xi[fl], yi[fl], zi[fl], xj[fl], yj[fl], zj[fl]) < contact_thr) ? 1 : 0;
            if (k) atomicAdd(&contacts[c], (unsigned long long)k);
        }
    }
    if (tally) {
        __syncthreads();
        if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(&tally[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    }
}

// ---- c. histograms, one edge table per column ----
// counts[q bins + b] += number of rows t of x [n, Q] with x[t, q] in bin b of edges[q (bins + 1) ..]: tors_bin against the column's own
// table.  grid (ceil(n / LSL_HIST_ROWS), ceil(Q / qt)), 256 threads, qt * (bins + 1) <= LSL_HCOL_CELLS.
__global__ void __launch_bounds__(256) k_hist_cols(unsigned long long *counts, const float *x, const double *edges, int n, int Q, int bins, int qt) {
    __shared__ double e[LSL_HCOL_CELLS];
    __shared__ int cnt[LSL_HCOL_CELLS];
    const int q0 = blockIdx.y * qt, nq = (Q - q0 < qt) ? (Q - q0) : qt;
    const int t0 = blockIdx.x * LSL_HIST_ROWS, nt = tile_rows(n, t0, LSL_HIST_ROWS);
    const double *es = edges + (size_t)q0 * (bins + 1);
    for (int i = threadIdx.x; i < nq * (bins + 1); i += 256) e[i] = es[i];
    for (int i = threadIdx.x; i < nq * bins; i += 256) cnt[i] = 0;
    __syncthreads();
    const float *xs = x + (size_t)t0 * Q + q0;
    for (int i = threadIdx.x; i < nt * nq; i += 256) {
        const int t = i / nq, q = i - t * nq;
        const int b = tors_bin((double)xs[(size_t)t * Q + q], e + q * (bins + 1), bins);
        if (b >= 0) atomicAdd(&cnt[q * bins + b], 1);
    }
    __syncthreads();
    flush_counts(counts + (size_t)q0 * bins, cnt, nq * bins);
}

// ---- d. Jensen-Shannon distance of two density histograms ----
// out[r] = jensenshannon(ha, hb), h[i] = (count[i] / measure[r, i]) / N + pseudo with N the row's total count (numpy's density=True, then
// the pseudo-count), then as k_js: both rows over their sums (added in bin order in fp64), m = (p + q) / 2, the terms added in bin order.
// N = 0 on either side (0 / 0) or a zero cell size (x / 0) gives NaN, as the same arithmetic in numpy.  grid rows, 256 threads.
__global__ void __launch_bounds__(256) k_js_density(double *out, const long long *a, const long long *b, const double *measure, int bins, double pseudo) {
    __shared__ long long tot[2][256];
    __shared__ double term[2][256];
    const long long *ra = a + (size_t)blockIdx.x * bins, *rb = b + (size_t)blockIdx.x * bins;
    const double *rm = measure + (size_t)blockIdx.x * bins;
    js_totals(tot, ra, rb, bins);
    const double na = (double)tot[0][0], nb = (double)tot[1][0];
    double first = 0.0, second = 0.0;  // (thread 0's: pass 0 the sums of ha and hb, pass 1 sum rel_entr(p, m) and sum rel_entr(q, m))
    double suma = 0.0, sumb = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            if (threadIdx.x == 0) term[0][0] = first, term[1][0] = second;
            __syncthreads();
            suma = term[0][0], sumb = term[1][0];
            __syncthreads();
            first = second = 0.0;
        }
        for (int i0 = 0; i0 < bins; i0 += 256) {
            const int i = i0 + (int)threadIdx.x;
            if (i < bins) {
                const double ha = (double)ra[i] / rm[i] / na + pseudo, hb = (double)rb[i] / rm[i] / nb + pseudo;
                if (pass == 0) {
                    term[0][threadIdx.x] = ha, term[1][threadIdx.x] = hb;
                } else {
                    const double p = ha / suma, q = hb / sumb, m = (p + q) / 2.0;
                    term[0][threadIdx.x] = tors_rel_entr(p, m), term[1][threadIdx.x] = tors_rel_entr(q, m);
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                const int lim = (bins - i0 < 256) ? (bins - i0) : 256;
                for (int j = 0; j < lim; ++j) first += term[0][j], second += term[1][j];
            }
            __syncthreads();
        }
    }
    const double js = first + second;
    if (threadIdx.x == 0) out[blockIdx.x] = sqrt((js < 0.0 ? 0.0 : js) / 2.0);
}
