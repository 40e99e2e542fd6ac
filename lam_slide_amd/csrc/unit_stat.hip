// The evaluation statistics' translation unit of liblamslide_hip.so (include/lsl_api.h): torsion and structure statistics of a sampled
// peptide trajectory, TICA and Koopman-reweighted TICA, k-means fitting, the reversible Markov state models, and rigid superposition.
#include "../../include/lsl_api.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "k_torsstat.hip.h"
#include "k_structstat.hip.h"
#include "k_tica.hip.h"
#include "k_wtica.hip.h"
#include "k_kmeans.hip.h"
#include "k_msm.hip.h"
#include "k_superpose.hip.h"

#include "host_api.hip.h"

LSL_UNIT_INFO;

extern "C" {

// ---- torsion statistics of a sampled peptide trajectory: dihedrals, histograms, lagged products, JS distance (k_torsstat.hip.h) ----
int lsl_dihedral_angles(const float *pos, const int32_t *quads, const int32_t *quads_host, int64_t F, int32_t A, int32_t Q, float *angles,
                        void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pos || !quads || !quads_host || !angles) return fail(-1, "null argument");
    if (A < 1 || A > LSL_TORS_MAX_A) return fail(-3, "A = %d outside the native form (1..%d atoms of a frame)", A, LSL_TORS_MAX_A);
    if (Q < 1 || Q > LSL_TORS_MAX_Q) return fail(-3, "Q = %d outside 1..%d quadruples", Q, LSL_TORS_MAX_Q);
    const int fpb = LSL_TORS_LDS_ATOMS / A;
    if (F < 1 || (F + fpb - 1) / fpb > 0x7fffffffLL) return fail(-3, "F = %lld frames: 1 .. %lld at A = %d", (long long)F, 0x7fffffffLL * fpb, A);
    for (int i = 0; i < 4 * Q; ++i)
        if (quads_host[i] < 0 || quads_host[i] >= A)
            return fail(-3, "quads[%d][%d] = %d outside the frame's atoms 0..%d", i / 4, i % 4, quads_host[i], A - 1);
    hipLaunchKernelGGL(k_dihedral, dim3((unsigned)((F + fpb - 1) / fpb)), dim3(256), 0, (hipStream_t)stream, angles, pos, (const int *)quads,
                       (long long)F, (int)A, (int)Q, fpb);
    LSL_CHECK_LAUNCH("lsl_dihedral_angles");
    return 0;
} LSL_API_CATCH

int lsl_histogram(const float *x, int32_t S, int32_t n, int32_t Q, const double *edges, int32_t bins, int64_t *counts, const int32_t *pairs,
                  const int32_t *pairs_host, int32_t P, const double *edges2a, const double *edges2b, int32_t bins2, int64_t *counts2,
                  void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !edges || !counts) return fail(-1, "null argument");
    if (S < 1 || S > 65535) return fail(-3, "S = %d outside 1..65535 series", S);
    if (n < 1 || Q < 1) return fail(-3, "n = %d and Q = %d must be positive", n, Q);
    if (bins < 1 || bins > LSL_HIST_MAX_BINS) return fail(-3, "bins = %d outside 1..%d", bins, LSL_HIST_MAX_BINS);
    const int qt = std::min<int>(Q, LSL_HIST_CELLS / bins);
    if ((Q + qt - 1) / qt > 65535) return fail(-3, "Q = %d columns of %d bins: at most %d", Q, bins, 65535 * qt);
    if (P < 0 || P > 65535) return fail(-3, "P = %d outside 0..65535 pairs", P);
    if (P > 0) {
        if (!pairs || !pairs_host || !edges2a || !edges2b || !counts2) return fail(-1, "null argument (P > 0 needs pairs, their host copy, both edge tables and counts2)");
        if (bins2 < 1 || bins2 > LSL_HIST2_MAX_BINS) return fail(-3, "bins2 = %d outside 1..%d", bins2, LSL_HIST2_MAX_BINS);
        for (int i = 0; i < 2 * P; ++i)
            if (pairs_host[i] < 0 || pairs_host[i] >= Q) return fail(-3, "pairs[%d][%d] = %d outside the columns 0..%d", i / 2, i % 2, pairs_host[i], Q - 1);
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned tb = (unsigned)(((long long)n + LSL_HIST_ROWS - 1) / LSL_HIST_ROWS);
    hipLaunchKernelGGL(k_hist1, dim3(tb, (unsigned)((Q + qt - 1) / qt), (unsigned)S), dim3(256), 0, st, (unsigned long long *)counts, x, edges, (int)n,
                       (int)Q, (int)bins, qt);
    LSL_CHECK_LAUNCH("lsl_histogram");
    if (P > 0) {
        hipLaunchKernelGGL(k_hist2, dim3(tb, (unsigned)P, (unsigned)S), dim3(256), 0, st, (unsigned long long *)counts2, x, (const int *)pairs, edges2a,
                           edges2b, (int)n, (int)Q, (int)P, (int)bins2);
        LSL_CHECK_LAUNCH("lsl_histogram (pairs)");
    }
    return 0;
} LSL_API_CATCH

static const char *lag_shape_error(int32_t S, int32_t n, int32_t C, int32_t nlag) {
    if (S < 1 || C < 1 || (long long)S * C > LSL_LAG_MAX_ROWS) return "S and C must be positive and S * C at most 65535 (series x channels of one call)";
    if (n < 1) return "n must be positive";
    if (nlag < 0 || nlag >= n) return "nlag outside 0..n-1 (lag k has n - k terms)";
    if ((long long)nlag + 1 > LSL_LAG_MAX_PART) return "nlag + 1 above 2^21 lags";
    return nullptr;
}

size_t lsl_lag_products_workspace_bytes(int32_t S, int32_t n, int32_t C, int32_t nlag) {
    if (lag_shape_error(S, n, C, nlag)) return 0;
    return (size_t)S * C * lag_segments(n, nlag).nseg * ((size_t)nlag + 1) * sizeof(double);
}

int lsl_lag_products(const float *x, int32_t S, int32_t n, int32_t C, int32_t nlag, float *ac, void *workspace, size_t workspace_bytes,
                     void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !ac || !workspace) return fail(-1, "null argument");
    if (const char *why = lag_shape_error(S, n, C, nlag)) return fail(-3, "S = %d, n = %d, C = %d, nlag = %d: %s", S, n, C, nlag, why);
    const size_t need = lsl_lag_products_workspace_bytes(S, n, C, nlag);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    const LagSplit sp = lag_segments(n, nlag);
    hipStream_t st = (hipStream_t)stream;
    const unsigned tiles = (unsigned)((nlag + LSL_LAG_TILE) / LSL_LAG_TILE);  // ceil((nlag + 1) / tile)
    hipLaunchKernelGGL(k_lag_partial, dim3(tiles, (unsigned)sp.nseg, (unsigned)(S * C)), dim3(LSL_LAG_TILE), 0, st, (double *)workspace, x, (int)n, (int)C,
                       (int)nlag, sp.cps);
    LSL_CHECK_LAUNCH("lsl_lag_products");
    hipLaunchKernelGGL(k_lag_final, dim3((unsigned)((nlag + 256) / 256), (unsigned)(S * C)), dim3(256), 0, st, ac, (const double *)workspace, (int)n,
                       (int)nlag, sp.nseg);
    LSL_CHECK_LAUNCH("lsl_lag_products (final)");
    return 0;
} LSL_API_CATCH

int lsl_js_distance(const int64_t *counts_a, const int64_t *counts_b, int32_t rows, int32_t bins, double *out, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts_a || !counts_b || !out) return fail(-1, "null argument");
    if (rows < 1 || bins < 1) return fail(-3, "rows = %d and bins = %d must be positive", rows, bins);
    hipLaunchKernelGGL(k_js, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, out, (const long long *)counts_a, (const long long *)counts_b, (int)bins);
    LSL_CHECK_LAUNCH("lsl_js_distance");
    return 0;
} LSL_API_CATCH

// ---- structure statistics of a sampled peptide trajectory: pair distances, per-frame statistics, column histograms, density JS (k_structstat.hip.h) ----
int lsl_pair_distances(const float *pos, const int32_t *pairs, const int32_t *pairs_host, int64_t F, int32_t A, int32_t P, float *dist,
                       void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pos || !pairs || !pairs_host || !dist) return fail(-1, "null argument");
    if (A < 1 || A > LSL_TORS_MAX_A) return fail(-3, "A = %d outside the native form (1..%d atoms of a frame)", A, LSL_TORS_MAX_A);
    if (P < 1 || P > LSL_PAIR_MAX_P) return fail(-3, "P = %d outside 1..%d pairs", P, LSL_PAIR_MAX_P);
    const int fpb = LSL_TORS_LDS_ATOMS / A;
    if (F < 1 || (F + fpb - 1) / fpb > 0x7fffffffLL) return fail(-3, "F = %lld frames: 1 .. %lld at A = %d", (long long)F, 0x7fffffffLL * fpb, A);
    for (int i = 0; i < 2 * P; ++i)
        if (pairs_host[i] < 0 || pairs_host[i] >= A)
            return fail(-3, "pairs[%d][%d] = %d outside the frame's atoms 0..%d", i / 2, i % 2, pairs_host[i], A - 1);
    hipLaunchKernelGGL(k_pair_dist, dim3((unsigned)((F + fpb - 1) / fpb)), dim3(256), 0, (hipStream_t)stream, dist, pos, (const int *)pairs,
                       (long long)F, (int)A, (int)P, fpb);
    LSL_CHECK_LAUNCH("lsl_pair_distances");
    return 0;
} LSL_API_CATCH

int lsl_ca_frame_stats(const float *pos, const int32_t *sel, const int32_t *sel_host, int64_t F, int32_t A, int32_t R, float clash_thr,
                       float break_thr, float contact_thr, float *rg, int32_t *flags, int64_t *tally, int64_t *contacts, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pos || !sel || !sel_host) return fail(-1, "null argument");
    if (A < 1) return fail(-3, "A = %d must be positive", A);
    if (R < 1 || R > LSL_CA_MAX_R) return fail(-3, "R = %d outside 1..%d selected atoms", R, LSL_CA_MAX_R);
    const int tf = std::min<int>(LSL_CA_TILE, LSL_CA_LDS_ATOMS / R);
    if (F < 1 || (F + tf - 1) / tf > 0x7fffffffLL) return fail(-3, "F = %lld frames: 1 .. %lld at R = %d", (long long)F, 0x7fffffffLL * tf, R);
    for (int i = 0; i < R; ++i)
        if (sel_host[i] < 0 || sel_host[i] >= A) return fail(-3, "sel[%d] = %d outside the frame's atoms 0..%d", i, sel_host[i], A - 1);
    if (!rg && !flags && !tally && !contacts) return 0;  // (nothing asked for)
    hipLaunchKernelGGL(k_ca_stats, dim3((unsigned)((F + tf - 1) / tf)), dim3(256), 0, (hipStream_t)stream, rg, (int *)flags, (unsigned long long *)tally,
                       (unsigned long long *)contacts, pos, (const int *)sel, (long long)F, (int)A, (int)R, tf, clash_thr, break_thr, contact_thr);
    LSL_CHECK_LAUNCH("lsl_ca_frame_stats");
    return 0;
} LSL_API_CATCH

int lsl_histogram_columns(const float *x, int32_t n, int32_t Q, const double *edges, int32_t bins, int64_t *counts, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !edges || !counts) return fail(-1, "null argument");
    if (n < 1 || Q < 1) return fail(-3, "n = %d and Q = %d must be positive", n, Q);
    if (bins < 1 || bins > LSL_HIST_MAX_BINS) return fail(-3, "bins = %d outside 1..%d", bins, LSL_HIST_MAX_BINS);
    const int qt = std::min<int>(Q, LSL_HCOL_CELLS / (bins + 1));
    if ((Q + qt - 1) / qt > 65535) return fail(-3, "Q = %d columns of %d bins: at most %d", Q, bins, 65535 * qt);
    const unsigned tb = (unsigned)(((long long)n + LSL_HIST_ROWS - 1) / LSL_HIST_ROWS);
    hipLaunchKernelGGL(k_hist_cols, dim3(tb, (unsigned)((Q + qt - 1) / qt)), dim3(256), 0, (hipStream_t)stream, (unsigned long long *)counts, x, edges,
                       (int)n, (int)Q, (int)bins, qt);
    LSL_CHECK_LAUNCH("lsl_histogram_columns");
    return 0;
} LSL_API_CATCH

int lsl_js_distance_density(const int64_t *counts_a, const int64_t *counts_b, const double *measure, int32_t rows, int32_t bins, double pseudo,
                            double *out, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts_a || !counts_b || !measure || !out) return fail(-1, "null argument");
    if (rows < 1 || bins < 1) return fail(-3, "rows = %d and bins = %d must be positive", rows, bins);
    hipLaunchKernelGGL(k_js_density, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, out, (const long long *)counts_a,
                       (const long long *)counts_b, measure, (int)bins, pseudo);
    LSL_CHECK_LAUNCH("lsl_js_distance_density");
    return 0;
} LSL_API_CATCH

// ---- TICA and state statistics of the peptide evaluation: lagged second moments, projection, nearest centre, transition counts (k_tica.hip.h) ----
static const char *moments_shape_error(int32_t S, int32_t n, int32_t F, int32_t lag) {
    if (S < 1 || S > 65535) return "S outside 1..65535 series";
    if (F < 1 || F > LSL_MOM_MAX_F) return "F outside the native form (1..128 features)";
    if (n < 2) return "n must be at least 2";
    if (lag < 1 || lag >= n) return "lag outside 1..n-1 (the window has n - lag rows)";
    return nullptr;
}

size_t lsl_lagged_moments_workspace_bytes(int32_t S, int32_t n, int32_t F, int32_t lag) {
    if (moments_shape_error(S, n, F, lag)) return 0;
    return (size_t)S * mom_segments(n, lag) * mom_entries(F) * sizeof(double);
}

int lsl_lagged_moments(const float *x, int32_t S, int32_t n, int32_t F, int32_t lag, double *moments, void *workspace, size_t workspace_bytes,
                       void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !moments || !workspace) return fail(-1, "null argument");
    if (const char *why = moments_shape_error(S, n, F, lag)) return fail(-3, "S = %d, n = %d, F = %d, lag = %d: %s", S, n, F, lag, why);
    const size_t need = lsl_lagged_moments_workspace_bytes(S, n, F, lag);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int nseg = mom_segments(n, lag), T = mom_block(F), nb = (F + T - 1) / T;
    const dim3 grid((unsigned)nseg, (unsigned)((nb * nb + 255) / 256), (unsigned)S);
    if (T == 2)
        hipLaunchKernelGGL(k_moments_partial<2>, grid, dim3(256), 0, st, (double *)workspace, x, (int)n, (int)F, (int)lag);
    else
        hipLaunchKernelGGL(k_moments_partial<4>, grid, dim3(256), 0, st, (double *)workspace, x, (int)n, (int)F, (int)lag);
    LSL_CHECK_LAUNCH("lsl_lagged_moments");
    const long long E = (long long)mom_entries(F);
    hipLaunchKernelGGL(k_moments_final, dim3((unsigned)((E + 255) / 256), (unsigned)S), dim3(256), 0, st, moments, (const double *)workspace, E, nseg);
    LSL_CHECK_LAUNCH("lsl_lagged_moments (final)");
    return 0;
} LSL_API_CATCH

// The bracket of a projection with running limits, lsl_project's (k_project) and lsl_project_wide's (`wide`: k_project_wide): lim's floats
// to keys, the projection, the keys back to floats.  `block`: the threads of the two one-workgroup launches, each entry's own.
static int project_with_limits(const char *entry, bool wide, unsigned block, const float *x, int n, int F, const double *mean, const double *W, int d,
                               float *y, float *lim, hipStream_t st) {
    if (lim) {
        hipLaunchKernelGGL(k_lim_keys, dim3(1), dim3(block), 0, st, lim, 2 * d);
        if (hipError_t e = hipGetLastError()) return fail(-10, "%s (limits to keys): %s", entry, hipGetErrorString(e));
    }
    if (wide)
        hipLaunchKernelGGL(k_project_wide<false>, dim3((unsigned)(((long long)n + LSL_WPROJ_ROWS - 1) / LSL_WPROJ_ROWS)), dim3(256), 0, st, y, (double *)nullptr,
                           x, mean, W, 0.0, (unsigned *)lim, n, F, d);
    else
        hipLaunchKernelGGL(k_project, dim3((unsigned)(((long long)n + LSL_PROJ_ROWS - 1) / LSL_PROJ_ROWS)), dim3(256), 0, st, y, x, mean, W, (unsigned *)lim, n, F, d);
    LSL_CHECK_LAUNCH(entry);
    if (lim) {
        hipLaunchKernelGGL(k_lim_floats, dim3(1), dim3(block), 0, st, lim, 2 * d);
        if (hipError_t e = hipGetLastError()) return fail(-10, "%s (keys to limits): %s", entry, hipGetErrorString(e));
    }
    return 0;
}

int lsl_project(const float *x, int32_t n, int32_t F, const double *mean, const double *W, int32_t d, float *y, float *lim, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !mean || !W || !y) return fail(-1, "null argument");
    if (n < 1) return fail(-3, "n = %d must be positive", n);
    if (F < 1 || F > LSL_MOM_MAX_F) return fail(-3, "F = %d outside the native form (1..%d features)", F, LSL_MOM_MAX_F);
    if (d < 1 || d > LSL_PROJ_MAX_D) return fail(-3, "d = %d outside the native form (1..%d output columns)", d, LSL_PROJ_MAX_D);
    return project_with_limits("lsl_project", false, 64, x, (int)n, (int)F, mean, W, (int)d, y, lim, (hipStream_t)stream);
} LSL_API_CATCH

// The centres clause of lsl_assign_centers and of the k-means entry points - k centres of d coordinates stay in LDS: 0, or the argument
// outside the native form ('d', then 'k').
static char centres_outside(int32_t d, int32_t k) {
    if (d < 1 || d > LSL_ASG_MAX_D) return 'd';
    if (k < 1 || k > LSL_ASG_MAX_K || (long long)k * d > LSL_ASG_CELLS) return 'k';
    return 0;
}

int lsl_assign_centers(const float *y, int32_t n, int32_t d, const float *centers, int32_t k, const int32_t *map, int32_t nstates, int32_t *labels,
                       int64_t *state_counts, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!y || !centers || !labels) return fail(-1, "null argument");
    if (n < 1) return fail(-3, "n = %d must be positive", n);
    const char outside = centres_outside(d, k);
    if (outside == 'd') return fail(-3, "d = %d outside the native form (1..%d coordinates)", d, LSL_ASG_MAX_D);
    if (outside == 'k')
        return fail(-3, "k = %d centres of d = %d outside the native form (1..%d centres, k * d <= %d: the centres stay in LDS)", k, d, LSL_ASG_MAX_K, LSL_ASG_CELLS);
    if ((map || state_counts) && (nstates < 1 || nstates > LSL_ASG_MAX_STATES))
        return fail(-3, "nstates = %d outside 1..%d (a map or a count table needs the number of states)", nstates, LSL_ASG_MAX_STATES);
    const int ra = std::min<int>(256, LSL_ASG_TILE / d);
    hipLaunchKernelGGL(k_assign, dim3((unsigned)(((long long)n + ra - 1) / ra)), dim3(256), 0, (hipStream_t)stream, (int *)labels,
                       (unsigned long long *)state_counts, y, centers, (const int *)map, (int)n, (int)d, (int)k, (int)nstates, ra);
    LSL_CHECK_LAUNCH("lsl_assign_centers");
    return 0;
} LSL_API_CATCH

int lsl_transition_counts(const int32_t *dtraj, int32_t S, int32_t n, int32_t lag, int32_t nstates, int64_t *counts, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!dtraj || !counts) return fail(-1, "null argument");
    if (S < 1 || S > 65535) return fail(-3, "S = %d outside 1..65535 series", S);
    if (n < 1) return fail(-3, "n = %d must be positive", n);
    if (lag < 1) return fail(-3, "lag = %d must be positive", lag);
    if (nstates < 1 || nstates > LSL_TR_MAX_STATES)
        return fail(-3, "nstates = %d outside the native form (1..%d: the counts of a workgroup stay in LDS)", nstates, LSL_TR_MAX_STATES);
    if (lag >= n) return 0;  // (no pair: nothing to add)
    const unsigned tb = (unsigned)(((long long)n - lag + LSL_TR_ROWS - 1) / LSL_TR_ROWS);
    hipLaunchKernelGGL(k_transitions, dim3(tb, (unsigned)S), dim3(256), 0, (hipStream_t)stream, (unsigned long long *)counts, (const int *)dtraj, (int)n,
                       (int)lag, (int)nstates);
    LSL_CHECK_LAUNCH("lsl_transition_counts");
    return 0;
} LSL_API_CATCH

// ---- Koopman-reweighted TICA on wide feature tables: weighted lagged moments, affine weights, the wide projection (k_wtica.hip.h) ----
static const char *wmom_shape_error(int32_t n, int32_t F, int32_t lag) {
    if (F < LSL_WMOM_MIN_F || F > LSL_WMOM_MAX_F) return "F outside the native form (129..2048 features; 1..128 are lsl_lagged_moments')";
    if (n < 2) return "n must be at least 2";
    if (lag < 1 || lag >= n) return "lag outside 1..n-1 (the window has n - lag rows)";
    return nullptr;
}

size_t lsl_weighted_moments_workspace_bytes(int32_t n, int32_t F, int32_t lag) {
    if (wmom_shape_error(n, F, lag)) return 0;
    return (size_t)wmom_plan(n, F, lag).nsplit * wmom_part_entries(F) * sizeof(double);
}

int lsl_weighted_moments(const float *x, int32_t n, int32_t F, int32_t lag, const double *w, double *moments, void *workspace, size_t workspace_bytes,
                         void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !moments || !workspace) return fail(-1, "null argument");
    if (const char *why = wmom_shape_error(n, F, lag)) return fail(-3, "n = %d, F = %d, lag = %d: %s", n, F, lag, why);
    const size_t need = lsl_weighted_moments_workspace_bytes(n, F, lag);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const WmomPlan p = wmom_plan(n, F, lag);
    hipLaunchKernelGGL(k_wmom_tiles, dim3((unsigned)p.jobs, (unsigned)p.nsplit), dim3(256), 0, st, (double *)workspace, x, w, (int)n, (int)F, (int)lag,
                       p.Te, p.T, p.q);
    LSL_CHECK_LAUNCH("lsl_weighted_moments");
    const long long E = 1 + 2LL * F + 3LL * F * F;
    hipLaunchKernelGGL(k_wmom_final, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, moments, (const double *)workspace, (int)F, p.nsplit);
    LSL_CHECK_LAUNCH("lsl_weighted_moments (final)");
    return 0;
} LSL_API_CATCH

int lsl_affine_weights(const float *x, int32_t m, int32_t F, const double *u, double c, double *w, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !u || !w) return fail(-1, "null argument");
    if (m < 1) return fail(-3, "m = %d must be positive", m);
    if (F < 1 || F > LSL_WMOM_MAX_F) return fail(-3, "F = %d outside the native form (1..%d features)", F, LSL_WMOM_MAX_F);
    hipLaunchKernelGGL(k_project_wide<true>, dim3((unsigned)(((long long)m + LSL_WPROJ_ROWS - 1) / LSL_WPROJ_ROWS)), dim3(256), 0, (hipStream_t)stream,
                       (float *)nullptr, w, x, (const double *)nullptr, u, c, (unsigned *)nullptr, (int)m, (int)F, 1);
    LSL_CHECK_LAUNCH("lsl_affine_weights");
    return 0;
} LSL_API_CATCH

int lsl_project_wide(const float *x, int32_t n, int32_t F, const double *mean, const double *W, int32_t d, float *y, float *lim, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!x || !mean || !W || !y) return fail(-1, "null argument");
    if (n < 1) return fail(-3, "n = %d must be positive", n);
    if (F < LSL_WMOM_MIN_F || F > LSL_WMOM_MAX_F)
        return fail(-3, "F = %d outside the native form (%d..%d features; 1..128 are lsl_project's)", F, LSL_WMOM_MIN_F, LSL_WMOM_MAX_F);
    if (d < 1 || d > LSL_WPROJ_MAX_D) return fail(-3, "d = %d outside the native form (1..%d output columns)", d, LSL_WPROJ_MAX_D);
    return project_with_limits("lsl_project_wide", true, 128, x, (int)n, (int)F, mean, W, (int)d, y, lim, (hipStream_t)stream);
} LSL_API_CATCH

// ---- k-means fitting: one Lloyd step of S independent problems, the reverse lookup of post_process (k_kmeans.hip.h) ----
static const char *kmeans_shape_error(int32_t S, int32_t n, int32_t d, int32_t k) {
    if (S < 1 || S > LSL_KM_MAX_S) return "S outside 1..65535 series";
    if (n < 1) return "n must be positive";
    const char outside = centres_outside(d, k);
    if (outside == 'd') return "d outside the native form (1..64 coordinates)";
    if (outside == 'k') return "k outside the native form (1..1024 centres, k * d <= 8192: the centres stay in LDS)";
    return nullptr;
}

size_t lsl_kmeans_workspace_bytes(int32_t S, int32_t n, int32_t d, int32_t k) {
    if (kmeans_shape_error(S, n, d, k)) return 0;
    const size_t units = (size_t)S * km_segments(n);
    return units * ((size_t)k * d + 1) * sizeof(double) + units * ((size_t)k + 1) * sizeof(int32_t);
}

int lsl_kmeans_step(const float *y, int32_t S, int32_t n, int32_t d, float *centers, int32_t k, int32_t *labels, int64_t *counts, double *state,
                    int32_t *done, int32_t update, double rel_tol, double center_tol, void *workspace, size_t workspace_bytes, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!y || !centers || !labels || !counts || !state || !done || !workspace) return fail(-1, "null argument");
    if (const char *why = kmeans_shape_error(S, n, d, k)) return fail(-3, "S = %d, n = %d, d = %d, k = %d: %s", S, n, d, k, why);
    if (!(rel_tol >= 0.0) || !(center_tol >= 0.0)) return fail(-3, "rel_tol = %g and center_tol = %g must not be negative (0 switches a rule off)", rel_tol, center_tol);
    const size_t need = lsl_kmeans_workspace_bytes(S, n, d, k);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int nseg = km_segments(n), G = km_group(n, d, k), per = 256 / G;
    const size_t units = (size_t)S * nseg;
    double *wsum = (double *)workspace, *winert = wsum + units * k * d;
    int *wcnt = (int *)(winert + units), *wchg = wcnt + units * k;
    const dim3 grid = (G == 256) ? dim3((unsigned)nseg, (unsigned)S) : dim3((unsigned)((S + per - 1) / per));
    const int q = (k * d + G - 1) / G;  // items (c, j) per thread, at most LSL_KM_MAX_Q: the next power of two is compiled
#define LSL_KM_LAUNCH(NQ) launch_kmeans_step<NQ>(grid, st, y, centers, (int *)labels, (const int *)done, wsum, winert, wcnt, wchg, (int)S, (int)n, (int)d, (int)k, nseg, G, (int)update)
    if (q <= 1) LSL_KM_LAUNCH(1);
    else if (q <= 2) LSL_KM_LAUNCH(2);
    else if (q <= 4) LSL_KM_LAUNCH(4);
    else if (q <= 8) LSL_KM_LAUNCH(8);
    else if (q <= 16) LSL_KM_LAUNCH(16);
    else LSL_KM_LAUNCH(32);
#undef LSL_KM_LAUNCH
    LSL_CHECK_LAUNCH("lsl_kmeans_step");
    hipLaunchKernelGGL(k_kmeans_final, dim3((unsigned)S), dim3(256), 0, st, centers, (long long *)counts, state, (int *)done, (const double *)wsum,
                       (const double *)winert, (const int *)wcnt, (const int *)wchg, (int)d, (int)k, nseg, (int)update, rel_tol, center_tol);
    LSL_CHECK_LAUNCH("lsl_kmeans_step (final)");
    return 0;
} LSL_API_CATCH

int lsl_kmeans_nearest_rows(const float *y, int32_t S, int32_t n, int32_t d, const float *centers, int32_t k, int32_t *rows, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!y || !centers || !rows) return fail(-1, "null argument");
    if (const char *why = kmeans_shape_error(S, n, d, k)) return fail(-3, "S = %d, n = %d, d = %d, k = %d: %s", S, n, d, k, why);
    const int P = n <= 64 ? 1 : 64;
    const long long items = (long long)S * k;
    if ((items * P + 255) / 256 > 2147483647LL) return fail(-3, "S = %d series of k = %d centres: more than 2^31 - 1 workgroups; split the batch", S, k);
    hipLaunchKernelGGL(k_nearest_rows, dim3((unsigned)((items * P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int *)rows, y, centers, items, (int)n,
                       (int)d, (int)k, P);
    LSL_CHECK_LAUNCH("lsl_kmeans_nearest_rows");
    return 0;
} LSL_API_CATCH

// ---- reversible maximum-likelihood Markov state models: active set, the row-sum iteration, the embedded transition matrix (k_msm.hip.h) ----
static const char *msm_shape_error(int32_t S, int32_t ns) {
    if (S < 1 || S > LSL_MSM_MAX_S) return "S outside 1..65535 series";
    if (ns < 1 || ns > LSL_MSM_MAX_STATES) return "ns outside the native form (1..128 states: fp64 K of a series stays in LDS)";
    return nullptr;
}

int lsl_msm_active_set(const int64_t *counts, int32_t S, int32_t ns, int32_t *active, int32_t *n_active, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts || !active || !n_active) return fail(-1, "null argument");
    if (const char *why = msm_shape_error(S, ns)) return fail(-3, "S = %d, ns = %d: %s", S, ns, why);
    hipLaunchKernelGGL(k_msm_active, dim3((unsigned)S), dim3(128), 0, (hipStream_t)stream, (const long long *)counts, (int)ns, (int *)active, (int *)n_active);
    LSL_CHECK_LAUNCH("lsl_msm_active_set");
    return 0;
} LSL_API_CATCH

int lsl_msm_reversible_step(const int64_t *counts, const int32_t *active, int32_t S, int32_t ns, int32_t iters, int32_t maxiter, double maxerr,
                            int32_t restart, double *x, int32_t *n_iter, double *err, int32_t *done, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts || !active || !x || !n_iter || !err || !done) return fail(-1, "null argument");
    if (const char *why = msm_shape_error(S, ns)) return fail(-3, "S = %d, ns = %d: %s", S, ns, why);
    if (iters < 0 || maxiter < 0) return fail(-3, "iters = %d and maxiter = %d must not be negative", iters, maxiter);
    if (maxerr != maxerr) return fail(-3, "maxerr is NaN (a negative maxerr never stops early)");
    hipStream_t st = (hipStream_t)stream;
#define LSL_MSM_LAUNCH(NSP) hipLaunchKernelGGL(k_msm_step<NSP>, dim3((unsigned)S), dim3(LSL_MSM_PARTS * NSP), 0, st, (const long long *)counts, (const int *)active, (int)ns, (int)iters, (int)maxiter, maxerr, (int)restart, x, (int *)n_iter, err, (int *)done)
    const int pad = msm_pad(ns);
    if (pad == 32) LSL_MSM_LAUNCH(32);
    else if (pad == 64) LSL_MSM_LAUNCH(64);
    else LSL_MSM_LAUNCH(128);
#undef LSL_MSM_LAUNCH
    LSL_CHECK_LAUNCH("lsl_msm_reversible_step");
    return 0;
} LSL_API_CATCH

int lsl_msm_transition_matrix(const int64_t *counts, const int32_t *active, const double *x, int32_t S, int32_t ns, double *T, double *pi, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!counts || !active || !x || !T || !pi) return fail(-1, "null argument");
    if (const char *why = msm_shape_error(S, ns)) return fail(-3, "S = %d, ns = %d: %s", S, ns, why);
    hipStream_t st = (hipStream_t)stream;
#define LSL_MSM_LAUNCH(NSP) hipLaunchKernelGGL(k_msm_tmatrix<NSP>, dim3((unsigned)S), dim3(256), 0, st, (const long long *)counts, (const int *)active, x, (int)ns, T, pi)
    const int pad = msm_pad(ns);
    if (pad == 32) LSL_MSM_LAUNCH(32);
    else if (pad == 64) LSL_MSM_LAUNCH(64);
    else LSL_MSM_LAUNCH(128);
#undef LSL_MSM_LAUNCH
    LSL_CHECK_LAUNCH("lsl_msm_transition_matrix");
    return 0;
} LSL_API_CATCH

// ---- rigid superposition of a sampled trajectory: Kabsch fit, RMSD, per-atom mean and RMSF (k_superpose.hip.h) ----
int lsl_superpose(const float *pos, const float *ref, int32_t ref_frames, const int32_t *sel, const int32_t *sel_host, int32_t n_sel,
                  const uint8_t *fixed, int64_t F, int32_t A, int32_t flags, float *out, float *rmsd, double *rot, double *trans, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    const bool center_only = (flags & LSL_SUP_CENTER_ONLY) != 0;
    if (!pos || (!ref && !center_only) || (sel == nullptr) != (sel_host == nullptr))
        return fail(-1, "null argument (a fit needs ref; sel and its host copy come together)");
    if (flags & ~LSL_SUP_CENTER_ONLY) return fail(-3, "flags = %d: only LSL_SUP_CENTER_ONLY (%d) is defined", flags, LSL_SUP_CENTER_ONLY);
    if (A < 1 || A > LSL_TORS_MAX_A) return fail(-3, "A = %d outside the native form (1..%d atoms of a frame)", A, LSL_TORS_MAX_A);
    const int fpb = LSL_TORS_LDS_ATOMS / A;
    if (F < 1 || (F + fpb - 1) / fpb > 0x7fffffffLL) return fail(-3, "F = %lld frames: 1 .. %lld at A = %d", (long long)F, 0x7fffffffLL * fpb, A);
    if (sel ? (n_sel < 1 || n_sel > LSL_TORS_MAX_A) : n_sel != A)
        return fail(-3, "n_sel = %d outside 1..%d selected atoms (without a table: all A = %d atoms)", n_sel, LSL_TORS_MAX_A, A);
    for (int i = 0; sel && i < n_sel; ++i)
        if (sel_host[i] < 0 || sel_host[i] >= A) return fail(-3, "sel[%d] = %d outside the frame's atoms 0..%d", i, sel_host[i], A - 1);
    if (center_only && rmsd) return fail(-3, "rmsd with LSL_SUP_CENTER_ONLY: there is no reference to measure against");
    if (!center_only) {
        if (ref_frames != 1 && (int64_t)ref_frames != F) return fail(-3, "ref_frames = %d: one shared reference frame (1) or one per frame (F = %lld)", ref_frames, (long long)F);
        const size_t frame_bytes = (size_t)A * 3 * sizeof(float);
        const char *ob = (const char *)out, *rb = (const char *)ref;
        if (out && ob < rb + (size_t)ref_frames * frame_bytes && rb < ob + (size_t)F * frame_bytes)
            return fail(-3, "out overlaps ref: the reference is read while the frames are written (copy the reference first)");
    }
    if (!out && !rmsd && !rot && !trans) return 0;  // (nothing asked for)
    hipLaunchKernelGGL(k_superpose, dim3((unsigned)((F + fpb - 1) / fpb)), dim3(256), 0, (hipStream_t)stream, out, rmsd, rot, trans, pos, ref,
                       (const int *)sel, (const unsigned char *)fixed, (long long)F, (int)A, (int)n_sel, fpb, (int)(!center_only && ref_frames != 1),
                       (int)center_only);
    LSL_CHECK_LAUNCH("lsl_superpose");
    return 0;
} LSL_API_CATCH

static const char *rmsf_shape_error(int64_t F, int32_t A) {
    if (A < 1) return "A must be positive";
    if (F < 1 || (F + LSL_RMSF_SEG - 1) / LSL_RMSF_SEG > 65535) return "F outside 1..8388480 frames (65535 segments)";
    return nullptr;
}

size_t lsl_atom_rmsf_workspace_bytes(int64_t F, int32_t A) {
    if (rmsf_shape_error(F, A)) return 0;
    return 2 * (size_t)((F + LSL_RMSF_SEG - 1) / LSL_RMSF_SEG) * 3 * (size_t)A * sizeof(double);
}

int lsl_atom_rmsf(const float *pos, int64_t F, int32_t A, double *mean_out, float *rmsf_out, void *workspace, size_t workspace_bytes,
                  void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pos || !workspace) return fail(-1, "null argument");
    if (const char *why = rmsf_shape_error(F, A)) return fail(-3, "F = %lld, A = %d: %s", (long long)F, A, why);
    const size_t need = lsl_atom_rmsf_workspace_bytes(F, A);
    if (workspace_bytes < need) return fail(-4, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    if (!mean_out && !rmsf_out) return 0;  // (nothing asked for)
    hipStream_t st = (hipStream_t)stream;
    const int nseg = (int)((F + LSL_RMSF_SEG - 1) / LSL_RMSF_SEG);
    const long long C = 3LL * A;
    double *first = (double *)workspace, *second = first + (size_t)nseg * C;
    const dim3 grid((unsigned)((C + 63) / 64), (unsigned)nseg);
    hipLaunchKernelGGL(k_atom_mean_partial<false>, grid, dim3(64), 0, st, first, (const double *)nullptr, pos, (long long)F, C, nseg);
    LSL_CHECK_LAUNCH("lsl_atom_rmsf");
    if (rmsf_out) {
        hipLaunchKernelGGL(k_atom_mean_partial<true>, grid, dim3(64), 0, st, second, (const double *)first, pos, (long long)F, C, nseg);
        LSL_CHECK_LAUNCH("lsl_atom_rmsf (second pass)");
    }
    hipLaunchKernelGGL(k_atom_rmsf_final, dim3((unsigned)(((long long)A + 255) / 256)), dim3(256), 0, st, mean_out, rmsf_out, (const double *)first,
                       (const double *)second, (long long)F, (int)A, nseg);
    LSL_CHECK_LAUNCH("lsl_atom_rmsf (final)");
    return 0;
} LSL_API_CATCH

}  // extern "C"
