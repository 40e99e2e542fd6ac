// The fragments the statistics kernels share (k_torsstat / k_structstat / k_tica / k_wtica / k_kmeans .hip.h): each piece of arithmetic that
// two of them must do alike is written here once, and a contract between two entry points - kmeans_fit's labels are assign_centers', a narrow
// and a wide model project alike, every histogram flushes its counts alike - holds because both sides call the same function.  Every
// fragment is inlined into a workgroup of 256 threads; none changes a kernel's grid, LDS layout or summation order.
#pragma once
#include "common.hip.h"

// ---- windows and counts ----
// The rows of the tile that starts at row `first` of `total`, in tiles of `per`: per, but for the last tile.
__device__ __forceinline__ int tile_rows(long long total, long long first, int per) { return (int)((total - first < per) ? (total - first) : per); }

// out[i] += cnt[i] over the cells of a workgroup's int32 LDS counts: one int64 integer atomic per non-zero cell (no order: exact).
__device__ __forceinline__ void flush_counts(unsigned long long *out, const int *cnt, int cells) {
    for (int i = threadIdx.x; i < cells; i += 256)
        if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
}

// ---- frames in LDS ----
// The workgroup's fpb consecutive frames of pos [F, A, 3] copied to `atoms` in one coalesced pass (fpb * A atoms fit it); *f0 the first
// frame, the return value the frames below F.  Ends with a barrier.
__device__ __forceinline__ int stage_frames(float *atoms, const float *pos, long long F, int A, int fpb, long long *f0) {
    *f0 = (long long)blockIdx.x * fpb;
    const int nf = tile_rows(F, *f0, fpb), n_float = nf * A * 3;
    const float *src = pos + (size_t)*f0 * A * 3;
    for (int i = threadIdx.x; i < n_float; i += 256) atoms[i] = src[i];
    __syncthreads();
    return nf;
}

// ---- nearest centre ----
// rows x d floats of src staged transposed, yt[j ra + r] (the lanes of a wave read consecutive words), by the G threads of a group.
__device__ __forceinline__ void stage_rows_transposed(float *yt, const float *src, int rows, int d, int ra, int lane, int G) {
    for (int i = lane; i < rows * d; i += G) {
        const int r = i / d, j = i - r * d;
        yt[j * ra + r] = src[i];
    }
}

// sum_j (a[j sa] - b[j])^2: fp64 differences of fp32 values, the fused sum over j ascending.  NaN when a or b holds one.
__device__ __forceinline__ double sq_dist_chain(const float *a, int sa, const float *b, int d) {
    double acc = 0.0;
    for (int j = 0; j < d; ++j) {
        const double diff = (double)a[j * sa] - (double)b[j];
        acc = fma(diff, diff, acc);
    }
    return acc;
}

// The lowest c < k that minimises sq_dist_chain of row r of the transposed tile yt (ra rows) against centres [k, d]: centres ascending,
// strict < (ties go to the lowest index, as np.argmin).  *best the winning distance, *nan whether the row holds a NaN (the caller's -1).
__device__ __forceinline__ int nearest_centre(const float *yt, int ra, int r, const float *centres, int d, int k, double *best, bool *nan) {
    bool has_nan = false;
    for (int j = 0; j < d; ++j) has_nan |= yt[j * ra + r] != yt[j * ra + r];
    int best_c = 0;
    double b = __builtin_inf();
    for (int c = 0; c < k; ++c) {
        const double acc = sq_dist_chain(yt + r, ra, centres + c * d, d);
        if (acc < b) b = acc, best_c = c;
    }
    *best = b, *nan = has_nan;
    return best_c;
}

// ---- running limits of a projection ----
// The order-preserving key of a float: a < b as floats (no NaN) <=> key(a) < key(b) as unsigned integers (-0 below +0).
__device__ __forceinline__ unsigned lim_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lim_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// A workgroup's LDS keys of `cols` columns: started at the keys of NaN patterns (no value has them); the key of every y[t, j] that is not
// NaN by LDS integer atomics; after a barrier, one integer atomic per column on keys [2 d] (keys[j] = min, keys[d + j] = max).
__device__ __forceinline__ void lim_init(unsigned *kmin, unsigned *kmax, int cols) {
    if ((int)threadIdx.x < cols) kmin[threadIdx.x] = 0xffffffffu, kmax[threadIdx.x] = 0u;
}
__device__ __forceinline__ void lim_update(unsigned *kmin, unsigned *kmax, int j, float v) {
    if (v == v) {
        const unsigned k = lim_key(v);
        atomicMin(&kmin[j], k), atomicMax(&kmax[j], k);
    }
}
__device__ __forceinline__ void lim_flush(unsigned *keys, const unsigned *kmin, const unsigned *kmax, int d) {
    if ((int)threadIdx.x < d && kmin[threadIdx.x] != 0xffffffffu) {  // (a workgroup whose column held only NaN adds nothing)
        atomicMin(&keys[threadIdx.x], kmin[threadIdx.x]);
        atomicMax(&keys[d + threadIdx.x], kmax[threadIdx.x]);
    }
}

// ---- Jensen-Shannon ----
// tot[0][0], tot[1][0] = the totals of two int64 rows of `bins` counts (integers: any order gives the same totals).  Ends with a barrier.
__device__ __forceinline__ void js_totals(long long (*tot)[256], const long long *ra, const long long *rb, int bins) {
    long long sa = 0, sb = 0;
    for (int i = threadIdx.x; i < bins; i += 256) sa += ra[i], sb += rb[i];
    tot[0][threadIdx.x] = sa, tot[1][threadIdx.x] = sb;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) tot[0][threadIdx.x] += tot[0][threadIdx.x + w], tot[1][threadIdx.x] += tot[1][threadIdx.x + w];
        __syncthreads();
    }
}
// (The other shared rule of k_js and k_js_density - thread 0 adds the 256 staged terms of a tile in bin order - stays written out in both:
// as a fragment it moved k_js's tile loop and the js_distance line of tools/torsion_stats_cost.py by 0.8 us: profiles/stat_fragments.txt.)
