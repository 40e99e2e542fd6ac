// Class losses of the first-stage decoder heads (lsl_class_loss_sums / lsl_class_loss_final): the cross-entropy terms of the four first-stage
// Loss classes - MaskedCrossEntropyLoss on the atom types (modules/losses.py:62-72; first_stage/md17.py) and nn.CrossEntropyLoss on team /
// group / aatype (first_stage/nba.py, peptide.py) - on logits [F, A, K], target [F, A] and an optional mask [F, A], F frames.  Per row, fp32:
//      lse = max_k l_k + log sum_k exp(l_k - max),   nll = lse - l_y,   smooth = lse - mean_k l_k,   loss = (1 - eps) nll + eps smooth
// (torch's definition; eps = label_smoothing, eps == 0 takes nll alone as torch does).  It is evaluated on d_k = l_k - max <= 0 with the
// maximum's own term exp(0) = 1 taken out of the sum: lg = log1p(sum_{k != argmax} exp d_k), nll = lg - d_y, smooth = lg - mean d.  A
// dominant logit of any size cancels before the log is added, and a row the model has right keeps its small loss (log(1 + 1e-20) is 0 in
// fp32, log1p(1e-20) is not).
//      loss = sum_f s_ce / sum_f n,     s_ce = sum of loss over the counted rows (mask nonzero or no mask, and target != -100),
//      n = rows with a nonzero mask (MaskedCrossEntropyLoss divides by mask.sum()), or without a mask rows with target != -100 (the mean of
//      nn.CrossEntropyLoss over the non-ignored rows)
// k_class_loss_frame writes (s_ce, n) of every frame, k_loss_final (CLASS_QUOTS) adds the two columns and divides.  With a confusion matrix [K, K]
// (i64, zeroed by the caller) every counted row with a target in range and no NaN logit adds one to cell [target, argmax] (lowest index
// among equal maxima) by an integer atomic: exact in any order, so several calls accumulate an epoch.
//
// Masked-out and ignored rows are SKIPPED (their logits are copied to LDS and never enter an operation), where MaskedCrossEntropyLoss
// multiplies by the mask: the two differ only when a masked-out logit is not finite (0 * NaN = NaN there, nothing here).  A counted row whose
// target is < 0 (and not -100) or >= K makes both sums of its frame NaN and touches nothing else (no logit is read with it); torch raises.
//
// Lanes and rows: a LANE PER ROW, one wave per frame.  K <= 128 (the real heads have 2, 3, 10 and 21 classes): a wave per row would leave
// most lanes idle at these widths and pay three 6-step DPP reductions (max, sum exp, sum) per row, a lane per row needs no cross-lane step
// until the frame's sum.  Read straight from memory, lane l would walk row l with a stride of K floats between lanes; instead the wave copies a
// tile of 64 rows to LDS with unit-stride loads and lane l reads row l of the tile there, at a row stride of K | 1 floats (odd: the 64 lanes
// hit distinct banks in each half-wave).  Dynamic LDS of 64 * (K | 1) floats - 2.8 KiB at K = 10, 33 KiB at K = 128, below the 64 KiB default
// limit - so the narrow heads keep many waves per CU; no scratch: the row is re-read from LDS in the second pass instead of being kept in
// K registers indexed at run time.
//
// Orders (k_loss_frag.hip.h, without its teams: always one wave per frame): lane l owns rows l, l + 64, ... of the frame and adds their
// losses in ascending order, the wave sums by DPP.  Every order is fixed by (A, K) alone.
#pragma once
#include "common.hip.h"
#include "k_loss_frag.hip.h"

#define LSL_CLS_MAX_K 128
#define LSL_CLS_IGNORE (-100)

__host__ __device__ inline size_t class_tile_bytes(int K) { return (size_t)64 * (K | 1) * sizeof(float); }

// sums[f * 2 + (0, 1)] = s_ce, n of frame f.  grid F, 64 threads (one wave), dynamic LDS class_tile_bytes(K).
__global__ void __launch_bounds__(64) k_class_loss_frame(float *sums, unsigned long long *confusion, const float *logits, const long long *target,
                                                         const unsigned char *mask, int A, int K, float eps) {
    extern __shared__ __align__(16) float tile[];
    const int lane = threadIdx.x, S = K | 1;
    const size_t row0 = (size_t)blockIdx.x * A;  // first row of the frame
    const float inv_k = 1.0f / (float)K;
    float s_ce = 0.0f, s_n = 0.0f;
    bool bad = false;
    for (int r0 = 0; r0 < A; r0 += 64) {
        const int rows = min(64, A - r0), cells = rows * K;
        const float *g = logits + (row0 + r0) * K;
        for (int e = lane; e < cells; e += 64) {
            const int r = e / K;
            tile[r * S + (e - r * K)] = g[e];
        }
        __syncthreads();
        if (lane < rows) {
            const size_t row = row0 + r0 + lane;
            const bool m = mask ? mask[row] != 0 : true;
            const long long y = m ? target[row] : LSL_CLS_IGNORE;
            const bool counted = m && y != LSL_CLS_IGNORE;
            s_n += (mask ? m : counted) ? 1.0f : 0.0f;
            if (counted && (y < 0 || y >= K)) bad = true;
            else if (counted) {
                const float *l = tile + lane * S;
                float mx = l[0];
                int arg = 0;
                bool nan = mx != mx;
                for (int k = 1; k < K; ++k) {
                    const float v = l[k];
                    nan |= v != v;
                    if (v > mx) mx = v, arg = k;  // (strict: the lowest index among equal maxima)
                }
                float se = 0.0f, sd = 0.0f;
                for (int k = 0; k < K; ++k) {
                    const float d = l[k] - mx;
                    se += k == arg ? 0.0f : expf(d);  // (the maximum itself: the 1 of log1p)
                    sd += d;
                }
                const float lg = log1pf(se), nll = lg - (l[(int)y] - mx);
                s_ce += eps > 0.0f ? (1.0f - eps) * nll + eps * (lg - sd * inv_k) : nll;
                if (confusion && !nan) atomicAdd(confusion + (size_t)y * K + arg, 1ull);
            }
        }
        __syncthreads();
    }
    s_ce = wave_sum_dpp(s_ce);
    s_n = wave_sum_dpp(s_n);
    const bool any_bad = __any(bad);
    if (lane == 0) {
        const float qnan = __builtin_nanf("");
        sums[(size_t)blockIdx.x * 2] = any_bad ? qnan : s_ce;
        sums[(size_t)blockIdx.x * 2 + 1] = any_bad ? qnan : s_n;
    }
}

// lsl_class_loss_final: loss = s_ce / n; a batch without a counted row gives NaN.
constexpr unsigned long long CLASS_QUOTS = loss_quot(0, 0, 1);
