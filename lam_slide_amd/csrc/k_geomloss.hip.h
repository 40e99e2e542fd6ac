// Geometry losses of the decoded positions (lsl_geom_loss_sums / lsl_geom_loss_final): what Loss.forward computes behind the SI term when
// calc_additional_losses is set (second_stage/md17.py:231-255) - MaskedMSELoss (losses.py:10-13), MaskedNormLoss (losses.py:31-34) and
// InterDistanceLoss (losses.py:126-134) on pred / target [F, A, D] with a mask [F, A], F = B*T frames:
//      pos_loss        = sum_f s_mse / sum_f n,        s_mse  = sum_a m_a mean_d (p - t)^2
//      dist            = sum_f s_norm / sum_f n,       s_norm = sum_a m_a ||p_a - t_a||,            n = sum_a m_a
//      inter_dist_loss = sum_f s_pair / sum_f n_pair,  s_pair = sum_ij m_i m_j (||p_i - p_j|| - ||t_i - t_j||)^2,   n_pair = n^2
// k_geom_loss_frame writes the five floats (s_mse, s_norm, n, s_pair, n_pair) of every frame, k_loss_final (GEOM_QUOTS) adds the columns and divides.
// The reference's two torch.cdist matrices [F, A, A] and its elementwise passes over them never exist: a frame's positions and mask sit in
// LDS (A <= 2048, D <= 4: at most 66 KiB), entity i walks j = 0 .. A-1 with broadcast reads.  Distances are sqrt(sum_d (x_i - x_j)^2) of
// coordinate differences (never a Gram matrix: cdist's matmul form for A > 25 cancels where this does not), so the diagonal is an exact 0.
//
// Masked-out entities are SKIPPED (a select on m_i, a wave-uniform branch on m_j), where the reference multiplies by the mask: the two differ
// only when a masked-out position is not finite (0 * inf = NaN there, nothing here).
//
// Orders (k_loss_frag.hip.h): the unit is a frame, the entities its A positions; thread l adds entity i's pair terms over ascending j into a
// row sum of its own and the row sums into its accumulator.  Every order is fixed by (A, D) alone.
#pragma once
#include "common.hip.h"
#include "k_loss_frag.hip.h"

#define LSL_GEOM_MAX_A 2048
#define LSL_GEOM_MAX_D 4

// LDS of one team: pred [A][D] f32 | target [A][D] f32 | mask [A] u8 (rounded up to 4 bytes: the next team's floats stay aligned)
__host__ __device__ inline size_t geom_team_bytes(int A, int D) { return (size_t)2 * A * D * 4 + (size_t)((A + 3) & ~3); }

// sums[f * 5 + (0..4)] = s_mse, s_norm, n, s_pair, n_pair of frame f.  grid ceil(F / (256 / TEAM)), 256 threads, dynamic LDS
// (256 / TEAM) * geom_team_bytes(A, D).
template <int D, int TEAM>
__global__ void __launch_bounds__(256) k_geom_loss_frame(float *sums, const float *pred, const float *target, const unsigned char *mask, int F, int A) {
    extern __shared__ __align__(16) unsigned char geom_lds[];
    const LossTeam<TEAM> tm(F);
    const int tl = tm.tl, AD = A * D;
    const long long frame = tm.unit;
    const bool live = tm.live;
    float *sp = reinterpret_cast<float *>(geom_lds + (size_t)tm.team * geom_team_bytes(A, D)), *st = sp + AD;
    unsigned char *sm = reinterpret_cast<unsigned char *>(st + AD);
    if (live) {
        const float *gp = pred + (size_t)frame * AD, *gt = target + (size_t)frame * AD;
        const unsigned char *gm = mask + (size_t)frame * A;
        for (int e = tl; e < AD; e += TEAM) sp[e] = gp[e], st[e] = gt[e];
        for (int a = tl; a < A; a += TEAM) sm[a] = gm[a] != 0;
    }
    __syncthreads();
    float s_mse = 0.0f, s_norm = 0.0f, s_n = 0.0f, s_pair = 0.0f;
    if (live) {
        for (int i = tl; i < A; i += TEAM) {
            const bool mi = sm[i] != 0;
            float pi[D], ti[D], sq = 0.0f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                pi[d] = sp[i * D + d], ti[d] = st[i * D + d];
                const float e = pi[d] - ti[d];
                sq = fmaf(e, e, sq);
            }
            float row = 0.0f;
            for (int j = 0; j < A; ++j) {
                if (!sm[j]) continue;  // (uniform over the lanes still in the i loop: each of them reads the same j)
                float dp = 0.0f, dt = 0.0f;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const float a = pi[d] - sp[j * D + d], b = ti[d] - st[j * D + d];
                    dp = fmaf(a, a, dp);
                    dt = fmaf(b, b, dt);
                }
                const float g = sqrtf(dp) - sqrtf(dt);  // (j == i: 0 - 0)
                row = fmaf(g, g, row);
            }
            s_mse += mi ? sq / (float)D : 0.0f;
            s_norm += mi ? sqrtf(sq) : 0.0f;
            s_n += mi ? 1.0f : 0.0f;
            s_pair += mi ? row : 0.0f;
        }
    }
    float v[4] = {s_mse, s_norm, s_n, s_pair};
    float *o = sums + (size_t)frame * 5;
    team_sums<TEAM>(live, v, [&](int k, float tot) {
        o[k] = tot;
        if (k == 2) o[4] = tot * tot;  // (n <= 2048: n^2 is exact in fp32)
    });
}

// lsl_geom_loss_final: pos_loss, dist, inter_dist_loss = s_mse / n, s_norm / n, s_pair / n_pair; a batch without a real entity gives NaN.
constexpr unsigned long long GEOM_QUOTS = loss_quot(0, 0, 2) | loss_quot(1, 1, 2) | loss_quot(2, 3, 4);
