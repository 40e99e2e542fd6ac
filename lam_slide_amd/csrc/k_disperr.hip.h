// Displacement errors of the decoded positions (lsl_disp_error_rows / lsl_disp_error_final): the evaluation tail of the trajectory models -
//      validation_step (second_stage/md17.py:82-86, nba.py:100-104, pedestrian.py:88-92), no mask:
//          ade = norm(true - pred, dim=-1).mean(dim=(1, 2)),   fde = norm(true[:, -1] - pred[:, -1], dim=-1).mean(dim=1)
//      test_step (nba.py:182-225, pedestrian.py:170-212; md17.py:157-169 averages the validation lines over its samples):
//          one row per real agent (attention_mask[:, -1]), error [N, K, Tf] = norm(traj - target[:, None]), ADE = mean over the frames,
//          FDE = last frame, each minimised on its own over the first num_runs samples
//      on_test_epoch_end (nba.py:240-245): the mean over the agents of all batches.
// k_disp_rows writes (ADE, FDE) of every (sample, scene, agent) and the two unmasked means of every (sample, scene); k_disp_final takes
// the minima over the samples and the fp64 sums an epoch mean is made of.  pred is read where the decoder left it, [K, B, Tp, A, D], the
// target where the batch holds it, [B, Tt, A, D]: the future frames are addressed by a frame offset each, the reference's permute /
// reshape / boolean-index copies never exist and nothing waits for the host.
//
// Orders (k_loss_frag.hip.h): the unit is one sample trajectory (k, b), the entities its A agents; a thread walks an agent's frames t = 0 ..
// Tf - 1 in ascending order, e_t = sqrtf(sum_d fmaf(delta_d, delta_d, .)) with d ascending, s += e_t in that order (loads of several frames
// may be in flight, the additions are not reordered).  Every order is fixed by (A, D, Tf) alone.  The final kernel takes k in ascending
// order.  sqrtf and the divisions are the correctly rounded ones.
#pragma once
#include "common.hip.h"
#include "k_loss_frag.hip.h"

#define LSL_DISP_MAX_D 4
#define LSL_DISP_MAX_UNITS 16777215LL  // K * B < 2^24: a grid of one 256-thread workgroup per unit stays below 2^32 threads, which every launch takes

// rows[((k B + b) A + a) * 2 + (0, 1)] = (sum_t e_t / Tf, e_{Tf-1}) of agent a in sample k of scene b; traj (may be null)
// [(k B + b) * 2 + (0, 1)] = (sum_a s_a / (Tf A), sum_a e_{Tf-1,a} / A).  pred [units, Tp, A, D] from frame t0p, target [B, Tt, A, D] from
// frame t0t, Tf frames of both.  grid ceil(units / (256 / TEAM)), 256 threads, no LDS but the four wave sums of the 256-thread form.
template <int D, int TEAM>
__global__ void __launch_bounds__(256) k_disp_rows(float *rows, float *traj, const float *pred, const float *target, long long units, int B, int Tp,
                                                   int t0p, int Tt, int t0t, int Tf, int A) {
    const LossTeam<TEAM> tm(units);
    const int tl = tm.tl;
    const long long unit = tm.unit;
    const bool live = tm.live;
    const size_t AD = (size_t)A * D;
    float t_ade = 0.0f, t_fde = 0.0f;
    if (live) {
        const float *gp = pred + ((size_t)unit * Tp + t0p) * AD, *gt = target + ((size_t)(unit % B) * Tt + t0t) * AD;
        float *gr = rows + (size_t)unit * A * 2;
        for (int a = tl; a < A; a += TEAM) {
            const float *pa = gp + (size_t)a * D, *ta = gt + (size_t)a * D;
            float s = 0.0f, e = 0.0f;
#pragma unroll 4
            for (int t = 0; t < Tf; ++t) {
                float sq = 0.0f;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const float delta = pa[t * AD + d] - ta[t * AD + d];
                    sq = fmaf(delta, delta, sq);
                }
                e = sqrtf(sq);
                s += e;
            }
            gr[(size_t)a * 2] = s / (float)Tf;
            gr[(size_t)a * 2 + 1] = e;
            t_ade += s;
            t_fde += e;
        }
    }
    if (!traj) return;  // (uniform over the grid)
    float v[2] = {t_ade, t_fde};
    const float n_ade = (float)Tf * (float)A, n_fde = (float)A;
    team_sums<TEAM>(live, v, [&](int k, float tot) {
        if (live) traj[(size_t)unit * 2 + k] = tot / (k == 0 ? n_ade : n_fde);
    });
}

// agents[(b A + a) * 2 + c] = min over k = 0 .. R - 1 of rows[k, b, a, c], k ascending, the two columns on their own, a NaN of any sample
// kept (torch.min); quiet NaN where mask[b, a] == 0 (mask null: every agent is real).  totals (fp64 [5], written, not accumulated) =
// sum minADE, sum minFDE, n over the real agents in (b, a) order, then sum traj ADE, sum traj FDE over the R * B units in (k, b) order
// (0 when traj is null).  One workgroup of 256 threads: all of them take minima, the first wave adds.
__global__ void __launch_bounds__(256) k_disp_final(float *agents, double *totals, const float *rows, const float *traj, const unsigned char *mask,
                                                    int R, int B, int A) {
    __shared__ double lane_sum[5][64];
    const long long BA = (long long)B * A, RB = (long long)R * B;
    for (long long i = threadIdx.x; i < BA; i += 256) {
        float ade = __builtin_nanf(""), fde = ade;
        if (!mask || mask[i]) {
            ade = rows[(size_t)i * 2], fde = rows[(size_t)i * 2 + 1];
            for (int k = 1; k < R; ++k) {
                const float a = rows[((size_t)k * BA + i) * 2], f = rows[((size_t)k * BA + i) * 2 + 1];
                ade = (a < ade || a != a) ? a : ade;  // (once NaN, it stays: nothing is below a NaN)
                fde = (f < fde || f != f) ? f : fde;
            }
        }
        agents[(size_t)i * 2] = ade, agents[(size_t)i * 2 + 1] = fde;
    }
    __syncthreads();  // (the first wave reads back what all four wrote: the barrier orders a workgroup's global stores and loads)
    if (threadIdx.x < 64) {
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        s[2] = lane_rows_add<2, 0>(s, agents, nullptr, BA, threadIdx.x, mask);
        if (traj) lane_rows_add<2, 0>(s + 3, traj, nullptr, RB, threadIdx.x);
#pragma unroll
        for (int c = 0; c < 5; ++c) lane_sum[c][threadIdx.x] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < 5) totals[threadIdx.x] = lane_order_total(lane_sum[threadIdx.x]);
}
