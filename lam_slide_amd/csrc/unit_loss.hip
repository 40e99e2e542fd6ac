// The losses' translation unit of liblamslide_hip.so (include/lsl_api.h): the geometry losses of the decoded positions, the peptide frame and
// torsion losses, the displacement errors (ADE / FDE, best-of-K) and the class losses of the decoder heads - per-frame sums, then one final
// launch each.  Every kernel built on k_loss_frag.hip.h is compiled here, the stochastic-interpolant objective's too (its entry points
// are part of the sampling path: lsl_api.hip).
#include "../../include/lsl_api.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "k_mm_frag.hip.h"  // (ic<N>)
#include "k_siloss.hip.h"
#include "k_geomloss.hip.h"
#include "k_peptloss.hip.h"
#include "k_disperr.hip.h"
#include "k_classloss.hip.h"

#include "host_api.hip.h"
#include "host_lds.hip.h"

LSL_UNIT_INFO;

namespace {

// ---- the losses: the team forms of k_loss_frag.hip.h, one dispatcher for D = 1..4, one launch of the quotient finals ----
// f(ic<D>) for the D of the call (checked by the caller: 1..4)
template <class Fn>
void dispatch_d(int D, Fn f) {
    switch (D) {
        case 1: f(ic<1>()); break;
        case 2: f(ic<2>()); break;
        case 3: f(ic<3>()); break;
        default: f(ic<4>()); break;
    }
}

// the five sums of every frame (k_geomloss.hip.h)
template <int D, int TEAM>
void launch_geom_frame(float *sums, const float *pred, const float *target, const unsigned char *mask, int F, int A, hipStream_t st) {
    auto kern = k_geom_loss_frame<D, TEAM>;
    if (TEAM == 256) LSL_ALLOW_LDS(kern, geom_team_bytes(LSL_GEOM_MAX_A, D));  // (above 64 KiB at D = 4)
    hipLaunchKernelGGL(kern, dim3(loss_team_grid<TEAM>(F)), dim3(256), (256 / TEAM) * geom_team_bytes(A, D), st, sums, pred, target, mask, F, A);
}

// the four sums of every peptide frame (k_peptloss.hip.h)
template <int TEAM>
void launch_peptide_frame(float *sums, const float *pred, const float *target_frame, const unsigned char *atom14_mask, const float *tors_target,
                          const unsigned char *tors_mask, const long long *aatype, const signed char *restab, int F, int R, int kind, hipStream_t st) {
    // (at most 4 * pept_team_bytes(4) or pept_team_bytes(146) = 24.7 KB of LDS: below the 64 KiB default)
    hipLaunchKernelGGL(k_peptide_loss_frame<TEAM>, dim3(loss_team_grid<TEAM>(F)), dim3(256), (256 / TEAM) * pept_team_bytes(R), st, sums, pred,
                       target_frame, atom14_mask, tors_target, tors_mask, aatype, restab, F, R, kind);
}

// per-agent and per-trajectory displacement errors (k_disperr.hip.h)
template <int D, int TEAM>
void launch_disp_rows(float *rows, float *traj, const float *pred, const float *target, long long units, int B, int Tp, int t0p, int Tt, int t0t,
                      int Tf, int A, hipStream_t st) {
    hipLaunchKernelGGL((k_disp_rows<D, TEAM>), dim3(loss_team_grid<TEAM>(units)), dim3(256), 0, st, rows, traj, pred, target, units, B, Tp, t0p, Tt,
                       t0t, Tf, A);
}

// lsl_geom_loss_final / lsl_peptide_loss_final / lsl_class_loss_final: out[0 .. NOUT - 1] from a [F, WA] and, WB > 0, b [F, WB]
template <int WA, int WB, int NOUT>
int loss_final(const char *name, const float *a, const float *b, int F, float *out, unsigned long long quots, void *stream) {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!a || (WB > 0 && !b) || !out) return fail(-1, "null argument");
    if (F <= 0) return fail(-3, "F must be positive");
    hipLaunchKernelGGL((k_loss_final<WA, WB, NOUT>), dim3(1), dim3(64), 0, (hipStream_t)stream, out, a, b, F, quots);
    LSL_CHECK_LAUNCH(name);
    return 0;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ---- the launches of the stochastic-interpolant objective (k_siloss.hip.h) for lsl_si_loss / lsl_si_reduce, which are entry points of
// lsl_api.hip (lsl_si_loss runs a network evaluation between the two); declared there ----
static_assert(sizeof(lsl_si_row) == sizeof(SiRow) && sizeof(SiRow) == 24 && LSL_SI_SLAB == LSL_SI_SLAB_ELEMS, "lsl_si_row layout / slab size");

void lsl_si_mix_launch(float *x, const float *x1, const float *x0, const lsl_si_row *rows, uint64_t per, uint64_t total, int cus, hipStream_t st) {
    const bool vec = per % 4 == 0 && aligned16(x) && aligned16(x1) && aligned16(x0);
    const unsigned grid = (unsigned)std::min<uint64_t>(((vec ? total / 4 : total) + 255) / 256, (uint64_t)cus * 16);
    if (vec)
        hipLaunchKernelGGL(k_si_mix<true>, dim3(grid), dim3(256), 0, st, x, x1, x0, (const SiRow *)rows, (unsigned long long)per, (unsigned long long)total);
    else
        hipLaunchKernelGGL(k_si_mix<false>, dim3(grid), dim3(256), 0, st, x, x1, x0, (const SiRow *)rows, (unsigned long long)per, (unsigned long long)total);
}

int lsl_si_reduce_launch(const float *pred, const float *x1, const float *x0, const lsl_si_row *rows, int B, uint64_t per, float *loss,
                         float *partial, hipStream_t st) {
    const size_t slabs = (size_t)((per + LSL_SI_SLAB_ELEMS - 1) / LSL_SI_SLAB_ELEMS);
    const bool vec = per % 4 == 0 && aligned16(pred) && aligned16(x1) && aligned16(x0);
    for (int b0 = 0; b0 < B; b0 += 65535) {  // (a grid has at most 65535 rows)
        const dim3 grid((unsigned)slabs, (unsigned)std::min(B - b0, 65535));
        const size_t o = (size_t)b0 * per;
        if (vec)
            hipLaunchKernelGGL(k_si_loss_partial<true>, grid, dim3(256), 0, st, partial + (size_t)b0 * slabs, pred + o, x1 + o, x0 + o,
                               (const SiRow *)rows + b0, (unsigned long long)per);
        else
            hipLaunchKernelGGL(k_si_loss_partial<false>, grid, dim3(256), 0, st, partial + (size_t)b0 * slabs, pred + o, x1 + o, x0 + o,
                               (const SiRow *)rows + b0, (unsigned long long)per);
    }
    hipLaunchKernelGGL(k_si_loss_final, dim3((unsigned)B), dim3(64), 0, st, loss, (const float *)partial, (const SiRow *)rows, (int)slabs,
                       (unsigned long long)per);
    LSL_CHECK_LAUNCH("si loss reduction");
    return 0;
}

extern "C" {

// ---- geometry losses of the decoded positions (k_geomloss.hip.h) ----
int lsl_geom_loss_sums(const float *pred, const float *target, const uint8_t *mask, int32_t F, int32_t A, int32_t D, float *sums, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pred || !target || !mask || !sums) return fail(-1, "null argument");
    if (F <= 0) return fail(-3, "F must be positive");
    if (A < 1 || A > LSL_GEOM_MAX_A) return fail(-3, "A = %d outside the native form (1..%d entities)", A, LSL_GEOM_MAX_A);
    if (D < 1 || D > LSL_GEOM_MAX_D) return fail(-3, "D = %d outside the native form (1..%d coordinates)", D, LSL_GEOM_MAX_D);
    hipStream_t st = (hipStream_t)stream;
    dispatch_d(D, [&](auto d) {
        if (loss_team(A) == 64)
            launch_geom_frame<d(), 64>(sums, pred, target, mask, F, A, st);
        else
            launch_geom_frame<d(), 256>(sums, pred, target, mask, F, A, st);
    });
    LSL_CHECK_LAUNCH("lsl_geom_loss_sums");
    return 0;
} LSL_API_CATCH

int lsl_geom_loss_final(const float *sums, int32_t F, float *out, void *stream) try {
    return loss_final<5, 0, 3>("lsl_geom_loss_final", sums, nullptr, F, out, GEOM_QUOTS, stream);
} LSL_API_CATCH

// ---- frame-local and torsion losses of the decoded peptide positions (k_peptloss.hip.h) ----
int lsl_peptide_loss_sums(const float *pred, const float *target_frame, const uint8_t *atom14_mask, const float *tors_target, const uint8_t *tors_mask,
                          const int64_t *aatype, const int8_t *restab, int32_t F, int32_t R, int32_t kind, float *sums, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pred || !target_frame || !atom14_mask || !tors_target || !tors_mask || !aatype || !restab || !sums) return fail(-1, "null argument");
    if (F <= 0) return fail(-3, "F must be positive");
    if (R < 1 || R > LSL_PEPT_MAX_R) return fail(-3, "R = %d outside the native form (1..%d residues)", R, LSL_PEPT_MAX_R);
    if (kind != 0 && kind != 1) return fail(-3, "kind = %d: 0 (MaskedCosineLoss) or 1 (MaskedCosineLossV2)", kind);
    hipStream_t st = (hipStream_t)stream;
    if (loss_team(R * 14) == 64)
        launch_peptide_frame<64>(sums, pred, target_frame, atom14_mask, tors_target, tors_mask, (const long long *)aatype, (const signed char *)restab, F, R, kind, st);
    else
        launch_peptide_frame<256>(sums, pred, target_frame, atom14_mask, tors_target, tors_mask, (const long long *)aatype, (const signed char *)restab, F, R, kind, st);
    LSL_CHECK_LAUNCH("lsl_peptide_loss_sums");
    return 0;
} LSL_API_CATCH

int lsl_peptide_loss_final(const float *geom_sums, const float *pept_sums, int32_t F, float *out, void *stream) try {
    return loss_final<5, 4, 5>("lsl_peptide_loss_final", geom_sums, pept_sums, F, out, PEPT_QUOTS, stream);
} LSL_API_CATCH

// ---- displacement errors of the decoded positions: ADE / FDE and best-of-K (k_disperr.hip.h) ----
int lsl_disp_error_rows(const float *pred, const float *target, int32_t K, int32_t B, int32_t Tp, int32_t t0p, int32_t Tt, int32_t t0t, int32_t Tf,
                        int32_t A, int32_t D, float *rows, float *traj, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!pred || !target || !rows) return fail(-1, "null argument");
    if (K < 1 || B < 1) return fail(-3, "K = %d and B = %d must be positive", K, B);
    if ((long long)K * B > LSL_DISP_MAX_UNITS) return fail(-3, "K * B = %lld sample trajectories: at most %lld", (long long)K * B, LSL_DISP_MAX_UNITS);
    if (A < 1) return fail(-3, "A = %d: at least one agent", A);
    if (D < 1 || D > LSL_DISP_MAX_D) return fail(-3, "D = %d outside the native form (1..%d coordinates)", D, LSL_DISP_MAX_D);
    if (Tf < 1) return fail(-3, "Tf = %d: at least one future frame", Tf);
    if (t0p < 0 || (long long)t0p + Tf > Tp) return fail(-3, "frames %d..%d outside pred's %d frames", t0p, t0p + Tf - 1, Tp);
    if (t0t < 0 || (long long)t0t + Tf > Tt) return fail(-3, "frames %d..%d outside target's %d frames", t0t, t0t + Tf - 1, Tt);
    hipStream_t st = (hipStream_t)stream;
    const long long units = (long long)K * B;
    dispatch_d(D, [&](auto d) {
        if (loss_team(A) == 64)
            launch_disp_rows<d(), 64>(rows, traj, pred, target, units, B, Tp, t0p, Tt, t0t, Tf, A, st);
        else
            launch_disp_rows<d(), 256>(rows, traj, pred, target, units, B, Tp, t0p, Tt, t0t, Tf, A, st);
    });
    LSL_CHECK_LAUNCH("lsl_disp_error_rows");
    return 0;
} LSL_API_CATCH

int lsl_disp_error_final(const float *rows, const float *traj, const uint8_t *mask, int32_t K, int32_t num_runs, int32_t B, int32_t A, float *agents,
                         double *totals, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!rows || !agents || !totals) return fail(-1, "null argument");
    if (K < 1 || B < 1 || A < 1) return fail(-3, "K = %d, B = %d and A = %d must be positive", K, B, A);
    if (num_runs < 1 || num_runs > K) return fail(-3, "num_runs = %d outside 1..K = %d", num_runs, K);
    hipLaunchKernelGGL(k_disp_final, dim3(1), dim3(256), 0, (hipStream_t)stream, agents, totals, rows, traj, mask, (int)num_runs, (int)B, (int)A);
    LSL_CHECK_LAUNCH("lsl_disp_error_final");
    return 0;
} LSL_API_CATCH

// ---- class losses of the decoder heads (k_classloss.hip.h) ----
int lsl_class_loss_sums(const float *logits, const int64_t *target, const uint8_t *mask, int32_t F, int32_t A, int32_t K, float label_smoothing,
                        float *sums, int64_t *confusion, void *stream) try {
    DeviceGuard dev_guard_((hipStream_t)stream);
    if (!logits || !target || !sums) return fail(-1, "null argument");
    if (F <= 0) return fail(-3, "F must be positive");
    if (A < 1) return fail(-3, "A = %d: at least one row per frame", A);
    if (K < 1 || K > LSL_CLS_MAX_K) return fail(-3, "K = %d outside the native form (1..%d classes)", K, LSL_CLS_MAX_K);
    if (!(label_smoothing >= 0.0f && label_smoothing < 1.0f)) return fail(-3, "label_smoothing = %g outside [0, 1)", (double)label_smoothing);
    hipLaunchKernelGGL(k_class_loss_frame, dim3((unsigned)F), dim3(64), class_tile_bytes(K), (hipStream_t)stream, sums, (unsigned long long *)confusion, logits,
                       (const long long *)target, mask, (int)A, (int)K, label_smoothing);
    LSL_CHECK_LAUNCH("lsl_class_loss_sums");
    return 0;
} LSL_API_CATCH

int lsl_class_loss_final(const float *sums, int32_t F, float *out, void *stream) try {
    return loss_final<2, 0, 1>("lsl_class_loss_final", sums, nullptr, F, out, CLASS_QUOTS, stream);
} LSL_API_CATCH

}  // extern "C"
