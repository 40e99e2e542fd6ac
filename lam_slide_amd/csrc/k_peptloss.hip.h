// Frame-local and torsion losses of the decoded peptide positions (lsl_peptide_loss_sums / lsl_peptide_loss_final): the two terms of the
// peptide Loss.forward (second_stage/peptide.py:293-378) that k_geomloss.hip.h does not already compute with entities = (residue, atom).
// pred [F, R, 14, 3] are the decoded atom14 positions of F = B*T frames of R residues:
//      pos_frame_loss = sum_f s_frame / sum_f n,      s_frame = sum_ra m_ra mean_d (local(pred)_rad - target_frame_rad)^2,   n = sum_ra m_ra
//      torsion_loss   = sum_f s_tors / sum_f n_tors,  s_tors  = sum_rk w_rk l_rk,                                             n_tors = sum_rk w_rk
// k_peptide_loss_frame writes the four floats (s_frame, n, s_tors, n_tors) of every frame, k_loss_final (PEPT_QUOTS) adds their columns and the
// five columns of k_geom_loss_frame (A = R*14, D = 3, the same mask) and divides: pos_loss, pos_frame_loss, inter_distance_loss, norm_loss,
// torsion_loss.
//
// Geometry, fp32 throughout.  frame(x, o, y) is the Gram-Schmidt frame of utils/rigid_utils.py:1093-1134 (from_3_points, eps = 1e-8):
//      e0 = (o - x) / sqrt(|o - x|^2 + eps),   e1 = (y - o) - e0 (e0 . (y - o)),  e1 /= sqrt(|e1|^2 + eps),   e2 = e0 x e1
// A residue's backbone frame is frame(C, CA, N) with the x and z axes flipped (modules/geometry.py:212-227; N, CA, C = atom14 slots 0, 1, 2
// of every residue type), so local(p) = (-e0 . (p - CA), e1 . (p - CA), -e2 . (p - CA)).  Torsion k of residue r (peptide.py:170-286) takes
// four atom37 positions a0..a3 - pre-omega (prev CA, prev C, N, CA), phi (prev C, N, CA, C), psi (N, CA, C, slot 4), chi 1..4 (the residue
// type's four chi atoms) - where atom37 slot s of a residue of type aa is the atom14 position restab names, or 0 where the atom37 mask of
// that type is 0 (restab = -1), and the residue before residue 0 is all zeros.  With v = a3 in frame(a1, a2, a0):
//      (sin, cos) = (v_z, v_y) / sqrt(v_z^2 + v_y^2 + 1e-8),  both negated for psi
//      l = 1 - cos_sim((sin, cos), target)   kind 0, MaskedCosineLoss   (each vector divided by max(its norm, 1e-8), then the dot product)
//      l = 1 - (sin, cos) . target           kind 1, MaskedCosineLossV2
//
// Masked-out atoms and torsions are SKIPPED (a select), where the reference multiplies by the mask: the two differ only when a masked-out
// value is not finite (0 * NaN = NaN there, nothing here).  Where the previous CA and C are absent the pre-omega of the reference is
// normalised rounding noise; its own torsions_mask is 0 exactly there.  An aatype outside 0..20 makes the four sums of its frame NaN: it
// is staged as "no type" (no table row is read with it) and the lane that staged it poisons its four accumulators.
//
// Orders (k_loss_frag.hip.h): the unit is a frame, the entities its R*14 atoms (the threshold of k_geom_loss_frame: a wave per frame for the
// tetrapeptides, R = 4); the frame's R*21 work items are its R*14 atoms followed by its R*7 torsions.  Every order is fixed by R alone.
#pragma once
#include "common.hip.h"
#include "k_geomloss.hip.h"

#define LSL_PEPT_MAX_R (LSL_GEOM_MAX_A / 14)  // 146: the frame's R*14 atoms are the entities of lsl_geom_loss_sums
#define LSL_PEPT_TYPES 21                     // 20 residue types + unknown
#define LSL_PEPT_TAB 20                       // restab row: atom14 index of atom37 slots 0, 1, 2, 4, then of the 4 x 4 chi atoms; -1 = masked

// LDS of one team: pred [R][14][3] f32 | residue type [R] i8 (-1 = none; rounded up to 4 bytes: the next team's floats stay aligned)
__host__ __device__ inline size_t pept_team_bytes(int R) { return (size_t)R * 42 * 4 + (size_t)((R + 3) & ~3); }

struct PeptVec {
    float x, y, z;
};
__device__ __forceinline__ PeptVec pv_sub(PeptVec a, PeptVec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float pv_dot(PeptVec a, PeptVec b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }

// e0, e1, e2 of frame(x, o, y)
__device__ __forceinline__ void pept_frame(PeptVec x, PeptVec o, PeptVec y, PeptVec &e0, PeptVec &e1, PeptVec &e2) {
    e0 = pv_sub(o, x);
    const float d0 = sqrtf(pv_dot(e0, e0) + 1e-8f);
    e0 = {e0.x / d0, e0.y / d0, e0.z / d0};
    e1 = pv_sub(y, o);
    const float dot = pv_dot(e0, e1);
    e1 = {e1.x - e0.x * dot, e1.y - e0.y * dot, e1.z - e0.z * dot};
    const float d1 = sqrtf(pv_dot(e1, e1) + 1e-8f);
    e1 = {e1.x / d1, e1.y / d1, e1.z / d1};
    e2 = {e0.y * e1.z - e0.z * e1.y, e0.z * e1.x - e0.x * e1.z, e0.x * e1.y - e0.y * e1.x};
}

// atom14 slot `slot` (-1: an atom the atom37 mask zeroes) of residue r; r < 0: the zeros in front of the chain
__device__ __forceinline__ PeptVec pept_atom(const float *sp, int r, int slot) {
    if (r < 0 || slot < 0) return {0.0f, 0.0f, 0.0f};
    const float *p = sp + (r * 14 + slot) * 3;
    return {p[0], p[1], p[2]};
}

// sums[f * 4 + (0..3)] = s_frame, n, s_tors, n_tors of frame f.  grid ceil(F / (256 / TEAM)), 256 threads, dynamic LDS
// (256 / TEAM) * pept_team_bytes(R).
template <int TEAM>
__global__ void __launch_bounds__(256) k_peptide_loss_frame(float *sums, const float *pred, const float *target_frame, const unsigned char *atom14_mask,
                                                            const float *tors_target, const unsigned char *tors_mask, const long long *aatype,
                                                            const signed char *restab, int F, int R, int kind) {
    extern __shared__ __align__(16) unsigned char pept_lds[];
    __shared__ signed char tab[LSL_PEPT_TYPES * LSL_PEPT_TAB];
    const LossTeam<TEAM> tm(F);
    const int tl = tm.tl, A = R * 14;
    const long long frame = tm.unit;
    const bool live = tm.live;
    float *sp = reinterpret_cast<float *>(pept_lds + (size_t)tm.team * pept_team_bytes(R));
    signed char *sa = reinterpret_cast<signed char *>(sp + A * 3);
    float s_frame = 0.0f, s_n = 0.0f, s_tors = 0.0f, s_nt = 0.0f;
    for (int e = threadIdx.x; e < LSL_PEPT_TYPES * LSL_PEPT_TAB; e += 256) tab[e] = restab[e];
    if (live) {
        const float *gp = pred + (size_t)frame * A * 3;
        for (int e = tl; e < A * 3; e += TEAM) sp[e] = gp[e];
        for (int r = tl; r < R; r += TEAM) {
            const long long aa = aatype[(size_t)frame * R + r];
            const bool known = aa >= 0 && aa < LSL_PEPT_TYPES;
            sa[r] = known ? (signed char)aa : (signed char)-1;
            if (!known) s_frame = s_n = s_tors = s_nt = __builtin_nanf("");
        }
    }
    __syncthreads();
    if (live) {
        for (int it = tl; it < R * 21; it += TEAM) {
            if (it < A) {  // atom (r, a): its position in the residue's backbone frame
                if (!atom14_mask[(size_t)frame * A + it]) continue;
                const int r = it / 14;
                const PeptVec ca = pept_atom(sp, r, 1);
                PeptVec e0, e1, e2;
                pept_frame(pept_atom(sp, r, 2), ca, pept_atom(sp, r, 0), e0, e1, e2);
                const PeptVec d = pv_sub(pept_atom(sp, r, it - r * 14), ca);
                const float *t = target_frame + ((size_t)frame * A + it) * 3;
                const float ex = -pv_dot(e0, d) - t[0], ey = pv_dot(e1, d) - t[1], ez = -pv_dot(e2, d) - t[2];
                s_frame += fmaf(ez, ez, fmaf(ey, ey, ex * ex)) / 3.0f;
                s_n += 1.0f;
            } else {  // torsion (r, k)
                const int q = it - A, r = q / 7, k = q - r * 7;
                if (!tors_mask[(size_t)frame * R * 7 + q]) continue;
                const int aa = sa[r], ap = r > 0 ? sa[r - 1] : 0;
                if (aa < 0 || ap < 0) continue;  // (no type: the frame's sums are NaN already)
                const signed char *row = tab + aa * LSL_PEPT_TAB, *prow = tab + ap * LSL_PEPT_TAB;
                const int rp = r - 1;  // (-1 in front of the chain: zeros)
                PeptVec a0, a1, a2, a3;
                if (k == 0)
                    a0 = pept_atom(sp, rp, prow[1]), a1 = pept_atom(sp, rp, prow[2]), a2 = pept_atom(sp, r, row[0]), a3 = pept_atom(sp, r, row[1]);
                else if (k == 1)
                    a0 = pept_atom(sp, rp, prow[2]), a1 = pept_atom(sp, r, row[0]), a2 = pept_atom(sp, r, row[1]), a3 = pept_atom(sp, r, row[2]);
                else if (k == 2)
                    a0 = pept_atom(sp, r, row[0]), a1 = pept_atom(sp, r, row[1]), a2 = pept_atom(sp, r, row[2]), a3 = pept_atom(sp, r, row[3]);
                else {
                    const signed char *c = row + 4 + (k - 3) * 4;
                    a0 = pept_atom(sp, r, c[0]), a1 = pept_atom(sp, r, c[1]), a2 = pept_atom(sp, r, c[2]), a3 = pept_atom(sp, r, c[3]);
                }
                PeptVec e0, e1, e2;
                pept_frame(a1, a2, a0, e0, e1, e2);
                const PeptVec d = pv_sub(a3, a2);
                const float vy = pv_dot(e1, d), vz = pv_dot(e2, d);
                const float den = sqrtf(fmaf(vz, vz, vy * vy) + 1e-8f);
                float sn = vz / den, cs = vy / den;
                if (k == 2) sn = -sn, cs = -cs;
                const float *t = tors_target + ((size_t)frame * R * 7 + q) * 2;
                float l;
                if (kind == 0) {
                    const float np = fmaxf(sqrtf(fmaf(cs, cs, sn * sn)), 1e-8f), nt = fmaxf(sqrtf(fmaf(t[1], t[1], t[0] * t[0])), 1e-8f);
                    l = 1.0f - fmaf(cs / np, t[1] / nt, (sn / np) * (t[0] / nt));
                } else {
                    l = 1.0f - fmaf(cs, t[1], sn * t[0]);
                }
                s_tors += l;
                s_nt += 1.0f;
            }
        }
    }
    // team_sums<TEAM> of the four values, written out: through the fragment this kernel gained six instructions and lsl_peptide_loss_sums
    // 0.1 us at the tetrapeptide shape, outside the parent's spread (profiles/loss_fragments.txt)
    s_frame = wave_sum_dpp(s_frame);
    s_n = wave_sum_dpp(s_n);
    s_tors = wave_sum_dpp(s_tors);
    s_nt = wave_sum_dpp(s_nt);
    if constexpr (TEAM == 64) {
        if (live && tl == 0) {
            float *o = sums + (size_t)frame * 4;
            o[0] = s_frame, o[1] = s_n, o[2] = s_tors, o[3] = s_nt;
        }
    } else {
        __shared__ float wsum[4][4];  // (the 256-thread form only)
        if ((threadIdx.x & 63) == 0) {
            float *w = wsum[threadIdx.x >> 6];
            w[0] = s_frame, w[1] = s_n, w[2] = s_tors, w[3] = s_nt;
        }
        __syncthreads();
        if (threadIdx.x < 4)  // thread k combines value k of the four waves in wave order
            sums[(size_t)frame * 4 + threadIdx.x] = ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
    }
}

// lsl_peptide_loss_final: pos_loss, pos_frame_loss, inter_distance_loss, norm_loss, torsion_loss from geom [F, 5] (columns 0..4: s_mse,
// s_norm, n, s_pair, n_pair) and pept [F, 4] (columns 5..8: s_frame, n, s_tors, n_tors).
constexpr unsigned long long PEPT_QUOTS = loss_quot(0, 0, 2) | loss_quot(1, 5, 6) | loss_quot(2, 3, 4) | loss_quot(3, 1, 2) | loss_quot(4, 7, 8);
//                                           s_mse / n          s_frame / n (pept)   s_pair / n_pair      s_norm / n           s_tors / n_tors
