/*
 * lsl_api.h -- C ABI of liblamslide_hip.so: the MI355X (gfx950) implementation of LaM-SLidE's
 * second-stage latent SiT sampling path.
 *
 * The reference implements this path in Python only (no FFI exists there).  Each entry point below
 * names the reference interface it stands in for; the Python binding that a reference maintainer
 * would add is shown in INTEGRATION.md and implemented in lam_slide_amd/_lib.py.
 *
 * Conventions
 *   - Every pointer marked "device" is HBM memory owned by the caller (PyTorch).  The library allocates
 *     no device memory; scratch comes from the caller's workspace (lsl_workspace_bytes).
 *   - All calls are asynchronous: work is enqueued on `stream` (a hipStream_t passed as void*), no
 *     internal synchronisation, no host<->device copies.
 *   - Return value 0 = ok, negative = error; lsl_last_error() returns a thread-local message.
 *     Nothing aborts or throws across this boundary (allocation failures and stray C++ exceptions become error codes).
 *   - Launches go to the device that owns `stream`, whatever the calling thread's current device is.
 *   - Tensors are row-major contiguous.  State layout [B, T, L, C] fp32 exactly as the reference's
 *     LatentSIV3.forward takes it (latent_si_v31.py:168-170).
 */
#ifndef LSL_API_H
#define LSL_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: these entry points are its whole export list */
#endif

/* 2: lsl_sample_ex takes n_trace; linear1 biases are read in whole 256-feature tiles (b1 zero-padded to a multiple of 256 floats);
 *    lsl_sample_ex, lsl_debug_taps, lsl_build_info exist.
 * 3: lsl_rk_lincomb / lsl_rk_dense / lsl_rk_error_ratio exist (state arithmetic of the adaptive and fixed-grid Runge-Kutta samplers);
 *    no signature of version 2 changed.
 * 4: lsl_model_set_attention_mode exists (attention_linear, mmdit.py:58-72); nothing else changed.
 * 5: lsl_model_set_tail, lsl_model_tail, lsl_profile_kernel_name exist; no signature of version 4 changed.
 * 6: lsl_model_set_ln_fuse, lsl_model_ln_fuse exist; no signature of version 5 changed.
 * 6, later: lsl_si_loss, lsl_si_reduce, lsl_si_loss_workspace_bytes added, no signature changed (a binding that needs them finds out by
 *    looking the symbols up: a library without them is stale).
 * 6, later still: lsl_geom_loss_sums, lsl_geom_loss_final added the same way.
 * 6, later still: lsl_peptide_loss_sums, lsl_peptide_loss_final added the same way.
 * 6, later still: lsl_disp_error_rows, lsl_disp_error_final added the same way.
 * 6, later still: lsl_dihedral_angles, lsl_histogram, lsl_lag_products_workspace_bytes, lsl_lag_products, lsl_js_distance added the same way.
 * 6, later still: lsl_lagged_moments_workspace_bytes, lsl_lagged_moments, lsl_project, lsl_assign_centers, lsl_transition_counts added the same way.
 * 6, later still: lsl_kmeans_workspace_bytes, lsl_kmeans_step, lsl_kmeans_nearest_rows added the same way.
 * 6, later still: lsl_debug_block_ex added the same way.
 * 6, later still: lsl_decode_heads, lsl_class_loss_sums, lsl_class_loss_final added the same way.
 * 6, later still: lsl_pair_distances, lsl_ca_frame_stats, lsl_histogram_columns, lsl_js_distance_density added the same way.
 * 6, later still: lsl_debug_mods_ex, lsl_debug_mods_steps, lsl_debug_embed, lsl_debug_head added the same way.
 * 6, later still: lsl_weighted_moments_workspace_bytes, lsl_weighted_moments, lsl_affine_weights, lsl_project_wide added the same way.
 * 6, later still: lsl_msm_active_set, lsl_msm_reversible_step, lsl_msm_transition_matrix added the same way.
 * 6, later still: lsl_superpose, lsl_atom_rmsf_workspace_bytes, lsl_atom_rmsf added the same way.
 * 6, later still: lsl_dopri_workspace_bytes, lsl_dopri_begin, lsl_dopri_advance, lsl_debug_dopri_coeffs added the same way.
 * 6, later still: lsl_forward_jvp_workspace_bytes, lsl_forward_jvp, lsl_dot_rows added the same way.
 * 6, later still: lsl_dopri_each_workspace_bytes, lsl_dopri_each_begin, lsl_dopri_each_advance added the same way.
 * 6, later still: lsl_dopri_logp_workspace_bytes, lsl_dopri_logp_begin, lsl_dopri_logp_advance, lsl_rademacher added the same way. */
#define LSL_VERSION 6

typedef struct lsl_model lsl_model;

/* Hyper-parameters of LatentSIV3.__init__ (latent_si_v31.py:68-121) that fix the weight shapes.
 * B, T, L arrive per call. */
typedef struct lsl_model_desc {
    int32_t in_dim;       /* C: in_dim == out_dim                                         */
    int32_t hidden;       /* D: hidden_size, multiple of 64, <= 512                        */
    int32_t heads;        /* H: num_heads                                                  */
    int32_t head_dim;     /* D / H (16, 24 or 32 in the shipped configs)                   */
    int32_t head_dim_pad; /* packed head width: 16 if head_dim == 16, else 32 (zero padded) */
    int32_t mlp_dim;      /* M = int(D * mlp_ratio), multiple of 32                        */
    int32_t depth;        /* number of layers (share_weights is resolved by the packer)    */
    int32_t vec_in_dim;   /* V, or 0 when the model has no vec_in                          */
    int32_t normalize;    /* F.layer_norm after the input embedding (latent_si_v31.py:173) */
    float theta;          /* RoPE base (mmdit.py:75-82)                                    */
} lsl_model_desc;

/* One ParallelMLPAttentionV2 (mmdit.py:215-249), packed by lam_slide_amd/packing.py:
 *   w1  bf16 [F1 rounded up to 256][D]   rows = [q heads | k heads | v heads | mlp], each head padded to
 *                      head_dim_pad; zero rows up to a whole 256-row tile (read without clamping)
 *   b1  f32  [F1 rounded up to 256], zero padded; F1 = 3*H*head_dim_pad + M (the tile kernels copy whole 256-feature tiles of it
 *                      into LDS: a buffer of exactly F1 floats would be read out of bounds)
 *   qs, ks f32 [head_dim_pad]  QKNorm scales (zero in the padding)
 *   w2  bf16 [D rounded up to 256][K2]   columns = [attention heads (padded) | mlp],  K2 = H*head_dim_pad + M
 *   b2  f32  [D]                                                                         */
typedef struct lsl_block_weights {
    const void *w1;
    const float *b1;
    const float *qs;
    const float *ks;
    const void *w2;
    const float *b2;
} lsl_block_weights;

/* The weight contract of SURVEY.md a2 as device pointers (fp32 unless noted). */
typedef struct lsl_weights {
    const float *x_in_w, *x_in_b;       /* [D,C], [D]    x_in                                   */
    const float *cond_w, *cond_b;       /* [D,C], [D]    cond_to_emb                            */
    const float *mask_emb;              /* [2,D]         mask_to_emb                            */
    const float *time_freqs;            /* [128]         exp(-ln(1e4) k/128) (mmdit.py:103-105)  */
    const float *time_w1, *time_b1;     /* [D,256], [D]  time_in.in_layer                       */
    const float *time_w2, *time_b2;     /* [D,D], [D]    time_in.out_layer                      */
    const float *vec_w1, *vec_b1;       /* [D,V], [D]    vec_in.in_layer  (NULL if V == 0)      */
    const float *vec_w2, *vec_b2;       /* [D,D], [D]    vec_in.out_layer                       */
    const float *mod_w, *mod_b;         /* [(6*depth+2)*D, D], [(6*depth+2)*D]: blocks.i.modulation.lin
                                           stacked in layer order, then adaLN_modulation.1       */
    const float *out_w, *out_b;         /* [C,D], [C]    linear                                 */
    const lsl_block_weights *blocks;    /* HOST array [2*depth]: spatial_0, temporal_0, spatial_1, ... */
} lsl_weights;

/* Arguments of one LatentSIV3.forward(x, t, x_cond, x_cond_mask, y) (latent_si_v31.py:168-188). */
typedef struct lsl_io {
    float *x;              /* device [B,T,L,C]: network input; the samplers update it in place      */
    const float *x_cond;   /* device [B,T,L,C]                                                       */
    const int64_t *mask;   /* device [B,T,L] values 0/1 (x_cond_mask, lightning_base.py:246-247)     */
    const float *y;        /* device [B,V] or NULL                                                   */
    const float *t;        /* device [B] (lsl_forward only)                                          */
    float *out;            /* device [B,T,L,C] (lsl_forward only)                                    */
    int32_t B, T, L;
} lsl_io;

/* One state update of a sampler.  Every sampler the reference builds from
 * Transport.get_drift / get_score (transport.py:158-226) with a fixed time grid is affine in
 * (state, network output, noise) with coefficients that depend only on t:
 *      m = network(x, t);   x <- ax * x + am * m + aw * w
 * ODE Euler (integrators.py:103-120 + torchdiffeq fixed-grid euler), Euler-Maruyama
 * (integrators.py:29-37) and the "Mean"/"Euler"/"Tweedie" last step (transport.py:267-299) all have
 * this form; lam_slide_amd/transport.py derives (ax, am, aw) in float64 from the same formulas. */
typedef struct lsl_step {
    float t;    /* time handed to the network, as fp32 (integrators.py:107-114) */
    float ax, am, aw;
} lsl_step;

/* Extended step record (lsl_sample_ex): x <- ax * x + am * network(x, t) + aw * w + as * saved, where `saved` is a copy of the state
 * taken by an earlier record of the same call.  Enough for every fixed-grid sampler of the reference that is affine per stage, e.g. the
 * stochastic Heun step (integrators.py:39-51) = three records:
 *     noise in, keep a copy :  x <- x + sqrt(2 g dt) w                         (LSL_STEP_NO_NETWORK | LSL_STEP_SAVE)
 *     predictor             :  x <- (1 + dt a(t)) x + dt b(t) net(x, t)
 *     corrector             :  x <- (1/2 + dt a(t')/2) x + dt b(t')/2 net(x, t') + saved / 2,   t' = t + dt
 * (drift(x, t) = a(t) x + b(t) net(x, t); the predictor's dt K1 is x_p - x_hat, so no division is needed). */
#define LSL_STEP_NO_NETWORK 1 /* no network evaluation: x <- ax * x + aw * w + as * saved (am is ignored) */
#define LSL_STEP_SAVE 2       /* after the update, copy the state into the call's saved-state buffer */
typedef struct lsl_step_ex {
    float t;
    float ax, am, aw, as;
    int32_t flags;
    int32_t noise_index; /* slice of `noise` / device-stream step number used for w; ignored when aw == 0 */
    int32_t trace_index; /* slice of `trace` that receives the state after this record, or -1 */
} lsl_step_ex;

int lsl_version(void);
/* Compiler and target the library was built with ("clang <version> gfx950"): the kernels' register budgets and hand-placed waits are checked
 * against ONE compiler's code generation (tests/test_isa_scan.py); bench.py records the string next to its numbers. */
const char *lsl_build_info(void);
const char *lsl_last_error(void);

/* LatentSIV3.__init__ counterpart: validates the shape (-> ValueError in the Python wrapper). */
int lsl_model_create(const lsl_model_desc *desc, lsl_model **out);
/* load_state_dict counterpart; pointers must stay alive while the model is used. */
int lsl_model_set_weights(lsl_model *m, const lsl_weights *w);
void lsl_model_destroy(lsl_model *m);

/* Trajectories processed per pass (cache-residency knob); 0 = library default. */
int lsl_model_set_chunk(lsl_model *m, int32_t trajectories_per_pass);

/* ParallelMLPAttentionV2's attention_mode (mmdit.py:222-229, used at mmdit.py:247 -> attention(), mmdit.py:40-53): 0 = "scaled_dot_product"
 * (the default of a new model, every shipped config), 1 = any other string = attention_linear (mmdit.py:58-72): q softmax over the head
 * channels, k softmax over the positions, out = (q hd^-1/2) (k^T v).  Replaces the reference's constructor keyword; may be changed between
 * calls (cached graphs are dropped).  Models in linear mode always take the general path (lsl_sampler_path == 0). */
int lsl_model_set_attention_mode(lsl_model *m, int32_t mode);

/* Decomposition of a ParallelMLPAttentionV2 sub-block (mmdit.py:240-249) behind the attention.  0 (default): linear1 computes q | k | v | mlp,
 * linear2 and the next LayerNorm are kernels of their own.  1: linear1 computes q | k | v only and ONE row-owning kernel (k_tail) runs the mlp
 * up-projection, GELU, linear2 over [attention | gelu(mlp)], the gated residual update and the next sub-block's LayerNorm + modulate: 8.6
 * instead of 13.2 KB of measured HBM traffic per token and sub-block at hidden 256 / mlp 1024, faster from about 10^5 tokens per pass, slower below
 * (a workgroup streams the whole weight image per 256 tokens).  The two forms are not bit-identical (other summation order in linear2 and in
 * the row statistics; same error against the fp32 reference), so the choice belongs to the MODEL HANDLE - never to the batch: a trajectory's
 * bits stay the same in any batch, shard or pass.  Returns -21 if the model has no instance (hidden 256 with heads * head_dim_pad = 256 and mlp_dim a multiple of 64).
 * Environment LSL_TAIL=1 / 0 sets the default of new handles / disables the form (A/B runs, tests). */
int lsl_model_set_tail(lsl_model *m, int32_t on);
int32_t lsl_model_tail(const lsl_model *m); /* 1 if the handle runs the tail form */

/* LayerNorm + modulate of a sub-block (latent_si_v31.py:50-51,57-58) inside linear1's activation load.  0 (default): a LayerNorm kernel writes the
 * bf16 operand `a`, linear1 reads it.  1: no LayerNorm launch - linear1 reads the fp32 residual stream, normalises and modulates its rows while
 * it turns them into MFMA fragments (1.5 KB of HBM traffic per token and sub-block less at hidden 512, measured; faster from about 10^5 tokens per pass,
 * slower at small launches).  Wherever the token-stationary linear1 runs with its modulation rows in LDS (one shared row, or >= 128 / 256 tokens
 * per trajectory at hidden <= 256 / above; the first sub-block of an evaluation when the embedding kernel can leave the statistics: hidden 256 / 512,
 * <= 32 input channels, normalize = false); elsewhere, and on handles in the tail form, the standalone kernel stays.  One more bf16 rounding of a
 * deviation-sized value than the standalone kernel: results differ at the level of the bf16 operand (same error class against the fp32
 * reference), so the choice belongs to the MODEL HANDLE, never to the batch.  Environment LSL_LN_FUSE=1 / 0: default of new handles / disabled. */
int lsl_model_set_ln_fuse(lsl_model *m, int32_t on);
int32_t lsl_model_ln_fuse(const lsl_model *m);

/* Trajectories the library processes per pass for a call of this size (<= B). */
int32_t lsl_pass_size(const lsl_model *m, int32_t B, int32_t T, int32_t L);

/* Which kernel family lsl_sample uses for trajectories of T x L tokens of this model: 0 = the general path (one launch per kernel per
 * sub-block, any shape), 1 = the trajectory-resident path (csrc/k_resident.hip.h: models of the pedestrian family - hidden 128, 4 heads
 * of 32, mlp 256 - with T*L <= 48 and T, L <= 32: one workgroup per trajectory runs whole groups of state updates in a single launch).  The answer
 * depends on the model and on T, L only, never on the batch, so a trajectory's result does not depend on what it is batched with. */
int32_t lsl_sampler_path(const lsl_model *m, int32_t T, int32_t L);

/* Bytes of caller-provided device scratch needed for a call with these sizes. */
size_t lsl_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L);

/* LatentSIV3.forward: io->out = network(io->x, io->t, io->x_cond, io->mask, io->y). */
int lsl_forward(lsl_model *m, const lsl_io *io, void *workspace, size_t workspace_bytes, void *stream);

/* The tangent pass of the network (forward mode): what Sampler.sample_ode_likelihood needs of the drift's divergence, eps . (J eps) for a
 * probe eps (modules/transport/transport.py:432-443 obtains the same scalar by autograd).  csrc/k_jvp.hip.h, DESIGN.md 6.2.
 *   io as for lsl_forward: io->t per trajectory, io->out receives the network output with the bits lsl_forward produces for the same
 *   arguments on the same handle; x_tangent, out_tangent: device f32 [B,T,L,C]; out_tangent = (d network / d x)(io->x) . x_tangent.  io->x and
 *   x_tangent are not modified.  The conditioning (t, y, x_cond, mask) has no tangent.
 *   Numerics: the tangent operands of linear1, linear2 and the two attention products are bf16 with fp32 accumulation like their primal
 *   twins, everything else fp32.  The tangent stream is linear operation by operation: a zero tangent gives zeros, and negating or doubling
 *   x_tangent negates or doubles out_tangent bit for bit.  No float atomics, fixed summation orders: a trajectory's tangent has the same bits
 *   alone, in any batch and at any pass size.
 *   The pass runs the default decomposition of the general path: a handle in the tail or ln_fuse form or in linear-attention mode is
 *   refused with -21 and a message that names the setter to call; the trajectory-resident path and hipGraph replay are not used.  Every
 *   shape lsl_forward accepts in softmax mode is accepted.  A tangent pass holds half the tokens of a forward pass (its scratch per token is
 *   about three times a forward's); the workspace is the forward's scratch of that pass size plus the tangent stream's.
 *   Returns -1 for a null pointer, -3 for B, T or L <= 0 or a workspace smaller than lsl_forward_jvp_workspace_bytes says (both before
 *   anything touches a GPU), -21 as above.  A refused call enqueues nothing. */
size_t lsl_forward_jvp_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L);
int lsl_forward_jvp(lsl_model *m, const lsl_io *io, const float *x_tangent, float *out_tangent, void *workspace, size_t workspace_bytes,
                    void *stream);
/* out[b] = sum_e a[b,e] * b[b,e] over per_trajectory elements (device f32 in, device f64 [B] out): fp64 sums of the exact fp32 products in a
 * fixed order (slabs of LSL_SI_SLAB elements, then the slab partials in order; no atomics): a trajectory's bits are the same in any batch.
 * scratch: device, at least B * ceil(per_trajectory / LSL_SI_SLAB) doubles.  B <= 65535, per_trajectory <= 2^31. */
int lsl_dot_rows(const float *a, const float *b, int32_t B, uint64_t per_trajectory, double *out, void *scratch, size_t scratch_bytes,
                 void *stream);

/* Stochastic-interpolant objective without gradients: Transport.training_losses (modules/transport/transport.py:116-156), the loss every
 * validation_step evaluates through Loss.forward (second_stage/md17.py:221) before it samples.  For every path (path.py:21-206), prediction
 * and loss weight the reference's loss of trajectory b is affine in three arrays; one record per trajectory carries the coefficients:
 *      xt     = alpha x1 + sigma x0                                            (path.py:124-134, ICPlan.compute_mu_t)
 *      r      = p pred + q1 x1 + q0 x0,      loss_b = w mean_{T,L,C}(r^2)       (transport.py:135-154, mean_flat)
 *   velocity: p = 1, q1 = -d_alpha, q0 = -d_sigma, w = 1        data:  p = 1, q1 = -1, q0 = 0, w = 1
 *   noise:    p = 1, q1 = 0, q0 = -1, w = W                     score: p = sigma, q1 = 0, q0 = 1, w = W
 *   W = 1 | (drift_var / sigma)^2 | drift_var / sigma^2 for loss_weight None | "velocity" | "likelihood"
 * lam_slide_amd/transport.py derives the records in float64 (Transport.si_rows).  Sums run in a fixed order (slabs of LSL_SI_SLAB elements
 * of one trajectory, no atomics): a trajectory's loss has the same bits in any batch, shard or pass. */
typedef struct lsl_si_row { float alpha, sigma, p, q1, q0, w; } lsl_si_row;
#define LSL_SI_SLAB 4096
/* lsl_workspace_bytes of the same sizes + one float per trajectory and slab. */
size_t lsl_si_loss_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L);
/* Transport.training_losses on given draws: io->x receives xt, io->t = device [B] times, io->out receives pred = network(xt, t, x_cond, mask, y)
 * exactly as lsl_forward computes it; x1, x0 device [B,T,L,C]; rows device [B]; loss device [B].  A refused call enqueues nothing. */
int lsl_si_loss(lsl_model *m, const lsl_io *io, const float *x1, const float *x0, const lsl_si_row *rows, float *loss,
                void *workspace, size_t workspace_bytes, void *stream);
/* The reduction alone, for predictions that came from somewhere else (any callable that left its output on the GPU, tests):
 * loss[b] = w_b mean(r^2) over the per_trajectory elements of trajectory b.  scratch: device, at least
 * B * ceil(per_trajectory / LSL_SI_SLAB) floats. */
int lsl_si_reduce(const float *pred, const float *x1, const float *x0, const lsl_si_row *rows, int32_t B, uint64_t per_trajectory,
                  float *loss, void *scratch, size_t scratch_bytes, void *stream);

/* Geometry losses of the decoded positions: what Loss.forward adds behind the SI term when calc_additional_losses is set
 * (second_stage/md17.py:231-255, nba.py, pedestrian.py alike) - MaskedMSELoss, MaskedNormLoss and InterDistanceLoss of modules/losses.py.
 * pred, target: device f32 [F, A, D] (F = B*T frames); mask: device u8 [F, A], nonzero = real entity.  Native form: 1 <= D <= 4, A <= 2048
 * (anything else is refused with -3; the binding's Loss takes its torch path then).  sums: device f32 [F, 5], per frame
 *      s_mse = sum_a m_a mean_d (p - t)^2,  s_norm = sum_a m_a ||p_a - t_a||,  n = sum_a m_a,
 *      s_pair = sum_ij m_i m_j (||p_i - p_j|| - ||t_i - t_j||)^2,  n_pair = n^2
 * with distances taken from coordinate differences; no [A, A] array exists in memory.  Masked-out entities are skipped, where the reference
 * multiplies by the mask: the results differ only when a masked-out position is not finite.  No atomics, every sum in an order fixed by
 * (A, D): a frame's five floats have the same bits in any batch or shard.  Nothing is allocated; a refused call enqueues nothing. */
int lsl_geom_loss_sums(const float *pred, const float *target, const uint8_t *mask, int32_t F, int32_t A, int32_t D, float *sums, void *stream);
/* out (device f32 [3]) = pos_loss, dist, inter_dist_loss = sum s_mse / sum n, sum s_norm / sum n, sum s_pair / sum n_pair over the F rows of sums
 * in index order, in fp64, each rounded once (rows of several shards may be concatenated first); no real entity at all: NaN, as the reference. */
int lsl_geom_loss_final(const float *sums, int32_t F, float *out, void *stream);

/* Frame-local and torsion losses of the decoded peptide positions: the two terms of the peptide Loss.forward (second_stage/peptide.py:293-378)
 * that lsl_geom_loss_sums with entities = (residue, atom), A = R*14, D = 3 does not compute.  F = B*T frames of R residues, all device, row-major:
 *   pred, target_frame  f32 [F, R, 14, 3]   decoded atom14 positions; the dataset's positions in each residue's backbone frame
 *   atom14_mask         u8  [F, R, 14]      nonzero = real atom
 *   tors_target         f32 [F, R, 7, 2]    (sin, cos) of pre-omega, phi, psi, chi1..4;   tors_mask u8 [F, R, 7], nonzero = counted
 *   aatype              i64 [F, R]          residue types 0..20 (20 = unknown), as the batch holds them
 *   restab              i8  [21, 20]        per residue type the atom14 index of atom37 slots 0, 1, 2, 4, then of the 4 x 4 chi atoms;
 *                                           -1 = a slot the atom37 mask of the type zeroes (its position is 0).  Entries are in -1..13.
 * sums: device f32 [F, 4], per frame
 *      s_frame = sum_ra m_ra mean_d (local(pred)_rad - target_frame_rad)^2,   n = sum_ra m_ra,   s_tors = sum_rk w_rk l_rk,   n_tors = sum_rk w_rk
 * local(p) = p in the residue's backbone frame: Gram-Schmidt on (C, CA, N) = atom14 slots 2, 1, 0 with eps 1e-8, x and z flipped, origin CA
 * (modules/geometry.py:212-227, utils/rigid_utils.py:1093-1134).  Torsion k takes four atom37 positions of the residue and the one before it
 * (zeros in front of residue 0), the frame of the first three and (sin, cos) = (z, y) / sqrt(z^2 + y^2 + 1e-8) of the fourth, negated for psi
 * (peptide.py:170-286).  kind 0: l = 1 - cosine_similarity(pred, target) (MaskedCosineLoss; each vector over max(norm, 1e-8));
 * kind 1: l = 1 - pred . target (MaskedCosineLossV2).  fp32 throughout.
 * Masked-out atoms and torsions are skipped, where the reference multiplies by the mask: the results differ only when a masked-out value is
 * not finite.  An aatype outside 0..20 makes the four sums of its frame NaN (nothing is clamped, no table row is read with it).
 * Native form: 1 <= R <= 146 (R*14 <= 2048, the entities of lsl_geom_loss_sums); anything else is refused with -3, as is kind outside {0, 1}
 * (the binding's PeptideLoss takes its torch path then).  No atomics, every sum in an order fixed by R: a frame's four floats have the
 * same bits in any batch, shard or position.  Nothing is allocated; a refused call enqueues nothing. */
int lsl_peptide_loss_sums(const float *pred, const float *target_frame, const uint8_t *atom14_mask, const float *tors_target, const uint8_t *tors_mask,
                          const int64_t *aatype, const int8_t *restab, int32_t F, int32_t R, int32_t kind, float *sums, void *stream);
/* out (device f32 [5]) = pos_loss, pos_frame_loss, inter_distance_loss, norm_loss, torsion_loss
 *   = sum s_mse / sum n, sum s_frame / sum n, sum s_pair / sum n_pair, sum s_norm / sum n, sum s_tors / sum n_tors
 * over the F rows of geom_sums [F, 5] (lsl_geom_loss_sums with A = R*14, D = 3, mask = atom14_mask) and pept_sums [F, 4], in index order, in
 * fp64, each rounded once (rows of several shards may be concatenated first); 0 / 0 is NaN, as the reference. */
int lsl_peptide_loss_final(const float *geom_sums, const float *pept_sums, int32_t F, float *out, void *stream);

/* Class losses of the first-stage decoder heads: the cross-entropy terms of the first-stage Loss classes - MaskedCrossEntropyLoss on the atom
 * types (modules/losses.py:62-72, first_stage/md17.py:176-178) and nn.CrossEntropyLoss on team / group / aatype (first_stage/nba.py:266-267,
 * peptide.py:443).  logits: device f32 [F, A, K]; target: device i64 [F, A]; mask: device u8 [F, A], nonzero = counted, or NULL;
 * 0 <= label_smoothing < 1.  Per row, in fp32 (torch's definition):
 *      lse = max_k l_k + log sum_k exp(l_k - max),  nll = lse - l_y,  smooth = lse - mean_k l_k,  loss = (1 - eps) nll + eps smooth
 * sums: device f32 [F, 2], per frame
 *      s_ce = sum of loss over the counted rows: mask nonzero (or mask NULL) and target != -100
 *      n    = with a mask the rows whose mask is nonzero (MaskedCrossEntropyLoss divides by mask.sum(); an ignored row adds 0 above),
 *             with NULL the rows whose target != -100 (nn.CrossEntropyLoss takes the mean over the non-ignored rows)
 * Masked-out rows are skipped, where the reference multiplies by the mask: the results differ only when a masked-out logit is not finite.
 * A counted row whose target is < 0 (and not -100) or >= K makes both sums of its frame NaN and touches nothing else (nothing is clamped, no
 * logit is read with it); torch raises there.
 * confusion: device i64 [K, K] or NULL, zeroed by the caller: every counted row with a target in range and no NaN logit adds one to cell
 * [target, argmax], the argmax being the lowest index among equal maxima.  Integer atomics only (exact in any order): several calls accumulate.
 * Native form: 1 <= K <= LSL_CLS_MAX_K, A >= 1; anything else is refused with -3.  No float atomics, every sum in an order fixed by (A, K):
 * a frame's two floats have the same bits in any batch, shard or position.  Nothing is allocated; a refused call enqueues nothing. */
int lsl_class_loss_sums(const float *logits, const int64_t *target, const uint8_t *mask, int32_t F, int32_t A, int32_t K, float label_smoothing,
                        float *sums, int64_t *confusion, void *stream);
/* out (device f32 [1]) = sum s_ce / sum n over the F rows of sums in index order, in fp64, rounded once (rows of several shards may be
 * concatenated first); 0 / 0 is NaN, as the reference. */
int lsl_class_loss_final(const float *sums, int32_t F, float *out, void *stream);

/* Displacement errors of the decoded positions: the evaluation tail of the trajectory models.  validation_step (second_stage/md17.py:82-86,
 * nba.py:100-104, pedestrian.py:88-92): ade = norm(true - pred, dim=-1).mean(dim=(1, 2)), fde = norm(true[:, -1] - pred[:, -1], dim=-1).mean(dim=1)
 * over the future frames and ALL entities; test_step (nba.py:182-225, pedestrian.py:170-212): per real agent the error [K, Tf] = norm(traj -
 * target), ADE = its mean over the frames, FDE = its last frame, each minimised on its own over the first num_runs samples.
 *   pred    device f32 [K, B, Tp, A, D]   the decoder's output of K samples of B scenes, as it left it; frames t0p .. t0p + Tf - 1 are read
 *   target  device f32 [B, Tt, A, D]      the batch's positions; frames t0t .. t0t + Tf - 1 are read (the full pos with t0t = cond_idx[1],
 *                                         or the future frames alone with t0t = 0: the same call, no slice is copied)
 *   rows    device f32 [K, B, A, 2]       per sample and agent (sum_t e_t / Tf, e_{Tf-1}),  e_t = sqrt(sum_d (pred - target)^2)
 *   traj    device f32 [K, B, 2] or NULL  per sample (sum_a sum_t e_t / (Tf A), sum_a e_{Tf-1} / A): the two validation_step lines
 * Native form: 1 <= D <= 4, A >= 1, Tf >= 1, 0 <= t0p, t0p + Tf <= Tp, 0 <= t0t, t0t + Tf <= Tt, K * B < 2^24 (a grid of K * B workgroups of 256 threads stays below 2^32 threads); anything else is refused with
 * -3 (the binding's displacement_errors takes its torch path for D > 4).  Indices are 64-bit: K*B*Tp*A*D may pass 2^31.  fp32 with correctly
 * rounded sqrt and division; no atomics; frames added in ascending order per agent, a thread's agents in ascending order, the wave by DPP,
 * the waves in wave order - every order fixed by (A, D, Tf): the floats of a sample trajectory have the same bits in any batch or shard.
 * Nothing is allocated, nothing is synchronised; a refused call enqueues nothing. */
int lsl_disp_error_rows(const float *pred, const float *target, int32_t K, int32_t B, int32_t Tp, int32_t t0p, int32_t Tt, int32_t t0t, int32_t Tf,
                        int32_t A, int32_t D, float *rows, float *traj, void *stream);
/* agents (device f32 [B, A, 2]) = the minimum over samples k = 0 .. num_runs - 1 (ascending) of the two columns of rows [K, B, A, 2], each on
 * its own; a NaN of any of those samples gives NaN (torch.min); quiet NaN where mask (device u8 [B, A], NULL = all agents real) is 0.
 * totals (device f64 [5], written, not accumulated) = sum minADE, sum minFDE, n over the real agents in (b, a) order, then the sums of the two
 * columns of traj [K, B, 2] over its first num_runs * B rows (0 when traj is NULL), in fp64 in index order: totals of several batches or
 * shards add before the division (on_test_epoch_end, nba.py:240-245).  1 <= num_runs <= K, else -3. */
int lsl_disp_error_final(const float *rows, const float *traj, const uint8_t *mask, int32_t K, int32_t num_runs, int32_t B, int32_t A, float *agents,
                         double *totals, void *stream);

/* Torsion statistics of a sampled peptide trajectory: what analyze_trajectory (eval_peptide.py:102-182) computes from the torsion features of
 * the sampled and the MD trajectory - histograms of every torsion and of chosen pairs, their Jensen-Shannon distances, and the lagged
 * products the decorrelation curves are made of.  Four independent calls; device pointers unless named host; nothing is allocated, nothing is
 * synchronised, a refused call enqueues nothing.  No float atomics: counts are integers added by integer atomics (exact in any order), every
 * float is a sum in a fixed order that does not depend on the grid, the batch or the position in the batch.
 *
 * lsl_dihedral_angles: angles [F, Q] f32 (radians, [-pi, pi]) of the Q atom quadruples of each of F frames pos [F, A, 3] f32,
 *   angle = atan2((b1 . c1) |b2|, c1 . c2),  b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, c1 = b2 x b3, c2 = b1 x b2   (fp32, every product and
 *   sum rounded on its own, in that order).  quads i32 [Q, 4] indexes the A atom slots of a frame - a general table, not a fixed set of
 *   torsions; quads_host is the same table in HOST memory: it is what the range check reads (an index outside 0..A-1: -3, before any launch;
 *   the device copy is the caller's to keep equal, an index outside the frame there gives NaN).  1 <= A <= 2044 (146 residues of 14 atoms: a
 *   frame in LDS), 1 <= Q <= 65536, F >= 1. */
int lsl_dihedral_angles(const float *pos, const int32_t *quads, const int32_t *quads_host, int64_t F, int32_t A, int32_t Q, float *angles,
                        void *stream);
/* lsl_histogram: counts i64 [S, Q, bins] += np.histogram(x[s, :, q], bins=edges)[0] of x [S, n, Q] f32, and for P > 0 counts2 i64 [S, P,
 *   bins2, bins2] += np.histogram2d(x[s, :, pairs[p][0]], x[s, :, pairs[p][1]], bins=(edges2a, edges2b))[0].  The tables are ADDED TO: zero
 *   them before the first call, chunks of a trajectory then accumulate exactly.  edges f64 [bins + 1], edges2a / edges2b f64 [bins2 + 1]:
 *   ascending edge tables, np.linspace(lo, hi, bins + 1) for the range= form.  A value is binned by comparison against the fp64 table (a
 *   multiply-and-floor estimate, then a walk against the table, as numpy corrects its own estimate): bin i holds edges[i] <= v < edges[i + 1],
 *   the last bin is closed on the right, values outside [edges[0], edges[bins]] and NaN are dropped, a pair is dropped when either coordinate
 *   is.  Given the same float32 values the counts equal numpy's as integers.  pairs i32 [P, 2] column indices, pairs_host the same table in
 *   HOST memory (checked: outside 0..Q-1 is -3).  1 <= bins <= 2048, 1 <= bins2 <= 90 (bins2^2 <= 8192 LDS cells), S <= 65535, P <= 65535.
 *   Overflow: a call adds at most n < 2^31 to a count; an int64 count overflows only after 2^63 samples in all - the caller's sum of n. */
int lsl_histogram(const float *x, int32_t S, int32_t n, int32_t Q, const double *edges, int32_t bins, int64_t *counts, const int32_t *pairs,
                  const int32_t *pairs_host, int32_t P, const double *edges2a, const double *edges2b, int32_t bins2, int64_t *counts2, void *stream);
/* lsl_lag_products: ac f32 [S, C, nlag + 1], ac[s, c, k] = (sum_{t < n - k} x[s, t, c] x[s, t + k, c]) / (n - k) of x [S, n, C] f32
 *   = statsmodels acovf(x, demean=False, adjusted=True, nlag=nlag).  A workgroup owns (series, channel, 256 lags, a segment of chunks of 448
 *   time steps); within a chunk a lag's terms are added in t order by fp32 fused multiply-adds (the longest fp32 addition chain is m = 448),
 *   chunks and segments in order in fp64, one division, one rounding to fp32: |error| <= (m + 8) 2^-24 for |x| <= 1.  The split is a function
 *   of (n, nlag) alone: a series' row has the same bits alone and inside a batch.  0 <= nlag < n (else -3), nlag + 1 <= 2^21, S * C <= 65535.
 *   workspace: lsl_lag_products_workspace_bytes(S, n, C, nlag) bytes of device memory (fp64 segment sums; 0 for a refused shape); -4 if
 *   workspace_bytes is smaller. */
size_t lsl_lag_products_workspace_bytes(int32_t S, int32_t n, int32_t C, int32_t nlag);
int lsl_lag_products(const float *x, int32_t S, int32_t n, int32_t C, int32_t nlag, float *ac, void *workspace, size_t workspace_bytes, void *stream);
/* lsl_js_distance: out f64 [rows] = scipy.spatial.distance.jensenshannon(counts_a[r], counts_b[r]) of two non-negative i64 tables [rows, bins]
 *   (a flattened 2-D table is a row): p, q = the rows over their sums, m = (p + q) / 2, sqrt((sum rel_entr(p, m) + sum rel_entr(q, m)) / 2),
 *   natural log, rel_entr(0, .) = 0, the bins added in index order in fp64.  A row that is all zero on either side gives NaN (0 / 0), as scipy. */
int lsl_js_distance(const int64_t *counts_a, const int64_t *counts_b, int32_t rows, int32_t bins, double *out, void *stream);

/* Structure statistics of a sampled peptide trajectory: what SIAtom14SampleCallback logs per validation epoch through traj_analysis
 * (utils/traj_utils.py:63-103, utils/backbone_utils.py, utils/tica_utils.py:12-39) - pair distances, the radius of gyration, the clash /
 * bond-break validity and the contact counts of the selected (C-alpha) atoms, histograms with one edge table per column and the
 * Jensen-Shannon distance of density histograms.  Four independent calls; device pointers unless named host; nothing is allocated, nothing
 * is synchronised, a refused call enqueues nothing.  No float atomics: counts are integers added by integer atomics (exact in any order),
 * every float is a sum in a fixed order that depends on the shape alone - a frame has the same bits alone and inside any batch.
 *
 * lsl_pair_distances: dist [F, P] f32 of the P atom pairs of each of F frames pos [F, A, 3] f32,
 *   dist[f, p] = sqrtf((dx dx + dy dy) + dz dz),  d = pos[f, pairs[p][0]] - pos[f, pairs[p][1]]   (fp32, every operation rounded on its own, in
 *   that order: np.linalg.norm(.., axis=-1) on float32).  pairs i32 [P, 2] indexes the A atom slots of a frame - a general table; pairs_host
 *   is the same table in HOST memory: it is what the range check reads (an index outside 0..A-1: -3, before any launch; the device copy is
 *   the caller's to keep equal, an index outside the frame there gives NaN and reads nothing).  1 <= A <= 2044 (a frame in LDS),
 *   1 <= P <= 65536, F >= 1. */
int lsl_pair_distances(const float *pos, const int32_t *pairs, const int32_t *pairs_host, int64_t F, int32_t A, int32_t P, float *dist,
                       void *stream);
/* lsl_ca_frame_stats: statistics of the R selected atoms sel i32 [R] (sel_host: the same table in HOST memory, range-checked: outside 0..A-1
 *   is -3; a device entry outside the frame stages NaN and reads nothing) of each of F frames pos [F, A, 3] f32; d_ij below is the fp32
 *   distance of lsl_pair_distances between selected atoms i and j.  Each output may be NULL.
 *   rg       f32 [F] = sqrt(mean_i |x_i - mean_j x_j|^2): fp64 from the fp32 coordinates, atoms in sel order (three coordinate sums over R,
 *            one division each; then the sum over i of (dx dx + dy dy) + dz dz, one division by R, one square root), rounded to fp32 once:
 *            mdtraj.compute_rg with unit masses.
 *   flags    i32 [F]: bit 0 if some i < j has d_ij < clash_thr, bit 1 if some d_{i,i+1} > break_thr; NaN compares false on both, as numpy
 *            (compute_validity: a frame is valid when flags is 0).
 *   tally    i64 [4] += (frames, frames with bit 0, frames with bit 1, frames with neither).
 *   contacts i64 [R, R] += for i < j only the number of frames with d_ij < contact_thr (compute_contact_matrix times the frames); cells
 *            with i >= j are untouched.
 *   tally and contacts are ADDED TO: zero them before the first call, chunks of a trajectory then accumulate exactly.  1 <= R <= 146,
 *   A >= 1, F >= 1. */
int lsl_ca_frame_stats(const float *pos, const int32_t *sel, const int32_t *sel_host, int64_t F, int32_t A, int32_t R, float clash_thr,
                       float break_thr, float contact_thr, float *rg, int32_t *flags, int64_t *tally, int64_t *contacts, void *stream);
/* lsl_histogram_columns: counts i64 [Q, bins] += np.histogram(x[:, q], bins=edges[q])[0] of x [n, Q] f32 with edges f64 [Q, bins + 1], one
 *   ascending table per column (compute_js_distance's np.linspace(ref_col.min(), ref_col.max(), .)).  Binning as lsl_histogram, against the
 *   column's own table: bin i holds edges[q][i] <= v < edges[q][i + 1], the last bin is closed on the right, values outside the table and
 *   NaN are dropped; given the same float32 values the counts equal numpy's as integers.  The table is ADDED TO.  1 <= bins <= 2048,
 *   n >= 1, Q >= 1 (at most 65535 column tiles of floor(4096 / (bins + 1)) columns). */
int lsl_histogram_columns(const float *x, int32_t n, int32_t Q, const double *edges, int32_t bins, int64_t *counts, void *stream);
/* lsl_js_distance_density: out f64 [rows] = scipy.spatial.distance.jensenshannon(h_a[r], h_b[r]) of the density histograms
 *   h[i] = (counts[r, i] / measure[r, i]) / N + pseudo, N the row's total count (exact, int64): numpy's density=True, n / db / n.sum(), plus
 *   discretize_features' pseudo-count.  counts_a, counts_b i64 [rows, bins]; measure f64 [rows, bins] the cell sizes - np.diff(edges) for
 *   a 1-D row, the flattened outer product of the two np.diff s for a 2-D table.  Then as lsl_js_distance: both rows over their sums (the
 *   sums added in bin order in fp64), m = (p + q) / 2, sqrt((sum rel_entr(p, m) + sum rel_entr(q, m)) / 2), the terms added in bin order
 *   in fp64.  A row with N = 0 on either side (0 / 0) or a zero cell size gives NaN, as the same arithmetic in numpy. */
int lsl_js_distance_density(const int64_t *counts_a, const int64_t *counts_b, const double *measure, int32_t rows, int32_t bins, double pseudo,
                            double *out, void *stream);

/* TICA and state statistics of the peptide evaluation: the second half of analyze_trajectory (eval_peptide.py:189-288, modules/analysis.py:36-56)
 * behind the cos / sin torsion features - the lagged second moments a TICA model is estimated from, the projection with its running ranges,
 * the nearest-centre assignment of kmeans.transform / analysis.discretize and the sliding-window transition counts of estimate_markov_model.
 * Four independent calls; device pointers; nothing is allocated, nothing is synchronised, a refused call enqueues nothing.  No float atomics:
 * integer atomics for counts and for minimum / maximum only, every float a sum in a fixed order that depends on the shape alone.
 *
 * lsl_lagged_moments: moments f64 [S, 2 F + 3 F^2] of x [S, n, F] f32 at lag, m = n - lag: per series sx [F] = sum_{t<m} x_t, sy [F] =
 *   sum_{t<m} x_{t+lag}, xx [F, F] = sum x_t x_t^T, yy [F, F] = sum x_{t+lag} x_{t+lag}^T, xy [F, F] = sum x_t x_{t+lag}^T, in that order, full
 *   row-major matrices.  Products in fp64 from the fp32 values (exact), added in fp64 in ascending t within a segment of 1024 time steps
 *   (segment g: t in [1024 g, 1024 (g + 1)) below m - a function of (n, lag) alone), segments in segment order; each of the five a direct sum
 *   over its own window: |error| <= (1024 + segments + 2) 2^-53 sum_t |x_a x_b|.  xx and yy are bit-symmetric; a series has the same bits
 *   alone and inside a batch.  1 <= F <= 128, n >= 2, 1 <= lag < n, S <= 65535 (else -3).  workspace: lsl_lagged_moments_workspace_bytes(S, n,
 *   F, lag) bytes of device memory (the fp64 segment sums: S * segments * (2 F + 3 F^2) * 8; 0 for a refused shape); -4 if smaller. */
size_t lsl_lagged_moments_workspace_bytes(int32_t S, int32_t n, int32_t F, int32_t lag);
int lsl_lagged_moments(const float *x, int32_t S, int32_t n, int32_t F, int32_t lag, double *moments, void *workspace, size_t workspace_bytes,
                       void *stream);
/* lsl_project: y f32 [n, d], y[t, j] = fp32(sum_f (x[t, f] - mean[f]) W[f, j]) of x [n, F] f32, mean f64 [F], W f64 [F, d]: the subtraction and
 *   the fused chain over f ascending in fp64, one rounding to fp32.  lim (or NULL): f32 [2, d], in and out: lim[0, j] = min(lim[0, j], min_t
 *   y[t, j]), lim[1, j] = max(lim[1, j], max_t y[t, j]), NaN values of y ignored - by integer atomics on an order-preserving key of the float
 *   (the table holds keys while the call runs), so the result has no order dependence; start it at (+inf, -inf); lim itself must hold no NaN.
 *   Two calls with one table give the joint ranges of two trajectories (eval_peptide.py:203-207) with no read-back.  1 <= F <= 128,
 *   1 <= d <= 16, n >= 1. */
int lsl_project(const float *x, int32_t n, int32_t F, const double *mean, const double *W, int32_t d, float *y, float *lim, void *stream);
/* lsl_assign_centers: labels i32 [n], labels[t] = argmin_c sum_j (y[t, j] - centers[c, j])^2 of y [n, d] f32 and centers [k, d] f32
 *   (kmeans.transform): differences and the fused sum over j ascending in fp64, ties to the lowest index as np.argmin; a row that holds a NaN
 *   gets -1.  map (or NULL) i32 [k]: the label is map[argmin] (msm.metastable_assignments[...]), -1 when that is outside 0..nstates-1.
 *   state_counts (or NULL) i64 [nstates] += the rows of each label in 0..nstates-1 (added to: chunks accumulate; the occupancies as exact
 *   integers).  The centres stay in LDS: k <= 1024, d <= 64, k * d <= 8192; nstates 1..1024 when map or state_counts is given (ignored
 *   otherwise). */
int lsl_assign_centers(const float *y, int32_t n, int32_t d, const float *centers, int32_t k, const int32_t *map, int32_t nstates, int32_t *labels,
                       int64_t *state_counts, void *stream);
/* lsl_transition_counts: counts i64 [S, nstates, nstates] += #{t < n - lag : dtraj[s, t] = i, dtraj[s, t + lag] = j} of dtraj i32 [S, n]: the
 *   sliding-window count matrix of estimate_markov_model(dtraj, lag).  A pair with either label outside 0..nstates-1 (the -1 of
 *   lsl_assign_centers) is skipped.  The table is ADDED TO.  lag >= n adds nothing and returns 0.  lag >= 1, 1 <= nstates <= 128 (int32 counts
 *   of a workgroup in LDS), S <= 65535. */
int lsl_transition_counts(const int32_t *dtraj, int32_t S, int32_t n, int32_t lag, int32_t nstates, int64_t *counts, void *stream);

/* Koopman-reweighted TICA on wide feature tables: run_tica of the peptide validation (utils/tica_utils.py:42-48) over tica_features, whose
 * 300 .. 1344 columns are past the 128 of lsl_lagged_moments / lsl_project.  Three independent calls on one series; device pointers; nothing is
 * allocated, nothing is synchronised, a refused call enqueues nothing.  No float atomics.
 *
 * lsl_weighted_moments: moments f64 [1 + 2 F + 3 F^2] of x [n, F] f32 at lag, m = n - lag, with the weights w f64 [m] (NULL: all ones; negative
 *   weights are legal): sw = sum_{t<m} w_t, sx [F] = sum w_t x_t, sy [F] = sum w_t x_{t+lag}, xx [F, F] = sum w_t x_t x_t^T, yy [F, F] =
 *   sum w_t x_{t+lag} x_{t+lag}^T, xy [F, F] = sum w_t x_t x_{t+lag}^T, in that order, full row-major matrices.
 *   Order.  A row is extended by a virtual column of ones, so sw, sx and sy are sums of the same kind as the matrix entries.  Entry (a, b), a <= b
 *   for xx and yy: p_t = w_t * (double)x_a (one rounding; exact for NULL), then acc = fma(p_t, (double)x_b, acc) over the rows of a segment in
 *   ascending t from zero (segment g: t in [1024 g, 1024 (g + 1)) below m); the segments' sums are added in ascending g to a second accumulator,
 *   which is added to the split's sum and cleared after every segment with (g + 1) % 1024 == 0 and at the end of a time split; time split s holds the
 *   segments [s q, (s + 1) q), q = ceil(segments / want), want = min(32, ceil(1024 / jobs), segments), jobs = Te (Te + 1) + T^2, Te = ceil((F + 1) /
 *   64), T = ceil(F / 64); the splits' sums are added in ascending s.  All of it is a function of (n, lag, F) alone: the bits of every output depend
 *   on (x, w, n, lag, F) only.  xx[b, a] and yy[b, a] are copies of entry (a, b): bit-symmetric.  At most LSL_WMOM_CHAIN = 4130 roundings lie on the
 *   path to an entry (1 + 1024 + 1024 + 2049 + 32, every n < 2^31): |error| <= 4130 * 2^-53 * sum_t |w_t x_a x_b|.  A NaN in a row reaches only
 *   the entries that row's value enters.
 *   129 <= F <= 2048, n >= 2, 1 <= lag < n (else -3; F <= 128 is lsl_lagged_moments').  workspace: lsl_weighted_moments_workspace_bytes(n, F, lag)
 *   bytes = splits * 3 (F + 1)^2 * 8 (at most 32 splits, one at F = 2048: 101 MB; independent of n beyond that; 0 for a refused shape); -4 if smaller.
 * lsl_affine_weights: w f64 [m], w[t] = (sum_f x[t, f] u[f]) + c of x [m, F] f32 (row stride F), u f64 [F]: the fused chain over f ascending in
 *   fp64 from zero, c added last.  1 <= F <= 2048, m >= 1.  The Koopman weights of the first m rows of a series.
 * lsl_project_wide: lsl_project's contract - y f32 [n, d], y[t, j] = fp32(sum_f (x[t, f] - mean[f]) W[f, j]), the subtraction and the fused chain
 *   over f ascending in fp64 from zero, one rounding to fp32; lim (or NULL) f32 [2, d] in and out, as there - for 129 <= F <= 2048, 1 <= d <= 64,
 *   n >= 1.  W streams through LDS in chunks of 32 features in ascending order: a row has the bits of the formula evaluated sequentially. */
size_t lsl_weighted_moments_workspace_bytes(int32_t n, int32_t F, int32_t lag);
int lsl_weighted_moments(const float *x, int32_t n, int32_t F, int32_t lag, const double *w, double *moments, void *workspace, size_t workspace_bytes,
                         void *stream);
int lsl_affine_weights(const float *x, int32_t m, int32_t F, const double *u, double c, double *w, void *stream);
int lsl_project_wide(const float *x, int32_t n, int32_t F, const double *mean, const double *W, int32_t d, float *y, float *lim, void *stream);

/* k-means fitting: S independent Lloyd problems y [S, n, d] f32 -> centers [S, k, d] f32 - the microstates of the peptide evaluation
 * (modules/analysis.py:42-44: S = 1, n ~ 10^6, k = 100) and the post_process branch of the NBA / pedestrian test_step (second_stage/nba.py:202-203,
 * 228-238: one problem per agent over its K final frames, k = num_runs).  Device pointers; nothing is allocated, nothing is synchronised, a
 * refused call enqueues nothing.  No float atomics (integer ones for the changed-label count only).  The seeding is the caller's: centers holds
 * the initial centres.  The algorithm is fixed here as mathematics; parity with pyemma's or torch_kmeans' own streams is not claimed.
 *
 * lsl_kmeans_step: one Lloyd iteration of every series whose done[s] is 0 (update != 0), or the final assignment of every series (update == 0).
 *   assign   labels[s, t] = the lowest c that minimises sum_j (y[s, t, j] - centers[s, c, j])^2 - the arithmetic of lsl_assign_centers (fp64
 *            differences, the fused sum over j ascending, strict <); a row that holds a NaN gets -1 and takes no part in sums, counts or inertia.
 *            labels i32 [S, n] is in and out: the previous labels are compared with the new ones (fill it with -2 before the first step).
 *   update   sum[c, j] over the rows labelled c in fp64: rows ascending in t within a segment of 2048 rows (segment g: t in [2048 g, 2048 (g + 1)),
 *            a function of n alone), segments in segment order; centers[s, c, j] = fp32(sum / count), one fp64 division and one rounding; an
 *            empty cluster keeps its centre bit for bit.  counts i64 [S, k]: the members of this assignment, exact.
 *   state    f64 [S, 4] = (iterations done, J, J of the iteration before, sum (new - old)^2 of the centres); J = the fp64 sum of the winning
 *            squared distances of this assignment, against the centres before the update, in an order fixed by (n, d, k).  Start it at zeros.
 *   done     i32 [S]: set after an iteration when no label changed, or rel_tol > 0 and |J_prev - J| <= rel_tol J_prev from the second iteration
 *            on, or center_tol > 0 and the shift <= center_tol^2.  A later call with update != 0 touches no buffer of such a series, so
 *            max_iter calls are enqueued with no host synchronisation.  update == 0 ignores done, leaves centers alone and writes labels, counts
 *            and state[s, 1] = J of the final centres.
 *   A series has the same bits alone, inside any batch and wherever it stands in it.  k <= 1024, d <= 64, k * d <= 8192 (the centres stay in
 *   LDS), n >= 1, 1 <= S <= 65535, tolerances >= 0 (else -3).  workspace: lsl_kmeans_workspace_bytes(S, n, d, k) bytes = S * segments *
 *   (8 (k d + 1) + 4 (k + 1)), segments = ceil(n / 2048); 0 for a refused shape; -4 if smaller.
 * lsl_kmeans_nearest_rows: rows i32 [S, k], rows[s, c] = the lowest t that minimises sum_j (y[s, t, j] - centers[s, c, j])^2 (same arithmetic);
 *   rows that hold a NaN are skipped; -1 when the series has no finite row.  The sample nearest each centre: what post_process selects. */
size_t lsl_kmeans_workspace_bytes(int32_t S, int32_t n, int32_t d, int32_t k);
int lsl_kmeans_step(const float *y, int32_t S, int32_t n, int32_t d, float *centers, int32_t k, int32_t *labels, int64_t *counts, double *state,
                    int32_t *done, int32_t update, double rel_tol, double center_tol, void *workspace, size_t workspace_bytes, void *stream);
int lsl_kmeans_nearest_rows(const float *y, int32_t S, int32_t n, int32_t d, const float *centers, int32_t k, int32_t *rows, void *stream);

/* Reversible maximum-likelihood Markov state models: what estimate_markov_model does behind the count matrix (eval_peptide.py:245-288,
 * modules/analysis.py:47-56: the microstate model, the coarse model and the sampled trajectory's model of every peptide).  S independent count
 * matrices, one resident workgroup each; device pointers; nothing is allocated, nothing is synchronised, a refused call enqueues nothing.  No
 * atomics.  The estimator is fixed here as mathematics; parity with a live pyemma is not claimed.
 *
 * For one count matrix C i64 [ns, ns] (an entry <= 0 counts as 0, the total below 2^53):
 *   active set A   the largest strongly connected component (by states) of the graph i -> j where C_ij > 0; a component of one state counts
 *                  only if C_ii > 0; among components of equal size the one holding the lowest state index; no candidate: A empty.
 *   restriction    C~ = C[A, A], c_i = sum_j C~_ij, K = C~ + C~^T (counts between A and the rest are dropped).
 *   iteration      x0_i = sum_j K_ij / sum_ij K_ij (from exact integers, one division).  Step: q_i = c_i / x_i, y_i = sum_{j : K_ij != 0}
 *                  K_ij / (q_i + q_j), x'_i = y_i / sum_i y_i, err = max_i |x_i - x'_i| / ((x_i + x'_i) / 2).  The step is counted, then the
 *                  series stops when !(err > maxerr) or when the count reaches maxiter (maxerr < 0 never stops early).
 *   result         pi = x; X_ij = K_ij / (q_i + q_j) (0 where K_ij = 0), T_ij = X_ij / sum_j X_ij.  |A| = 1: T = [1], pi = [1], no step.
 *
 * lsl_msm_active_set: active i32 [S, ns] (0/1) and n_active i32 [S] of counts i64 [S, ns, ns].
 * lsl_msm_reversible_step: at most `iters` further steps of every series whose done[s] is 0, never past maxiter in total.  x f64 [S, ns] (0
 *   outside A), n_iter i32 [S], err f64 [S] and done i32 [S] are the state, in and out: a call resumes exactly where the last one stopped, so
 *   ceil(maxiter / iters) calls are enqueued with no host synchronisation - a series whose done[s] is set leaves before it loads anything and
 *   none of its buffers is touched.  restart != 0 first sets the state from the counts, whatever it held: x0, n_iter = 0, err = 0, and done
 *   for |A| <= 1.  done[s] = 1: the stop test held (converged); 2: maxiter steps were counted and the last did not pass it.
 *   Order.  y_i: with NSP = 32 / 64 / 128 the padded size (the least that holds ns), part h < 8 of row i adds its terms of the columns
 *   [h NSP / 8, (h + 1) NSP / 8) in ascending j from zero, and the eight parts are added in ascending h; sum_i y_i: a balanced
 *   tree over each group of min(NSP, 64) rows (row i with i ^ 1, then ^ 2, ...; a row outside A adds +0), the two groups of NSP = 128 in order.  A function of (ns, A) alone: a series has the same bits alone,
 *   inside any batch and however the steps are split over calls.  Every division is IEEE fp64; a zero entry of K is skipped, not divided.
 * lsl_msm_transition_matrix: T f64 [S, ns, ns] = the identity with the block of A written in (row sums of X in ascending j), pi f64 [S, ns]
 *   = x on A and 0 outside: the embedding of eval_peptide.py:261-271.
 * 1 <= ns <= 128 (fp64 K of a series stays in LDS), 1 <= S <= 65535, iters >= 0, maxiter >= 0, maxerr not NaN (else -3). */
int lsl_msm_active_set(const int64_t *counts, int32_t S, int32_t ns, int32_t *active, int32_t *n_active, void *stream);
int lsl_msm_reversible_step(const int64_t *counts, const int32_t *active, int32_t S, int32_t ns, int32_t iters, int32_t maxiter, double maxerr,
                            int32_t restart, double *x, int32_t *n_iter, double *err, int32_t *done, void *stream);
int lsl_msm_transition_matrix(const int64_t *counts, const int32_t *active, const double *x, int32_t S, int32_t ns, double *T, double *pi, void *stream);

/* Rigid superposition of a sampled trajectory: what the reference does through mdtraj before a trajectory is written or analysed
 * (eval_peptide.py:347 traj.superpose(traj); utils/traj_utils.py:54-60 create_trajectory = center_coordinates() then superpose(traj, 0)) -
 * the Kabsch fit of every frame onto a reference, its RMSD, and the per-atom mean and RMSF.  Device pointers unless named host; nothing is
 * allocated, nothing is synchronised, a refused call enqueues nothing.  No atomics.  All arithmetic is fp64 on the exact fp32 inputs in a
 * fixed order, every output is rounded once: a frame has the same bits alone and inside any batch, an atom the same bits at any A.  The
 * functions are fixed here as mathematics; mdtraj fits in float32 by QCP, parity with a live mdtraj is not claimed.
 *
 * lsl_superpose: for each of F frames x = pos[f] [A, 3] f32 and its reference y = ref[0] (ref_frames == 1) or ref[f] (ref_frames == F), over the
 *   n_sel selected atoms sel i32 [n_sel] (sel_host: the same table in HOST memory, range-checked: outside 0..A-1 is -3; both NULL: all A
 *   atoms, n_sel == A):
 *     cx, cy  the centroids of the selection (lane l of a wave adds the selected atoms l, l + 64, .. in order, the 64 lanes are combined by the
 *             butterfly lane ^ 1, ^ 2, .. ^ 32; one division by n_sel) - every sum below has this order;
 *     S       = sum_i (x_i - cx)(y_i - cy)^T;  R = the proper rotation (det +1, never a reflection) minimising sum_i |R (x_i - cx) - (y_i - cy)|^2:
 *             the unit eigenvector q of the largest eigenvalue of Horn's 4 x 4 matrix K(S) by 8 cyclic Jacobi sweeps (a fixed count), its
 *             first nonzero component positive, R = R(q).  S == 0 exactly (one selected atom, coincident atoms) gives R = 1;
 *     out     f32 [F, A, 3] = R (x_a - cx) + cy for EVERY atom a of the frame; an atom with fixed[a] != 0 (fixed u8 [A], or NULL) is copied
 *             through unchanged (the zeroed padding slots of an atom14 frame);
 *     rmsd    f32 [F] = sqrt(sum_i |R (x_i - cx) - (y_i - cy)|^2 / n_sel), from the fp64 residuals (a frame against itself gives 0, not 1e-7);
 *     rot     f64 [F, 3, 3] = R;  trans f64 [F, 3] = cy - R cx:  out = R x + trans.
 *   flags = LSL_SUP_CENTER_ONLY: out = x - cx (center_coordinates), rot = 1, trans = -cx; ref is not read and may be NULL, rmsd must be NULL.
 *   Each output may be NULL; all NULL is 0 without a launch.  out may be pos (a frame is in LDS before it is written); out must not overlap
 *   ref (-3).  A frame holding NaN among its selected atoms (or its reference's) gives NaN for that frame only.  1 <= A <= 2044 (a frame
 *   in LDS), 1 <= n_sel <= 2044, F >= 1, ref_frames 1 or F.
 * lsl_atom_rmsf: mean_out f64 [A, 3] = mean_f pos[f, a] and rmsf_out f32 [A] = sqrt(mean_f |pos[f, a] - mean_a|^2) of pos [F, A, 3] f32, each
 *   may be NULL.  The frames are split in segments of 128; a column's sum is the segments' sums (frames in order) added in segment order,
 *   the second pass ((x - mean)^2 per coordinate) likewise, then (sx + sy) + sz, one division by F, one square root.  workspace: device
 *   memory of lsl_atom_rmsf_workspace_bytes(F, A) bytes (0 for a refused shape; too small: -4).  A >= 1, 1 <= F <= 8388480. */
#define LSL_SUP_CENTER_ONLY 1
int lsl_superpose(const float *pos, const float *ref, int32_t ref_frames, const int32_t *sel, const int32_t *sel_host, int32_t n_sel,
                  const uint8_t *fixed, int64_t F, int32_t A, int32_t flags, float *out, float *rmsd, double *rot, double *trans, void *stream);
size_t lsl_atom_rmsf_workspace_bytes(int64_t F, int32_t A);
int lsl_atom_rmsf(const float *pos, int64_t F, int32_t A, double *mean_out, float *rmsf_out, void *workspace, size_t workspace_bytes,
                  void *stream);

/* Sampler loop (Sampler.sample_ode / sample_sde inner loops): applies n_steps affine updates to io->x
 * in place.  noise: device [n_noise, B*T*L*C] standard-normal draws, slice s belongs to step s (the
 * reference draws one tensor per Euler-Maruyama step whether or not g(t) is zero, integrators.py:30);
 * steps >= n_noise must have aw == 0.  noise == NULL: steps with aw != 0 draw on the device
 * (Philox4x32-10 keyed by seed, counter = (step, global element index + elem_offset); elem_offset makes
 * sharded runs reproduce the unsharded stream).
 * trace: optional device [n_trace, B*T*L*C]: a record with trace_index k >= 0 writes the state after it to slice k (k < n_trace is
 * checked; -1 = not recorded; anything below -1 is rejected), or NULL (every trace_index is then ignored). */
int lsl_sample_ex(lsl_model *m, const lsl_io *io, const lsl_step_ex *steps, int32_t n_steps,
                  const float *noise, int32_t n_noise, uint64_t seed, uint64_t elem_offset, float *trace, int32_t n_trace,
                  void *workspace, size_t workspace_bytes, void *stream);
/* The same with plain records: record s uses noise slice / stream step s and writes trace slice s (trace: [n_steps, B*T*L*C] or NULL). */
int lsl_sample(lsl_model *m, const lsl_io *io, const lsl_step *steps, int32_t n_steps,
               const float *noise, int32_t n_noise, uint64_t seed, uint64_t elem_offset, float *trace,
               void *workspace, size_t workspace_bytes, void *stream);

/* Initial state of a sampling call: x[0..n) ~ N(0,1) from the same counter stream as the per-step noise (reserved step index
 * 0xFFFFFFFF), element e of the call = global element elem_offset + e.  Stands in for `torch.randn_like(x_cond)`
 * (models/composites/lightning_base.py:231); shard-invariant by construction. */
int lsl_randn(float *x, uint64_t n, uint64_t seed, uint64_t elem_offset, void *stream);

/* Runge-Kutta arithmetic of the adaptive ODE sampler on the device (the reference's default ODE method is torchdiffeq's dopri5,
 * modules/transport/transport.py:486-494 -> integrators.py:67-78; torchdiffeq's rk_common.py does these combinations with torch ops).  fp32;
 * every term is a rounded product added to the rounded running sum in list order (no FMA contraction), reductions in a fixed order: results
 * are deterministic and independent of the launch shape.  n_x, n_k <= 8; `out` may alias a term.
 *   lsl_rk_lincomb:     out[i] = sum_j c[j] x[j][i]                       (stage states, solution, mid-point, dense-output coefficients)
 *   lsl_rk_dense:       out[i] = e + x (d + x (c + x (b + x a)))           (dense output at the fraction x of an accepted step)
 *   lsl_rk_error_ratio: *ratio = sqrt(mean_i (err[i] / (atol + rtol max(|y0[i]|, |y1[i]|)))^2), err = sum_j c[j] k[j]
 *                       (the step controller's one scalar; `ratio` is a device pointer, `scratch` >= LSL_RK_SCRATCH_BYTES device bytes) */
#define LSL_RK_SCRATCH_BYTES 8192
int lsl_rk_lincomb(float *out, const float *const *x, const float *c, int32_t n_x, uint64_t n, void *stream);
int lsl_rk_dense(float *out, const float *a, const float *b, const float *c, const float *d, const float *e, float x, uint64_t n, void *stream);
int lsl_rk_error_ratio(float *ratio, const float *y0, const float *y1, const float *const *k, const float *c, int32_t n_k, float atol, float rtol,
                       uint64_t n, void *scratch, void *stream);

/* Adaptive Dormand-Prince 5(4) with the step controller on the device (lam_slide_amd/transport.py: dopri5_solve is the host restatement;
 * csrc/k_dopri5.hip.h the kernels).  The controller's state lives in the caller's workspace; every kernel of an attempt reads it there, so
 * an attempt takes no host value, is enqueued without a synchronisation, and is replayed as a hipGraph under the rule of lsl_sample
 * (LSL_GRAPH: the first attempt of a key runs eagerly, the second is captured, later ones replay; same bits).  State arithmetic: the
 * rounding contract of lsl_rk_* above; time and controller arithmetic: fp64.  The error norm runs over the whole state [B,T,L,C].
 *
 * The workspace (lsl_dopri_workspace_bytes) starts with the records a caller reads back with one small copy:
 *   LSL_DOPRI_CTL_OFFSET    lsl_dopri_ctl
 *   LSL_DOPRI_LOG_OFFSET    fp64 [LSL_DOPRI_MAX_ATTEMPTS][4]: row a = (t, dt, ratio, accepted) of attempt a (a < accepted + rejected)
 *   LSL_DOPRI_STATE_OFFSET  fp32 [B,T,L,C]: the current state y (the solution at lsl_dopri_ctl.t)
 * behind them nine more state-sized buffers (stage state, network output, k_1..k_7), the time vector, the reduction scratch, the network's
 * workspace (lsl_workspace_bytes) and the output times.
 *
 *   lsl_dopri_begin    io->x = y(grid[0]) (read only; io->t / io->out unused); grid: n_out non-decreasing output times on the host;
 *                      out: device [n_out][B,T,L,C].  Writes out[j] = y for every leading j with grid[j] <= grid[0], evaluates f(t0, y) and
 *                      chooses the first step size (Hairer's rule, one more evaluation).  The network is given the time t (reverse: 1 - t)
 *                      rounded to fp32; the drift is vx y + vm net(y, t) with (vx, vm) of the path and prediction evaluated in fp64 at that
 *                      fp32 time.  max_steps <= LSL_DOPRI_MAX_ATTEMPTS.
 *   lsl_dopri_advance  n_attempts attempts: six stages, the error ratio, accept (ratio <= 1) or reject, the next step size
 *                      dt min(10, max(0.9 ratio^-0.2, ratio < 1 ? 1 : 0.2)) (dt 10 at ratio 0); an accepted step writes every pending out[j]
 *                      with grid[j] <= t + dt by 4th-order dense output.  Same io (x_cond, mask, y, B, T, L) and workspace as begin.  Once
 *                      `done` is set (the last output time reached, or status != 0) an attempt changes nothing: enqueue as many as convenient,
 *                      read the controller, repeat while !done.
 * Device pointers in, nothing allocated, nothing synchronised; a refused call enqueues nothing. */
#define LSL_DOPRI_MAX_ATTEMPTS 100000
#define LSL_DOPRI_CTL_OFFSET 0
#define LSL_DOPRI_LOG_OFFSET 256
#define LSL_DOPRI_STATE_OFFSET (256 + 32 * LSL_DOPRI_MAX_ATTEMPTS)
enum { LSL_PATH_LINEAR = 0, LSL_PATH_GVP = 1, LSL_PATH_VP = 2 };                               /* path.py: ICPlan, GVPCPlan, VPCPlan */
enum { LSL_PRED_VELOCITY = 0, LSL_PRED_DATA = 1, LSL_PRED_NOISE = 2, LSL_PRED_SCORE = 3 };     /* transport.py: ModelType */
enum { LSL_DOPRI_OK = 0, LSL_DOPRI_MAX_STEPS = 1, LSL_DOPRI_NON_FINITE = 2 };                  /* lsl_dopri_ctl.status */
typedef struct lsl_dopri_desc {
    int32_t path_type, model_type, reverse, max_steps;
    double rtol, atol; /* (the kernels take them rounded to fp32, as lsl_rk_error_ratio does) */
} lsl_dopri_desc;
typedef struct lsl_dopri_ctl {
    double t, dt, t_lo;          /* current time; the step size of the next attempt; where the last accepted step began */
    double ratio, t_new, dt_next; /* the current attempt's decision: error ratio, t + dt, the step size that follows */
    double rtol, atol;
    float *out;                  /* lsl_dopri_begin's out */
    int32_t accept, out_end;     /* decision: 1 = accepted; an accepted step writes out[next_out .. out_end) */
    int32_t accepted, rejected, nfe, next_out, done, status;
    int32_t n_out, max_steps, path_type, model_type, reverse;
} lsl_dopri_ctl;
size_t lsl_dopri_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L, int32_t n_out);
int lsl_dopri_begin(lsl_model *m, const lsl_io *io, const lsl_dopri_desc *desc, const double *grid, int32_t n_out, float *out, void *workspace,
                    size_t workspace_bytes, void *stream);
int lsl_dopri_advance(lsl_model *m, const lsl_io *io, int32_t n_attempts, void *workspace, size_t workspace_bytes, void *stream);

/* The same solver with one step controller per trajectory: a call on B trajectories is B independent adaptive solves.  Each trajectory has
 * its own lsl_dopri_ctl record (time, step size, decision, output cursor, counters, status), its own error norm over its [T,L,C] elements and
 * its own log; the network is evaluated once per stage for all of them, at one time per trajectory (io->t's [B] form).  Trajectory b of a call
 * has the bits of lsl_dopri_begin / lsl_dopri_advance on that trajectory alone (B = 1): the kernels give a trajectory the launch shape, the
 * element order and the reductions of that call (csrc/k_dopri5.hip.h).  A trajectory that is done (its last output time reached, a
 * non-finite error ratio, max_steps attempts) changes nothing any more - its state, its rows of `out` and its record stay - while the others
 * go on; the network still evaluates its rows.  max_steps bounds each trajectory's attempts.
 *
 * The workspace (lsl_dopri_each_workspace_bytes) starts with what a caller reads back:
 *   LSL_DOPRI_EACH_SUMMARY_OFFSET             lsl_dopri_each_summary: written behind begin and behind every attempt; the one small copy of a poll
 *   LSL_DOPRI_EACH_CTL_OFFSET                 lsl_dopri_ctl[B], record b at + b * sizeof of the record (128 bytes); the fields mean what they
 *                                             mean above, for trajectory b; `out` is begin's out
 *   LSL_DOPRI_EACH_LOG_OFFSET(B)              fp64 [B][log_rows][4]: row a of trajectory b = (t, dt, ratio, accepted) of its attempt a, for
 *                                             a < min(accepted + rejected, log_rows); later attempts are counted, not logged; log_rows >= 0
 *   LSL_DOPRI_EACH_STATE_OFFSET(B, log_rows)  fp32 [B,T,L,C]: the current states (trajectory b at its own time lsl_dopri_ctl.t)
 * behind them the buffers of lsl_dopri_begin (nine state-sized ones, the time vector, two reduction scratches of
 * B * ceil(T L C / 256, at most 2048) floats, the network's workspace, the output times).
 *
 *   lsl_dopri_each_begin    as lsl_dopri_begin; out: device [n_out][B,T,L,C], trajectory b's rows written as its own accepted steps cover
 *                           the output times.  B <= 65535, log_rows <= LSL_DOPRI_MAX_ATTEMPTS.
 *   lsl_dopri_each_advance  n_attempts attempts of every trajectory that is not done; same io and workspace as the begin call on this
 *                           handle (which recorded n_out and log_rows for it; -3 without one).  Enqueue as many as convenient, read the
 *                           summary, repeat while !done.  Replayed as a hipGraph under the rule of lsl_dopri_advance.
 * Argument checks, error codes and "a refused call enqueues nothing" as above. */
#define LSL_DOPRI_EACH_SUMMARY_OFFSET 0
#define LSL_DOPRI_EACH_CTL_OFFSET 256
#define LSL_DOPRI_EACH_LOG_OFFSET(B) (256 + 256 * ((128 * (size_t)(B) + 255) / 256))
#define LSL_DOPRI_EACH_STATE_OFFSET(B, log_rows) (LSL_DOPRI_EACH_LOG_OFFSET(B) + 256 * ((32 * (size_t)(B) * (size_t)(log_rows) + 255) / 256))
typedef struct lsl_dopri_each_summary {
    int32_t B;            /* trajectories of the call */
    int32_t n_done;       /* trajectories whose record has done = 1 */
    int32_t n_failed;     /* of those, the ones with status != LSL_DOPRI_OK */
    int32_t max_attempts; /* the largest accepted + rejected over the trajectories */
    int32_t done;         /* 1 = n_done == B: further attempts change nothing */
} lsl_dopri_each_summary;
size_t lsl_dopri_each_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L, int32_t n_out, int32_t log_rows);
int lsl_dopri_each_begin(lsl_model *m, const lsl_io *io, const lsl_dopri_desc *desc, const double *grid, int32_t n_out, float *out,
                         int32_t log_rows, void *workspace, size_t workspace_bytes, void *stream);
int lsl_dopri_each_advance(lsl_model *m, const lsl_io *io, int32_t n_attempts, void *workspace, size_t workspace_bytes, void *stream);

/* The adaptive solve of Sampler.sample_ode_likelihood on the device: the same solver on the augmented vector [x | logp],
 * with one tangent pass (lsl_forward_jvp's) per evaluation.  each = 0: one controller, a vector of B T L C + B elements, the logp entries
 * behind all of x (the layout the host path concatenates); each = 1: a controller per trajectory, B vectors of T L C + 1 elements, trajectory
 * b with the bits of the each = 0 call on [b:b+1].  Launch shapes and the error norm's summation order are those of lsl_rk_error_ratio on
 * the concatenated vector.  The right-hand side at solver time s = t + alpha dt, with tn = (float)(1 - s) and (vx, vm) at (double)tn:
 *   k_x[i]    = -(fp32(vx) x[i] + fp32(vm) net[i])         net = network(x, tn)
 *   k_logp[b] = (float)(vx T L C + vm dot_b)               dot_b = sum_e eps[b,e] j[b,e] (lsl_dot_rows' order), j = (d net / d x) eps
 * The probe eps: a device tensor [B,T,L,C] read in place at every evaluation, or (eps = NULL) drawn on the device in front of every tangent
 * pass: trajectory b's evaluation e, element i is lsl_rademacher's value for (probe_seeds[b], e, i), e being the evaluation count of the
 * trajectory's record (begin: 0 and 1; stage s of an attempt: nfe + s), i the index inside the trajectory.  probe_seeds: device uint64 [B],
 * copied at begin.  Exactly one of eps / probe_seeds is given.
 *
 * The workspace (lsl_dopri_logp_workspace_bytes) starts with the records of lsl_dopri_begin (each = 0) or lsl_dopri_each_begin (each = 1) at
 * the same offsets, read back the same way; with so = LSL_DOPRI_STATE_OFFSET or LSL_DOPRI_EACH_STATE_OFFSET(B, log_rows):
 *   so                                            fp32 [B,T,L,C]: the current x
 *   LSL_DOPRI_LOGP_SIDE_OFFSET(so, B T L C)       fp32 [B]: the current logp (the accumulated change of the log-density)
 * desc->reverse must be 1 (the drift is evaluated at 1 - t); the records carry reverse = 1 | LSL_DOPRI_NEGATED: the network's time is
 * reversed AND the x drift is negated, the side elements are integrated beside it - the record of an augmented solve.  The bit is
 * informational, for whoever reads a record back: no kernel tests it (lsl_dopri_logp_* always negate), and setting it in the desc of another
 * entry point is refused like any reverse value but 0 and 1.
 * One workspace layout per (B, T, L, n_out, each, log_rows): the state-sized probe buffer is part of it whether the probe is drawn or given.
 *   lsl_dopri_logp_begin    as lsl_dopri_[each_]begin; out: device [n_out][B,T,L,C], out_logp: device [n_out][B] (0 at the leading output
 *                           times).  each = 0: log_rows is not used (LSL_DOPRI_MAX_ATTEMPTS rows).  B <= 65535.
 *   lsl_dopri_logp_advance  as lsl_dopri_each_advance: same io and workspace as the begin call on this handle (-3 without one); eps, where
 *                           given, is read again.  Attempts are enqueued eagerly (the tangent pass is not replayed as a hipGraph).
 * The tangent pass keeps its refusals (-21: tail, ln_fuse, linear attention); a path x prediction pair without a finite velocity on the
 * interval ends with LSL_DOPRI_NON_FINITE.  Argument checks, error codes and "a refused call enqueues nothing" as above. */
#define LSL_DOPRI_NEGATED 2 /* bit of lsl_dopri_ctl.reverse */
#define LSL_DOPRI_LOGP_SIDE_OFFSET(state_offset, n_state) ((state_offset) + 256 * ((4 * (size_t)(n_state) + 255) / 256))
size_t lsl_dopri_logp_workspace_bytes(const lsl_model *m, int32_t B, int32_t T, int32_t L, int32_t n_out, int32_t each, int32_t log_rows);
int lsl_dopri_logp_begin(lsl_model *m, const lsl_io *io, const lsl_dopri_desc *desc, const double *grid, int32_t n_out, float *out, float *out_logp,
                         int32_t each, int32_t log_rows, const float *eps, const uint64_t *probe_seeds, void *workspace, size_t workspace_bytes,
                         void *stream);
int lsl_dopri_logp_advance(lsl_model *m, const lsl_io *io, int32_t n_attempts, void *workspace, size_t workspace_bytes, void *stream);
/* out[i] = +1 or -1 for (seed, eval_index, i), i < n: the Philox4x32-10 stream of lsl_randn (counter = (i / 4, eval_index, 0), key = seed), the
 * top bit of word i % 4.  The probe draw of lsl_dopri_logp_*. */
int lsl_rademacher(float *out, uint64_t n, uint64_t seed, uint32_t eval_index, void *stream);

/* Test hook: out[i] = (vx, vm) of the drift vx y + vm net(y, t) at the fp32 times t[0..n), fp64, as the kernels of lsl_dopri_* evaluate them */
int lsl_debug_dopri_coeffs(int32_t path_type, int32_t model_type, const float *t, int32_t n, double *out, void *stream);

/* Test hooks: run a single kernel of the path on caller buffers (parity tests of intermediates). */
int lsl_debug_block(lsl_model *m, int32_t block_index /* 0..2*depth-1 */, const float *h_in, float *h_out,
                    const float *mods /* [B, (6*depth+2)*D] */, int32_t B, int32_t T, int32_t L,
                    void *workspace, size_t workspace_bytes, void *stream);
/* lsl_debug_block with two more arguments (lsl_debug_block is this call with a_out = NULL, mod_rows = B: same plan, same kernels, same bits):
 *   a_out    NULL, or bf16 [B*T*L][hidden]: linear1's operand, LayerNorm + modulate of h_in as the LayerNorm kernel left it.  Copied right
 *            behind the LayerNorm launch, which every debug plan runs (tail and ln_fuse handles skip it in network evaluations only): on a
 *            tail handle k_tail overwrites that buffer with the next sub-block's operand, so a copy after the block would hand out that one.
 *   mod_rows B: `mods` holds a row per trajectory; 1: one row [(6*depth+2)*D] shared by every trajectory - the kernels run their shared-row
 *            forms (modulation stride 0: one row in k_linear2_ws's gate table), as a sampler's evaluations do.  Anything else: -3. */
int lsl_debug_block_ex(lsl_model *m, int32_t block_index, const float *h_in, float *h_out, void *a_out, const float *mods, int32_t mod_rows,
                       int32_t B, int32_t T, int32_t L, void *workspace, size_t workspace_bytes, void *stream);
/* The same sub-block up to and including attention (LayerNorm + modulate, linear1 with its epilogue, attention), then the two
 * intermediate buffers as the kernels leave them:
 *   qkv_out bf16 [B*T*L][3 * H * head_dim_pad]  q (after QK-norm and RoPE, times head_dim^-1/2 * log2 e) | k (after QK-norm and RoPE) | v,
 *                                               head-major inside each third
 *   z_out   bf16 [B*T*L][H * head_dim_pad + M]  attention output (head-major) | GELU(mlp)
 * (reference taps: mmdit.py:241-248 q_norm / k_norm / apply_rope / attention / gelu). */
int lsl_debug_taps(lsl_model *m, int32_t block_index, const float *h_in, const float *mods, int32_t B, int32_t T, int32_t L,
                   void *qkv_out, void *z_out, void *workspace, size_t workspace_bytes, void *stream);
int lsl_debug_mods(lsl_model *m, const float *t, const float *y, int32_t B, float *vec_out, float *mods_out,
                   void *workspace, size_t workspace_bytes, void *stream);
/* The fp32 frame of an evaluation on caller buffers - the conditioning chain, the two embeddings, the output head - through the launch
 * helpers an evaluation uses (one dispatch rule).  Every `*_out` below may be NULL unless said otherwise.
 *
 * lsl_debug_mods with more arguments (lsl_debug_mods is this call with t_scalar = 0 and the four taps NULL: same kernels, same bits):
 *   t          device [B], or NULL: every row takes t_scalar - with B = 1 the sampler's single-row route (the wave-per-output kernel whatever
 *              the width); NULL requires y == NULL (the route has no class vector), else -3
 *   tfeat_out  [B, 256] the sinusoidal features, hid_out [B, hidden] the first layer's SiLU output: the fp32 operands the next layer read
 *   yhid_out, yemb_out  [B, hidden] the two layers of vec_in(y); only with y
 * vec_out [B, hidden] and mods_out [B, (6*depth+2)*hidden] are required. */
int lsl_debug_mods_ex(lsl_model *m, const float *t, float t_scalar, const float *y, int32_t B, float *vec_out, float *mods_out, float *tfeat_out,
                      float *hid_out, float *yhid_out, float *yemb_out, void *workspace, size_t workspace_bytes, void *stream);
/* The modulation tables of `count` sampler records at once, as lsl_sample_ex computes them for a group of records of a model without class
 * conditioning: times HOST [count]; mods_out [count, (6*depth+2)*hidden] (required), vec_out [count, hidden].  Row s has the bits of
 * lsl_debug_mods_ex(t = NULL, t_scalar = times[s], B = 1).  count above the group size of the model, or a class-conditioned model: -3.
 * workspace: lsl_workspace_bytes(m, 1, 1, 1). */
int lsl_debug_mods_steps(lsl_model *m, const float *times, int32_t count, float *mods_out, float *vec_out, void *workspace, size_t workspace_bytes,
                         void *stream);
/* The two embeddings of a pass of B trajectories (an evaluation with one shared modulation row): cond_emb = cond_to_emb(x_cond) + biases +
 * mask_emb[mask] (once per sample), then h = x_in(x) + cond_emb with what the handle attaches to it.
 *   cond_emb_out [n, hidden]; h_out [n, hidden] in front of the normalize LayerNorm; hn_out [n, hidden] behind it (equal to h_out on models
 *   without normalize); stats_out float2 [n] = (rstd, -mean rstd) of every row of h, eps 1e-6: ln_fuse handles whose embedding leaves them
 *   (no normalize, in_dim <= 32, hidden 256 / 512, a pass the fused linear1 takes), -3 elsewhere.  n = B*T*L.
 * workspace: lsl_workspace_bytes(m, B, T, L). */
int lsl_debug_embed(lsl_model *m, const float *x, const float *x_cond, const int64_t *mask, int32_t B, int32_t T, int32_t L, float *cond_emb_out,
                    float *h_out, float *hn_out, void *stats_out, void *workspace, size_t workspace_bytes, void *stream);
/* The output head on the caller's residual rows h [n, hidden] with mods as in lsl_debug_block_ex (mod_rows 1 or B; the final shift | scale
 * of every row is read).  rec == NULL: out [n, in_dim] = the network output.  Else one record of lsl_sample_ex applied to x [n, in_dim] in
 * place: x <- ax x + am m + aw w + as saved, with w = noise [n, in_dim] or, when noise is NULL, the device stream at (seed, step
 * rec->noise_index, element elem_offset + e); trace and save_out [n, in_dim] receive the new state (rec->trace_index and LSL_STEP_SAVE are
 * not consulted: the pointers say it); saved is required when as != 0.  No workspace. */
int lsl_debug_head(lsl_model *m, const float *h, const float *mods, int32_t mod_rows, float *x, float *out, const lsl_step_ex *rec, const float *noise,
                   uint64_t seed, uint64_t elem_offset, float *trace, const float *saved, float *save_out, int32_t B, int32_t T, int32_t L,
                   void *stream);

/* Measurement hooks (bench.py roofline leg): bracket every launch of one kernel class with HIP events on
 * the stream it is launched on.  kernel: 0 linear1 GEMM, 1 linear2 GEMM, 2 attention, 3 LayerNorm+modulate,
 * 4 output head + state update, 5 input embedding, 6 modulation tables; -1 disables.
 * lsl_profile_read synchronises on the recorded events and returns their summed duration. */
int lsl_profile_enable(lsl_model *m, int32_t kernel, int32_t max_launches);
/* Name of the kernel the profiled class launched in the passes since lsl_profile_enable ("" if none): the label of a timing comes from the
 * library's own dispatch, not from a copy of its rule. */
const char *lsl_profile_kernel_name(const lsl_model *m);
int lsl_profile_read(lsl_model *m, double *total_ms, int32_t *launches);

/* ------------------------------------------------------------------------------------------------
 * Frozen stage-1 decode of the sampled latents: the step right after the sampler and the
 * second half of the parity metric ("decoded coordinates").  Stands in for
 *   first_stage.decode(latents, entities) = Decoder(post_quant(latents), entities)
 *   (models/composites/lightning_base.py:28-31,42-44; models/components/decoder.py:12-102;
 *    blocks: modules/torch_modules.py:104-264; entity table: modules/entity_embeddings.py:7-33).
 * fp32 throughout.  One block = PreNorm(Attention) + residual, PreNorm(FeedForward(dim)) + residual. */
typedef struct lsl_dec_block {
    const float *ln_w, *ln_b;        /* attn.norm                                  [dim]                  */
    const float *lnc_w, *lnc_b;      /* attn.norm_context (cross-attention blocks) [context_dim], else NULL */
    const float *w_q;                /* self: attn.fn.to_qkv.weight [3*inner, dim]; cross: attn.fn.to_q.weight [inner, dim] */
    const float *w_kv;               /* cross: attn.fn.to_kv.weight [2*inner, context_dim]; self: NULL    */
    const float *w_out, *b_out;      /* attn.fn.to_out [dim, inner], [dim]                                */
    const float *q_scale, *k_scale;  /* attn.fn.norm.{query,key}_norm.scale [dim_head], NULL without qk_norm */
    const float *ff_ln_w, *ff_ln_b;  /* ff.norm                                                           */
    const float *ff_w1, *ff_b1;      /* ff.fn.net.0.0 [dim, dim]                                          */
    const float *ff_w2, *ff_b2;      /* ff.fn.net.1   [dim, dim]                                          */
} lsl_dec_block;

typedef struct lsl_decoder_desc {    /* Decoder.__init__ arguments (decoder.py:14-29) + post_quant input width */
    int32_t in_dim;                  /* C of the sampled latents (post_quant = LayerNorm(C, no affine) + Linear(C, dim_latent)) */
    int32_t dim_latent, dim_query, dim_emb, n_entities;
    int32_t heads_latent, dim_head_latent, heads_cross, dim_head_cross;
    int32_t num_block_attn, num_block_cross;
    int32_t act;                     /* 1 = erf GELU (src.modules.torch_modules.GELU), 2 = nn.GELU(approximate="tanh") */
    int32_t out_dim;                 /* width of the decoded output head (3 for "pos")                    */
    int32_t num_split;               /* DecoderQuerySplitter (decoder.py:313-411, peptide): every latent becomes num_split context tokens
                                        for the output block; 0 or 1 = plain Decoder                           */
} lsl_decoder_desc;

typedef struct lsl_decoder_weights {
    const float *pq_w, *pq_b;        /* post_quant.1 [dim_latent, C], [dim_latent]                        */
    const float *table;              /* decoder.entity_embedding.embedding.weight [n_entities, dim_emb], rows ALREADY clipped to
                                        max_norm (nn.Embedding(max_norm=1) renormalises looked-up rows at forward time)      */
    const float *qm_w, *qm_b;        /* decoder.query_mlp.1 [dim_query, dim_emb]                          */
    const lsl_dec_block *self_blocks;   /* HOST array [num_block_attn]  decoder.self_attn_blocks.i       */
    const lsl_dec_block *cross_blocks;  /* HOST array [num_block_cross] decoder.cross_attn_blocks.i      */
    lsl_dec_block out_block;            /* decoder.output_block (queries attend to the latents)          */
    const float *ext_w, *ext_b;      /* decoder.extender.1 (1x1 Conv1d) as [num_split * dim_latent, dim_latent] with rows reordered to
                                        (split, feature): row n * dim_latent + d = conv channel d * num_split + n; NULL without split */
    const float *head_w1, *head_b1;  /* decoder.output_layers.<name>.0 [dim_query, dim_query]             */
    const float *head_w2, *head_b2;  /* decoder.output_layers.<name>.2 [out_dim, dim_query]               */
} lsl_decoder_weights;

typedef struct lsl_decoder lsl_decoder;
int lsl_decoder_create(const lsl_decoder_desc *desc, const lsl_decoder_weights *w, lsl_decoder **out);
void lsl_decoder_destroy(lsl_decoder *d);
size_t lsl_decode_workspace_bytes(const lsl_decoder *d, int32_t frames, int32_t L, int32_t A);
/* z: device [frames, L, C] latents; entities: device [frames, A] int64; out: device [frames, A, out_dim].
 * Limits (lsl_decoder_create / lsl_decode return -3 outside them):
 *   - in_dim, dim_latent, dim_query, dim_emb, heads_latent * dim_head_latent and heads_cross * dim_head_cross are multiples of 4
 *     (16-byte row loads); dim_head_latent and dim_head_cross are 1..64; out_dim is free.
 *   - One attention call keeps the keys and values of a (frame, head) in 64 KiB of LDS, in a head tile of 16 / 32 / 64 floats for
 *     dim_head <= 16 / <= 32 / <= 64: (2 * keys * tile + keys) * 4 <= 65536, i.e. at most 496 / 252 / 127 keys.  A self block has L keys
 *     (dim_head_latent), a cross block A keys and the output block L * max(num_split, 1) keys (dim_head_cross).  The query axis is free.
 *   - The shape is checked block by block as the launches are enqueued: a refused call has written nothing to `out` (only the last launch
 *     does), but the stages before the refused block have been enqueued on `stream` and have overwritten the workspace.
 *   - An entity index outside 0..n_entities-1 reads the nearest row of the table (negative: row 0, too large: the last row); the
 *     reference's nn.Embedding raises instead, so a caller that wants that error checks the indices itself. */
int lsl_decode(lsl_decoder *d, const float *z, const int64_t *entities, int32_t frames, int32_t L, int32_t A, float *out,
               void *workspace, size_t workspace_bytes, void *stream);

#define LSL_DECODE_MAX_HEADS 8
typedef struct lsl_decoder_head {    /* decoder.output_layers.<name>: Linear(dim_query, dim_query), act, Linear(dim_query, out_dim) */
    const float *w1, *b1;            /* decoder.output_layers.<name>.0 [dim_query, dim_query]             */
    const float *w2, *b2;            /* decoder.output_layers.<name>.2 [out_dim, dim_query]               */
    int32_t out_dim;
} lsl_decoder_head;
/* Decoder.forward returns every head of output_layers from one trunk (decoder.py:97-102): the trunk of lsl_decode once (post_quant ..
 * output_block), then heads[0..n_heads-1] on the same rows.  heads, outs: HOST arrays; outs[h]: device f32 [frames, A, heads[h].out_dim].
 * 1 <= n_heads <= LSL_DECODE_MAX_HEADS; the head the handle was created with is not evaluated unless it is listed.  Head h has the same
 * bits as lsl_decode on a handle created with that head's weights (the same launches in the same order), plain Decoder and
 * DecoderQuerySplitter alike.  Workspace: lsl_decode_workspace_bytes, unchanged (the hidden buffer is reused head after head on the
 * stream).  The limits and the refusal behaviour of lsl_decode apply unchanged: a refused call has written to no outs[h]. */
int lsl_decode_heads(lsl_decoder *d, const lsl_decoder_head *heads, int32_t n_heads, const float *z, const int64_t *entities,
                     int32_t frames, int32_t L, int32_t A, float *const *outs, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Frozen stage-1 encode, the step before setup_conditioning: stands in for
 *   quant(Encoder(x, entities, mask))      (models/components/encoder.py:34-41,96-103; lightning_base.py:22-25,37-40)
 * where x is the output of the dataset-specific prepare_inputs (first_stage/<dataset>.py), which stays the caller's. */
typedef struct lsl_encoder_desc {    /* Encoder.__init__ arguments (encoder.py:46-61)                       */
    int32_t dim_input, dim_emb, n_entities, dim_latent, num_latents;
    int32_t heads_cross, dim_head_cross, heads_latent, dim_head_latent;
    int32_t num_block_cross, num_block_attn;
    int32_t act;                     /* 1 = erf GELU, 2 = tanh GELU                                       */
} lsl_encoder_desc;

typedef struct lsl_encoder_weights {
    const float *table;              /* encoder.entity_embedding.embedding.weight, rows already clipped to max_norm */
    const float *mlp_w1, *mlp_b1;    /* encoder.mlp.0 [dim_latent, dim_input + dim_emb]                    */
    const float *mlp_w2, *mlp_b2;    /* encoder.mlp.2 [dim_input + dim_emb, dim_latent]                    */
    const float *latents;            /* encoder.latents [num_latents, dim_latent]                          */
    const lsl_dec_block *cross_blocks;  /* HOST array [num_block_cross] encoder.cross_attn_blocks.i (latents attend to the context) */
    const lsl_dec_block *self_blocks;   /* HOST array [num_block_attn]  encoder.blocks_attn.i            */
    const float *quant_w, *quant_b;  /* quant.0 [dim_latent, dim_latent]; quant.1 = LayerNorm without affine */
} lsl_encoder_weights;

typedef struct lsl_encoder lsl_encoder;
int lsl_encoder_create(const lsl_encoder_desc *desc, const lsl_encoder_weights *w, lsl_encoder **out);
void lsl_encoder_destroy(lsl_encoder *e);
size_t lsl_encode_workspace_bytes(const lsl_encoder *e, int32_t frames, int32_t A);
/* x: device [frames, A, dim_input]; entities: device [frames, A] int64; mask: device [frames, A] bytes, non-zero = real entity,
 * or NULL (all real: the same bits as a mask of ones); out: device [frames, num_latents, dim_latent].
 * Limits, as for lsl_decode: dim_input, dim_emb, dim_latent and both heads * dim_head are multiples of 4, dim_head is 1..64; a cross
 * block has A keys (head tile of dim_head_cross: A <= 496 / 252 / 127), a self block num_latents keys (tile of dim_head_latent); -3
 * beyond that, with nothing written to `out` and the earlier stages enqueued; entity indices are clamped to the table.
 * A masked-out entity never reaches the latents, whatever x holds there (finite).  A frame whose mask is all zero has no softmax: its
 * latents are NaN (softmax over a row of -inf, as in tests' oracle; what F.scaled_dot_product_attention of the reference returns for
 * such a row has differed between PyTorch versions, NaN or zeros, so do not pass an empty frame), and the other frames of the call
 * are unaffected. */
int lsl_encode(lsl_encoder *e, const float *x, const int64_t *entities, const unsigned char *mask, int32_t frames, int32_t A, float *out,
               void *workspace, size_t workspace_bytes, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* LSL_API_H */
