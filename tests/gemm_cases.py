"""The case table of the per-element GEMM tests (test_gemm_cases.py on the CPU, test_hip_gemm.py on the MI355X): models and shapes that
reach every form of the LayerNorm + modulate kernels, of linear1 (k_linear1_ts at every instance, wave count and work split; the tile GEMM
with EpiLinear1), of linear2 (k_linear2_ws at every instance, slice count and token-range shape; the tile GEMM with EpiLinear2) and of
k_tail, at the token counts where each changes behaviour; the launch rules of csrc/host_launch.hip.h and csrc/host_eval.hip.h restated
with the CU count as a parameter; the fp64 references; the per-element bars.  Not a test module.

What is compared.  lsl_debug_block_ex hands out `a`, the bf16 operand LayerNorm + modulate leaves for linear1, and the updated residual
stream; lsl_debug_taps hands out q | k | v and z = [attention | GELU(mlp)] as the kernels leave them.  Every reference below is computed
in fp64 from the very bf16 operand the kernel read (the tapped `a` for linear1 and the tail's up-projection, the tapped z for linear2) and
from the packed weights of lam_slide_amd.packing.pack_block (bf16 w1, w2; fp32 b1, b2, qs, ks: the bytes the kernels read, padded head
columns included), so that only the kernel's own roundings separate the two.  On a tail handle linear1 runs as a q | k | v-only launch
whose output no call hands out: it is seen through h_out (attention of its q | k | v, then the out-projection) against the z of
lsl_debug_taps, whose linear1 is the full launch - the two launches promise the same bits.  That view is limited: under the k_tail bar
(some tens of times linear2's, below) a single wrong q / k / v element of that launch, diluted by the softmax and the out-projection, can
stay inside; a comparison with the plain handle's h_out would be no tighter (the two differ by the same rounding of the GELU operand).  What
the view does catch is what a launch gets wrong at this size: a wrong block, tile, segment or plane of q | k | v moves whole attention rows.
The launch's own bits need a tap of ws.qkv behind a tail handle's block, which the library does not have yet.

Bars, per element.  u = 2^-24 (one fp32 operation, round to nearest), u_b = 2^-9 (one rounding to bf16, round to nearest even), S =
sum_k |w_k x_k| + |bias| of the element's chain.  bf16 keeps 8 significant bits, so half a unit in the last place of a value y in
[2^e, 2^(e+1)) is 2^(e-8) = u_b 2^(e+1): the rounding term is written rnd(y) = u_b P(y) with P(y) the power of two above |y| - between
u_b |y| and 2 u_b |y|, and what the format gives: u_b |y| alone would put an exactly rounded output of the lower half of a binade outside
the bar.  Where the rounded value is y + d with |d| <= t, the term is rnd(|y| + t) (the value may cross into the next binade) plus t.
  * Accumulation, in any order: |acc_hat - acc| <= (K + 2) u S.  Assumptions: the product of two bf16 values is exact in fp32 (8 x 8
    significand bits); every addition of the chain - inside a 16-deep MFMA step or between steps, whatever the tree - rounds its result
    within u relative; an element's chain has at most K additions of products and one of the bias, so every term passes through at most
    K + 1 roundings: (1 + u)^(K + 1) - 1 <= (K + 2) u for K <= 2 048.  No cancellation is assumed: the bound is the worst case, about
    sqrt(K) above what random rounding gives, and still 2^-13 of S at K = 1 536 - a dropped k-step (16 / K of S) is far outside.
  * a = bf16(LN_1e-6(h) (1 + scale) + shift):  rnd(|a| + t) + t, t = |1 + scale| (24 u |xhat| + 16 u rstd mean|h|) + 4 u |a|, with
    xhat = (h - mean) rstd.  The statistics are fp32 sums of at most 8 values per lane and a 6-level wave tree (14 additions deep): the mean
    moves by at most 14 u mean|h| (2 u more for the subtraction and the product with rstd); rstd = rsqrt(sum of squares / D + eps)
    moves by half the relative error of its sum (2 u per square, 14 u of tree: 8 u) plus 2 u of v_rsq_f32 and 1 u of the product: 24 u
    of xhat with the subtraction's own rounding and its sensitivity to the mean.  1 + scale, the product and the addition of the shift are
    3 roundings, each at most u max(|a|, |xhat (1 + scale)|): 4 u |a| with the shift's cancellation covered by the xhat term.
  * v = bf16(acc):  rnd(|v| + t) + t, t = (K + 2) u S.
  * GELU(mlp) = bf16(gelu(acc)):  rnd(|g| + t) + t, t = 1.13 (K + 2) u S + 7e-7 + 4 u |g|: |gelu'| <= 1.13 carries the accumulation term,
    7e-7 is the fit error stated beside gelu_fast (common.hip.h), 4 u |g| its last product and sum.
  * q, k = bf16(premul rr R(pos) (s . x)), rr = rsqrt(mean_d x_d^2 + eps), x = acc:  with e_d = (K + 2) u S_d the accumulation term of
    channel d, to first order  |dq_i| <= premul rr (|c s_0| e_0 + |sn s_1| e_1)  (the rotation of the pair that holds i)
                                        + |q_i| rr^2 (1 / hd) sum_d |x_d| e_d      (through the normalisation);
    the fp32 epilogue adds (hd / 2 + 12) u premul rr (|s_0 x_0| + |s_1 x_1|): hd fused multiply-adds of the sum of squares (hd / 2 u on
    rr), its scaling, v_rsq_f32 (2 u), the pre-multiplier, and per output the table entry (cos or sin rounded to fp32 times the scale
    rounded once: 2 u), one product, one fused multiply-add and the product with rr.  The table error: run_tables (csrc/host_eval.hip.h)
    has k_rope_scaled form the angle p theta^(-2j/hd) in fp64 and round cos and sin once to fp32, as oracle.latent_net.rope_cos_sin
    does, which is the table the reference uses; the two fp64 angles differ by a few units of 2^-53 p, i.e. by p 2^-50 at most in cos and
    sin: the term grows with the position and is added to the 12 u (it is below u up to 6 10^7 positions).  The bar is rnd(|q| + t) + t
    with t the sum of these.  Padded channels of q and k must be exactly 0 (zero weight rows, zero bias, identity rotation, zero scale).
  * linear2, h_out = fma(gate, acc + b2, h):  |gate| (K2 + 3) u S + 2 u |h_out|, S = sum |w z| + |b2|: the chain from zero, the bias
    added behind it (one more rounding than linear1's, which starts from the bias), one rounding of the fused update, and one u |h_out| of
    slack for the reference's own h_out against the kernel's exact fma operand.
  * k_tail: the up-projection's GELU is rounded to bf16 between two chains that each run in an order of their own, and no call hands that
    operand out.  The reference therefore keeps g_j = gelu(u_j) unrounded (u_j in fp64 from the tapped `a`), and the bar carries the
    operand's error through the down-projection:
        |gate| [ (K2 + 3) u S + sum_j |w2_j| (rnd(|g_j| + t_j) + t_j) ] + 2 u |h_out|,   t_j = 1.13 (D + 2) u S1_j + 7e-7 + 4 u |g_j|,
    S = sum |wo z_attn| + sum_j |w2_j g_j| + |b2|.  This is weaker than the linear2 bar: at M = 512 (K2 = 768) the rounding term is
    between 2^-9 / (771 2^-24) = 42 and 85 times the accumulation term on the mlp share of S, so the bar is some tens of times
    linear2's - test_gemm_cases.py prints the ratio of the two per tail case (median 37 at M = 512).  It still catches every mutation of the list
    (a dropped 32-feature mlp block is 32 / M of the mlp share, not 2^-9 of it).
What the kernels measure in units of these bars on MI355X: profiles/gemm_rowwise_parity.txt.

Tilings the product build can reach (gemm_variant restated below, enumerated in test_gemm_cases.py): linear1 on the tile GEMM runs 5, 10
and 11.  Tiling 12 is unreachable: it needs K % 128 == 0, and every hidden size with K % 128 == 0 that lsl_model_create accepts (128, 256,
384, 512) is an instance of k_linear1_ts whose only shape conditions (F1 and heads x head_dim_pad multiples of 64, the LDS need) hold for
every such model packing.make_dims produces, so linear1 never reaches the tile GEMM there.  linear2 on the tile GEMM runs 7, 11, 15 and
28; 10 is unreachable for it (K2 is always a multiple of 64).  No knob forces a tiling here.

The inputs of a case are h_in = randn [B, T, L, D] and mods = 0.3 randn [B, 8 D] (generator seed 3, as attention_cases.inputs); on the
shared arms every trajectory gets row 0.  The weights are oracle.latent_net.random_params(seed 21) with linear1 / linear2 weights rounded
to bf16 beforehand, so that the oracle and the packed tensors hold the same numbers."""
import functools
import math
from collections import namedtuple

import torch

from oracle import latent_net

U = 2.0 ** -24
UB = 2.0 ** -9
LOG2E = 1.4426950408889634
GELU_SLOPE, GELU_FIT = 1.13, 7e-7
LDS_BUDGET = 160 * 1024
CUS = 256  # the MI355X; every rule below takes the count as a parameter

# ---- models: depth 1, in_dim 16: name -> (hidden, heads, mlp_ratio) ----------------------------------------------------------------------
MODELS = {
    "d64h2r1": (64, 2, 1),        # K = 64: one k-tile; F1 = 256, K2 = 128
    "d64h2r5": (64, 2, 5),        # F1 = 512: tiling 5 above 40 960 tokens
    "d64h4r2": (64, 4, 2),        # 16-wide heads; F1 = 320: ragged, tiling 10
    "d128h4r2": (128, 4, 2),      # k_linear1_ts<32, 128>, k_linear2_ws<384>, one slice
    "d128h8r2": (128, 8, 2),      # <16, 128>
    "d192h8r1": (192, 8, 1),      # 24 of 32; F1 = 960: partial last feature tile; linear2 11 / 28
    "d256h8r2": (256, 8, 2),      # <32, 256>, k_linear2_ws<768>, two slices; k_tail M = 512
    "d256h16r2": (256, 16, 2),    # <16, 256>
    "d256h8r025": (256, 8, 0.25),  # k_tail M = 64
    "d256h8r05": (256, 8, 0.5),   # k_tail M = 128
    "d256h16r4": (256, 16, 4),    # k_tail M = 1024
    "d320h10r1": (320, 10, 1),    # tile GEMM, K = 320
    "d384h16r2": (384, 16, 2),    # <32, 384>, 24 of 32, k_linear2_ws<1280>, three slices
    "d384h24r2": (384, 24, 2),    # <16, 384>; K2 = 1152: linear2 on the tile GEMM
    "d384h16r1": (384, 16, 1),    # K2 = 896: linear2 11 / 28 on a 384-wide model
    "d448h16r1": (448, 16, 1),    # tile GEMM, K = 448: 7 k-tiles; 28 of 32; linear2 11 / 15
    "d512h16r2": (512, 16, 2),    # <32, 512>, 4 and 8 waves, k_linear2_ws<1536>, four slices
    "d512h32r2": (512, 32, 2),    # <16, 512>
    "d512h16r1": (512, 16, 1),    # K2 = 1024: linear2 11 / 7
}
Dims = namedtuple("Dims", "D H hd hdp HHD M Mp F1 K2")


def net_shape(model):
    D, H, r = MODELS[model]
    return latent_net.NetShape(depth=1, in_dim=16, hidden_size=D, num_heads=H, mlp_ratio=r)


def dims(model):
    """packing.make_dims restated: padded heads, the mlp width rounded up so that heads x head_dim_pad + M is a multiple of 64."""
    D, H, r = MODELS[model]
    hd = D // H
    hdp = 16 if hd <= 16 else 32
    M = int(D * r)
    Mp = (M + 31) // 32 * 32
    if (H * hdp + Mp) % 64:
        Mp += 32
    return Dims(D, H, hd, hdp, H * hdp, M, Mp, 3 * H * hdp + Mp, H * hdp + Mp)


# ---- the launch rules restated (csrc/host_launch.hip.h; Lin1Cfg, Lin2Cfg, TailCfg of the kernels' headers) -------------------------------
LIN1_TS_HIDDEN = (128, 256, 384, 512)  # LSL_LIN1_TS_INSTANCES: each at 16- and 32-wide heads
LIN2_WS_INSTANCES = {1536: (3, 3), 1280: (4, 4), 768: (3, 3), 384: (3, 3)}  # LSL_LIN2_WS_INSTANCES: K2 -> (chunks, ring slots)


def lin1_lds(D, F, nw=8, lnf=False):
    """Lin1Cfg::lds_bytes / lds_bytes_lnf: weight ring (4 slots up to K = 256, else 3) + staging + bias (+ the modulation slots)."""
    ring = (4 if D <= 256 else 3) * 32 * (2 * D + 16)
    return ring + nw * 4096 + 4 * F + ((3 if D <= 256 else 2) * 2 * D * 4 if lnf else 0)


def linear1_ts_ok(hdp, D, F1, HHD, N):
    return F1 % 64 == 0 and HHD % 64 == 0 and N >= 1 and hdp in (16, 32) and D in LIN1_TS_HIDDEN and lin1_lds(D, F1) <= LDS_BUDGET


def linear1_ts_waves(D, N):
    return 4 if D == 512 and N <= 10240 else 8


def linear1_lnf_ok(hdp, D, F1, HHD, N, tpt, mod_stride):
    if not linear1_ts_ok(hdp, D, F1, HHD, N):
        return False
    min_tpt = 128 if D <= 256 else 256  # (LN_SLOTS >= 3: TT / 2, else TT, of the 8-wave instance)
    return (mod_stride == 0 or tpt >= min_tpt) and lin1_lds(D, F1, lnf=True) <= LDS_BUDGET


Lin1Split = namedtuple("Lin1Split", "TT ntile NB wpt grid ranges")


def linear1_ts_split(D, F1, N, cus=CUS):
    """launch_linear1_ts_t's work split and the kernel's (tile, block) range of every workgroup (k_lin1.hip.h "Work split")."""
    TT = 32 * linear1_ts_waves(D, N)
    ntile, NB = (N + TT - 1) // TT, F1 // 32
    units = ntile * NB
    wpt = min(cus // ntile, NB // 2)
    wpt = wpt if wpt >= 2 else 0
    grid = wpt * ntile if wpt else min(cus, units // 2)
    ranges = []
    for b in range(grid):
        if wpt:
            tile, part = divmod(b, wpt)
            i0 = tile * NB + ((NB * part // wpt) & ~1)
            i1 = tile * NB + (NB if part + 1 == wpt else (NB * (part + 1) // wpt) & ~1)
        else:
            i0 = (units * b // grid) & ~1
            i1 = units if b + 1 == grid else (units * (b + 1) // grid) & ~1
        ranges.append((i0, i1))
    return Lin1Split(TT, ntile, NB, wpt, grid, ranges)


def gemm_variant(lin2, F, K, N, cus=CUS):
    if lin2 and F % 192 == 0 and F % 256 != 0 and K % 64 == 0 and ((N + 127) // 128) * (F // 192) * 2 >= cus:
        return 28
    if F % 256 != 0 and F % 256 <= 128:
        return 11 if lin2 and K % 64 == 0 else 10
    tiles256 = ((N + 255) // 256) * ((F + 255) // 256)
    if K % 64 == 0 and tiles256 * (2 if lin2 else 4) <= cus * (1 if lin2 else 5):
        return 11
    return (7 if K % 128 == 0 else 15) if lin2 else (12 if K % 128 == 0 else 5)


GEMM_TILE = {5: (256, 256, 64, 2), 10: (128, 128, 32, 3), 11: (128, 128, 64, 2), 12: (256, 256, 64, 2), 7: (256, 256, 64, 2),
             15: (256, 256, 64, 2), 28: (192, 128, 64, 3)}  # tiling -> (features, tokens, k-tile depth, ring slots): launch_gemm


def linear2_ws_shape_ok(D, K2, ws_on=True):
    return ws_on and D % 128 == 0 and D <= 512 and K2 in LIN2_WS_INSTANCES


Lin2Grid = namedtuple("Lin2Grid", "slices rpx gate_rows ranges")


def linear2_ws_grid(F, N, tpt, shared, cus=CUS):
    slices, nblk = F // 128, (N + 31) // 32
    rpx = max(1, cus // (8 * slices))
    while rpx > 1 and 8 * rpx > nblk:
        rpx -= 1
    ranges = 8 * rpx
    max_blocks = (nblk + ranges - 1) // ranges + 1
    sizes = [nblk * (r + 1) // ranges - nblk * r // ranges for r in range(ranges)]  # blocks of every token range (the kernel's blk0, blk1)
    return Lin2Grid(slices, rpx, 1 if shared else (max_blocks * 32 + tpt - 1) // tpt + 1, sizes)


def linear2_ws_max_gate_rows(K2):
    """(160 KiB - Lin2Cfg::GATE) / 512: ring + hand-off + the hi waves' residual images (two blocks each) + bias come first."""
    nch, ns = LIN2_WS_INSTANCES[K2]
    kc = K2 // 2 // nch
    gate = ns * 32 * (4 * kc + 16) + 4 * 4096 + 4 * 8192 + 512
    return (163840 - gate) // 512


def tail_shape_ok(D, HHD, M):
    ring, wave = 4 * (D // 16) * 1024, 8 * max(4096, (D // 16 - D // 32) * 1024)  # TailCfg<256, 256>
    return D == 256 and HHD == 256 and M % 64 == 0 and M >= 64 and ring + wave + 4 * M <= LDS_BUDGET


def tail_grid(N, cus=CUS):
    return min((N + 31) // 32, cus)


def ln_form(D, N, cus=CUS):
    """launch_ln_mod_t: (kernel, workgroups)."""
    if D % 256 == 0:
        return "k_ln_modulate_v4", min((N + 3) // 4, cus * 16)
    return "k_ln_modulate", (N + 3) // 4


# ---- the plan of a debug_block pass and the labels lsl_profile_kernel_name reports (plan_pass, label_block: csrc/host_eval.hip.h) --------
Plan = namedtuple("Plan", "lin1 lin2 lin1_ts waves gemm1 lin2_kind gemm2 grid2 planes split")


def handle_flags(handle):
    parts = handle.split("+")
    return parts[0], "shared" in parts  # plain | tail | lnf, shared modulation row


def plan(case, cus=CUS, ws_on=True):
    """What lsl_debug_block_ex runs for the case (both sub-blocks: no rule below depends on the axis except the planes)."""
    model, B, T, L, handle = case[:5]
    d = dims(model)
    kind, shared = handle_flags(handle)
    tail = kind == "tail"
    n, tpt = B * T * L, T * L
    F1 = 3 * d.HHD if tail else d.F1
    ts = linear1_ts_ok(d.hdp, d.D, F1, d.HHD, n)
    waves = linear1_ts_waves(d.D, n)
    g1 = None if ts else gemm_variant(False, F1, d.D, n, cus)
    if ts:
        lin1 = "k_linear1_ts<%d, %d, %d>%s" % (d.hdp, d.D, waves, " (q | k | v)" if tail else "")
    else:
        lin1 = "k_gemm_glds<EpiLinear1<%d>> (tiling %d)" % (d.hdp, g1)
    w2p = not tail and linear2_ws_shape_ok(d.D, d.K2, ws_on)
    grid2 = linear2_ws_grid(d.D, n, tpt, shared, cus) if w2p and n * 4 * d.D < 2 ** 32 else None
    on_ws = grid2 is not None and grid2.gate_rows <= linear2_ws_max_gate_rows(d.K2)
    ln_stats = kind == "lnf" and w2p and linear1_lnf_ok(d.hdp, d.D, d.F1, d.HHD, n, tpt, 0 if shared else 1)
    assert not (ln_stats and not on_ws), case  # (plan_pass refuses such a pass)
    g2 = None
    if tail:
        assert tail_shape_ok(d.D, d.HHD, d.Mp), case
        lin2 = ["k_tail<%d, %d>" % (d.D, d.HHD)] * 2
        k2 = "tail"
    elif on_ws:
        # (lin2_stats: ln_stats and a next sub-block - of the two sub-blocks of a depth-1 model only the first)
        lin2 = ["k_linear2_ws<%d>%s" % (d.K2, " (+ row statistics)" if ln_stats and bi == 0 else "") for bi in (0, 1)]
        k2 = "ws"
    else:
        g2 = gemm_variant(True, d.D, d.K2, n, cus)
        lin2 = ["k_gemm_glds<EpiLinear2> (tiling %d)" % g2] * 2
        k2 = "gemm"
    # q / k / v as planes on the SPATIAL sub-block (the temporal one never): token-stationary linear1 and attention_stream_mode 2 with at most
    # 256 positions, i.e. 129 <= L <= 256 (qkv_planes_ok; attention_cases.plan_axis restates the attention side in full).  No label names the
    # layout, so the GPU run does not confirm this flag: it only says which cases are meant to reach the plane stores.
    planes = ts and d.H % (64 // d.hdp) == 0 and 129 <= L <= 256
    return Plan(lin1, tuple(lin2), ts, waves, g1, k2, g2, grid2 if on_ws else None, planes, linear1_ts_split(d.D, F1, n, cus) if ts else None)


# ---- the case table: (model, B, T, L, handle form, linear1 label, linear2 label of sub-block 0) ------------------------------------------
# handle form: plain | tail | lnf, "+shared" = one modulation row (mod_rows = 1).  Both sub-blocks of a case are checked.  The labels are
# written out by `_c` from the short forms below and test_gemm_cases.py derives them again from `plan`.
def _ts(model, nw, qkv=False):
    d = dims(model)
    return "k_linear1_ts<%d, %d, %d>%s" % (d.hdp, d.D, nw, " (q | k | v)" if qkv else "")


def _g1(model, tiling):
    return "k_gemm_glds<EpiLinear1<%d>> (tiling %d)" % (dims(model).hdp, tiling)


def _ws(model, stats=False):
    return "k_linear2_ws<%d>%s" % (dims(model).K2, " (+ row statistics)" if stats else "")


def _g2(tiling):
    return "k_gemm_glds<EpiLinear2> (tiling %d)" % tiling


TAIL = "k_tail<256, 256>"


def _c(model, B, T, L, handle, lin1, lin2):
    return (model, B, T, L, handle, lin1, lin2)


def _ts_ws(model, nw, shapes, handle="plain"):
    return tuple(_c(model, B, T, L, handle, _ts(model, nw), _ws(model)) for B, T, L in shapes)


CASES = (
    # -- hidden 128 (k_ln_modulate<2, 2>, k_linear1_ts<., 128, 8>, k_linear2_ws<384>: one slice, 32 token ranges per XCD) -------------------
    # n = 1, 3, 4, 5 (LayerNorm: one workgroup of four waves, a partial one, two), 31, 32, 33 (linear2 blocks), 255, 256, 257 (linear1 tile)
    *_ts_ws("d128h4r2", 8, ((1, 1, 1), (3, 1, 1), (1, 2, 2), (5, 1, 1), (1, 31, 1), (2, 2, 8), (11, 1, 3), (5, 3, 17), (1, 2, 128), (1, 257, 1))),
    *_ts_ws("d128h8r2", 8, ((1, 1, 1), (3, 1, 11), (1, 255, 1), (2, 1, 129), (7, 5, 9))),
    # 7, 8 and 9 blocks of 32 tokens; three tokens per trajectory (two or three gate rows inside a block); the shared row
    *_ts_ws("d128h4r2", 8, ((70, 1, 3), (85, 3, 1), (1, 3, 86), (96, 1, 3))),
    *_ts_ws("d128h4r2", 8, ((3, 1, 1), (11, 1, 3), (5, 3, 17), (96, 1, 3)), "plain+shared"),
    # one token per trajectory: 65 or 97 gate rows of 172
    *_ts_ws("d128h4r2", 8, ((33, 1, 1), (300, 1, 1))),
    # -- hidden 256 (k_ln_modulate_v4<4>, k_linear1_ts<., 256, 8>, k_linear2_ws<768>: two slices) -------------------------------------------
    *_ts_ws("d256h8r2", 8, ((1, 1, 1), (1, 3, 1), (2, 2, 1), (5, 1, 1), (1, 1, 31), (1, 32, 1), (3, 11, 1), (1, 5, 51), (1, 256, 1), (257, 1, 1))),
    *_ts_ws("d256h16r2", 8, ((1, 1, 1), (3, 1, 11), (1, 1, 255), (2, 129, 1), (7, 5, 9))),
    *_ts_ws("d256h8r2", 8, ((70, 1, 3), (85, 3, 1), (1, 3, 86), (3, 11, 1), (1, 5, 51)), "plain+shared"),
    # planes on the spatial sub-block (L = 160), rows on the temporal one; a wide q | k | v pitch
    *_ts_ws("d256h8r2", 8, ((1, 2, 160),)), *_ts_ws("d128h4r2", 8, ((1, 3, 129),)),
    # the gate-table limit at one token per trajectory (124 rows): 8 192 tokens are 256 blocks, two per range + 1 -> 97 rows; 8 193 -> 129
    _c("d256h8r2", 8192, 1, 1, "plain", _ts("d256h8r2", 8), _ws("d256h8r2")),
    _c("d256h8r2", 8193, 1, 1, "plain", _ts("d256h8r2", 8), _g2(11)),
    # ln_fuse handles (the + row statistics instance on the first sub-block): shared row, or 128 tokens and more per trajectory
    _c("d256h8r2", 3, 11, 1, "lnf+shared", _ts("d256h8r2", 8), _ws("d256h8r2", True)),
    _c("d256h8r2", 2, 2, 80, "lnf", _ts("d256h8r2", 8), _ws("d256h8r2", True)),
    _c("d128h4r2", 96, 1, 3, "lnf+shared", _ts("d128h4r2", 8), _ws("d128h4r2", True)),
    _c("d384h16r2", 1, 5, 51, "lnf+shared", _ts("d384h16r2", 8), _ws("d384h16r2", True)),
    _c("d512h16r2", 1, 3, 86, "lnf", _ts("d512h16r2", 4), _ws("d512h16r2", True)),
    # -- hidden 384 (k_ln_modulate<6, 2>, k_linear1_ts<., 384, 8>, k_linear2_ws<1280>: three slices, 10 ranges per XCD) ----------------------
    *_ts_ws("d384h16r2", 8, ((1, 1, 4), (1, 31, 1), (2, 1, 16), (1, 33, 1), (3, 1, 11), (1, 5, 51), (2, 1, 128), (1, 257, 1), (1, 3, 86))),
    *_ts_ws("d384h16r2", 8, ((1, 1, 1), (3, 1, 11), (1, 3, 86)), "plain+shared"),
    _c("d384h24r2", 1, 5, 51, "plain", _ts("d384h24r2", 8), _g2(11)), _c("d384h24r2", 3, 1, 11, "plain", _ts("d384h24r2", 8), _g2(11)),
    # -- hidden 512 (k_ln_modulate_v4<8>, k_linear1_ts<., 512, 4 | 8>, k_linear2_ws<1536>: four slices, 8 ranges per XCD) ---------------------
    # 4 waves: tiles of 128 tokens: n = 1, 127, 128, 129 and a ragged last tile
    *_ts_ws("d512h16r2", 4, ((1, 31, 1), (2, 16, 1), (1, 127, 1), (2, 1, 64), (1, 3, 43), (3, 1, 11), (1, 5, 51), (1, 3, 86))),
    *_ts_ws("d512h32r2", 4, ((1, 1, 5), (3, 1, 11), (1, 129, 1))),
    *_ts_ws("d512h16r2", 4, ((1, 1, 1), (1, 3, 86), (1, 5, 51)), "plain+shared"),
    # token ranges of exactly 2, of 2 and 3, of exactly 3 blocks on 64 ranges
    *_ts_ws("d512h16r2", 4, ((1, 16, 256), (2, 40, 64), (3, 1, 2048))),
    # 28 gate rows: three tokens per trajectory fit with ranges of one block (23 rows), not with two (33)
    _c("d512h16r2", 85, 1, 3, "plain", _ts("d512h16r2", 4), _ws("d512h16r2")), _c("d512h16r2", 86, 3, 1, "plain", _ts("d512h16r2", 4), _g2(11)),
    # either side of 10 240 tokens: 4 and 8 waves
    _c("d512h16r2", 2, 20, 256, "plain", _ts("d512h16r2", 4), _ws("d512h16r2")), _c("d512h16r2", 1, 10241, 1, "plain", _ts("d512h16r2", 8), _ws("d512h16r2")),
    _c("d512h32r2", 1, 1, 10241, "plain+shared", _ts("d512h32r2", 8), _ws("d512h32r2")),
    # -- the even cut of k_linear1_ts: more than CUs / 2 tiles -------------------------------------------------------------------------------
    _c("d128h4r2", 1, 129, 255, "plain", _ts("d128h4r2", 8), _ws("d128h4r2")), _c("d128h8r2", 2, 255, 65, "plain+shared", _ts("d128h8r2", 8), _ws("d128h8r2")),
    _c("d512h16r2", 1, 255, 129, "plain", _ts("d512h16r2", 8), _ws("d512h16r2")),
    # -- linear1 on the tile GEMM --------------------------------------------------------------------------------------------------------------
    # hidden 64 (K = 64: one k-tile for two ring slots): tiling 11 at n = 1, 127, 128, 129; 10 on the ragged F1 = 320; 5 above 40 960 tokens
    *(_c("d64h2r1", B, T, L, "plain", _g1("d64h2r1", 11), _g2(11)) for B, T, L in ((1, 1, 1), (1, 127, 1), (2, 1, 64), (3, 43, 1), (5, 3, 1))),
    *(_c("d64h4r2", B, T, L, "plain", _g1("d64h4r2", 10), _g2(11)) for B, T, L in ((1, 1, 1), (1, 1, 127), (1, 128, 1), (1, 3, 43), (4, 1, 1))),
    _c("d64h4r2", 3, 1, 11, "plain+shared", _g1("d64h4r2", 10), _g2(11)),
    _c("d64h2r5", 1, 160, 256, "plain", _g1("d64h2r5", 11), _g2(11)), _c("d64h2r5", 1, 257, 160, "plain", _g1("d64h2r5", 5), _g2(11)),
    # hidden 192 (F1 = 960: 3.75 feature tiles of 256; K = 192: three k-tiles): 11 up to 20 480 tokens, 5 above; linear2 28 from 16 257
    *(_c("d192h8r1", B, T, L, "plain", _g1("d192h8r1", 11), _g2(11)) for B, T, L in ((1, 1, 1), (1, 127, 1), (1, 1, 129), (3, 1, 11), (2, 127, 64))),
    _c("d192h8r1", 1, 16257, 1, "plain", _g1("d192h8r1", 11), _g2(28)), _c("d192h8r1", 1, 80, 256, "plain+shared", _g1("d192h8r1", 11), _g2(28)),
    _c("d192h8r1", 1, 255, 81, "plain", _g1("d192h8r1", 5), _g2(28)),
    # hidden 320 (K = 320: five k-tiles): 11 up to 16 384 tokens, 5 above
    *(_c("d320h10r1", B, T, L, "plain", _g1("d320h10r1", 11), _g2(11)) for B, T, L in ((1, 1, 1), (5, 1, 1), (1, 3, 43), (3, 1, 11))),
    _c("d320h10r1", 1, 64, 256, "plain", _g1("d320h10r1", 11), _g2(11)), _c("d320h10r1", 1, 255, 65, "plain", _g1("d320h10r1", 5), _g2(11)),
    # hidden 448 (K = 448: seven k-tiles; 28 of 32): 11 up to 10 240 tokens, 5 above; linear2 11 up to 16 384, 15 above
    *(_c("d448h16r1", B, T, L, "plain", _g1("d448h16r1", 11), _g2(11)) for B, T, L in ((1, 1, 1), (1, 1, 3), (1, 129, 1), (3, 1, 11))),
    _c("d448h16r1", 1, 40, 256, "plain", _g1("d448h16r1", 11), _g2(11)), _c("d448h16r1", 1, 255, 41, "plain", _g1("d448h16r1", 5), _g2(11)),
    _c("d448h16r1", 1, 64, 256, "plain", _g1("d448h16r1", 5), _g2(11)), _c("d448h16r1", 1, 10495, 1, "plain", _g1("d448h16r1", 5), _g2(11)),
    _c("d448h16r1", 1, 1, 10497, "plain", _g1("d448h16r1", 5), _g2(11)), _c("d448h16r1", 1, 16385, 1, "plain+shared", _g1("d448h16r1", 5), _g2(15)),
    # -- linear2 on the tile GEMM: 7 from 16 385 tokens (K2 = 1024), 28 from 8 065 on the 384-wide model, 11 below each ------------------------
    *(_c("d512h16r1", B, T, L, "plain", _ts("d512h16r1", 4), _g2(11)) for B, T, L in ((1, 1, 1), (1, 127, 1), (1, 1, 128), (3, 43, 1))),
    _c("d512h16r1", 1, 64, 256, "plain", _ts("d512h16r1", 8), _g2(11)), _c("d512h16r1", 1, 16385, 1, "plain", _ts("d512h16r1", 8), _g2(7)),
    _c("d384h16r1", 1, 63, 128, "plain", _ts("d384h16r1", 8), _g2(11)), _c("d384h16r1", 1, 8065, 1, "plain", _ts("d384h16r1", 8), _g2(28)),
    _c("d384h16r1", 1, 3, 43, "plain+shared", _ts("d384h16r1", 8), _g2(11)),
    # -- k_tail (hidden 256, 8 x 32 or 16 x 16 heads): M = 64, 128, 512, 1024; n = 1, 31, 32, 33; 8 193 tokens: two wave tiles per workgroup ----
    *(_c(m, B, T, L, "tail", _ts(m, 8, True), TAIL) for m in ("d256h8r025", "d256h8r05", "d256h8r2", "d256h16r4")
      for B, T, L in ((1, 1, 1), (1, 31, 1), (2, 1, 16), (11, 1, 3))),
    _c("d256h16r2", 3, 1, 11, "tail", _ts("d256h16r2", 8, True), TAIL), _c("d256h16r2", 1, 5, 51, "tail+shared", _ts("d256h16r2", 8, True), TAIL),
    _c("d256h8r2", 11, 1, 3, "tail+shared", _ts("d256h8r2", 8, True), TAIL), _c("d256h8r05", 33, 1, 1, "tail", _ts("d256h8r05", 8, True), TAIL),
    _c("d256h8r025", 1, 8193, 1, "tail", _ts("d256h8r025", 8, True), TAIL), _c("d256h8r2", 3, 2731, 1, "tail+shared", _ts("d256h8r2", 8, True), TAIL),
)


def case_id(case):
    return case[0] + "-" + "x".join(str(v) for v in case[1:4]) + "-" + case[4]


def n_tokens(case):
    return case[1] * case[2] * case[3]


def ws_cases():
    """The cases whose linear2 runs k_linear2_ws: rerun on the tile GEMM in a child with LSL_LIN2_WS=0."""
    return tuple(c for c in CASES if c[6].startswith("k_linear2_ws"))


WS_OFF_KNOB = "LSL_LIN2_WS"


# ---- parameters and inputs -----------------------------------------------------------------------------------------------------------------
def bf16(x):
    return x.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def params(model):
    """random_params(seed 21) with linear1 / linear2 weights rounded to bf16 (what pack_block rounds them to)."""
    sh = net_shape(model)
    p = latent_net.random_params(sh, seed=21)
    for k in sorted(p):
        if k.endswith(("linear1.weight", "linear2.weight")):
            p[k] = bf16(p[k])
    return sh, p


BLOCK_NAMES = ("blocks.0.spatial_block", "blocks.0.temporal_block")


@functools.lru_cache(maxsize=None)
def packed(model, bi):
    """pack_block's tensors of sub-block bi on the CPU: w1 [F1 up to 256][D], w2 [D up to 256][K2] bf16; b1, b2, qs, ks fp32."""
    from lam_slide_amd import packing
    sh, p = params(model)
    dm = packing.make_dims(1, sh.in_dim, sh.hidden_size, sh.num_heads, sh.mlp_ratio, None, False, sh.theta)
    d = dims(model)
    assert (dm.hhd, dm.mlp_dim_pad, dm.f1, dm.k2, dm.head_dim_pad) == (d.HHD, d.Mp, d.F1, d.K2, d.hdp), (model, dm)
    return packing.pack_block(p, BLOCK_NAMES[bi], dm, "cpu")


@functools.lru_cache(maxsize=4)
def inputs(model, B, T, L, shared=False):
    D = MODELS[model][0]
    g = torch.Generator().manual_seed(3)
    h = torch.randn(B, T, L, D, generator=g)
    mods = (torch.randn(B, 8 * D, generator=g) * 0.3).contiguous()
    if shared:
        mods = mods[:1].expand(B, 8 * D).contiguous()
    return h, mods


def premul_of(model):
    return LOG2E / math.sqrt(dims(model).hd)


def token_geometry(B, T, L, bi, device="cpu"):
    """(trajectory, position along the attended axis) of every token."""
    n = torch.arange(B * T * L, device=device)
    return n // (T * L), ((n // L) % T if bi & 1 else n % L)


def mod_rows(mods, bi, D, traj):
    """shift, scale, gate [n, D] of sub-block bi for every token (run_block: mods + (bi / 2) 6 D + (temporal ? 3 D : 0))."""
    o = 3 * D if bi & 1 else 0
    m = mods.double()
    return m[traj, o:o + D], m[traj, o + D:o + 2 * D], m[traj, o + 2 * D:o + 3 * D]


def rope_table(model, n_pos, device="cpu"):
    """cos, sin [n_pos, hd / 2] as run_tables builds them: fp64 angles, rounded once to fp32 (oracle.latent_net.rope_cos_sin)."""
    sh = net_shape(model)
    cs, sn = latent_net.rope_cos_sin(n_pos, sh.head_dim, sh.theta)
    return cs.double().to(device), sn.double().to(device)


def rnd(y):
    """Half a unit in the last place of bf16 at |y|: u_b times the power of two above |y| (0 at 0)."""
    _, e = torch.frexp(y.abs())
    return torch.where(y == 0, torch.zeros_like(y), UB * torch.ldexp(torch.ones_like(y), e))


def rounded(y, t):
    """The bar of bf16(y + d), |d| <= t."""
    return rnd(y.abs() + t) + t


# ---- fp64 references with their bars: every function returns {name: (reference, bar)} on the device of its operands ----------------------
def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def a_reference(h, shift, scale):
    """h [n, D] fp64; shift, scale [n, D]: LayerNorm (eps 1e-6) + modulate and its bar."""
    mean = h.mean(-1, keepdim=True)
    dev = h - mean
    rstd = torch.rsqrt((dev * dev).mean(-1, keepdim=True) + 1e-6)
    xhat = dev * rstd
    a = xhat * (1 + scale) + shift
    inner = (1 + scale).abs() * (24 * U * xhat.abs() + 16 * U * rstd * h.abs().mean(-1, keepdim=True)) + 4 * U * a.abs()
    return {"a": (a, rounded(a, inner))}


def _chain(x, w, b):
    """x [n, K], w [F, K], b [F] fp64 -> acc = x w^T + b and S = |x| |w|^T + |b|."""
    return x @ w.t() + b, x.abs() @ w.abs().t() + b.abs()


def linear1_reference(a, pk, model, pos, cos, sin, mlp=True, swap_scales=False):
    """The linear1 outputs from the tapped operand a [n, D] (fp64 of bf16 values): q, k [n, H, hd] (q times the pre-multiplier), v
    [n, H, hd], gelu [n, Mp], each with its bar.  cos, sin: [n_pos, hd / 2]; pos [n]."""
    d = dims(model)
    dev = a.device
    K, H, hd, hdp = d.D, d.H, d.hd, d.hdp
    w1, b1 = pk["w1"].double().to(dev), pk["b1"].double().to(dev)
    acc, S = _chain(a, w1[:d.F1], b1[:d.F1]) if mlp else _chain(a, w1[:3 * d.HHD], b1[:3 * d.HHD])
    e = (K + 2) * U * S
    out = {}
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]  # [n, 1, hd / 2]
    for i, name in enumerate(("q", "k")):
        x = acc[:, i * d.HHD:(i + 1) * d.HHD].reshape(-1, H, hdp)[:, :, :hd]
        ex = e[:, i * d.HHD:(i + 1) * d.HHD].reshape(-1, H, hdp)[:, :, :hd]
        sc = pk["ks" if (i == 1) != swap_scales else "qs"].double().to(dev)[:hd]
        pre = premul_of(model) if i == 0 else 1.0
        rr = torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6)
        y, ey = x * sc, ex * sc.abs()
        y0, y1, e0, e1 = y[..., 0::2], y[..., 1::2], ey[..., 0::2], ey[..., 1::2]
        r0, r1 = c * y0 - s * y1, s * y0 + c * y1
        q = pre * rr * torch.stack([r0, r1], -1).reshape(x.shape)
        rot = pre * rr * torch.stack([c.abs() * e0 + s.abs() * e1, s.abs() * e0 + c.abs() * e1], -1).reshape(x.shape)
        norm = q.abs() * rr * rr * (x.abs() * ex).mean(-1, keepdim=True)
        mag = (y0.abs() + y1.abs()).repeat_interleave(2, -1)
        fp32 = ((hd / 2 + 12) * U + pos.double()[:, None, None] * 2.0 ** -50) * pre * rr * mag
        out[name] = (q, rounded(q, rot + norm + fp32))
    v = acc[:, 2 * d.HHD:3 * d.HHD].reshape(-1, H, hdp)[:, :, :hd]
    ev = e[:, 2 * d.HHD:3 * d.HHD].reshape(-1, H, hdp)[:, :, :hd]
    out["v"] = (v, rounded(v, ev))
    if mlp:
        g = gelu64(acc[:, 3 * d.HHD:])
        out["gelu"] = (g, rounded(g, GELU_SLOPE * e[:, 3 * d.HHD:] + GELU_FIT + 4 * U * g.abs()))
    return out


def linear2_reference(h, z, gate, pk, model):
    """h_out = h + gate (z W2^T + b2) from the tapped z [n, K2] (fp64 of bf16 values), h [n, D], gate [n, D] (fp64 of fp32 values)."""
    d = dims(model)
    dev = h.device
    acc, S = _chain(z, pk["w2"].double().to(dev)[:d.D], pk["b2"].double().to(dev))
    ref = h + gate * acc
    return {"h_out": (ref, gate.abs() * (d.K2 + 3) * U * S + 2 * U * ref.abs())}


def tail_reference(h, a, z_attn, gate, pk, model, with_linear2_bar=False):
    """k_tail: the up-projection and its GELU in fp64 from the tapped a, unrounded, then linear2 over [tapped attention | gelu]."""
    d = dims(model)
    dev = h.device
    w1, b1 = pk["w1"].double().to(dev), pk["b1"].double().to(dev)
    w2, b2 = pk["w2"].double().to(dev)[:d.D], pk["b2"].double().to(dev)
    u, S1 = _chain(a, w1[3 * d.HHD:d.F1], b1[3 * d.HHD:d.F1])
    g = gelu64(u)
    acc, S = _chain(torch.cat([z_attn, g], -1), w2, b2)
    eg = rounded(g, GELU_SLOPE * (d.D + 2) * U * S1 + GELU_FIT + 4 * U * g.abs())
    ref = h + gate * acc
    lin2_bar = gate.abs() * (d.K2 + 3) * U * S + 2 * U * ref.abs()
    bar = lin2_bar + gate.abs() * (eg @ w2[:, d.HHD:].abs().t())
    out = {"h_out": (ref, bar)}
    if with_linear2_bar:
        out["linear2_bar"] = (ref, lin2_bar)
    return out


def worst(got, ref_bar):
    """(worst |got - ref| / bar, its flat index); non-finite values count as infinite."""
    ref, bar = ref_bar
    r = (got.double().reshape(ref.shape) - ref).abs() / bar.clamp_min(1e-300)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), i


def heads_real(x, model):
    """[n, HHD] (padded heads) -> real channels [n, H, hd] and the padded ones [n, H, hdp - hd]."""
    d = dims(model)
    x = x.reshape(-1, d.H, d.hdp)
    return x[:, :, :d.hd], x[:, :, d.hd:]


def pad_heads(x, model):
    """[n, H, hd] -> [n, HHD] with zero padded channels."""
    d = dims(model)
    out = torch.zeros(x.shape[0], d.H, d.hdp, dtype=x.dtype, device=x.device)
    out[:, :, :d.hd] = x
    return out.reshape(x.shape[0], d.HHD)


# ---- the kernels' roundings, emulated on the CPU, with the mutations of test_gemm_cases.py -----------------------------------------------
def _chain32(x, w, b, bias_first, drop=None):
    """fp32 accumulation in 16-deep steps, k ascending: from the bias (linear1) or from zero with the bias added behind (linear2).
    drop = (token tile of 32, feature tile of 32, k-step): that step is left out of that 32 x 32 tile."""
    x, w, b = x.float(), w.float(), b.float()
    acc = b.expand(x.shape[0], -1).clone() if bias_first else torch.zeros(x.shape[0], w.shape[0])
    for ks in range(0, x.shape[1], 16):
        step = x[:, ks:ks + 16] @ w[:, ks:ks + 16].t()
        if drop is not None and drop[2] == ks // 16:
            step[32 * drop[0]:32 * drop[0] + 32, 32 * drop[1]:32 * drop[1] + 32] = 0
        acc = acc + step
    return acc if bias_first else acc + b


def emulate_a(h, shift, scale):
    """k_ln_modulate: fp32 statistics, one bf16 rounding."""
    h = h.float()
    mean = h.mean(-1, keepdim=True)
    dev = h - mean
    rstd = torch.rsqrt((dev * dev).mean(-1, keepdim=True) + 1e-6)
    return bf16(dev * rstd * (1.0 + scale.float()) + shift.float())


def emulate_linear1(a, pk, model, pos, cos, sin, mlp=True, drop=None, no_bias_tile=None, pos_shift_token=None, swap_scales=False,
                    premul=True, untouched_from=None):
    """EpiLinear1's arithmetic in fp32 on the bf16 operand a: q, k, v [n, H, hd] and gelu [n, Mp] as bf16 values.  Mutations: drop (as
    _chain32), no_bias_tile (feature tile of 32 without its bias), pos_shift_token (that token rotated at its position + 1),
    swap_scales, premul=False, untouched_from (rows from that token on are left zero: a partial last tile that was not written)."""
    d = dims(model)
    H, hd, hdp = d.H, d.hd, d.hdp
    F = d.F1 if mlp else 3 * d.HHD
    b1 = pk["b1"][:F].clone()
    if no_bias_tile is not None:
        b1[32 * no_bias_tile:32 * no_bias_tile + 32] = 0
    acc = _chain32(a, pk["w1"][:F], b1, True, drop)
    if pos_shift_token is not None:
        pos = pos.clone()
        pos[pos_shift_token] = (pos[pos_shift_token] + 1) % cos.shape[0]
    c, s = cos.float()[pos][:, None, :], sin.float()[pos][:, None, :]
    out = {}
    for i, name in enumerate(("q", "k")):
        x = acc[:, i * d.HHD:(i + 1) * d.HHD].reshape(-1, H, hdp)[:, :, :hd]
        sc = pk["ks" if (i == 1) != swap_scales else "qs"][:hd]
        pre = float(premul_of(model)) if i == 0 and premul else 1.0
        rr = torch.rsqrt((x * x).sum(-1, keepdim=True) * (1.0 / hd) + 1e-6) * pre
        x0, x1, s0, s1 = x[..., 0::2], x[..., 1::2], sc[0::2], sc[1::2]
        r0 = rr * ((c * s0) * x0 - (s * s1) * x1)
        r1 = rr * ((s * s0) * x0 + (c * s1) * x1)
        out[name] = bf16(torch.stack([r0, r1], -1).reshape(x.shape))
    out["v"] = bf16(acc[:, 2 * d.HHD:3 * d.HHD].reshape(-1, H, hdp)[:, :, :hd])
    if mlp:
        out["gelu"] = bf16(gelu64(acc[:, 3 * d.HHD:].double()).float())
    if untouched_from is not None:
        for k in out:
            out[k] = out[k].clone()
            out[k][untouched_from:] = 0
    return out


def emulate_linear2(h, z, gate, pk, model, drop=None, no_bias_tile=None, gate_block=None, residual_next=False, untouched_from=None):
    """EpiLinear2 / k_linear2_ws: the fp32 chain from zero, + bias, fma with the gate onto the residual.  Mutations: drop, no_bias_tile,
    gate_block = (block of 32 tokens, tokens per trajectory): that block takes the gate rows of the next trajectory; residual_next: every
    row is updated onto the residual row of the next token; untouched_from."""
    d = dims(model)
    b2 = pk["b2"].clone()
    if no_bias_tile is not None:
        b2[32 * no_bias_tile:32 * no_bias_tile + 32] = 0
    acc = _chain32(z, pk["w2"][:d.D], b2, False, drop)
    gate = gate.float()
    if gate_block is not None:
        blk, tpt = gate_block
        rows = torch.arange(32 * blk, min(32 * blk + 32, h.shape[0]))
        gate = gate.clone()
        gate[rows] = gate[(rows + tpt) % h.shape[0]]
    hh = h.float().roll(-1, 0) if residual_next else h.float()
    out = (gate.double() * acc.double() + hh.double()).float()
    if untouched_from is not None:
        out[untouched_from:] = h.float()[untouched_from:]
    return out


def emulate_tail(h, a, z_attn, gate, pk, model, drop_mlp_block=None, **kw):
    """k_tail: the up-projection from its bias in fp32, GELU rounded to bf16, then linear2's chain over [attention | gelu].
    drop_mlp_block: that 32-feature block of the mlp never reaches the down-projection."""
    d = dims(model)
    u = _chain32(a, pk["w1"][3 * d.HHD:d.F1], pk["b1"][3 * d.HHD:d.F1], True)
    g = bf16(gelu64(u.double()).float())
    if drop_mlp_block is not None:
        g[:, 32 * drop_mlp_block:32 * drop_mlp_block + 32] = 0
    return emulate_linear2(h, torch.cat([z_attn.float(), g], -1), gate, pk, model, **kw)
