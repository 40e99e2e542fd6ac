"""The case table of the per-row attention tests (test_attention_cases.py on the CPU, test_hip_attention.py on the MI355X): models and
shapes that reach every form plan_attention (csrc/host_launch.hip.h) can pick - k_attention_tiny, the three instances of
k_attention_rows the default path uses and the three behind LSL_ATTN_STREAM=0, k_attention_stream short / grouped / long / chunked /
chunked with the denominator column, k_attention_linear - at the lengths where each changes behaviour; the fp64 references; the
per-element bounds; and the conditions (key coverage, softmax regime, form) under which a passing comparison means something.  Not a
test module.

Reference.  lsl_debug_taps hands out the bf16 q | k | v exactly as the attention kernel reads them (q already times head_dim^-1/2 log2 e)
and its bf16 output z.  In fp64, with exact products of those bf16 values:  s = q k^T,  p = 2^s / sum_j 2^s,  o = p v,  A = p |v|.
Only the kernel's own roundings separate z from o.

Bound of the MFMA forms (k_attention_rows, k_attention_stream).  u = 2^-8 is the relative error of one round-to-nearest-even to bf16
(pack2, common.hip.h).
  * every unnormalised probability is rounded once (p_frag): the numerator sum_j p_j v_j moves by at most u A, the denominator by at
    most u (relative), which moves o by at most u |o| <= u A;
  * the output row is rounded once more (o_pack): at most u |o| <= u A.
Total 3 u A; the bar is 4 u A = 2^-6 A per element.  The spare u A covers the second-order terms, the fp32 accumulation of scores and
sums and v_exp_f32 (at |s| <= 300 and 32 channels together below 1e-3 relative).
Bound of k_attention_tiny (fp32 probabilities): 2^-8 |o| + (S + head_dim + 16) 2^-23 A - the output rounding plus an fp32 chain of
S + head_dim + 16 operations with a factor 2.
k_attention_linear (read: csrc/k_attn.hip.h) unpacks bf16 rows into fp32 and stays there - channel maxima, __expf, the context sums,
the normalisation and the output products are all fp32, the one bf16 rounding is row_pack on the way out - so its bound is the tiny
kernel's with A_lin = q_s (k_s^T |v|) in place of A.
What the kernels measure in these units on MI355X: profiles/attention_rowwise_parity.txt (MFMA forms 0.66 .. 2.26 u A; the emulation
of the same roundings on the CPU, test_attention_cases.py: 0.7 .. 1.7 u A).

Key coverage.  At the sharp gain of a case, every key position j has p_j >= 0.25 for some (sequence, head, query) of the fp64
reference: a key that is dropped, duplicated or wrongly masked then moves some element by about 0.25 |v - o| against a bar of
0.016 A.  Every case has 16 or more (sequence, head) pairs on each axis for that.

The inputs of a case are h_in = randn [B, T, L, D] and mods = 0.3 randn [B, 8 D] (generator seed 3), the weights
oracle.latent_net.random_params(seed 21) with the query / key norm scales multiplied by the arm's gain.  On the CPU the same h_in and
mods go through the oracle's LayerNorm + modulate and latent_net.attn_mlp_block (what latent_net.forward runs per sub-block), so the
conditions evaluated there are those of the GPU run up to the bf16 rounding of linear1."""
import functools
import math
from collections import namedtuple

import torch

from oracle import latent_net

U = 2.0 ** -8
LOG2E = 1.4426950408889634
MFMA_BAR_UA = 4.0  # 2^-6 A in units of u A

# ---- models: depth 1, mlp_ratio 1, in_dim 16 (every one accepted by lsl_model_create) -----------------------------------------------
MODELS = {
    "d64h2": (64, 2),      # 32 wide, tile-GEMM linear1, heads not a multiple of 8
    "d128h4": (128, 4),    # 32 wide, token-stationary linear1
    "d128h8": (128, 8),    # 16 wide
    "d192h8": (192, 8),    # 24 of 32, tile-GEMM linear1: token-major rows
    "d384h16": (384, 16),  # 24 of 32, token-stationary: planes
    "d256h8": (256, 8),    # 32 wide, heads a multiple of 8
    "d256h16": (256, 16),  # 16 wide
    "d448h16": (448, 16),  # 28 of 32: padded without the denominator column
}
LIN1_TS_HIDDEN = (128, 256, 384, 512)  # LSL_LIN1_TS_INSTANCES, host_launch.hip.h:170


def net_shape(model, linear=False):
    D, H = MODELS[model]
    return latent_net.NetShape(depth=1, in_dim=16, hidden_size=D, num_heads=H, mlp_ratio=1,
                               attention_mode="linear" if linear else "scaled_dot_product")


def head_dims(model):
    D, H = MODELS[model]
    hd = D // H
    return hd, (16 if hd <= 16 else 32)


# ---- plan_attention restated (csrc/host_launch.hip.h:393-480: attention_stream_mode, attention_grouped_ok, attention_rows_max_s,
# plan_attention; the planes rule: qkv_planes_ok, :483-486; a.bound: attention_args, csrc/host_eval.hip.h:237) ------------------------
LDS_BUDGET = 160 * 1024
Plan = namedtuple("Plan", "kernel form S n_seq inner outer_stride pos_stride blk planes bound")


def rows_max_s(hdp):
    return ((LDS_BUDGET - 16 * 4) // (4 * hdp)) & ~31


def plan_axis(model, B, T, L, temporal, linear=False, stream=True, group=True, planes_on=True):
    """What the attention of one axis runs: the kernel class lsl_profile_kernel_name reports, the finer form, the axis geometry
    (token of (seq, pos) = (seq // inner) * outer_stride + seq % inner + pos * pos_stride), the block of a packed launch, whether q / k / v
    travel as planes, whether k_attention_rows is given the Cauchy-Schwarz bound."""
    D, H = MODELS[model]
    hd, hdp = head_dims(model)
    if temporal:
        S, n_seq, inner, outer, pstr = T, B * L, L, T * L, L
    else:
        S, n_seq, inner, outer, pstr = L, B * T, 1, L, 1
    mk = lambda kernel, form, blk=0, planes=False: Plan(kernel, form, S, n_seq, inner, outer, pstr, blk, planes, S > 96)  # noqa: E731
    if linear:
        return mk("k_attention_linear", "linear")
    grouped = group and stream and 2 <= S <= 8 and S & (S - 1) == 0 and not temporal and H % 8 == 0
    Sk = 32 if grouped else S
    mode = 0 if not stream else 2 if Sk >= 129 else 1 if 8 < Sk <= 32 and H % 8 == 0 else 0
    if mode:  # (launches of 2^31 units and more leave the stream kernel: no case comes near)
        if mode == 1:
            return mk("k_attention_stream", "grouped" if grouped else "short", blk=S if grouped else 0)
        planes = planes_on and not temporal and D in LIN1_TS_HIDDEN and H % (64 // hdp) == 0 and S <= 256
        form = "long" if S <= 256 else "chunked_den" if (hdp, hd) == (32, 24) else "chunked"
        return mk("k_attention_stream", form, planes=planes)
    rt = "k_attention_rows / k_attention_tiny"
    if S <= 8:
        return mk(rt, "tiny")
    Sp = (S + 31) & ~31
    assert Sp <= rows_max_s(hdp), (model, S)
    if Sp > 256:
        return mk(rt, "rows<16,1,0>")
    if Sp <= 32:
        return mk(rt, "rows<4,4,1>")
    if Sp <= 64:
        return mk(rt, "rows<4,2,2>")
    if Sp <= 128:
        return mk(rt, "rows<4,1,4>")
    return mk(rt, "rows<4,1,6>" if Sp <= 192 else "rows<4,1,8>")


def is_mfma(form):
    return form not in ("tiny", "linear")


# ---- the case table: (model, B, T, L, form of the spatial axis (positions l), form of the temporal axis (positions t)) -----------------
# Both sub-blocks of a case are checked.  The forms are written out and test_attention_cases.py derives them again from plan_axis.
def _c(model, B, T, L, sp, tm):
    return (model, B, T, L, sp, tm)


R441, R422, R414 = "rows<4,4,1>", "rows<4,2,2>", "rows<4,1,4>"
CASES = (
    # tiny: temporal S in {1, 3, 5, 7, 8}; spatial L in {2, 4, 8} with 4 or 2 heads; spatial L in {3, 6}
    _c("d128h4", 4, 1, 2, "tiny", "tiny"), _c("d128h4", 2, 3, 4, "tiny", "tiny"), _c("d128h4", 1, 5, 8, "tiny", "tiny"),
    _c("d64h2", 3, 7, 3, "tiny", "tiny"), _c("d64h2", 2, 8, 6, "tiny", "tiny"), _c("d128h4", 2, 5, 3, "tiny", "tiny"),
    _c("d128h8", 2, 1, 3, "tiny", "tiny"), _c("d128h8", 1, 5, 3, "tiny", "tiny"), _c("d256h16", 1, 7, 6, "tiny", "tiny"),
    _c("d128h8", 1, 8, 6, "tiny", "tiny"), _c("d256h16", 1, 3, 6, "tiny", "tiny"),
    # stream grouped: L in {2, 4, 8} packed 32 / L sequences to a tile; B T L = 12 (one partial tile), 44 (ragged last tile), 64
    _c("d128h8", 2, 3, 2, "grouped", "tiny"), _c("d128h8", 22, 1, 2, "grouped", "tiny"), _c("d128h8", 4, 8, 2, "grouped", "tiny"),
    _c("d128h8", 1, 3, 4, "grouped", "tiny"), _c("d128h8", 11, 1, 4, "grouped", "tiny"), _c("d128h8", 2, 8, 4, "grouped", "tiny"),
    _c("d128h8", 1, 8, 8, "grouped", "tiny"),
    _c("d256h8", 2, 3, 2, "grouped", "tiny"), _c("d256h8", 22, 1, 2, "grouped", "tiny"), _c("d256h8", 4, 8, 2, "grouped", "tiny"),
    _c("d256h8", 1, 3, 4, "grouped", "tiny"), _c("d256h8", 11, 1, 4, "grouped", "tiny"), _c("d256h8", 2, 8, 4, "grouped", "tiny"),
    _c("d256h8", 1, 8, 8, "grouped", "tiny"),
    # stream short: S in {9, 16, 31, 32} on either axis; 8 and 16 heads; 16, 24 and 32 wide
    *(_c(m, 1, T, L, "short", "short") for m in ("d128h8", "d256h8", "d256h16", "d384h16")
      for T, L in ((9, 32), (32, 9), (16, 31), (31, 16))),
    # rows<4,4,1>: S in {9, 31, 32}, 2 and 4 heads; d64h2 with 9 or 31 sequences: n_seq H = 18 / 62, the last workgroup holds 2 items
    _c("d64h2", 1, 9, 31, R441, R441), _c("d64h2", 1, 32, 9, R441, R441), _c("d128h4", 1, 9, 32, R441, R441),
    _c("d128h4", 1, 31, 9, R441, R441), _c("d128h4", 1, 32, 31, R441, R441),
    # rows<4,2,2>: S in {33, 63, 64}
    *(_c(m, 1, T, L, R422, R422) for m in ("d128h4", "d128h8") for T, L in ((33, 64), (63, 33), (64, 63))),
    # rows<4,1,4>: S in {65, 96, 97, 127, 128} (the Cauchy-Schwarz bound from 97); 24 and 28 wide: the denominator column inside rows
    *(_c(m, 1, T, L, R414, R414) for m in ("d128h4", "d128h8") for T, L in ((65, 96), (96, 97), (97, 127), (127, 128), (128, 65))),
    _c("d192h8", 1, 65, 128, R414, R414), _c("d192h8", 1, 97, 96, R414, R414), _c("d384h16", 1, 65, 128, R414, R414),
    _c("d384h16", 1, 97, 96, R414, R414), _c("d448h16", 1, 65, 97, R414, R414),
    # stream long: S in {129, 160, 255, 256}; spatial on a token-stationary model: planes; temporal, and the 192-wide model: rows
    *(_c("d128h4", 1, 4, L, "long", "tiny") for L in (129, 160, 255, 256)),
    *(_c("d128h8", 1, 2, L, "long", "tiny") for L in (129, 160, 255, 256)),
    *(_c("d128h4", 1, T, 4, "tiny", "long") for T in (129, 160, 255, 256)),
    *(_c("d128h8", 1, T, 2, "grouped", "long") for T in (129, 160, 255, 256)),
    _c("d192h8", 1, 2, 129, "long", "tiny"), _c("d192h8", 1, 2, 256, "long", "tiny"), _c("d448h16", 1, 1, 255, "long", "tiny"),
    # stream chunked: S in {257, 288, 511, 512, 513} (257: the last chunk holds one key, the last query group one row)
    *(_c("d128h4", 1, T, 4, "tiny", "chunked") for T in (257, 288, 511, 512, 513)),
    *(_c("d128h8", 1, T, 2, "grouped", "chunked") for T in (257, 288, 511, 512, 513)),
    _c("d128h8", 1, 2, 257, "chunked", "tiny"), _c("d128h4", 1, 4, 513, "chunked", "tiny"), _c("d448h16", 1, 257, 1, "tiny", "chunked"),
    # ... with the denominator column (24 of 32): S in {257, 513, 1000}
    *(_c("d384h16", 1, T, 2, "grouped", "chunked_den") for T in (257, 513, 1000)), _c("d192h8", 1, 513, 2, "grouped", "chunked_den"),
)
# the persistent loop of k_attention_stream: more than three units per workgroup on the 2-per-CU grid of a 256-CU device
# (long: n_seq H = 1600 units; short: n_seq H / 8 = 1544) - both K | V images and the wrap-around of the unit walk
PERSISTENT_CASES = (
    _c("d256h16", 1, 100, 129, "long", R414),
    _c("d128h8", 193, 8, 9, "short", "tiny"),
)
PERSISTENT_UNITS = {PERSISTENT_CASES[0]: 100 * 16, PERSISTENT_CASES[1]: 193 * 8 * 8 // 8}
# attention_mode "linear": S in {1, 2, 33, 257} at 16, 24 and 32 wide
LINEAR_CASES = tuple(_c(m, B, T, L, "linear", "linear") for m in ("d128h8", "d192h8", "d128h4") for B, T, L in ((2, 1, 2), (1, 33, 257)))

# softmax regimes: (case, sub-block) x four arms.  The regime each arm intends, per kernel:
#   stream: "shifted" = the launch-wide predicate sqrt(qmax2 kmax2) premul 1.02 <= 60 holds (no per-query bound is computed);
#           otherwise per 32-query tile |q_i| sqrt(kmax2) 1.02 <= 60 for all its queries, else the exact max pass
#   rows with the bound (axis longer than 96): per tile |q_i| max_j |k_j| 1.001 <= 60;  rows without: always the max pass
# The mixed arm replaces the query scale by g (1 + 0.5 randn): the launch-wide predicate fails and the tile maxima of the per-query bound
# spread +- 10 % around their median, which g puts at 60 (g = 2.6 gave medians of 32.7, 33.6 and 28.5 on the three bounded cases; the rows
# kernel's bound uses the keys' real norms, smaller than head_dim max ks^2).
REGIME_CASES = (
    (_c("d128h4", 1, 4, 160, "long", "tiny"), 0, "mixed4.7"),
    (_c("d128h4", 1, 300, 4, "tiny", "chunked"), 1, "mixed4.7"),
    (_c("d128h4", 1, 100, 4, "tiny", R414), 1, "mixed5.5"),
    (_c("d128h4", 1, 4, 40, R422, "tiny"), 0, "mixed4.7"),
)


def regime_arms(mixed):
    return ("unit", "sharp", mixed, "max")


INTENDED = {"bounded": dict(unit="shifted", sharp="shifted", mixed="mixed", max="max"),
            "unbounded_rows": dict(unit="max", sharp="max", mixed="max", max="max")}
SHARP_GAIN2 = {16: 6.0, 24: 5.0, 28: 4.5, 32: 4.0}  # scores x gain^2, below the launch-wide predicate of every model of the table
MAX_GAIN = 6.0

# fallback arms, one child process each (the knobs are read once per process): environment, cases
STREAM_OFF_CASES = (
    *(_c("d128h4", 1, T, 4, "tiny", f) for T, f in ((129, "rows<4,1,6>"), (192, "rows<4,1,6>"), (193, "rows<4,1,8>"), (256, "rows<4,1,8>"),
                                                    (257, "rows<16,1,0>"))),
    *(_c("d128h8", 1, T, 2, "tiny", f) for T, f in ((129, "rows<4,1,6>"), (192, "rows<4,1,6>"), (193, "rows<4,1,8>"), (256, "rows<4,1,8>"),
                                                    (257, "rows<16,1,0>"))),
    # the LDS limit.  One sequence (4 / 8 (sequence, head) pairs) leaves keys uncovered at the sharp gain (minimum p_j 0.06 / 0.13 on the
    # oracle): 6 / 3 sequences, 24 pairs each (0.37 / 0.33)
    _c("d128h4", 1, 1248, 6, "tiny", "rows<16,1,0>"), _c("d128h8", 1, 2528, 3, "tiny", "rows<16,1,0>"),
    _c("d128h8", 4, 8, 2, "tiny", "tiny"), _c("d128h8", 2, 8, 4, "tiny", "tiny"), _c("d128h8", 1, 8, 8, "tiny", "tiny"),
)
GROUP_OFF_CASES = (
    _c("d128h8", 4, 8, 2, "tiny", "tiny"), _c("d128h8", 11, 1, 4, "tiny", "tiny"), _c("d128h8", 1, 8, 8, "tiny", "tiny"),
    _c("d256h8", 2, 3, 2, "tiny", "tiny"), _c("d256h8", 2, 8, 4, "tiny", "tiny"), _c("d256h8", 1, 8, 8, "tiny", "tiny"),
)
PLANES_CASE = _c("d128h4", 1, 4, 160, "long", "tiny")
FALLBACK_ARMS = {
    "stream_off": ({"LSL_ATTN_STREAM": "0"}, STREAM_OFF_CASES),
    "group_off": ({"LSL_ATTN_GROUP": "0"}, GROUP_OFF_CASES),
    "planes_off": ({"LSL_QKV_PLANES": "0"}, (PLANES_CASE,)),
    "planes_on": ({}, (PLANES_CASE,)),
}
FALLBACK_KNOBS = ("LSL_ATTN_STREAM", "LSL_ATTN_GROUP", "LSL_QKV_PLANES")


def arm_flags(arm):
    return dict(stream=arm != "stream_off", group=arm != "group_off", planes_on=arm != "planes_off")


def case_id(case):
    return case[0] + "-" + "x".join(str(n) for n in case[1:4])


def case_plans(case, linear=False, **kw):
    model, B, T, L = case[:4]
    return plan_axis(model, B, T, L, False, linear, **kw), plan_axis(model, B, T, L, True, linear, **kw)


# ---- parameters and inputs -----------------------------------------------------------------------------------------------------------
def sharp_gain(model):
    return math.sqrt(SHARP_GAIN2[head_dims(model)[0]])


@functools.lru_cache(maxsize=None)
def params(model, arm, linear=False):
    """random_params(seed 21) with both norm scales of both sub-blocks times the arm's gain; mixed: a non-uniform query scale."""
    sh = net_shape(model, linear)
    p = latent_net.random_params(sh, seed=21)
    hd = sh.head_dim
    mixed = float(arm[5:]) if arm.startswith("mixed") else None
    gain = 1.0 if mixed else {"unit": 1.0, "sharp": sharp_gain(model), "max": MAX_GAIN}[arm]
    g = torch.Generator().manual_seed(77)
    for k in sorted(p):
        if k.endswith("query_norm.scale") and mixed:
            p[k] = mixed * (1.0 + 0.5 * torch.randn(hd, generator=g))
        elif k.endswith(("query_norm.scale", "key_norm.scale")):
            p[k] = p[k] * gain
    return sh, p


@functools.lru_cache(maxsize=8)
def inputs(model, B, T, L):
    D = MODELS[model][0]
    g = torch.Generator().manual_seed(3)
    h = torch.randn(B, T, L, D, generator=g)
    mods = (torch.randn(B, 8 * D, generator=g) * 0.3).contiguous()
    return h, mods


def premul_of(sh):
    return LOG2E / math.sqrt(sh.head_dim) if sh.attention_mode == "scaled_dot_product" else 1.0


def bf16(x):
    return x.to(torch.bfloat16).to(torch.float32)


def oracle_taps(case, arm, bi, linear=False, dtype=torch.float32):
    """The oracle's taps of sub-block bi on the case's inputs (LayerNorm + modulate as latent_net.forward, then attn_mlp_block):
    q_rope, k_rope [G, H, S, hd], z [G, S, 3 D + M], attn [G, S, D], in `dtype`."""
    model, B, T, L = case[:4]
    sh, p = params(model, arm, linear)
    p = latent_net.cast_params(p, dtype)
    h, mods = inputs(model, B, T, L)
    h, mods = h.to(dtype), mods.to(dtype)
    D = sh.hidden_size
    o = 3 * D if bi & 1 else 0
    shift, scale = mods[:, o:o + D][:, None, None, :], mods[:, o + D:o + 2 * D][:, None, None, :]
    u = latent_net.layer_norm(h, 1e-6) * (1 + scale) + shift
    taps = {}
    if bi & 1:
        cs, sn = latent_net.rope_cos_sin(T, sh.head_dim, sh.theta)
        latent_net.attn_mlp_block(p, "blocks.0.temporal_block", u.permute(0, 2, 1, 3).reshape(B * L, T, D), cs.to(dtype), sn.to(dtype), sh, taps)
    else:
        cs, sn = latent_net.rope_cos_sin(L, sh.head_dim, sh.theta)
        latent_net.attn_mlp_block(p, "blocks.0.spatial_block", u.reshape(B * T, L, D), cs.to(dtype), sn.to(dtype), sh, taps)
    return taps


def token_rows(x, B, T, L, temporal):
    """The oracle's axis layout [G, H, S, c] as token-major rows [n, H, c] (spatial: G = (b, t); temporal: G = (b, l)), by permutation."""
    H, c = x.shape[1], x.shape[3]
    if not temporal:
        return x.permute(0, 2, 1, 3).reshape(B * T * L, H, c)
    return x.reshape(B, L, H, T, c).permute(0, 3, 1, 2, 4).reshape(B * T * L, H, c)


def oracle_rows(case, arm, bi, linear=False, dtype=torch.float32, rounded=True):
    """What lsl_debug_taps would hand out if linear1 were the oracle's: qkv [n, 3, H, hdp] token-major (q times the pre-multiplier, bf16
    values unless rounded=False, padded channels zero) and the oracle's attention output [n, H, hd]."""
    model, B, T, L = case[:4]
    sh, _ = params(model, arm, linear)
    H, hd = sh.num_heads, sh.head_dim
    hdp = head_dims(model)[1]
    D = sh.hidden_size
    t = oracle_taps(case, arm, bi, linear, dtype)
    G, S = t["z"].shape[:2]
    v = t["z"][..., 2 * D:3 * D].reshape(G, S, H, hd).permute(0, 2, 1, 3)
    rnd = (lambda x: bf16(x.float()).to(dtype)) if rounded else (lambda x: x)
    qkv = torch.zeros(B * T * L, 3, H, hdp, dtype=dtype)
    for i, x in enumerate((t["q_rope"] * premul_of(sh), t["k_rope"], v)):
        qkv[:, i, :, :hd] = token_rows(rnd(x), B, T, L, bi & 1)
    attn = token_rows(t["attn"].reshape(G, S, H, hd).permute(0, 2, 1, 3), B, T, L, bi & 1)
    return qkv, attn


# ---- tapped rows -> the axis ------------------------------------------------------------------------------------------------------------
def axis_index(pl):
    """token of (seq, pos), [n_seq, S]: AttnArgs' stride pattern (k_attn.hip.h:25)."""
    seq = torch.arange(pl.n_seq)[:, None]
    pos = torch.arange(pl.S)[None, :]
    return (seq // pl.inner) * pl.outer_stride + seq % pl.inner + pos * pl.pos_stride


def axis_view(rows, pl):
    """[n, H, c] token-major -> [n_seq, H, S, c]"""
    return rows[axis_index(pl)].permute(0, 2, 1, 3)


def axis_qkv(qkv, pl, hd):
    """q, k, v [n_seq, H, S, hd] in fp64 from tapped rows [n, 3, H, hdp]; the padded channels of q and k must be exactly zero (they would
    enter every score)."""
    if qkv.shape[-1] > hd:
        assert float(qkv[:, :2, :, hd:].abs().max()) == 0.0
    return tuple(axis_view(qkv[:, i, :, :hd].double(), pl) for i in range(3))


# ---- fp64 references ----------------------------------------------------------------------------------------------------------------------
SoftmaxRef = namedtuple("SoftmaxRef", "o A cover")  # o, A [G, H, S, hd]; cover [S]: max over (sequence, head, query) of p_j


def _slices(G, S):
    step = max(1, (1 << 22) // max(1, S * S))  # (sequence, head) pairs per slice: at most 4 Mi scores (32 MiB of doubles) at a time
    return [(a, min(G, a + step)) for a in range(0, G, step)]


def softmax_reference(q, k, v, keys=None, kv_roll=0):
    """s = q k^T, p = 2^s / sum_j 2^s, o = p v, A = p |v| in fp64.  `keys` (an index list) and `kv_roll` serve the mutations of the CPU
    tests: attend these key positions instead of all / the keys and values of the sequence kv_roll further on."""
    G, H, S, hd = q.shape
    if kv_roll:
        k, v = k.roll(-kv_roll, 0), v.roll(-kv_roll, 0)
    if keys is not None:
        k, v = k[:, :, keys], v[:, :, keys]
    qf, kf, vf = (x.reshape(G * H, x.shape[2], hd) for x in (q, k, v))
    o, A = torch.empty_like(qf), torch.empty_like(qf)
    cover = torch.zeros(kf.shape[1], dtype=torch.float64)
    for a, b in _slices(G * H, S):
        s = qf[a:b] @ kf[a:b].transpose(1, 2)
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        p = p / p.sum(-1, keepdim=True)
        o[a:b] = p @ vf[a:b]
        A[a:b] = p @ vf[a:b].abs()
        if p.numel():
            cover = torch.maximum(cover, p.amax((0, 1)))
    return SoftmaxRef(o.reshape(G, H, S, hd), A.reshape(G, H, S, hd), cover)


def linear_reference(q, k, v):
    """attention_linear in fp64 on the tapped q (no pre-multiplier), k, v [G, H, S, hd]: q_s = softmax over channels x hd^-1/2, k_s =
    softmax over positions, out = q_s (k_s^T v), A_lin = q_s (k_s^T |v|)."""
    hd = q.shape[-1]
    qs = torch.softmax(q, -1) * hd ** -0.5
    ks = torch.softmax(k, -2).transpose(-1, -2)
    return SoftmaxRef(qs @ (ks @ v), qs @ (ks @ v.abs()), None)


def element_bar(form, ref, S, hd):
    if is_mfma(form):
        return MFMA_BAR_UA * U * ref.A
    return U * ref.o.abs() + (S + hd + 16) * 2.0 ** -23 * ref.A


def worst(z, ref, form, S, hd):
    """(worst |z - o| in units of u A, worst |z - o| / bar): the second must not exceed 1; non-finite differences count as infinite."""
    d = (z.double() - ref.o).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    tiny_a = ref.A.clamp_min(1e-300)
    return float((d / (U * tiny_a)).max()), float((d / element_bar(form, ref, S, hd).clamp_min(1e-300)).max())


# ---- the kernels' roundings, emulated (CPU tests) -----------------------------------------------------------------------------------
def emulate(q, k, v, form, keys=None, kv_roll=0, q_roll=0):
    """softmax forms: fp32 scores; MFMA forms round the unnormalised probabilities to bf16 (the denominator sums the rounded ones) and the
    output to bf16; tiny keeps fp32 probabilities and rounds the output.  Mutations as softmax_reference, and q_roll: query row i is
    answered with row i + q_roll's."""
    G, H, S, hd = q.shape
    if kv_roll:
        k, v = k.roll(-kv_roll, 0), v.roll(-kv_roll, 0)
    if keys is not None:
        k, v = k[:, :, keys], v[:, :, keys]
    qf, kf, vf = (x.reshape(G * H, x.shape[2], hd).float() for x in (q, k, v))
    o = torch.empty_like(qf)
    for a, b in _slices(G * H, S):
        s = qf[a:b] @ kf[a:b].transpose(1, 2)
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        if is_mfma(form):
            p = bf16(p)
        o[a:b] = bf16((p @ vf[a:b]) / p.sum(-1, keepdim=True))
    o = o.reshape(G, H, S, hd)
    return o.roll(-q_roll, 2) if q_roll else o


def emulate_linear(q, k, v):
    hd = q.shape[-1]
    qs = torch.softmax(q.float(), -1) * hd ** -0.5
    ks = torch.softmax(k.float(), -2).transpose(-1, -2)
    return bf16(qs @ (ks @ v.float()))


def mutations(pl):
    """name -> keyword arguments of `emulate` for every mutation defined on this axis."""
    S = pl.S
    out = {}
    if S >= 2:
        out["last_key_dropped"] = dict(keys=list(range(S - 1)))
        out["last_key_twice"] = dict(keys=list(range(S)) + [S - 1])
        out["neighbour_row"] = dict(q_roll=1)
    if S > 256:
        out["key_256_dropped"] = dict(keys=[j for j in range(S) if j != 256])
    if pl.blk:
        out["mask_shifted_one_block"] = dict(kv_roll=1)
    return out


# ---- the kernels' softmax-regime predicates --------------------------------------------------------------------------------------------
def regime(pl, q, k, qs, ks, premul, hd):
    """Which softmax path the kernel takes on this axis, from the tapped q, k [G, H, S, hd] and the norm scales: "shifted" (every query
    tile by the bound), "max" (every tile the exact max pass), "mixed", or "ambiguous" when a decision lies within 2 % of the threshold
    (k_attn.hip.h:240-245 rows, :457-460 and :523-528 stream)."""
    if pl.form in ("tiny", "linear"):
        return "n/a"
    if pl.kernel != "k_attention_stream" and not pl.bound:
        return "max"
    G, H, S, _ = q.shape
    qn = q.double().norm(dim=-1)  # [G, H, S] (the pre-multiplier is in the tapped q)
    if pl.kernel == "k_attention_stream":
        qmax2, kmax2 = hd * float(qs.double().pow(2).max()), hd * float(ks.double().pow(2).max())
        whole = math.sqrt(qmax2 * kmax2) * premul * 1.02
        if whole <= 60 * 0.98:
            return "shifted"
        if whole <= 60 * 1.02:
            return "ambiguous"
        m = qn * math.sqrt(kmax2) * 1.02
        if pl.blk:  # tiles of 32 consecutive tokens
            m = m.permute(1, 0, 2).reshape(H, G * S)
    else:
        m = qn * k.double().norm(dim=-1).amax(-1, keepdim=True) * 1.001
    n = m.shape[-1]
    pad = (-n) % 32 if n > 32 else 0
    m = torch.nn.functional.pad(m, (0, pad), value=0.0)
    tiles = m.reshape(-1, 32 if n > 32 else n).amax(-1)  # a tile is shifted iff none of its queries exceeds 60
    under, over = tiles <= 60 * 0.98, tiles > 60 * 1.02
    if bool(under.all()):
        return "shifted"
    if bool(over.all()):
        return "max"
    return "mixed" if bool(under.any()) and bool(over.any()) else "ambiguous"


def intended_regime(pl, arm):
    if pl.form in ("tiny", "linear"):
        return "n/a"
    kind = "bounded" if pl.kernel == "k_attention_stream" or pl.bound else "unbounded_rows"
    return INTENDED[kind]["mixed" if arm.startswith("mixed") else arm]
