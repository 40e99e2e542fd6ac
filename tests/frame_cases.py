"""The case table of the per-element tests of the fp32 frame of an evaluation (test_frame_cases.py on the CPU, test_hip_frame.py on the
MI355X): the kernels of csrc/k_small.hip.h in front of and behind the sub-blocks - the conditioning chain (k_time_features,
k_time_features_steps, k_dense_rows, k_dense_tiled, k_dense_mfma), the two embeddings (k_embed, k_embed_mfma), k_ln_inplace, the
k_embed<STATS> + k_ln_finalize pair of ln_fuse handles and the output head fused with the sampler's update (k_head_step_mfma) - at every
launch form launch_dense, launch_embed and launch_head_mfma (csrc/host_launch.hip.h) can choose, restated here with the CU count as a
parameter; the fp64 references; the per-element bars; fp32 emulations of each family with their mutations.  Not a test module.

What is compared.  lsl_debug_mods_ex, lsl_debug_mods_steps, lsl_debug_embed and lsl_debug_head run the launch helpers of an evaluation on
caller buffers and hand out every intermediate.  Each reference is computed in fp64 from the very fp32 operands the kernel read: the tapped
time features for the first dense layer, the tapped hidden row for the second, the tapped conditioning vector for the tables, the tapped
cond embedding as the state embedding's base, the caller's x, h and mods for the head.  Only a kernel's own roundings separate the two.

Bars, per element, u = 2^-24 (one fp32 operation, round to nearest).  Derived from the kernels' arithmetic, not measured:
  * a chain of K multiply-adds in any order (FMA chains, the exact-fp32 MFMA with its four-way partial sum, lane sums + wave tree):
    (K + 3) u sum|w x| + u |result|: every term passes through at most K + 2 roundings, (1 + u)^(K + 2) - 1 <= (K + 3) u for K <= 512.
  * every added term (bias, bias2, mask row, base, add row): one u of the sum it produces - u |acc + b|, then u |acc + b + add|; the
    embedding's u |bias + bias2|, u |bias + bias2 + mask row|, u |result|.  Nothing beyond these: the code below is this formula.
  * time features: K_TRIG u absolute (|cos|, |sin| <= 1) against cos / sin in fp64 of the fp32 argument fl(fl(1000 t) f_k), the two
    multiplications the kernel does, reproduced on the CPU in fp32 (the exact product differs by up to 1e-4 at arguments up to 1000).
  * silu(x) = x / (1 + __expf(-x)): |silu| ((K_EXP + |x|) e / (1 + e) + 3) u, e = exp(-x): __expf's own error K_EXP u plus the
    rounding |x| u of its argument (the product with log2 e inside it), both scaled by the exponential's share e / (1 + e) of the
    denominator; one u each for the sum, the division and slack for the reference's own rounding.  A silu in front of a chain (PRE)
    enters through sum |w| bar(silu(x)); behind it (POST) the chain's bar is carried by |silu'| <= 1.1.
  * LayerNorm (k_ln_inplace, the head's rows): the statistics term of gemm_cases.a_reference without the bf16 rounding,
    (22 + K_RSQ) u |xhat| + 16 u rstd mean|h| (the mean: at most 8 values per lane and a 6-level tree, 14 additions, 2 u for the
    subtraction and product; rstd: half the relative error of its sum, 8 u, + K_RSQ u of rsqrtf + 1 u, and the subtraction's own
    rounding) + 2 u |out|; modulated: times |1 + scale|, + 4 u |a| (1 + scale, the product, the shift).
  * head: m = a Wo^T + bo: the LayerNorm + modulate error carried through sum |Wo|, + (D + 3) u sum|Wo a| + u (|m - bo| + |m|).
  * state update x <- ax x + am m + aw w + as saved: |am| bar(m) + 4 u (|ax x| + |am m| + |aw w| + |as saved|).
  * stats_out = (rstd, -mean rstd) of k_embed<STATS> + k_ln_finalize: relative (14 + K_RSQ) u + 16 u mean|h| max_p|d_p| rstd^2 for
    rstd (the wave sums of 4 values per lane, the pairwise combination q = sum_p m2_p + gsz d_p^2 whose d_p = mean_p - mean carries
    the means' error, the division, the eps, rsqrtf); -mean rstd: that relative bar + u on |mean rstd|, + 18 u mean|h| rstd of the mean.
The three constants that do not follow from the code: the HIP math-function accuracy tables are not part of the ROCm install this was
written against, so they were MEASURED on the first MI355X run (profiles/frame_rowwise_parity.txt, "constants"): the worst error of every
tapped tfeat (cosf / sinf at |a| <= 1000), hid (silu behind a 256-deep chain) and rstd (stats_out) element against its fp64 reference in
units of u max(|value|, 1), times 4 (the sample is finite, the bound is per ulp), never above 16 - a coarser approximation still fails.
Measured: tfeat 0.982 -> K_TRIG = 3.93; hid 6.456 (it carries the 256-deep chain in front of the silu) -> K_EXP = 16, the cap; rstd
2.193 (it carries the statistics' sums) -> K_RSQ = 8.77.

Bit equalities instead of bars: trace and save_out equal x; device noise equals the library's own draw (lsl_sample_ex's no-network
record) at the same seed / step / offset; lsl_debug_mods equals lsl_debug_mods_ex without the extras; every row of lsl_debug_mods_steps
equals the single-row lsl_debug_mods_ex(t = NULL) at that time; the STATS embedding's h equals the plain handle's; mod_rows = 1 equals
mod_rows = B fed identical rows; unused outputs are finite.

One sequence the head cannot see.  A workgroup that walks (single-trajectory tile, straddling tile, single-trajectory tile of the FIRST
tile's trajectory) does not exist: a workgroup's tiles ascend and trajectories are contiguous token ranges, so a third tile in the first
tile's trajectory puts the second one inside it as well.  The table pins what does exist: (single A, straddling, single C: the registers
reload) and (single A, single A: no reload, then straddling A | B), and the CPU test derives both from head_form.

Weights: oracle.latent_net.random_params(seed 21) of a depth-1 model with heads of 32 channels and mlp_ratio 2; the frame's weights are
fp32 throughout.  Inputs: generator seed 5; times uniform in [0, 1) (arguments up to 1000); the mask in runs of 37 tokens, so that runs
cross every tile edge; mask_to_emb's two rows are independent N(0, 1) rows, |difference| ~ 1 against bars of ~ 1e-6."""
import functools
import math
from collections import namedtuple

import torch

from oracle import latent_net

U = 2.0 ** -24
CUS = 256  # the MI355X; every rule below takes the count as a parameter
LDS_BUDGET = 160 * 1024
# measured on MI355X, x 4, capped at 16 (module docstring; profiles/frame_rowwise_parity.txt): worst tfeat 0.982, hid 6.456, rstd 2.193
K_TRIG, K_EXP, K_RSQ = 4 * 0.982, min(16.0, 4 * 6.456), 4 * 2.193
HIDDEN = (64, 128, 192, 256, 320, 384, 448, 512)


# ---- models ------------------------------------------------------------------------------------------------------------------------------
def net_shape(C, D, V=None, normalize=False):
    return latent_net.NetShape(depth=1, in_dim=C, hidden_size=D, num_heads=D // 32, mlp_ratio=2, vec_in_dim=V, normalize=normalize)


@functools.lru_cache(maxsize=8)
def params(C, D, V=None, normalize=False):
    sh = net_shape(C, D, V, normalize)
    return sh, latent_net.random_params(sh, seed=21)


def frame_weights(p, dev="cpu"):
    """The fp32 tensors PackedWeights hands to the library, in fp64, by the library's names."""
    g = lambda k: p[k].double().to(dev)  # noqa: E731
    w = {"x_in_w": g("x_in.weight"), "x_in_b": g("x_in.bias"), "cond_w": g("cond_to_emb.weight"), "cond_b": g("cond_to_emb.bias"),
         "mask_emb": g("mask_to_emb.weight"), "time_w1": g("time_in.in_layer.weight"), "time_b1": g("time_in.in_layer.bias"),
         "time_w2": g("time_in.out_layer.weight"), "time_b2": g("time_in.out_layer.bias"),
         "mod_w": torch.cat([g("blocks.0.modulation.lin.weight"), g("adaLN_modulation.1.weight")]),
         "mod_b": torch.cat([g("blocks.0.modulation.lin.bias"), g("adaLN_modulation.1.bias")]),
         "out_w": g("linear.weight"), "out_b": g("linear.bias")}
    if "vec_in.in_layer.weight" in p:
        w.update({"vec_w1": g("vec_in.in_layer.weight"), "vec_b1": g("vec_in.in_layer.bias"),
                  "vec_w2": g("vec_in.out_layer.weight"), "vec_b2": g("vec_in.out_layer.bias")})
    return w


def time_freqs():
    return torch.exp(-math.log(10000.0) * torch.arange(0, 128, dtype=torch.float32) / 128)


# ---- the launch rules restated (csrc/host_launch.hip.h, csrc/host_eval.hip.h) ------------------------------------------------------------
DenseForm = namedtuple("DenseForm", "kernel kq row_tile")


def dense_form(I, rows, single):
    """launch_dense: the kernel, its k per wave (k_dense_mfma) and the rows of a workgroup's tile (0: every row, one wave per output)."""
    if single and rows == 1 and I <= 512:
        return DenseForm("k_dense_rows", 0, 0)
    if I in (128, 256):
        return DenseForm("k_dense_mfma", I // 4, 32)
    if I % 4 == 0:
        return DenseForm("k_dense_tiled", 0, 64)
    return DenseForm("k_dense_rows", 0, 0)


def dense_label(form, pre, post):
    return "%s<%d, %d%s>" % (form.kernel, pre, post, ", %d" % form.kq if form.kq else "")


def mods_chain(D, rows, single, V=None):
    """The forms of a lsl_debug_mods_ex call: {tensor: (form, PRE, POST, I)} in launch order."""
    out = {}
    if V:
        out["yhid"] = (dense_form(V, rows, False), 0, 1, V)
        out["yemb"] = (dense_form(D, rows, False), 0, 0, D)
    out["hid"] = (dense_form(256, rows, single), 0, 1, 256)
    out["vec"] = (dense_form(D, rows, single), 0, 0, D)
    out["mods"] = (dense_form(D, rows, single), 1, 0, D)
    return out


def mods_label(D, rows, single, V=None):
    """The label of profile class 6 behind lsl_debug_mods_ex: run_yemb's chain, then run_mods'."""
    ch = mods_chain(D, rows, single, V)
    lab = lambda k: dense_label(*ch[k][:3])  # noqa: E731
    s = "k_time_features > %s > %s > %s" % (lab("hid"), lab("vec"), lab("mods"))
    return "%s > %s ; %s" % (lab("yhid"), lab("yemb"), s) if V else s


STEPS_LABEL = "k_time_features_steps > k_dense_rows<0, 1> > k_dense_rows<0, 0> > k_dense_rows<1, 0> (row ranges of 8, 8, 16)"


def steps_ranges(count):
    """run_mods_steps: (launches of k_time_features_steps, rows of every range of the 8-row layers, of the 16-row layer)."""
    def cut(per):
        gy = (count + per - 1) // per
        rpb = (count + gy - 1) // gy
        return [min(count, (y + 1) * rpb) - y * rpb for y in range(gy) if y * rpb < count]
    return (count + 47) // 48, cut(8), cut(16)


EmbedForm = namedtuple("EmbedForm", "label kind cmax nd ck tok grid tiles tiles_per_wg w_lds dq ngrp")


def embed_form(mode, C, D, n, stats=False, cus=CUS):
    """launch_embed<mode>: label, register form (CMAX, ND) or MFMA form (CK), tile size, grid, tiles, tiles of the busiest workgroup."""
    if C > 32 and C % 8 == 0 and C <= 128 and D % 32 == 0:
        ngrp = (D // 32 + 2) // 3
        units = ((n + 31) // 32) * ngrp
        return EmbedForm("k_embed_mfma<%d, %d> (32-token tiles)" % (mode, C // 8), "mfma", 0, 0, C // 8, 32, (units + 3) // 4, (n + 31) // 32, 1,
                         False, 0, ngrp)
    tok = 64
    w_lds = C == 32 and D % 4 == 0 and D <= 512
    if w_lds:
        while tok > 16 and (n + tok - 1) // tok < 2 * cus:
            tok //= 2
    tiles = (n + tok - 1) // tok
    grid = min(tiles, 2 * cus)
    cmax, nd = (32, 4) if C <= 32 else (64, 2) if C <= 64 else (96, 2) if C <= 96 else (128, 1)
    with_stats = bool(stats) and mode == 1 and C <= 32 and D % 256 == 0 and D <= 512
    label = "k_embed<%d, %d, %d%s> (%d-token tiles%s)" % (cmax, mode, nd, ", true" if with_stats else "", tok,
                                                          ", weights through LDS" if w_lds else ", scalar weight loads" if C & 3 else "")
    return EmbedForm(label, "reg", cmax, nd, 0, tok, grid, tiles, (tiles + grid - 1) // grid, w_lds, D // nd, 0)


def embed_label(C, D, n, stats=False, cus=CUS):
    """The label of profile class 5 behind lsl_debug_embed: the cond embedding, then the state embedding."""
    return "%s ; %s" % (embed_form(0, C, D, n, False, cus).label, embed_form(1, C, D, n, stats, cus).label)


def dq_class(dq):
    return "div" if dq < 256 and 256 % dq == 0 else "nodiv" if dq < 256 else "eq" if dq == 256 else "between" if dq < 512 else "two"


HeadForm = namedtuple("HeadForm", "label ne vec one_slab per_cu grid tiles tiles_per_wg")


def head_form(D, C, n, cus=CUS):
    """launch_head_mfma: label, <NE, VEC>, one slab or cycled slabs, workgroups per CU, grid, 32-token tiles, tiles of the busiest workgroup."""
    ne = D // 64
    vec = 2 if ne % 2 == 0 else 1
    one = C <= 32
    rows, parts = 32 * (D + 4) * 4, 4 * 32 * 33 * 4
    lds = max(rows, parts) if one else rows + parts
    per_cu = 2 if 2 * lds <= LDS_BUDGET else 1
    tiles = (n + 31) // 32
    grid = min(tiles, cus * per_cu)
    label = "k_head_step_mfma<%d, %d> (%s, %d per CU)" % (ne, vec, "one slab" if one else "cycled slabs", per_cu)
    return HeadForm(label, ne, vec, one, per_cu, grid, tiles, (tiles + grid - 1) // grid)


def head_walk(form, wg, n, tpt, shared):
    """What workgroup wg meets on its tiles: per tile ("single", trajectory, reload) or ("straddle", first, last) - the kernel's cur_traj
    logic restated (a straddling tile leaves the registers alone)."""
    cur, out = -1, []
    for tile in range(wg, form.tiles, form.grid):
        n0 = 32 * tile
        first, last = (0, 0) if shared else (n0 // tpt, min(n0 + 31, n - 1) // tpt)
        if first == last:
            out.append(("single", first, first != cur))
            cur = first
        else:
            out.append(("straddle", first, last))
    return out


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------
# dense: ("mods", D, V, rows, single) -> lsl_debug_mods_ex; ("steps", D, count) -> lsl_debug_mods_steps against the single-row calls
def _dense_cases():
    out = []
    for D in HIDDEN:
        out.append(("mods", D, None, 1, True))    # the sampler's single row: k_dense_rows at every width, all three PRE / POST pairs
        out.append(("mods", D, None, 33, False))  # MFMA at 128 / 256, tiled elsewhere; the first layer (I = 256) always MFMA
    for rows in (1, 2, 31, 32, 64, 65):            # the 32-row tiles of k_dense_mfma (every layer at 128), the 64-row tiles of k_dense_tiled
        out += [("mods", 128, None, rows, False), ("mods", 192, None, rows, False)]
    out.append(("mods", 256, None, 65, False))
    # vec_in: MFMA <0, 1, 32 / 64> at 128 / 256 inputs, tiled <0, 1> at 12 / 24 (a k loop that ends inside a 16-deep chunk), rows <0, 1> at 3 / 5;
    # its output is the `add` of the second layer (add_mod 0: a row per trajectory)
    out += [("mods", 256, 128, 33, False), ("mods", 128, 256, 65, False), ("mods", 64, 12, 31, False), ("mods", 320, 24, 65, False),
            ("mods", 192, 3, 2, False), ("mods", 512, 5, 33, False), ("mods", 384, 5, 64, False), ("mods", 448, 12, 1, False)]
    out += [("steps", 192, c) for c in (1, 7, 8, 9, 16, 17, 48, 49, 50)]
    out += [("steps", 512, 50), ("steps", 128, 17), ("steps", 64, 9)]
    return tuple(out)


DENSE_CASES = _dense_cases()

# embed: (C, D, n, handle), handle: plain | norm (normalize=True: k_ln_inplace behind the embedding) | lnf (ln_fuse: STATS + k_ln_finalize)
# the LDS form halves its tile while the launch has fewer than 2 CUs tiles: 16 tokens up to n = 32 (2 CUs - 1), 32 up to 64 (2 CUs - 1), 64 above
EMB_T16_MAX, EMB_T32_MAX = 32 * (2 * CUS - 1), 64 * (2 * CUS - 1)
EMB_MULTI = 64 * 2 * CUS + 64 + 7  # 514 tiles of 64 tokens on 512 workgroups: two of them walk two tiles, the last tile holds 7 tokens


def _embed_cases():
    out = []
    small = (1, 31, 32, 33)
    # k_embed<32, ., 4>: scalar weight loads (C = 1, 3, 6), 16-byte loads (4, 8, 28), through LDS (32); DQ = D / 4: 16 .. 128
    for C, D in ((1, 64), (3, 192), (6, 320), (4, 128), (8, 512), (28, 448), (32, 256), (32, 320)):
        out += [(C, D, n, "plain") for n in small]
    # <64, ., 2> (36, 60), <96, ., 2> (68, 92), <128, ., 1> (100, 124): in_dim above 32 that is no multiple of 8
    for C, D in ((36, 64), (60, 192), (68, 128), (92, 512), (100, 64), (124, 256), (100, 320), (124, 384), (100, 448), (124, 512)):
        out += [(C, D, n, "plain") for n in small]
    # k_embed_mfma<., CK>, CK = 5 .. 16; D / 32 not a multiple of 3 at 64 (one group of two tiles), 128 (3 + 1), 256 (3 + 3 + 2), 320, 512
    for ck, D in zip(range(5, 17), (64, 128, 192, 256, 320, 384, 448, 512, 128, 256, 320, 512)):
        out += [(8 * ck, D, n, "plain") for n in small]
        out.append((8 * ck, D if D // 32 % 3 else 320, 97 if ck % 2 else 130, "plain"))  # several token tiles, a ragged last one, ragged feature groups
    # the LDS form on either side of each tile-size change, and above 64 * 2 * CUs
    for n in (EMB_T16_MAX, EMB_T16_MAX + 1, EMB_T32_MAX, EMB_T32_MAX + 1, EMB_MULTI):
        out.append((32, 512 if n == EMB_MULTI else 256, n, "plain"))
    # more tiles than workgroups at every DQ class of every register form
    out += [(8, 64, EMB_MULTI, "plain"), (6, 192, EMB_MULTI, "plain"),                                   # ND 4: div, nodiv
            (36, 64, EMB_MULTI, "plain"), (60, 192, EMB_MULTI, "plain"), (36, 512, EMB_MULTI, "plain"),  # <64, 2>: div, nodiv, eq
            (68, 128, EMB_MULTI, "plain"), (92, 320, EMB_MULTI, "plain"), (92, 512, EMB_MULTI, "plain"),  # <96, 2>: div, nodiv, eq
            (100, 64, EMB_MULTI, "plain"), (124, 192, EMB_MULTI, "plain"), (100, 256, EMB_MULTI, "plain"),  # <128, 1>: div, nodiv, eq
            (124, 320, EMB_MULTI, "plain"), (100, 384, EMB_MULTI, "plain"), (124, 448, EMB_MULTI, "plain"),  # between (the k_embed fix)
            (100, 512, EMB_MULTI, "plain")]                                                              # two trips
    # normalize: k_ln_inplace<NE, VEC> at every hidden size; n = 1, 3, 4, 5: a partial workgroup of four waves
    for i, D in enumerate(HIDDEN):
        out += [((8, 32, 36, 72)[i % 4], D, n, "norm") for n in (1, 5, 33)]
    out += [(16, 256, 3, "norm"), (16, 256, 4, "norm")]
    # ln_fuse handles: STATS at hidden 256 (one part) and 512 (two), with and without the LDS weight path
    for C, D in ((8, 256), (32, 256), (32, 512), (4, 512)):
        out += [(C, D, n, "lnf") for n in (1, 33, 257, 1000)]
    out += [(32, 512, EMB_MULTI, "lnf"), (8, 256, EMB_MULTI, "lnf")]
    return tuple(out)


EMBED_CASES = _embed_cases()

# head: (D, C, B, tpt, rows) with T = 1, L = tpt; rows "B" (a modulation row per trajectory) or "1" (shared); every record variant runs in every case
HEAD_VARIANTS = ("out", "aw0", "noise", "devnoise", "saved", "trace")
HEAD_SEQ = {  # the multi-tile cases: name -> (case, workgroup, what it must meet)
    "reload": ((256, 32, 83, 400, "B"), 0, [("single", 0, True), ("straddle", 40, 41), ("single", 81, True)]),
    "noreload": ((128, 4, 2, 32785, "B"), 0, [("single", 0, True), ("single", 0, False), ("straddle", 0, 1), ("single", 1, True), ("single", 1, False)]),
    "reload-1percu": ((512, 33, 39, 432, "B"), 0, [("single", 0, True), ("straddle", 18, 19), ("single", 37, True)]),
    "reload-cycled": ((448, 64, 83, 400, "B"), 0, [("single", 0, True), ("straddle", 40, 41), ("single", 81, True)]),
    "reload-512": ((512, 3, 83, 400, "B"), 0, [("single", 0, True), ("straddle", 40, 41), ("single", 81, True)]),
    "shared": ((384, 31, 83, 400, "1"), 0, [("single", 0, True), ("single", 0, False), ("single", 0, False)]),
}
HEAD_CHANNELS = (1, 3, 4, 31, 32, 33, 64, 96, 100)


def _head_cases():
    out = []
    for i, D in enumerate(HIDDEN):
        for j, n in enumerate((1, 31, 32, 33)):
            out.append((D, HEAD_CHANNELS[(2 * i + j) % 9], n, 1, "B"))  # one token per trajectory: every tile of more than one token straddles
    for i, C in enumerate(HEAD_CHANNELS):  # three trajectories of 23 tokens on three tiles: single, straddling, straddling + ragged
        out.append((HIDDEN[(3 * i + 1) % 8], C, 3, 23, "B"))
        out.append((HIDDEN[(3 * i + 4) % 8], C, 3, 23, "1"))
    out += [(512, 100, 5, 13, "B"), (512, 64, 1, 33, "B"), (64, 100, 2, 40, "B")]
    out += [c for c, _, _ in HEAD_SEQ.values()]
    return tuple(dict.fromkeys(out))


HEAD_CASES = _head_cases()


def dense_id(c):
    return "mods-d%d-v%s-r%d%s" % (c[1], c[2] or 0, c[3], "-single" if c[4] else "") if c[0] == "mods" else "steps-d%d-c%d" % c[1:]


def embed_id(c):
    return "c%d-d%d-n%d-%s" % c


def head_id(c):
    return "d%d-c%d-%dx%d-rows%s" % c


def head_n(c):
    return c[2] * c[3]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def dense_inputs(c):
    g = torch.Generator().manual_seed(5)
    if c[0] == "steps":
        return torch.rand(c[2], generator=g), None
    _, D, V, rows, single = c
    t = torch.rand(rows, generator=g)
    return t, (torch.randn(rows, V, generator=g) if V else None)


def mask_of(n):
    return ((torch.arange(n) // 37) % 2).to(torch.int64)


def embed_inputs(c):
    C, D, n, _ = c
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, C, generator=g), torch.randn(n, C, generator=g), mask_of(n)


def head_inputs(c):
    """h [n, D], mods [B or 1, 8 D], x, noise, saved [n, C]; the rows of h differ in scale and offset so that the statistics matter."""
    D, C, B, tpt, rows = c
    n = B * tpt
    g = torch.Generator().manual_seed(5)
    h = torch.randn(n, D, generator=g) * (0.5 + torch.rand(n, 1, generator=g)) + 0.3 * torch.randn(n, 1, generator=g)
    mods = (torch.randn(B if rows == "B" else 1, 8 * D, generator=g) * 0.3).contiguous()
    x, noise, saved = (torch.randn(n, C, generator=g) for _ in range(3))
    return h, mods, x, noise, saved


HEAD_RECORDS = {  # variant -> (ax, am, aw, as)
    "aw0": (0.9, -0.4, 0.0, 0.0), "noise": (1.1, 0.3, 0.7, 0.0), "devnoise": (0.8, 0.5, -0.6, 0.0), "saved": (0.5, 0.25, 0.0, 0.5),
    "trace": (1.0, 0.125, 0.3, 0.0)}
HEAD_SEED, HEAD_STEP, HEAD_OFFSET = 77, 3, 1234567


# ---- fp64 references with their bars: (reference, bar) on the device of the operands -------------------------------------------------------
def silu64(x):
    return x / (1.0 + torch.exp(-x))


def silu_bar(x):
    share = 1.0 / (1.0 + torch.exp(x))  # e / (1 + e), e = exp(-x)
    return silu64(x).abs() * ((K_EXP + x.abs()) * share + 3.0) * U


def time_args(t32):
    """fl(fl(1000 t) f_k) [rows, 128], the kernel's two fp32 multiplications (on the CPU: IEEE fp32, as v_mul_f32), as fp64."""
    t32 = t32.detach().cpu().float()
    return ((t32 * 1000.0)[:, None] * time_freqs()[None]).double()


def tfeat_reference(t32, dev="cpu"):
    a = time_args(t32).to(dev)
    ref = torch.cat([torch.cos(a), torch.sin(a)], -1)
    return ref, torch.full_like(ref, K_TRIG * U)


def dense_reference(x, W, b, add, pre, post):
    """out = post(pre(x) W^T + b + add) from the fp32 operand x [rows, I] (as fp64); W [O, I], b [O], add [rows, O] or None."""
    xin, ein = (silu64(x), silu_bar(x)) if pre else (x, None)
    acc, S = xin @ W.t(), xin.abs() @ W.abs().t()
    v = acc + b if add is None else acc + b + add
    bar = (x.shape[1] + 3) * U * S + U * acc.abs() + U * (acc + b).abs()  # the chain; the bias added to it
    if add is not None:
        bar = bar + U * v.abs()  # the add row added to that
    if pre:
        bar = bar + ein @ W.abs().t()
    if post:
        return silu64(v), 1.1 * bar + silu_bar(v)
    return v, bar


def mods_references(taps, t32, y, w, single_time=None):
    """Every tensor of a lsl_debug_mods_ex call from the operands its kernel read: taps = {tfeat, hid, vec, mods[, yhid, yemb]} fp32."""
    dev = taps["hid"].device
    d = {k: v.double() for k, v in taps.items()}
    out = {"tfeat": tfeat_reference(t32, dev)}
    add = None
    if y is not None:
        out["yhid"] = dense_reference(y.double().to(dev), w["vec_w1"], w["vec_b1"], None, False, True)
        out["yemb"] = dense_reference(d["yhid"], w["vec_w2"], w["vec_b2"], None, False, False)
        add = d["yemb"]
    out["hid"] = dense_reference(d["tfeat"], w["time_w1"], w["time_b1"], None, False, True)
    out["vec"] = dense_reference(d["hid"], w["time_w2"], w["time_b2"], add, False, False)
    out["mods"] = dense_reference(d["vec"], w["mod_w"], w["mod_b"], None, True, False)
    return out


def embed_reference(mode, x, w, mask=None, base=None):
    """mode 0: x_cond W_c^T + (cond_b + x_in_b) + mask_emb[mask]; mode 1: x W_x^T + base.  x [n, C] fp64."""
    W = w["cond_w"] if mode == 0 else w["x_in_w"]
    acc, S = x @ W.t(), x.abs() @ W.abs().t()
    K = x.shape[1]
    if mode == 0:
        me = w["mask_emb"][(mask != 0).long()]
        b0 = w["cond_b"] + w["x_in_b"]
        ref = acc + (b0 + me)
        # the chain; bias + bias2; the mask row added to that; the sum added to the chain
        return ref, (K + 3) * U * S + U * acc.abs() + U * (b0.abs() + (b0 + me).abs() + ref.abs())
    ref = acc + base
    return ref, (K + 3) * U * S + U * acc.abs() + U * ref.abs()


def _stats(h, eps):
    mean = h.mean(-1, keepdim=True)
    dev = h - mean
    rstd = torch.rsqrt((dev * dev).mean(-1, keepdim=True) + eps)
    return mean, dev * rstd, rstd


def ln_reference(h, eps=1e-5):
    """k_ln_inplace: (h - mean) rstd."""
    _, xhat, rstd = _stats(h, eps)
    return xhat, (22 + K_RSQ) * U * xhat.abs() + 16 * U * rstd * h.abs().mean(-1, keepdim=True) + 2 * U * xhat.abs()


def stats_reference(h, gsz=256):
    """k_embed<STATS> + k_ln_finalize: (rstd, -mean rstd) [n, 2] of every row, eps 1e-6."""
    mean, _, rstd = _stats(h, 1e-6)
    dp = (h.reshape(h.shape[0], -1, gsz).mean(-1) - mean).abs().amax(-1, keepdim=True)
    mabs = h.abs().mean(-1, keepdim=True)
    rel = (14 + K_RSQ) * U + 16 * U * mabs * dp * rstd * rstd
    ref = torch.cat([rstd, -mean * rstd], -1)
    bar = torch.cat([rstd * rel, (mean * rstd).abs() * (rel + U) + 18 * U * mabs * rstd], -1)
    return ref, bar


def head_reference(h, shift, scale, w):
    """m = Linear(LayerNorm_1e-6(h) (1 + scale) + shift): h [n, D], shift, scale [n, D] (every token's rows), fp64."""
    _, xhat, rstd = _stats(h, 1e-6)
    a = xhat * (1 + scale) + shift
    ea = (1 + scale).abs() * ((22 + K_RSQ) * U * xhat.abs() + 16 * U * rstd * h.abs().mean(-1, keepdim=True)) + 4 * U * a.abs()
    Wo, bo = w["out_w"], w["out_b"]
    m, S = a @ Wo.t() + bo, a.abs() @ Wo.abs().t()
    return m, ea @ Wo.abs().t() + (h.shape[1] + 3) * U * S + U * ((m - bo).abs() + m.abs())


def final_rows(mods, D, traj):
    """shift, scale [n, D] of the head for every token: the adaLN rows behind the block's six (run_eval: mods + depth 6 D)."""
    m = mods.double()
    return m[traj, 6 * D:7 * D], m[traj, 7 * D:8 * D]


def step_reference(m_ref_bar, x, rec, w_noise=None, saved=None):
    """x <- ax x + am m + aw w + as saved."""
    m, bm = m_ref_bar
    ax, am, aw, as_ = rec
    terms = [ax * x, am * m] + ([aw * w_noise] if aw != 0 else []) + ([as_ * saved] if as_ != 0 else [])
    return sum(terms), abs(am) * bm + 4 * U * sum(t.abs() for t in terms)


def worst(got, ref_bar):
    """(worst |got - ref| / bar, its flat index); non-finite values count as infinite."""
    ref, bar = ref_bar
    r = (got.double().reshape(ref.shape) - ref).abs() / bar.clamp_min(1e-300)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), i


def ulps(got, ref):
    """The worst |got - ref| in units of u max(|ref|, 1): the measurement behind K_TRIG, K_EXP, K_RSQ."""
    return float(((got.double() - ref).abs() / (U * ref.abs().clamp_min(1.0))).max())


# ---- the kernels' summation orders, emulated in fp32 on the CPU, with the mutations of test_frame_cases.py ---------------------------------
def _silu32(x):
    return x / (1.0 + torch.exp(-x))


def emulate_dense(form, x, W, b, add, pre, post, drop=None, no_bias=None, add_mod=0, add_rows_wrong=None):
    """fp32: k_dense_rows (a lane's 8 strided terms, then the wave tree), k_dense_tiled (k ascending), k_dense_mfma (a quarter of k per
    wave, ((p0 + p1) + p2) + p3).  Mutations: drop = (row tile, k-step of 16) on the
    rows of that tile (k 16 s .. 16 s + 15 in every form); no_bias = a row tile that misses the bias; add_rows_wrong = m: the add row is taken % m."""
    x, W, b = x.float(), W.float(), b.float()
    xin = _silu32(x) if pre else x
    rows, I = x.shape
    tile = form.row_tile or rows

    if drop is not None:  # (the step's inputs of that tile's rows zeroed: the same sum without the step)
        xin = xin.clone()
        xin[tile * drop[0]:tile * drop[0] + tile, 16 * drop[1]:16 * drop[1] + 16] = 0

    def prod(k0, k1):
        return xin[:, k0:k1] @ W[:, k0:k1].t()

    if form.kernel == "k_dense_mfma":
        kq = form.kq
        parts = []
        for wv in range(4):
            acc = torch.zeros(rows, W.shape[0])
            for k in range(wv * kq, (wv + 1) * kq, 2):
                acc = acc + prod(k, k + 2)
            parts.append(acc)
        v = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    elif form.kernel == "k_dense_tiled":
        v = torch.zeros(rows, W.shape[0])
        for k in range(0, I, 16):
            v = v + prod(k, min(k + 16, I))
    else:
        lanes = torch.zeros(rows, W.shape[0], 64)
        for k in range(0, I, 64):
            for j in range(4):
                sl = slice(k + 16 * j, min(k + 16 * j + 16, I))
                if sl.start >= I:
                    break
                p = xin[:, None, sl] * W[None, :, sl]
                lanes[:, :, 16 * j:16 * j + p.shape[-1]] += p
        w = lanes
        while w.shape[-1] > 1:
            w = w[..., :w.shape[-1] // 2] + w[..., w.shape[-1] // 2:]
        v = w[..., 0]
    bias = b.expand(rows, -1).clone()
    if no_bias is not None:
        bias[tile * no_bias:tile * no_bias + tile] = 0
    v = v + bias
    if add is not None:
        idx = torch.arange(rows)
        if add_rows_wrong:
            idx = idx % add_rows_wrong
        elif add_mod:
            idx = idx % add_mod
        v = v + add.float()[idx]
    return _silu32(v) if post else v


def emulate_embed(mode, x, wts, mask, base, form, cus=CUS, drop_c=None, no_bias=False, other_mask_row=None, stale_xs=False):
    """fp32 k_embed (c ascending, then the added row) / k_embed_mfma (the same chain, (b0 + row) added behind it).  Mutations: drop_c = (tile,
    c): that input of that tile's tokens is left out; no_bias: the last tile misses bias + bias2; other_mask_row = tile: its tokens take
    the other mask_emb row; stale_xs (the defect k_embed had at 256 < DQ < 512): features >= 256 of every tile but a workgroup's last are
    computed from the inputs the first trip left staged - the workgroup's LAST tile - with only every 256th element, the ones the
    D - 256 threads of the second trip restage, replaced by the tile's own."""
    W = (wts["cond_w"] if mode == 0 else wts["x_in_w"]).float()
    x = x.float()
    n, C = x.shape
    D = W.shape[0]
    tok = form.tok
    tile_of = torch.arange(n) // tok
    acc = torch.zeros(n, D)
    for c in range(C):
        term = x[:, c:c + 1] * W[None, :, c]
        if drop_c is not None and drop_c[1] == c:
            term[tile_of == drop_c[0]] = 0
        acc = acc + term
    if stale_xs:
        assert form.kind == "reg" and 256 < form.dq < 512
        xs_of = x.clone()  # what features >= 256 see as the tile's inputs
        for wg in range(form.grid):
            tiles = list(range(wg, form.tiles, form.grid))
            last = tiles[-1]
            for t in tiles[:-1]:
                # second trip: threads 0 .. DQ - 257 restage elements i = tid, tid + 256, ... of xs[tok][CMAX]; the rest is the first trip's last tile
                cur = torch.zeros(tok, form.cmax)
                lo, hi = tok * last, min(tok * last + tok, n)
                cur[:hi - lo, :C] = x[lo:hi]
                new = torch.zeros(tok, form.cmax)
                lo2, hi2 = tok * t, min(tok * t + tok, n)
                new[:hi2 - lo2, :C] = x[lo2:hi2]
                flat, fnew = cur.reshape(-1), new.reshape(-1)
                for tid in range(form.dq - 256):
                    flat[tid::256] = fnew[tid::256]
                xs_of[lo2:hi2] = flat.reshape(tok, form.cmax)[:hi2 - lo2, :C]
        acc2 = torch.zeros(n, D)
        for c in range(C):
            acc2 = acc2 + xs_of[:, c:c + 1] * W[None, :, c]
        acc[:, 256:] = acc2[:, 256:]
    if mode == 0:
        b0 = wts["cond_b"].float() + wts["x_in_b"].float()
        b0 = b0.expand(n, -1).clone()
        if no_bias:
            b0[tile_of == form.tiles - 1] = 0
        m = (mask != 0).long().clone()
        if other_mask_row is not None:
            m[tile_of == other_mask_row] ^= 1
        return acc + (b0 + wts["mask_emb"].float()[m])
    return acc + base.float()


def emulate_ln(h, eps):
    h = h.float()
    mean = h.mean(-1, keepdim=True)
    dev = h - mean
    return dev * torch.rsqrt((dev * dev).mean(-1, keepdim=True) + eps)


def emulate_stats(h, gsz=256):
    """k_embed<STATS>'s per-group (mean, m2) and k_ln_finalize's pairwise combination, fp32."""
    g = h.float().reshape(h.shape[0], -1, gsz)
    mp = g.mean(-1)
    m2 = ((g - mp[..., None]) ** 2).sum(-1)
    mean = mp.sum(-1) / mp.shape[1]
    q = (m2 + gsz * (mp - mean[:, None]) ** 2).sum(-1)
    rstd = torch.rsqrt(q / (gsz * mp.shape[1]) + 1e-6)
    return torch.stack([rstd, -mean * rstd], -1)


def emulate_head(h, mods, wts, C, tpt, shared, form, rec=None, x=None, w_noise=None, saved=None, neighbour_row=False, stale=False,
                 drop=None, no_bias=False, unwritten_last_slab=False):
    """fp32 k_head_step_mfma: LayerNorm + modulate, a quarter of k per wave in 2-deep steps, ((p0 + p1) + p2) + p3 + bo, the update.
    Mutations: neighbour_row: the rows of a straddling tile all take the tile's FIRST trajectory's shift / scale; stale: a
    single-trajectory tile that follows a tile of another trajectory in its workgroup keeps the earlier shift / scale; drop = (tile,
    k-step of 8); no_bias: the last tile misses bo; unwritten_last_slab: the channels of the last slab (c >= 32 (slabs - 1)) stay as they were."""
    n, D = h.shape
    traj = torch.zeros(n, dtype=torch.long) if shared else torch.arange(n) // tpt
    row_of = traj.clone()
    for wg in range(form.grid):
        cur = -1
        for tile in range(wg, form.tiles, form.grid):
            lo, hi = 32 * tile, min(32 * tile + 32, n)
            first, last = int(traj[lo]), int(traj[hi - 1])
            if first == last:
                if stale and cur >= 0 and cur != first:
                    row_of[lo:hi] = cur
                else:
                    cur = first
            elif neighbour_row:
                row_of[lo:hi] = first
    m32 = mods.float()
    shift, scale = m32[row_of, 6 * D:7 * D], m32[row_of, 7 * D:8 * D]
    a = emulate_ln(h, 1e-6) * (1.0 + scale) + shift
    Wo, bo = wts["out_w"].float(), wts["out_b"].float()
    kw = D // 4
    parts = []
    tile_of = torch.arange(n) // 32
    for wv in range(4):
        acc = torch.zeros(n, C)
        for k in range(wv * kw, (wv + 1) * kw, 2):
            p = a[:, k:k + 2] @ Wo[:, k:k + 2].t()
            if drop is not None and k // 8 == drop[1]:
                p[tile_of == drop[0]] = 0
            acc = acc + p
        parts.append(acc)
    b = bo.expand(n, -1).clone()
    if no_bias:
        b[tile_of == form.tiles - 1] = 0
    m = ((parts[0] + parts[1]) + parts[2]) + parts[3] + b
    if rec is None:
        out, before = m, torch.zeros(n, C)
    else:
        ax, am, aw, as_ = rec
        out = ax * x.float() + am * m
        if aw != 0:
            out = out + aw * w_noise.float()
        if as_ != 0:
            out = out + as_ * saved.float()
        before = x.float()
    if unwritten_last_slab:
        c0 = 32 * ((C - 1) // 32)
        out = out.clone()
        out[:, c0:] = before[:, c0:]
    return out
