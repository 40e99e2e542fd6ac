"""k_linear1_ts as its own translation unit (csrc/unit_lin1.hip, compiled with options of its own; no scratch at hidden 512): the hidden-512
instances - 16 heads of 32, mlp_ratio 2 - on the work splits where the code AROUND the steady block loop runs most: segment heads, section
changes inside a segment, tile boundaries, the drain and the last flush.

  * the even cut: 257 * 256 - 37 = 65 755 tokens are 257 tiles (more than 256, so the (tile, block) sequence is cut evenly over the workgroups:
    20 560 blocks over 256 workgroups = 80.3 each, so the ranges start inside the q, k, v and mlp sections, every range crosses a tile boundary,
    and the last tile is ragged);
  * the shared tile: 600 tokens are 3 tiles, several workgroups per tile, every range one segment (4 waves on the default path, 8 in the fused form);
  * 4 waves on 128-token tiles: 7 680 tokens on the default handle;
  * q / k / v as head-major planes on a spatial sub-block (129 <= L <= 256) and as rows on a temporal one.

Through lsl_debug_block_ex / lsl_debug_taps (test_hip_gemm.check_case: both sub-blocks, every element of a, q, k, v, GELU(mlp) and h_out against
its fp64 reference at the bars of gemm_cases.py) on a default and on an ln_fuse handle.  Those two calls hand out the operand `a`, so they run the
standalone LayerNorm in front of the default linear1 on either handle; the fused instance k_linear1_ts<32, 512, 8, true> runs in a network
evaluation only.  It is therefore checked there, on the same token counts: against the default handle - itself held to fp64 above - at the bar of
tests/test_hip_lnf.py (3e-5 relative L2: the two operands differ by an ulp of bf16 here and there), against the oracle where the CPU can afford
it, and bit for bit between a trajectory alone and in a batch of 3."""
import pytest
import torch

import gemm_cases as gc
from conftest import parity, rel_l2
from test_hip_gemm import check_case
from test_hip_lnf import build, inputs

pytestmark = pytest.mark.gpu

MODEL = "d512h16r2"
EVEN_CUT = (5, 13151, 1)   # 257 * 256 - 37 tokens; the temporal sub-block attends over 13 151 positions, the spatial one over 1
SHARED_TILE = (1, 3, 200)  # 600 tokens; planes on the spatial sub-block
FOUR_WAVES = (1, 30, 256)  # 7 680 tokens; planes on the spatial sub-block
CASES = tuple((MODEL, *shape, handle) for shape in (EVEN_CUT, SHARED_TILE) for handle in ("plain", "lnf")) + ((MODEL, *FOUR_WAVES, "plain"),)
NET = dict(depth=2, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2, vec_in_dim=8)  # (a vector input: one modulation row per trajectory)
FUSED_LABEL = "k_linear1_ts<32, 512, 8, true> (LayerNorm fused)"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def test_the_shapes_reach_the_paths_they_are_meant_for():
    assert EVEN_CUT[0] * EVEN_CUT[1] * EVEN_CUT[2] == 257 * 256 - 37
    for case in CASES:
        pl, n = gc.plan(case), gc.n_tokens(case)
        assert pl.lin1_ts and pl.lin2_kind == "ws", case
        assert pl.waves == (8 if n > 10240 else 4), case
        assert pl.planes == (129 <= case[3] <= 256), case
    d = gc.dims(MODEL)
    assert (d.D, d.hdp, d.F1 // 32) == (512, 32, 80)
    assert -(-gc.n_tokens(CASES[0]) // 256) == 257 > gc.CUS
    assert gc.CUS // -(-600 // 256) >= 2 and gc.CUS // -(-7680 // 128) >= 2  # several workgroups per tile


@pytest.mark.parametrize("case", CASES, ids=gc.case_id)
def test_hidden_512_elements_against_fp64(case, dev):
    check_case(case, dev)


@pytest.fixture(scope="module")
def nets(dev):
    sh, p, fused = build(NET, dev, True)
    _, _, default = build(NET, dev, False)
    return sh, p, fused, default


def evaluate(net, args, dev, profile=False):
    """One network evaluation; with `profile`, also what the linear1 class launched (lsl_profile_kernel_name, class 0)."""
    from lam_slide_amd import _lib
    lib = _lib.load()
    if profile:
        _lib.check(lib.lsl_profile_enable(net._handle, 0, 4))
    out = net(*(v.to(dev) if v is not None else None for v in args))
    torch.cuda.synchronize()
    name = None
    if profile:
        name = lib.lsl_profile_kernel_name(net._handle).decode()
        lib.lsl_profile_enable(net._handle, -1, 0)
    return out, name


@pytest.mark.parametrize("shape", (EVEN_CUT, SHARED_TILE), ids=lambda s: "x".join(map(str, s)))
def test_fused_instance_against_the_default_handle(shape, nets, dev):
    sh, p, fused, default = nets
    args = inputs(sh, *shape)
    got, name = evaluate(fused, args, dev, profile=True)
    base, _ = evaluate(default, args, dev)
    assert name == FUSED_LABEL, name
    assert torch.isfinite(got).all()
    tag = "lin1_unit.fused." + "x".join(map(str, shape))
    print(f"{tag}: relative L2 against the default handle {rel_l2(got.cpu(), base.cpu()):.3e}")
    parity(tag + ".vs_default", rel_l2(got.cpu(), base.cpu()), 3e-5)
    assert not torch.equal(got, base), "the fused form was expected to run (its operand differs from the default path's by an ulp somewhere)"
    if shape == SHARED_TILE:  # (600 tokens: the CPU oracle is affordable)
        from oracle import latent_net
        want = latent_net.forward(p, sh, *args)
        parity(tag + ".vs_oracle", rel_l2(got.cpu(), want), 6e-4)


def test_fused_instance_gives_a_trajectory_the_same_bits_alone_and_in_a_batch_of_three(nets, dev):
    sh, _, fused, _ = nets
    B, (_, T, L) = 3, SHARED_TILE
    args = inputs(sh, B, T, L)  # 1 800 tokens: 8 tiles; alone: 3 tiles
    full, name = evaluate(fused, args, dev, profile=True)
    assert name == FUSED_LABEL, name
    for k in (0, 2):
        one, name = evaluate(fused, tuple(v[k:k + 1] if v is not None else None for v in args), dev, profile=True)
        assert name == FUSED_LABEL, name
        assert torch.equal(full[k:k + 1], one), f"trajectory {k}: alone vs in the batch of {B}"
