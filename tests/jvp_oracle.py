"""CPU references for the tangent pass of the network (``lsl_forward_jvp``, ``LatentSIV3.jvp``), both by ``torch.func.jvp`` over the pinned
oracle network (``oracle/latent_net.py``) in float64:

  (a) ``jvp_fp64``   the exact directional derivative of the oracle network;
  (b) ``jvp_bf16``   the same network with the operands of the four large products of every sub-block rounded to bf16 - linear1 (its
      LayerNorm'ed input and its weight), the two attention products (q, k; the probabilities, v) and linear2 (its input and its weight) -
      for the primal and the tangent alike: the rounding applies to the primal value and, as the derivative rule of the rounding, to the
      tangent value.  Everything else stays float64.  This is the CPU model of the device's rounding that the GPU tests take their bars
      from (the model leaves out the kernels' fp32 accumulation order, exp2 / rsqrt, the GELU fit and the rounding of the pre-scaled q).

Test infrastructure only."""
from __future__ import annotations

import contextlib
import math

import torch

from oracle import latent_net


class _RoundBf16(torch.autograd.Function):
    """x rounded to bf16 (kept in x's dtype); forward-mode rule: the tangent rounded the same way."""

    @staticmethod
    def forward(x):
        return x.float().bfloat16().to(x.dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass

    @staticmethod
    def jvp(ctx, xt):
        return xt.float().bfloat16().to(xt.dtype)

    @staticmethod
    def backward(ctx, g):  # (the generic likelihood path differentiates in reverse mode: the cotangent rounded the same way)
        return g.float().bfloat16().to(g.dtype)


def rnd(x):
    return _RoundBf16.apply(x)


def attn_mlp_block_bf16(p, pre, u, cos, sin, sh, taps=None, tag=""):
    """``latent_net.attn_mlp_block`` (softmax attention) with bf16 operands of its four large products."""
    G, S, D = u.shape
    H, hd = sh.num_heads, sh.head_dim
    z = torch.nn.functional.linear(rnd(u), rnd(p[pre + ".linear1.weight"]), p[pre + ".linear1.bias"])
    qkv, mlp = z[..., : 3 * D], z[..., 3 * D:]
    qkv = qkv.reshape(G, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = latent_net.head_rms(q, p[pre + ".norm.query_norm.scale"]).to(v.dtype)
    k = latent_net.head_rms(k, p[pre + ".norm.key_norm.scale"]).to(v.dtype)
    q, k = latent_net.rotate_pairs(q, cos, sin), latent_net.rotate_pairs(k, cos, sin)
    s = torch.matmul(rnd(q), rnd(k).transpose(-1, -2)) / math.sqrt(hd)
    a = torch.matmul(rnd(torch.softmax(s, dim=-1)), rnd(v))
    a = a.permute(0, 2, 1, 3).reshape(G, S, D)
    zin = rnd(torch.cat([a, latent_net.gelu_erf(mlp)], dim=-1))
    return torch.nn.functional.linear(zin, rnd(p[pre + ".linear2.weight"]), p[pre + ".linear2.bias"])


@contextlib.contextmanager
def _bf16_blocks():
    keep = latent_net.attn_mlp_block
    latent_net.attn_mlp_block = attn_mlp_block_bf16
    try:
        yield
    finally:
        latent_net.attn_mlp_block = keep


def _jvp(p, sh, x, t, x_cond, mask, y, tangent):
    p64 = latent_net.cast_params(p, torch.float64)
    args = (t.double(), x_cond.double(), mask, None if y is None else y.double())
    out, out_t = torch.func.jvp(lambda xx: latent_net.forward(p64, sh, xx, *args), (x.double(),), (tangent.double(),))
    return out.detach(), out_t.detach()


def jvp_fp64(p, sh, x, t, x_cond, mask, y, tangent):
    """(out, out_tangent) of the oracle network in float64: oracle (a)."""
    return _jvp(p, sh, x, t, x_cond, mask, y, tangent)


def jvp_bf16(p, sh, x, t, x_cond, mask, y, tangent):
    """(out, out_tangent) with bf16 operands of the four large products, primal and tangent alike: oracle (b)."""
    assert sh.attention_mode == "scaled_dot_product"
    with _bf16_blocks():
        return _jvp(p, sh, x, t, x_cond, mask, y, tangent)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def model_errors(p, sh, x, t, x_cond, mask, y, tangent):
    """What the bars of the GPU tests are made of: oracle (a), and the relative L2 errors of oracle (b) against it (primal, tangent)."""
    out, out_t = jvp_fp64(p, sh, x, t, x_cond, mask, y, tangent)
    b_out, b_out_t = jvp_bf16(p, sh, x, t, x_cond, mask, y, tangent)
    return out, out_t, rel(b_out, out), rel(b_out_t, out_t)


def rademacher(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(2, tuple(shape), generator=g).float() * 2 - 1
