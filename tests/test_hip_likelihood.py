"""GPU tests of the tangent pass (``lsl_forward_jvp`` / ``LatentSIV3.jvp``), ``lsl_dot_rows`` and ``Sampler.sample_ode_likelihood`` on the
device path, against the CPU oracles of tests/jvp_oracle.py.

Bars.  The tangent's bar comes from a CPU model of the device's rounding, not from the device code: oracle (b) rounds the operands of the four
large products to bf16 for primal and tangent alike; its relative L2 errors against the fp64 oracle (a) on a case are e_p (primal) and e_t
(tangent), and the device's tangent must be within 4 max(e_t, e_p) of oracle (a).  The factor 4 covers what the model leaves out (the kernels'
fp32 accumulation order, exp2 / rsqrt, the GELU fit, the rounding of the pre-scaled q).  The existing forward is measured against the same model
in the same run (ratio = error / e_p); where its own ratio exceeds 2 the factor of that case is twice that ratio, and the record says so.
Every figure is printed ("PARITY name measured bar", "JVP-RATIO case forward tangent"); profiles/jvp_parity.txt keeps a run's lines.

Shapes: every case of tests/golden/f2_shapes.npz (hd 16 / 24 / 32, S in {2, 8, 30, 33, 40, 64}, normalize, y, shared weights, ragged tiles)
and the smallest shapes at which the remaining edges can go wrong: an axis of length 1 on either side (o' = v'), (2, 33, 3), hd 24 with a
65-long axis (hidden 192 / 8 heads: a hidden size must be a multiple of 64, so hd 24 cannot be had at hidden 96), the first temporal length
past 256, in_dim 3, three trajectories with different t and y rows, and the first spatial length at which the plan leaves the primal
q | k | v as head-major planes (another path of the pass), and axes of 8 and 9 positions (the threshold between the attention JVP's two
kernels; the cases above have axes on both sides of it at 16- and 32-wide heads), and 96 input channels at hd 24 (the peptide model's
embedding and head kernels)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import jvp_oracle
from conftest import parity, rel_l2, shape_from
from oracle import latent_net

pytestmark = pytest.mark.gpu

EXTRA_CASES = {
    # name: (NetShape kwargs, B, T, L, weight seed)
    "t1_l7": (dict(depth=1, in_dim=8, hidden_size=64, num_heads=4), 1, 1, 7, 31),
    "t7_l1": (dict(depth=1, in_dim=8, hidden_size=64, num_heads=4), 1, 7, 1, 32),
    "b2_t33_l3": (dict(depth=1, in_dim=8, hidden_size=64, num_heads=4), 2, 33, 3, 33),
    "hd24_t3_l65": (dict(depth=1, in_dim=12, hidden_size=192, num_heads=8, mlp_ratio=1), 1, 3, 65, 34),
    "t257_l2": (dict(depth=1, in_dim=8, hidden_size=64, num_heads=2), 1, 257, 2, 35),
    "in_dim3": (dict(depth=1, in_dim=3, hidden_size=64, num_heads=4), 1, 4, 5, 36),
    "b3_t_y": (dict(depth=1, in_dim=8, hidden_size=128, num_heads=4, vec_in_dim=16), 3, 5, 6, 37),
    # the first spatial length whose primal q | k | v travel as head-major planes (token-stationary linear1, long stream attention)
    "planes_l129": (dict(depth=1, in_dim=8, hidden_size=128, num_heads=4), 1, 2, 129, 38),
    # the two sides of the threshold between the attention JVP's kernels: an axis of 8 positions (a lane per query), one of 9 (matrix cores)
    "t9_l8": (dict(depth=1, in_dim=8, hidden_size=64, num_heads=4), 1, 9, 8, 39),
    # the peptide model's frame at a small size: 96 input channels (the wide-input embedding, in place on the tangent; the head at C = 96), hd 24
    "c96_hd24": (dict(depth=1, in_dim=96, hidden_size=192, num_heads=8, mlp_ratio=1), 1, 3, 5, 40),
}
LINEARITY_CASES = ("hd16_s8x30", "hd24_s2x64", "hd32_s40x33")  # one per head width


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def build_net(sh, params, dev):
    from lam_slide_amd import LatentSIV3
    net = LatentSIV3(depth=sh.depth, in_dim=sh.in_dim, hidden_size=sh.hidden_size, num_heads=sh.num_heads, vec_in_dim=sh.vec_in_dim,
                     mlp_ratio=sh.mlp_ratio, theta=sh.theta, normalize=sh.normalize, share_weights=sh.share_weights,
                     attention_mode=sh.attention_mode, reset_parameters=False)
    net.load_state_dict(params)
    return net.to(dev)


class Case:
    """Inputs, weights and a seeded +-1 tangent of one case; the oracle side is computed once, on the CPU, and shared."""

    def __init__(self, name, sh, p, x, t, x_cond, mask, y):
        self.name, self.sh, self.p = name, sh, p
        self.x, self.t, self.x_cond, self.mask, self.y = x, t, x_cond, mask, y
        self.tangent = jvp_oracle.rademacher(x.shape, 1000 + len(name))
        self._oracle = None
        self._device = {}

    def oracle(self):
        if self._oracle is None:
            self._oracle = jvp_oracle.model_errors(self.p, self.sh, self.x, self.t, self.x_cond, self.mask, self.y, self.tangent)
        return self._oracle  # out (a), out_tangent (a), e_p, e_t

    def on(self, dev):
        if dev not in self._device:
            net = build_net(self.sh, self.p, dev)
            args = [v.to(dev) if v is not None else None for v in (self.x, self.t, self.x_cond, self.mask, self.y)]
            self._device[dev] = (net, args)
        return self._device[dev]


@pytest.fixture(scope="module")
def cases(golden):
    out = {}
    f = golden("f2_shapes.npz")
    for n in sorted({k.split("/")[0] for k in f.raw.files}):
        g = f.group(n)
        sh = shape_from({k[6:]: v for k, v in g.items() if k.startswith("shape.")})
        out[n] = Case(n, sh, latent_net.random_params(sh, seed=int(g["weight_seed"])), g["x"], g["t"], g["x_cond"], g["mask"], g.get("y"))
    for n, (kw, B, T, L, seed) in EXTRA_CASES.items():
        sh = latent_net.NetShape(**kw)
        gen = torch.Generator().manual_seed(seed)
        x, xc = torch.randn(B, T, L, sh.in_dim, generator=gen), torch.randn(B, T, L, sh.in_dim, generator=gen)
        mask = (torch.rand(B, T, L, generator=gen) > 0.5).long()
        t = torch.rand(B, generator=gen)
        y = torch.randn(B, sh.vec_in_dim, generator=gen) if sh.vec_in_dim else None
        out[n] = Case(n, sh, latent_net.random_params(sh, seed=seed), x, t, xc, mask, y)
    return out


F2_NAMES = ("hd16_s8x30", "hd24_s2x64", "hd32_s64x5_norm_y", "hd16_share", "hd32_s40x33")


def tangent_factor(name, fwd_ratio):
    """4, or twice the forward's own ratio against the same model where that exceeds 2 (printed: the record says so)."""
    if fwd_ratio > 2.0:
        print(f"JVP-NOTE {name}: the forward's own ratio {fwd_ratio:.2f} exceeds 2: factor {2 * fwd_ratio:.2f} instead of 4")
        return 2.0 * fwd_ratio
    return 4.0


@pytest.mark.parametrize("name", F2_NAMES + tuple(EXTRA_CASES))
def test_jvp_parity(name, cases, golden, dev):
    """out is the forward's bits; out_tangent within the modelled bar of the fp64 oracle."""
    assert set(F2_NAMES) == {k.split("/")[0] for k in golden("f2_shapes.npz").raw.files}
    c = cases[name]
    net, (x, t, xc, mask, y) = c.on(dev)
    want = net(x, t, xc, mask, y)
    out, out_t = net.jvp(x, t, xc, mask, y, tangent=c.tangent.to(dev))
    assert net.last_path == "hip-jvp"
    assert torch.equal(out, want), name
    o_out, o_out_t, e_p, e_t = c.oracle()
    err_p, err_t = rel_l2(out.cpu(), o_out), rel_l2(out_t.cpu(), o_out_t)
    fwd_ratio, tan_ratio = err_p / e_p, err_t / max(e_t, e_p)
    print(f"JVP-RATIO {name} model e_p {e_p:.3e} e_t {e_t:.3e} forward {fwd_ratio:.3f} tangent {tan_ratio:.3f}")
    parity(f"jvp.{name}", err_t, tangent_factor(name, fwd_ratio) * max(e_t, e_p))


@pytest.mark.parametrize("name", LINEARITY_CASES)
def test_jvp_is_linear_bit_for_bit(name, cases, dev):
    c = cases[name]
    net, (x, t, xc, mask, y) = c.on(dev)
    v = c.tangent.to(dev)
    _, j = net.jvp(x, t, xc, mask, y, tangent=v)
    _, j0 = net.jvp(x, t, xc, mask, y, tangent=torch.zeros_like(v))
    _, jn = net.jvp(x, t, xc, mask, y, tangent=-v)
    _, j2 = net.jvp(x, t, xc, mask, y, tangent=2 * v)
    assert float(j.abs().max()) > 0 and torch.isfinite(j).all()
    assert torch.count_nonzero(j0) == 0
    assert torch.equal(jn, -j)
    assert torch.equal(j2, 2 * j)


def test_jvp_batch_and_pass_independence(cases, dev):
    """Trajectory b alone, in the batch, and with one trajectory per pass: identical bits for out and out_tangent."""
    c = cases["b3_t_y"]
    net, (x, t, xc, mask, y) = c.on(dev)
    v = c.tangent.to(dev)
    out, out_t = net.jvp(x, t, xc, mask, y, tangent=v)
    net.set_chunk(1)
    try:
        out_1, out_t_1 = net.jvp(x, t, xc, mask, y, tangent=v)
    finally:
        net.set_chunk(0)
    assert torch.equal(out_1, out) and torch.equal(out_t_1, out_t)
    for b in range(x.shape[0]):
        s = slice(b, b + 1)
        o_b, ot_b = net.jvp(x[s].contiguous(), t[s].contiguous(), xc[s].contiguous(), mask[s].contiguous(), y[s].contiguous(), tangent=v[s].contiguous())
        assert torch.equal(o_b, out[s]) and torch.equal(ot_b, out_t[s]), b


@pytest.mark.parametrize("per", [1, 4095, 4096, 4097, 3 * 4096 + 5])
def test_dot_rows(per, dev):
    """Against a float64 numpy dot.  The products of two fp32 values are exact in fp64, so the error of any fp64 summation order of n terms is
    at most n 2^-53 sum |a b| (to first order; the factor n - 1 rounded up); a row's bits are the same alone and in the batch."""
    from lam_slide_amd.transport import dot_rows
    B = 3
    g = torch.Generator().manual_seed(per)
    a, b = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g)
    got = dot_rows(a.to(dev), b.to(dev))
    assert got.dtype == torch.float64 and tuple(got.shape) == (B,)
    a64, b64 = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
    for r in range(B):
        want = float(np.dot(a64[r], b64[r]))
        bound = per * 2.0 ** -53 * float(np.abs(a64[r] * b64[r]).sum())
        err = abs(float(got[r]) - want)
        print(f"DOT-ROWS per {per} row {r} err {err:.3e} bound {bound:.3e}")
        assert err <= bound
        alone = dot_rows(a[r:r + 1].to(dev), b[r:r + 1].to(dev))
        assert torch.equal(alone[0], got[r])


def _sampler(path, pred, **kw):
    from lam_slide_amd import CreateTransport, Sampler
    return Sampler(CreateTransport(path, pred)(), **kw)


@pytest.mark.parametrize("path,pred", [("Linear", "velocity"), ("GVP", "noise")])
def test_one_euler_step_on_the_device_path(path, pred, cases, dev):
    """z and delta_logp of one Euler step against the fp64 oracle, within the bars of test_jvp_parity carried through the step:
    z = x - dt (vx x + vm net):      |z - z_ref| <= |dt vm| |net - net_ref| + the fp32 arithmetic of the update (three roundings: 2^-22 |z|)
    delta = dt (vx N + vm eps . j):  |delta - delta_ref| <= |dt vm| sqrt(N) |j - j_ref| (Cauchy-Schwarz, |eps| = sqrt(N)) + 2^-22 |delta|."""
    c = cases["hd16_s8x30"]
    net, (x, t, xc, mask, y) = c.on(dev)
    s = _sampler(path, pred)
    eps = c.tangent
    fn = s.sample_ode_likelihood(sampling_method="euler", num_steps=2, eps=eps.to(dev))
    logp, z = fn(x, net, x_cond=xc, x_cond_mask=mask)
    assert s.last_path == "likelihood-device" and s.last_ode_stats["nfe"] == 1
    tr = s.transport
    t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False, last_step_size=0.0)
    dt = t1 - t0
    tf = float(torch.tensor(1.0 - t0, dtype=torch.float32))
    vx, vm = tr.velocity_coeffs(tf)
    tt = torch.full((x.shape[0],), tf)
    o_out, o_j, e_p, e_t = jvp_oracle.model_errors(c.p, c.sh, c.x, tt, c.x_cond, c.mask, c.y, eps)
    n_el = c.x[0].numel()
    z_ref = c.x.double() - dt * (vx * c.x.double() + vm * o_out)
    delta_ref = dt * (vx * n_el + vm * (eps.double() * o_j).reshape(x.shape[0], -1).sum(1))
    logp_ref = tr.prior_logp(z_ref) - delta_ref
    fwd = net(x, tt.to(dev), xc, mask, y)
    factor = tangent_factor("euler-step", rel_l2(fwd.cpu(), o_out) / e_p)
    z_bar = factor * e_p * abs(dt * vm) * float(o_out.norm() / z_ref.norm()) + 2.0 ** -22
    parity(f"likelihood.step.{path}.{pred}.z", rel_l2(z.cpu(), z_ref), z_bar)
    delta = tr.prior_logp(z.cpu().double()) - logp.cpu().double()
    d_bar = abs(dt * vm) * math.sqrt(n_el) * factor * max(e_t, e_p) * float(o_j.norm()) + 2.0 ** -22 * float(delta_ref.abs().max()) \
        + 2.0 ** -22 * float(logp_ref.abs().max())  # (logp = prior - delta is rounded to fp32 at the size of the prior term)
    parity(f"likelihood.step.{path}.{pred}.delta_logp", float((delta - delta_ref).abs().max()), d_bar)


@pytest.mark.parametrize("method,num_steps", [("euler", 5), ("dopri5", 50)])
def test_multi_step_likelihood_against_the_generic_path(method, num_steps, golden, dev):
    """euler with 4 steps and the default dopri5 with a fixed probe on the F1 shape: logp and z of the device path against the generic path
    on oracle (a) in fp64; bar = 4 x the error the generic path on oracle (b) shows in the same solve."""
    f = golden("f1_block.npz")
    sh = shape_from(f.group("shape"))
    p = f.group("p")
    x, xc, mask, y = f["x"], f["x_cond"], f["mask"], f["y"]
    eps = jvp_oracle.rademacher(x.shape, 77)
    p64 = latent_net.cast_params(p, torch.float64)

    def oracle_a(xx, tt, **kw):
        return latent_net.forward(p64, sh, xx, tt, kw["x_cond"], kw["x_cond_mask"], kw["y"])

    def oracle_b(xx, tt, **kw):
        with jvp_oracle._bf16_blocks():
            return latent_net.forward(p64, sh, xx, tt, kw["x_cond"], kw["x_cond_mask"], kw["y"])

    kw64 = dict(x_cond=xc.double(), x_cond_mask=mask, y=y.double())
    ref = {}
    for tag, model in (("a", oracle_a), ("b", oracle_b)):
        s = _sampler("Linear", "velocity")
        fn = s.sample_ode_likelihood(sampling_method=method, num_steps=num_steps, eps=eps.double())
        ref[tag] = fn(x.double(), model, **kw64)
        assert s.last_path == "likelihood-generic"
    net = build_net(sh, p, dev)
    s = _sampler("Linear", "velocity")
    fn = s.sample_ode_likelihood(sampling_method=method, num_steps=num_steps, eps=eps.to(dev))
    logp, z = fn(x.to(dev), net, x_cond=xc.to(dev), x_cond_mask=mask.to(dev), y=y.to(dev))
    assert s.last_path == "likelihood-device"
    print(f"LIKELIHOOD-NFE {method} {s.last_ode_stats['nfe']}")
    if method == "euler":
        assert s.last_ode_stats["nfe"] == num_steps - 1
    z_model, logp_model = rel_l2(ref["b"][1], ref["a"][1]), float((ref["b"][0] - ref["a"][0]).abs().max())
    print(f"LIKELIHOOD-LOGP {method} oracle {[float(v) for v in ref['a'][0]]} device {[float(v) for v in logp.cpu()]}")
    parity(f"likelihood.{method}.z", rel_l2(z.cpu(), ref["a"][1]), 4 * z_model)
    parity(f"likelihood.{method}.logp", float((logp.cpu().double() - ref["a"][0]).abs().max()), 4 * logp_model)


def test_refusals_enqueue_nothing(dev):
    """Linear-attention, tail and ln_fuse handles: NotImplementedError from the sampler, -21 from the library, and the output buffers keep
    their sentinel."""
    from lam_slide_amd import _lib
    kw = dict(depth=1, in_dim=8, hidden_size=256, num_heads=8, mlp_ratio=2)
    B, T, L = 1, 4, 5
    g = torch.Generator().manual_seed(3)
    x, xc = torch.randn(B, T, L, 8, generator=g).to(dev), torch.randn(B, T, L, 8, generator=g).to(dev)
    mask, t = torch.ones(B, T, L, dtype=torch.long, device=dev), torch.full((B,), 0.5, device=dev)
    setters = {"linear": "lsl_model_set_attention_mode", "tail": "lsl_model_set_tail", "ln_fuse": "lsl_model_set_ln_fuse"}
    for form, setter in setters.items():
        sh = latent_net.NetShape(**kw, attention_mode="linear" if form == "linear" else "scaled_dot_product")
        net = build_net(sh, latent_net.random_params(sh, seed=9), dev)
        if form == "tail":
            net.set_tail(True)
        if form == "ln_fuse":
            net.set_ln_fuse(True)
        net.ensure_packed(dev)
        s = _sampler("Linear", "velocity")
        with pytest.raises(NotImplementedError):
            s.sample_ode_likelihood(sampling_method="euler", num_steps=2)(x, net, x_cond=xc, x_cond_mask=mask)
        with pytest.raises(ValueError, match=setter):
            net.jvp(x, t, xc, mask, tangent=torch.ones_like(x))
        out, out_t = torch.full_like(x, 7.0), torch.full_like(x, 9.0)
        io, keep = net.make_io(x, xc, mask, None, t, out)
        ws = torch.empty(1 << 26, dtype=torch.uint8, device=dev)
        tan = torch.ones_like(x)
        rc = _lib.load().lsl_forward_jvp(net._handle, C.byref(io), tan.data_ptr(), out_t.data_ptr(), ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert rc == -21 and setter in _lib.last_error(), (form, rc, _lib.last_error())
        assert bool((out == 7.0).all()) and bool((out_t == 9.0).all()), form
        del keep
