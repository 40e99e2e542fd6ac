"""``Transport.prior_logp`` and ``Sampler.sample_ode_likelihood`` on the generic (torch) path, the argument checks of the tangent pass's C
entry points, and the CPU oracles the GPU tests take their bars from (tests/jvp_oracle.py).  No GPU needed."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import jvp_oracle
from conftest import ROOT
from oracle import latent_net

SYMBOLS = ("lsl_forward_jvp_workspace_bytes", "lsl_forward_jvp", "lsl_dot_rows")
PATHS, PREDS = ("Linear", "GVP", "VP"), ("velocity", "data", "noise", "score")


def _sampler(path="Linear", pred="velocity", **kw):
    from lam_slide_amd import CreateTransport, Sampler
    return Sampler(CreateTransport(path, pred)(), **kw)


# ---- prior_logp ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(3, 4, 5, 6), (2, 7)])
def test_prior_logp_closed_form(shape, dtype):
    tr = _sampler().transport
    z = torch.randn(*shape, generator=torch.Generator().manual_seed(1)).to(dtype)
    got = tr.prior_logp(z)
    assert got.dtype == dtype and tuple(got.shape) == (shape[0],)
    n = z[0].numel()
    for b in range(shape[0]):
        want = -0.5 * n * math.log(2 * math.pi) - 0.5 * float((z[b].double() ** 2).sum())
        assert abs(float(got[b]) - want) <= (1e-12 if dtype == torch.float64 else 2e-6) * abs(want)


# ---- the generic path ----
def test_generic_path_closed_form_diagonal_jacobian():
    """net(x, t) = x a with a per-channel a: the Jacobian is diagonal, so eps . J eps is its trace for ANY +-1 probe.  Linear path, velocity
    prediction (the drift is the network): dx/ds = -a x, d logp / ds = trace, over s in [t0, t1]."""
    B, T, L, Cc = 2, 3, 4, 5
    g = torch.Generator().manual_seed(0)
    a = torch.rand(Cc, generator=g, dtype=torch.float64) - 0.3
    x = torch.randn(B, T, L, Cc, generator=g, dtype=torch.float64)
    s = _sampler("Linear", "velocity")
    tr = s.transport
    t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False, last_step_size=0.0)
    fn = s.sample_ode_likelihood(sampling_method="dopri5", rtol=1e-6, atol=1e-8)  # (eps=None: a fresh probe per evaluation)
    logp, z = fn(x, lambda xx, tt: xx * a)
    assert s.last_path == "likelihood-generic" and s.last_ode_stats["nfe"] > 0
    z_want = x * torch.exp(-a * (t1 - t0))
    delta_want = T * L * float(a.sum()) * (t1 - t0)
    assert float((z - z_want).norm() / z_want.norm()) <= 1e-5
    delta = tr.prior_logp(z) - logp
    assert float((delta - delta_want).abs().max()) <= 1e-5 * abs(delta_want)
    assert float((logp - (tr.prior_logp(z_want) - delta_want)).abs().max()) <= 1e-5 * float(tr.prior_logp(z_want).abs().max())


@pytest.fixture(scope="module")
def small_net():
    sh = latent_net.NetShape(depth=1, in_dim=4, hidden_size=64, num_heads=4)
    p64 = latent_net.cast_params(latent_net.random_params(sh, seed=5), torch.float64)
    g = torch.Generator().manual_seed(2)
    B, T, L = 2, 3, 4
    x = torch.randn(B, T, L, 4, generator=g, dtype=torch.float64)
    xc = torch.randn(B, T, L, 4, generator=g, dtype=torch.float64)
    mask = (torch.rand(B, T, L, generator=g) > 0.5).long()
    eps = jvp_oracle.rademacher(x.shape, 3).double()

    def model(xx, tt, x_cond, x_cond_mask):
        return latent_net.forward(p64, sh, xx, tt, x_cond, x_cond_mask)

    return model, x, dict(x_cond=xc, x_cond_mask=mask), eps


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("path", PATHS)
def test_generic_path_against_a_hand_written_jvp_loop(path, pred, small_net):
    """Three Euler steps with a fixed probe: the method's reverse-mode expression against a loop written here with torch.func.jvp over the
    oracle network in float64 (eps . J^T eps = eps . J eps)."""
    model, x, kw, eps = small_net
    s = _sampler(path, pred)
    tr = s.transport
    if path == "VP" and pred in ("data", "noise"):
        # check_interval starts the VP path at t0 = 0, so the first drift is evaluated at time 1, where sigma = 0 and these two predictions
        # divide by it: the reference's expression returns NaN there; the float64 host arithmetic of this package raises instead
        with pytest.raises(ZeroDivisionError):
            s.sample_ode_likelihood(sampling_method="euler", num_steps=4, eps=eps)(x, model, **kw)
        return
    logp, z = s.sample_ode_likelihood(sampling_method="euler", num_steps=4, eps=eps)(x, model, **kw)
    assert s.last_ode_stats["nfe"] == 3
    t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False, last_step_size=0.0)
    grid = [float(v) for v in torch.linspace(t0, t1, 4)]
    n_el = x[0].numel()
    xs, delta = x.clone(), torch.zeros(x.shape[0], dtype=torch.float64)
    for ta, tb in zip(grid[:-1], grid[1:]):
        tf = float(torch.tensor(1.0 - ta, dtype=torch.float32))
        tv = torch.full((x.shape[0],), tf, dtype=torch.float64)
        out, j = torch.func.jvp(lambda xx: model(xx, tv, **kw), (xs,), (eps,))
        vx, vm = tr.velocity_coeffs(tf)
        xs = xs + (tb - ta) * -(vx * xs + vm * out)
        delta = delta + (tb - ta) * (vx * n_el + vm * (eps * j).reshape(x.shape[0], -1).sum(1))
    want = tr.prior_logp(xs) - delta
    assert float((z - xs).norm() / xs.norm()) <= 1e-7
    assert float(((logp - want).abs() / want.abs()).max()) <= 1e-7


def test_probe_draws():
    B, T, L, Cc = 2, 2, 3, 4
    x = torch.randn(B, T, L, Cc, generator=torch.Generator().manual_seed(4))
    seen = []

    def model(xx, tt):
        return xx * 0.5

    # eps=None: the reference expression's draw, first thing of the first evaluation
    torch.manual_seed(11)
    want = torch.randint(2, x.size(), dtype=torch.float, device=x.device) * 2 - 1
    s = _sampler()
    orig = torch.randint
    calls = []

    def spy(*a, **k):
        out = orig(*a, **k)
        calls.append(out * 2 - 1)
        return out

    torch.manual_seed(11)
    torch.randint = spy
    try:
        s.sample_ode_likelihood(sampling_method="euler", num_steps=3)(x, model)
    finally:
        torch.randint = orig
    assert len(calls) == s.last_ode_stats["nfe"] == 2 and torch.equal(calls[0], want) and not torch.equal(calls[0], calls[1])

    # a tensor is reused at every evaluation: the solve is deterministic
    eps = jvp_oracle.rademacher(x.shape, 9)
    runs = [_sampler().sample_ode_likelihood(sampling_method="euler", num_steps=3, eps=eps)(x, model) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])

    # a callable is called once per evaluation
    def make(shape, device):
        seen.append((shape, device))
        return torch.ones(shape, device=device)

    for method, kw in (("euler", dict(num_steps=3)), ("rk4", dict(num_steps=3)), ("dopri5", dict(num_steps=3))):
        seen.clear()
        s = _sampler()
        s.sample_ode_likelihood(sampling_method=method, eps=make, **kw)(x, model)
        assert len(seen) == s.last_ode_stats["nfe"] > 0 and seen[0] == (tuple(x.shape), x.device), method
    with pytest.raises(ValueError):
        _sampler().sample_ode_likelihood(sampling_method="euler", num_steps=3, eps=torch.ones(3))(x, model)
    with pytest.raises(NotImplementedError):
        _sampler().sample_ode_likelihood(sampling_method="bosh3")


def test_latent_net_on_the_cpu_says_why():
    """A LatentSIV3 the device path cannot serve raises NotImplementedError (here: not on a GPU), never a silent torch fall-back."""
    from lam_slide_amd import LatentSIV3
    net = LatentSIV3(depth=1, in_dim=4, hidden_size=64, num_heads=4)
    x = torch.zeros(1, 2, 3, 4)
    with pytest.raises(NotImplementedError, match="GPU"):
        _sampler().sample_ode_likelihood(sampling_method="euler", num_steps=2)(x, net, x_cond=x, x_cond_mask=torch.zeros(1, 2, 3, dtype=torch.long))
    with pytest.raises(RuntimeError):
        net.jvp(x, torch.zeros(1), x, torch.zeros(1, 2, 3, dtype=torch.long), tangent=x)


# ---- the C ABI ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    return _lib.load()


def test_symbols_in_header_exports_and_binding(lib):
    from lam_slide_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    exports = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*lsl_\*;", exports)  # (the map exports every lsl_ symbol)
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
        assert re.fullmatch(r"lsl_[a-z_]+", s) and getattr(lib, s).argtypes is not None
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6 and ", ".join(SYMBOLS) + " added" in header


def _handle(lib, hidden=64, heads=4, mlp=128):
    from lam_slide_amd import _lib
    hd = hidden // heads
    desc = _lib.ModelDesc(8, hidden, heads, hd, 16 if hd <= 16 else 32, mlp, 1, 0, 0, 10000.0)
    h = C.c_void_p()
    _lib.check(lib.lsl_model_create(C.byref(desc), C.byref(h)))
    return h


def test_argument_checks_before_anything_touches_a_gpu(lib):
    """Host memory stands in for every pointer: a refused call dereferences none of them."""
    from lam_slide_amd import _lib
    buf = (C.c_char * 256)()
    p = C.addressof(buf)
    h = _handle(lib)
    try:
        io = _lib.IO(p, p, p, None, p, p, 1, 2, 3)
        assert lib.lsl_forward_jvp(None, C.byref(io), p, p, p, 256, None) == -1
        assert lib.lsl_forward_jvp(h, None, p, p, p, 256, None) == -1
        assert lib.lsl_forward_jvp(h, C.byref(io), None, p, p, 256, None) == -1
        assert lib.lsl_forward_jvp(h, C.byref(io), p, None, p, 256, None) == -1
        assert lib.lsl_dot_rows(None, p, 1, 4, p, p, 256, None) == -1
        assert lib.lsl_dot_rows(p, p, 1, 4, None, p, 256, None) == -1
        assert lib.lsl_dot_rows(p, p, 0, 4, p, p, 256, None) == -3 and lib.lsl_dot_rows(p, p, 1, 0, p, p, 256, None) == -3
        assert lib.lsl_forward_jvp_workspace_bytes(None, 1, 2, 3) == 0 and lib.lsl_forward_jvp_workspace_bytes(h, 0, 2, 3) == 0
        for shape in ((0, 2, 3), (1, 0, 3), (1, 2, -1)):
            bad = _lib.IO(p, p, p, None, p, p, *shape)
            assert lib.lsl_forward_jvp(h, C.byref(bad), p, p, p, 256, None) == -3
            assert lib.lsl_last_error().decode() == "B, T, L must be positive"
        need = lib.lsl_forward_jvp_workspace_bytes(h, 1, 2, 3)
        assert need > lib.lsl_workspace_bytes(h, 1, 2, 3) > 0  # the forward's scratch plus the tangent stream's
        assert lib.lsl_forward_jvp(h, C.byref(io), p, p, p, need - 1, None) == -3
        assert lib.lsl_last_error().decode().startswith("workspace too small")
        assert lib.lsl_forward_jvp(h, C.byref(io), p, p, None, need, None) == -3
        # a pass holds fewer tokens than a forward pass: 4096 trajectories of 64 tokens are one forward pass and two tangent passes
        assert lib.lsl_pass_size(h, 4096, 8, 8) == 4096
        assert lib.lsl_forward_jvp_workspace_bytes(h, 4096, 8, 8) == lib.lsl_forward_jvp_workspace_bytes(h, 2048, 8, 8)
        assert lib.lsl_forward_jvp_workspace_bytes(h, 2048, 8, 8) > lib.lsl_forward_jvp_workspace_bytes(h, 1024, 8, 8)
    finally:
        lib.lsl_model_destroy(h)


def test_forms_the_pass_does_not_run_are_refused_with_the_setter(lib):
    from lam_slide_amd import _lib
    buf = (C.c_char * 256)()
    p = C.addressof(buf)
    io = _lib.IO(p, p, p, None, p, p, 1, 2, 3)
    cases = (("lsl_model_set_attention_mode", 64, 4, 128), ("lsl_model_set_tail", 256, 8, 512), ("lsl_model_set_ln_fuse", 64, 4, 128))
    for setter, hidden, heads, mlp in cases:
        h = _handle(lib, hidden, heads, mlp)
        try:
            assert getattr(lib, setter)(h, 1) == 0, (setter, lib.lsl_last_error())
            assert lib.lsl_forward_jvp(h, C.byref(io), p, p, p, 1 << 40, None) == -21
            msg = lib.lsl_last_error().decode()
            assert "call " + setter + "(m, 0)" in msg, msg
            assert getattr(lib, setter)(h, 0) == 0
            assert lib.lsl_forward_jvp(h, C.byref(io), p, p, p, 16, None) == -3  # (now the next check in line: the workspace)
        finally:
            lib.lsl_model_destroy(h)


# ---- the oracles of the GPU tests ----
@pytest.mark.parametrize("kw,B,T,L", [
    (dict(depth=2, in_dim=8, hidden_size=64, num_heads=4), 2, 5, 6),
    (dict(depth=2, in_dim=8, hidden_size=128, num_heads=4, normalize=True, vec_in_dim=16), 2, 7, 9),
], ids=["d64", "d128_norm_y"])
def test_jvp_oracles_run_and_the_rounding_model_is_in_its_band(kw, B, T, L):
    """Oracle (a) is the derivative (a central difference of the fp64 network agrees), and oracle (b)'s errors against it have the size of
    bf16 operand rounding (2^-9 per operand, a few products deep: 1e-5 .. 1e-3), the tangent's of the order of the primal's."""
    sh = latent_net.NetShape(**kw)
    p = latent_net.random_params(sh, seed=3)
    g = torch.Generator().manual_seed(1)
    x, xc = torch.randn(B, T, L, sh.in_dim, generator=g), torch.randn(B, T, L, sh.in_dim, generator=g)
    mask = (torch.rand(B, T, L, generator=g) > 0.5).long()
    t = torch.rand(B, generator=g)
    y = torch.randn(B, sh.vec_in_dim, generator=g) if sh.vec_in_dim else None
    v = jvp_oracle.rademacher(x.shape, 7)
    out, out_t, e_p, e_t = jvp_oracle.model_errors(p, sh, x, t, xc, mask, y, v)
    p64 = latent_net.cast_params(p, torch.float64)
    f = lambda xx: latent_net.forward(p64, sh, xx, t.double(), xc.double(), mask, None if y is None else y.double())  # noqa: E731
    assert jvp_oracle.rel(out, f(x.double())) == 0.0
    h = 1e-3  # (the oracle rotates and normalises in fp32: its 1e-7 noise over 2 h, against a truncation error of h^2)
    fd = (f(x.double() + h * v.double()) - f(x.double() - h * v.double())) / (2 * h)
    assert jvp_oracle.rel(fd, out_t) < 2e-3
    print(f"JVP-MODEL {kw} e_p {e_p:.3e} e_t {e_t:.3e} ratio {e_t / e_p:.2f}")
    assert 1e-5 < e_p < 1e-3 and 1e-5 < e_t < 1e-3 and 0.3 < e_t / e_p < 3.0
    _, z = jvp_oracle.jvp_fp64(p, sh, x, t, xc, mask, y, torch.zeros_like(v))
    assert torch.count_nonzero(z) == 0
