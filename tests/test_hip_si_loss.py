"""GPU tests of the stochastic-interpolant objective on the device (``lsl_si_loss`` / ``lsl_si_reduce`` behind
``Transport.training_losses``): the fused call against the reference-generated fixtures F15 / F16 and the CPU oracle, the fused call IS
the forward, batch independence, and the reference's ``Loss.forward`` call pattern taking the fused path.

Bars.  ``pred`` is one network evaluation: the bars the same model classes already have (f1.forward / f9.sampled 5e-4, the md17_bench /
ln_fuse / tail forwards 6e-4).  The loss is not given a bar of its own that the network's bf16 error could hide a reduction bug under:
with r = p pred + q1 x1 + q0 x0 and loss = w mean(r^2), the triangle inequality on ||r|| gives
    |sqrt(loss_b) - sqrt(loss_ref_b)| <= (eps_b kappa_b + 1e-5) sqrt(loss_ref_b),   kappa_b = p_b ||pred_ref_b|| / ||r_ref_b||,
where eps_b is the MEASURED relative error of that trajectory's ``pred`` and 1e-5 is the bar of the reduction alone (fixture times in
[0.05, 0.9]: one fp32 ulp through the worst-conditioned coefficient is 6e-7; the device adds a summation order over <= 2^20 terms).
Measured values: profiles/si_loss_parity.txt."""
import enum

import pytest
import torch

from conftest import parity, rel_l2

pytestmark = pytest.mark.gpu

PATHS, PREDS, WEIGHTS = ("Linear", "GVP", "VP"), ("velocity", "data", "noise", "score"), (None, "velocity", "likelihood")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def build_net(sh, params, dev, tail=None, ln_fuse=None):
    from lam_slide_amd import LatentSIV3
    net = LatentSIV3(depth=sh.depth, in_dim=sh.in_dim, hidden_size=sh.hidden_size, num_heads=sh.num_heads, vec_in_dim=sh.vec_in_dim,
                     mlp_ratio=sh.mlp_ratio, theta=sh.theta, normalize=sh.normalize, reset_parameters=False)
    net.load_state_dict(params)
    net = net.to(dev).requires_grad_(False)
    if tail is not None:
        net.set_tail(tail)
    if ln_fuse is not None:
        net.set_ln_fuse(ln_fuse)
    net.ensure_packed(dev)
    return net


def rel_rows(a, b):
    return float(((a.double() - b.double()).abs() / b.double().abs()).max())


def check_loss(name, got_pred, got_loss, ref_pred, ref_loss, rows, x1, x0, pred_bar):
    """The bars of the module docstring: ``pred`` under ``pred_bar``, every trajectory's loss inside the triangle inequality."""
    got_pred, got_loss = got_pred.cpu(), got_loss.cpu()
    assert torch.isfinite(got_pred).all() and torch.isfinite(got_loss).all()
    parity(f"{name}.pred", rel_l2(got_pred, ref_pred), pred_bar)
    for b in range(x1.shape[0]):
        p, q1, q0 = (float(rows[b, i]) for i in (2, 3, 4))
        r_ref = p * ref_pred[b].double() + q1 * x1[b].double() + q0 * x0[b].double()
        kappa = abs(p) * float(ref_pred[b].double().norm()) / float(r_ref.norm())
        eps = rel_l2(got_pred[b], ref_pred[b])
        dev_ = abs(float(got_loss[b]) ** 0.5 - float(ref_loss[b]) ** 0.5) / float(ref_loss[b]) ** 0.5
        parity(f"{name}.sqrt_loss[{b}] (eps {eps:.2e} kappa {kappa:.2f})", dev_, eps * kappa + 1e-5)


def test_f16_fused_against_the_reference_model_step(golden, dev):
    """F16 = the reference's real md17 ``Wrapper.model_step``; here the same weights, draws and latents through ONE ``lsl_si_loss``."""
    from lam_slide_amd import CreateTransport
    from oracle import latent_net
    f, f9 = golden("f16_model_step.npz"), golden("f9_sample.npz")
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=64, mlp_ratio=2, num_heads=4)
    net = build_net(sh, f9.group("backbone"), dev)
    tr = CreateTransport("GVP", "data")()
    kw = {"x_cond": f["x_cond"].to(dev), "x_cond_mask": f["mask"].to(dev)}
    with torch.no_grad():
        out = tr.training_losses(model=net.forward, x1=f["latents"].to(dev), model_kwargs=kw, t=f["t"].to(dev), x0=f["x0"].to(dev))
    assert tr.last_path == "fused" and net.last_path == "hip" and set(out) == {"pred", "loss"} and out["loss"].shape == (2,)
    check_loss("f16.fused", out["pred"], out["loss"], f["pred"], f["loss"], tr.si_rows(f["t"]), f["latents"], f["x0"], 5e-4)
    si = float(f.group("losses")["si_loss"])
    print(f"f16.fused si_loss {float(out['loss'].mean()):.6f} reference {si:.6f}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("pred", PREDS)
def test_reduction_alone_matches_reference(golden, dev, path, pred):
    """``lsl_si_reduce`` on the fixture's own ``pred``: what is left is the affine table and the device's summation order."""
    from lam_slide_amd import CreateTransport, si_reduce
    f = golden("f15_si_loss.npz")
    for weight in WEIGHTS:
        want = f.group(f"{path}_{pred}_{weight}")
        rows = CreateTransport(path, pred, weight)().si_rows(f["t"])
        got = si_reduce(want["pred"].to(dev).contiguous(), f["x1"].to(dev), f["x0"].to(dev), rows).cpu()
        parity(f"f15.reduce.{path}.{pred}.{weight}", rel_rows(got, want["loss"]), 1e-5)


@pytest.mark.parametrize("per", [3 * 4096 + 5, 7, 2 * 4096, 4096 + 4])
def test_reduction_slab_edges_and_scalar_tail(dev, per):
    from lam_slide_amd import CreateTransport, si_reduce
    g = torch.Generator().manual_seed(per)
    B = 3
    pred, x1, x0 = (torch.randn(B, per, generator=g) for _ in range(3))
    t = torch.tensor([0.2, 0.55, 0.8])
    for kind, weight in (("velocity", None), ("score", "likelihood")):
        rows = CreateTransport("GVP", kind, weight)().si_rows(t)
        r = rows[:, 2:3].double() * pred.double() + rows[:, 3:4].double() * x1.double() + rows[:, 4:5].double() * x0.double()
        want = rows[:, 5].double() * (r ** 2).mean(dim=1)
        got = si_reduce(pred.to(dev), x1.to(dev), x0.to(dev), rows).cpu()
        parity(f"reduce.per{per}.{kind}", rel_rows(got, want), 1e-5)
        # a trajectory's bits do not depend on its batch, nor on the 16-byte / scalar access form (a slice at an odd element offset)
        for b in range(B):
            alone = si_reduce(pred[b:b + 1].to(dev), x1[b:b + 1].to(dev), x0[b:b + 1].to(dev), rows[b:b + 1]).cpu()
            assert torch.equal(alone, got[b:b + 1]), (per, kind, b)
        if per % 4 == 0:
            pad = lambda v: torch.cat([torch.zeros(1), v.reshape(-1)]).to(dev)[1:].reshape(B, per)  # noqa: E731  (4-byte aligned only)
            shifted = si_reduce(pad(pred), pad(x1), pad(x0), rows).cpu()
            assert torch.equal(shifted, got), (per, kind)


def test_fused_call_is_the_forward(dev):
    """``pred`` of ``lsl_si_loss`` is bit-equal to ``net.forward`` on the ``xt`` the call wrote, ``xt`` is alpha x1 + sigma x0 (one
    product and the fused sum rounded once each: within one ulp at the operands' magnitude), and the loss is the reduction of exactly that ``pred``."""
    from lam_slide_amd import CreateTransport, si_reduce
    from oracle import latent_net
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2, vec_in_dim=16)
    net = build_net(sh, latent_net.random_params(sh, seed=5), dev)
    g = torch.Generator().manual_seed(6)
    B, T, L = 3, 6, 40
    x1, x0, xc = (torch.randn(B, T, L, 32, generator=g).to(dev) for _ in range(3))
    mask = (torch.rand(B, T, L, generator=g) < 0.3).long().to(dev)
    y = torch.randn(B, 16, generator=g).to(dev)
    t = torch.tensor([0.13, 0.5, 0.97]).to(dev)
    kw = {"x_cond": xc, "x_cond_mask": mask, "y": y}
    for path, kind in (("GVP", "data"), ("VP", "noise"), ("Linear", "velocity")):
        tr = CreateTransport(path, kind, "likelihood")()
        with torch.no_grad():
            out = tr.si_loss(net, x1, t, x0, kw)
            again = net(out["xt"], t, xc, mask, y)
        assert tr.last_path == "fused"
        assert torch.equal(out["pred"], again), (path, kind)
        rows = tr.si_rows(t)
        a, s = (rows[:, i].double().reshape(B, 1, 1, 1) for i in (0, 1))
        pa, ps = a * x1.cpu().double(), s * x0.cpu().double()
        err = (out["xt"].cpu().double() - (pa + ps)).abs()
        assert bool((err <= 2.0 ** -23 * (pa.abs() + ps.abs())).all()), (path, kind, float(err.max()))
        assert torch.equal(out["loss"], si_reduce(out["pred"], x1, x0, rows)), (path, kind)


def test_batch_independence_and_chunking_bit_exact(dev):
    """The library's standing rule - a trajectory's bits do not depend on its batch - for the objective, at the shape of
    test_hip_parity.test_batch_independence_and_chunking_bit_exact with five different times."""
    from lam_slide_amd import CreateTransport, SecondStageSampler, si_reduce
    from oracle import latent_net
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2)
    net = build_net(sh, latent_net.random_params(sh, seed=3), dev)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(5, 12, 24, 32, generator=g).to(dev)
    x0 = torch.randn(5, 12, 24, 32, generator=g).to(dev)
    t = torch.tensor([0.07, 0.31, 0.5, 0.77, 0.93]).to(dev)
    tr = CreateTransport("GVP", "data")()
    rows = tr.si_rows(t)
    # the reduction
    anything = torch.randn(5, 12, 24, 32, generator=g).to(dev)
    five = si_reduce(anything, lat, x0, rows)
    for b in range(5):
        assert torch.equal(si_reduce(anything[b:b + 1].contiguous(), lat[b:b + 1].contiguous(), x0[b:b + 1].contiguous(), rows[b:b + 1]), five[b:b + 1]), b
    # the whole call
    drv = SecondStageSampler(net, tr, cond_idx=(0, 4))
    full = drv.model_step(lat, t=t, x0=x0)
    assert tr.last_path == "fused" and torch.isfinite(full["loss"]).all() and torch.isfinite(full["pred"]).all()
    net.set_chunk(2)
    chunked = drv.model_step(lat, t=t, x0=x0)
    net.set_chunk(0)
    assert torch.equal(full["pred"], chunked["pred"]) and torch.equal(full["loss"], chunked["loss"]), "passes of 2 + 2 + 1 trajectories"
    for b in range(5):
        one = drv.model_step(lat[b:b + 1], t=t[b:b + 1], x0=x0[b:b + 1])
        assert torch.equal(one["pred"], full["pred"][b:b + 1]), f"trajectory {b}: pred alone vs in the batch of 5"
        assert torch.equal(one["loss"], full["loss"][b:b + 1]), f"trajectory {b}: loss alone vs in the batch of 5"
    # a shard draws what the unsharded call draws for its rows
    drv.reseed(11)
    whole = drv.model_step(lat)
    t_all, x0_all = drv.last_draws
    t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps)
    assert t_all.shape == (5,) and t0 <= float(t_all.min()) and float(t_all.max()) <= t1 and len(set(t_all.tolist())) == 5
    drv.reseed(11)
    shard = drv.model_step(lat[2:5], first_index=2)
    t_sh, x0_sh = drv.last_draws
    assert torch.equal(t_sh, t_all[2:5]) and torch.equal(x0_sh, x0_all[2:5])
    assert torch.equal(shard["loss"], whole["loss"][2:5]) and torch.equal(shard["pred"], whole["pred"][2:5])
    drv.reseed(11)
    drv.model_step(lat)
    other = drv.model_step(lat)  # the next call of the object draws from another stream
    assert not torch.equal(drv.last_draws[0], t_all) and not torch.equal(other["loss"], whole["loss"])


BENCH_CASES = {
    # NetShape kwargs, B, T, L, handle options
    "md17_bench.default": (dict(depth=4, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2), 2, 30, 256, {}),
    "md17_bench.ln_fuse": (dict(depth=4, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2), 2, 30, 256, {"ln_fuse": True}),
    "nba_y.tail": (dict(depth=2, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=4, vec_in_dim=24, normalize=True), 7, 20, 8, {"tail": True}),
}


@pytest.mark.parametrize("name", sorted(BENCH_CASES))
def test_benchmark_shapes_against_oracle(name, dev):
    from lam_slide_amd import CreateTransport
    from oracle import latent_net
    kw, B, T, L, opts = BENCH_CASES[name]
    sh = latent_net.NetShape(**kw)
    p = latent_net.random_params(sh, seed=23)
    net = build_net(sh, p, dev, **opts)
    assert net.ln_fuse == bool(opts.get("ln_fuse")) and net.tail == bool(opts.get("tail"))
    g = torch.Generator().manual_seed(3)
    x1, x0, xc = (torch.randn(B, T, L, sh.in_dim, generator=g) for _ in range(3))
    mask = (torch.rand(B, T, L, generator=g) < 0.3).long()
    t = torch.rand(B, generator=g) * 0.85 + 0.05
    y = torch.randn(B, sh.vec_in_dim, generator=g) if sh.vec_in_dim else None
    tr = CreateTransport("GVP", "data")()
    mk = {"x_cond": xc, "x_cond_mask": mask, **({"y": y} if y is not None else {})}
    ref = tr.training_losses(lambda xt, tt, **k: latent_net.forward(p, sh, xt, tt, k["x_cond"], k["x_cond_mask"], k.get("y")), x1, mk, t=t, x0=x0)
    assert tr.last_path == "generic"
    with torch.no_grad():
        out = tr.training_losses(net, x1.to(dev), {k: v.to(dev) for k, v in mk.items()}, t=t.to(dev), x0=x0.to(dev))
    assert tr.last_path == "fused"
    check_loss(f"si.{name}", out["pred"], out["loss"], ref["pred"], ref["loss"], tr.si_rows(t), x1, x0, 6e-4)


def test_reference_loss_forward_takes_the_fused_path(dev):
    """The reference's loop, unchanged: ``Loss.forward`` (second_stage/md17.py:219-234) calls ``model.si.training_losses(model=model,
    x1=..., model_kwargs=...)`` with the LightningModule ITSELF and then compares ``model.si.model_type`` with its own ``ModelType.DATA``.
    A LightningModule-shaped object around this package's backbone and Transport must take the fused path: exactly one ``lsl_si_loss``
    call, no call of the module's ``forward``."""
    import lam_slide_amd
    from lam_slide_amd import CreateTransport, _lib
    from oracle import latent_net
    lam_slide_amd.install()

    class ModelType(enum.Enum):  # the reference's own enum (transport.py:15-21), a different class of the same name
        NOISE = enum.auto()
        SCORE = enum.auto()
        VELOCITY = enum.auto()
        DATA = enum.auto()

    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=128, num_heads=4, mlp_ratio=2)
    calls = {"forward": 0, "si_loss": 0}

    class Module(torch.nn.Module):  # SecondStageCondLightningBase: forward == backbone(x=xt, t=t, **kw) (lightning_base.py:173-174)
        def __init__(self):
            super().__init__()
            self.backbone = build_net(sh, latent_net.random_params(sh, seed=0), dev)
            self.si = CreateTransport("GVP", "data")()

        def forward(self, xt, t, **model_kwargs):
            calls["forward"] += 1
            return self.backbone(x=xt, t=t, **model_kwargs)

    def loss_forward(model, batch):  # transcription of the call pattern of Loss.forward
        out = model.si.training_losses(model=model, x1=batch["x1"], model_kwargs=batch["model_kwargs"])
        pred_latent = out["pred"]
        si_loss = out["loss"].mean()
        assert model.si.model_type == ModelType.DATA, "Additional losses are currently only supported for DATA model"
        return {"si_loss": si_loss, "loss": si_loss * 1.0}, pred_latent

    model = Module()
    g = torch.Generator().manual_seed(9)
    x1, xc = (torch.randn(2, 6, 40, 32, generator=g).to(dev) for _ in range(2))
    batch = {"x1": x1, "model_kwargs": {"x_cond": xc, "x_cond_mask": torch.zeros(2, 6, 40, dtype=torch.long, device=dev)}}
    lib = _lib.load()
    real = lib.lsl_si_loss

    def counting(*a):
        calls["si_loss"] += 1
        return real(*a)

    lib.lsl_si_loss = counting
    try:
        torch.manual_seed(5)
        with torch.no_grad():
            losses, pred = loss_forward(model, batch)
    finally:
        lib.lsl_si_loss = real
    assert calls == {"forward": 0, "si_loss": 1} and model.si.last_path == "fused" and model.backbone.last_path == "hip"
    assert pred.shape == x1.shape and torch.isfinite(pred).all() and float(losses["loss"]) > 0
    # the generic path on the same object is what calls the module's forward (the counter above counts)
    with torch.no_grad():
        gen = model.si.training_losses(lambda xt, tt, **kw: model.forward(xt, tt, **kw), x1, batch["model_kwargs"])
    assert model.si.last_path == "generic" and calls == {"forward": 1, "si_loss": 1} and gen["pred"].shape == x1.shape
    with torch.enable_grad():  # a trainable backbone with grad mode on is refused, not silently evaluated
        model.backbone.requires_grad_(True)
        with pytest.raises(RuntimeError, match="no_grad"):
            loss_forward(model, batch)
