"""What every library path that takes the network's conditioning as ``model_kwargs`` says to a wrong set of them (lam_slide_amd/transport.py:
``check_model_kwargs``): the fused sampler, the device-side adaptive solver in both step controls, ``Transport.si_loss`` and
``sample_ode_likelihood``.  Every case is refused before a kernel of the library runs; the expected texts are written out here, not taken from
the package."""
import pytest
import torch

from test_hip_parity import build_net

pytestmark = pytest.mark.gpu

B, T, L = 1, 2, 2


@pytest.fixture(scope="module")
def setup():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from oracle import latent_net
    dev = torch.device("cuda:0")
    sh = latent_net.NetShape(depth=1, in_dim=8, hidden_size=64, num_heads=4, mlp_ratio=2)
    net = build_net(sh, latent_net.random_params(sh, seed=1), dev)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, L, sh.in_dim, generator=g).to(dev)
    kw = {"x_cond": torch.randn(B, T, L, sh.in_dim, generator=g).to(dev), "x_cond_mask": torch.ones(B, T, L, dtype=torch.long, device=dev)}
    return net, x, kw


def _fused(net, x, kw):
    from lam_slide_amd import CreateTransport, Sampler
    s = Sampler(CreateTransport("Linear", "velocity")())
    try:
        return s.sample_ode(sampling_method="euler", num_steps=3)(x, net, **kw)
    finally:
        assert s.last_path is None  # (nothing ran)


def _device(step_control):
    def run(net, x, kw):
        from lam_slide_amd import CreateTransport, Sampler
        s = Sampler(CreateTransport("Linear", "velocity")())
        try:
            return s.sample_ode(sampling_method="dopri5", num_steps=3, controller="device", step_control=step_control)(x, net, **kw)
        finally:
            assert s.last_path is None and s.last_ode_stats is None
    return run


def _si_loss(net, x, kw):
    from lam_slide_amd import CreateTransport
    tr = CreateTransport("Linear", "velocity")()
    with torch.no_grad():
        return tr.si_loss(net, x, torch.full((B,), 0.5, device=x.device), torch.ones_like(x), kw)


def _likelihood(net, x, kw):
    from lam_slide_amd import CreateTransport, Sampler
    s = Sampler(CreateTransport("Linear", "velocity")())
    return s.sample_ode_likelihood(sampling_method="euler", num_steps=2, eps=torch.ones_like(x))(x, net, **kw)


# the samplers compare the conditioning with the state themselves; the loss and the likelihood leave it to the call's argument block
SAMPLERS_SAY = "Expected all tensors to be on the same device, but x_cond is on cpu and the state is on cuda:0"
ARGUMENT_BLOCK_SAYS = "Expected all tensors to be on the same device, but x_cond is on cpu and x is on cuda:0"
PATHS = {"fused": (_fused, SAMPLERS_SAY), "device-batch": (_device("batch"), SAMPLERS_SAY), "device-trajectory": (_device("trajectory"), SAMPLERS_SAY),
         "si_loss": (_si_loss, ARGUMENT_BLOCK_SAYS), "likelihood": (_likelihood, ARGUMENT_BLOCK_SAYS)}


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("case", ["extra", "missing", "elsewhere"])
def test_wrong_model_kwargs_are_refused_with_the_same_words(path, case, setup):
    net, x, kw = setup
    run, elsewhere = PATHS[path]
    if case == "extra":
        bad, exc, text = dict(kw, zeta=None, alpha=1), TypeError, "unexpected model kwargs ['alpha', 'zeta']"
    elif case == "missing":
        bad, exc, text = {"x_cond_mask": kw["x_cond_mask"]}, TypeError, "missing model kwarg 'x_cond'"
    else:
        bad, exc, text = dict(kw, x_cond=kw["x_cond"].cpu()), RuntimeError, elsewhere
    with pytest.raises(exc) as err:
        run(net, x, bad)
    assert str(err.value) == text
