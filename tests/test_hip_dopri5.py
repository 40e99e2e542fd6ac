"""GPU tests of the adaptive dopri5 sampler with the step controller on the device (``sample_ode(controller="device")``:
lsl_dopri_begin / lsl_dopri_advance, csrc/k_dopri5.hip.h).

  * replay: every logged attempt performed again with the host path's arithmetic (``_RkOps`` + ``LatentSIV3.forward``) at the logged
    (t, dt) gives the logged error ratio, the outputs and the final state bit for bit; the controller's decisions follow its formula
  * the shipped transport (GVP / data) against ``controller="host"`` in the solver's own norm
  * the exact solution around a network that returns a constant; the drift coefficients of all 12 path x prediction pairs
  * over-enqueued attempts, chunked passes, grid edges, hipGraph replay against eager, the attempt limit and a NaN
Shapes: the f4 fixture's model at its shape (1536 state elements: six workgroups of the error norm) and a seeded model of hidden 64 /
depth 1 on T = 5, L = 7, C = 3 with B = 1 (105 elements: one workgroup) and B = 3 (315: two, and tails of every element-wise kernel).
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import shape_from
from test_dopri5_controller import exact_solution, solver_norm
from test_hip_parity import build_net

pytestmark = pytest.mark.gpu

# Distance of the device solve from the host-controller solve on the same network, in the solver's norm, per output slice: the value measured
# on MI355X.  The bound of the tests is ten times this, and never above 0.05.
HOST_DISTANCE_MEASURED = 0.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def f4(golden, dev):
    f = golden("f4_sampler.npz")
    sh = shape_from(f.group("shape"))
    net = build_net(sh, f.group("p"), dev)
    return net, f["init"].to(dev), {"x_cond": f["x_cond"].to(dev), "x_cond_mask": f["mask"].to(dev)}


def small_case(dev, B, seed=21, T=5, L=7, C=3):
    from oracle import latent_net
    sh = latent_net.NetShape(depth=1, in_dim=C, hidden_size=64, num_heads=4, mlp_ratio=2)
    net = build_net(sh, latent_net.random_params(sh, seed=seed), dev)
    g = torch.Generator().manual_seed(seed + B)
    init = torch.randn(B, T, L, C, generator=g).to(dev)
    kw = {"x_cond": torch.randn(B, T, L, C, generator=g).to(dev), "x_cond_mask": (torch.rand(B, T, L, generator=g) < 0.3).long().to(dev)}
    return net, init, kw


@pytest.fixture(scope="module")
def small(dev):
    cache = {}

    def get(B):
        if B not in cache:
            cache[B] = small_case(dev, B)
        return cache[B]

    return get


def _sampler(path="GVP", pred="data", **attrs):
    from lam_slide_amd import CreateTransport, Sampler
    s = Sampler(CreateTransport(path, pred)())
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


def host_drift(s, net, kw, reverse=False):
    """f(t, x) of the host path (Sampler._sample_ode_dopri5)"""
    from lam_slide_amd.transport import _f32
    return lambda t, x: s._vel(x, torch.ones(x.size(0), device=x.device) * (_f32(1 - t) if reverse else t), net, **kw)[0]


def controller_dt(dt, ratio):
    return dt * 10.0 if ratio == 0.0 else dt * min(10.0, max(0.9 / ratio ** 0.2, 1.0 if ratio < 1.0 else 0.2))


def replay(s, net, init, kw, grid, rtol, atol, log):
    """Every attempt of ``log`` again with _RkOps and LatentSIV3.forward; asserts the logged ratios and decisions; returns (outputs, state)"""
    from lam_slide_amd.transport import _DP_ALPHA, _DP_BETA, _DP_C_ERR, _DP_C_MID, _RkOps
    ops = _RkOps(init)
    f = host_drift(s, net, kw)
    y = init.contiguous()
    fy = f(grid[0], y)
    outs = [y for g in grid if g <= grid[0]]
    for a, (t, dt, ratio, accepted) in enumerate(log.tolist()):
        k = [fy]
        for al, beta in zip(_DP_ALPHA, _DP_BETA):
            yi = ops.lincomb([(1.0, y)] + [(dt * b, kj) for b, kj in zip(beta, k) if b != 0.0])
            k.append(f(t + al * dt, yi))
        got = ops.error_ratio(y, yi, [(dt * c, kj) for c, kj in zip(_DP_C_ERR, k) if c != 0.0], atol, rtol)
        assert got == ratio, (a, got, ratio)  # (both are float32 values held in float64: the same bits)
        assert accepted == float(ratio <= 1.0), (a, ratio, accepted)
        if a + 1 < len(log):
            t_next, dt_next = log[a + 1, 0].item(), log[a + 1, 1].item()
            assert t_next == (t + dt if accepted else t), (a, t, dt, t_next)
            want = controller_dt(dt, ratio)
            assert abs(dt_next - want) <= 4 * math.ulp(want), (a, dt_next, want)
        if not accepted:
            continue
        y_mid = ops.lincomb([(1.0, y)] + [(dt * c, kj) for c, kj in zip(_DP_C_MID, k) if c != 0.0])
        fa, fb, y1 = k[0], k[-1], yi
        d = ops.lincomb([(dt, fa)])
        c = ops.lincomb([(dt, fb), (-4 * dt, fa), (-11.0, y), (-5.0, y1), (16.0, y_mid)])
        b = ops.lincomb([(5 * dt, fa), (-3 * dt, fb), (18.0, y), (14.0, y1), (-32.0, y_mid)])
        aa = ops.lincomb([(2 * dt, fb), (-2 * dt, fa), (-8.0, y1), (-8.0, y), (16.0, y_mid)])
        while len(outs) < len(grid) and grid[len(outs)] <= t + dt:
            outs.append(ops.poly4(aa, b, c, d, y, (grid[len(outs)] - t) / ((t + dt) - t)))
        y, fy = y1, fb
    return outs, y


@pytest.mark.parametrize("case", ["f4", "small-B1", "small-B3"])
def test_logged_attempts_replay_bit_for_bit(case, f4, small, dev):
    """Linear path, velocity prediction: (vx, vm) = (0, 1) exactly, so the host arithmetic at the logged (t, dt) is the device's."""
    net, init, kw = f4 if case == "f4" else small(int(case[-1]))
    s = _sampler("Linear", "velocity")
    res = s.get_sample_fn("ODE", dict(num_steps=6, controller="device"))(init, net, **kw)
    assert s.last_path == "dopri5-device" and net.last_path == "hip" and res.shape == (6,) + init.shape
    log, stats = s.last_ode_log, s.last_ode_stats
    assert len(log) == stats["accepted"] + stats["rejected"] and stats["nfe"] == 2 + 6 * len(log) and stats["accepted"] >= 2
    assert int(log[:, 3].sum()) == stats["accepted"]
    grid = [float(g) for g in torch.linspace(0, 1, 6)]
    outs, y = replay(s, net, init, kw, grid, 1e-3, 1e-6, log)
    assert len(outs) == 6
    for j, o in enumerate(outs):
        assert torch.equal(res[j], o), j
    assert torch.equal(s.last_ode_state, y)
    assert torch.equal(res[0], init)


def host_and_device(net, init, kw, options, monkeypatch=None, **attrs):
    """The same ODE call with both controllers: (host result, device result, host sampler, device sampler, host error ratios)"""
    from lam_slide_amd.transport import _RkOps
    ratios = []
    if monkeypatch is not None:
        orig = _RkOps.error_ratio
        monkeypatch.setattr(_RkOps, "error_ratio", lambda self, *a: ratios.append(orig(self, *a)) or ratios[-1])
    sh = _sampler(**attrs)
    want = sh.get_sample_fn("ODE", dict(options, controller="host"))(init, net, **kw)
    if monkeypatch is not None:
        monkeypatch.undo()
    sd = _sampler(**attrs)
    got = sd.get_sample_fn("ODE", dict(options, controller="device"))(init, net, **kw)
    assert sh.last_path == "dopri5" and sd.last_path == "dopri5-device"
    return want, got, sh, sd, ratios[3:]  # (the first three are d0, d1, d2 of the initial step)


def assert_close_to_host(name, want, got, rtol, atol):
    assert got.shape == want.shape
    bound = min(10 * HOST_DISTANCE_MEASURED, 0.05)
    errs = [solver_norm(got[j], want[j], rtol, atol) for j in range(len(want))]
    print(f"PARITY {name} measured {max(errs):.3e} bar {bound:.1e} (per slice: {' '.join(f'{e:.2e}' for e in errs)})")
    assert max(errs) <= bound, (name, errs, bound)


@pytest.mark.parametrize("tag,tol", [("default", {}), ("tight", {"rtol": 1e-4, "atol": 1e-7})])
@pytest.mark.parametrize("case", ["f4", "small-B3"])
def test_shipped_transport_against_the_host_controller(case, tag, tol, f4, small, dev, monkeypatch):
    net, init, kw = f4 if case == "f4" else small(3)
    if case == "f4":  # (the fixture's own initial state has a host ratio of 1.0004 at the tight tolerances; seed 0 keeps every ratio 8e-3 away from 1)
        init = torch.randn(init.shape, generator=torch.Generator().manual_seed(0)).to(dev)
    want, got, sh, sd, ratios = host_and_device(net, init, kw, dict(tol, num_steps=8), monkeypatch)
    assert len(ratios) == sh.last_ode_stats["accepted"] + sh.last_ode_stats["rejected"]
    assert not [r for r in ratios if 0.999 <= r <= 1.001], ratios  # precondition: no decision of the host solve is a coin toss
    print(f"dopri5.{case}.{tag}: {len(ratios)} attempts, host ratio nearest to 1 at distance {min(abs(r - 1) for r in ratios):.2e}")
    assert sd.last_ode_stats == sh.last_ode_stats
    assert_close_to_host(f"dopri5.{case}.{tag}", want, got, tol.get("rtol", 1e-3), tol.get("atol", 1e-6))
    assert torch.equal(got[0], init)


@pytest.mark.parametrize("reverse", [False, True])
def test_exact_solution_with_a_constant_network(reverse, dev):
    """Head zeroed (out_w = 0, out_b = c): the network returns c, and GVP / data has the closed solution of
    test_dopri5_controller.exact_solution.  The ODE is contracting, so the accepted steps' local errors (each at most 1 in the solver's
    norm) add up at worst: the error of every output slice is at most the number of accepted steps.
    That argument needs the scale atol + rtol |x| of an element at an output time to be the scale the controller saw at the ends of the step
    around it.  An element that passes through zero inside a step has an arbitrarily small scale there (the host solver on the CPU shows a
    single element at 200 times its scale with the state at 7e-4 relative error), so the case keeps the state away from zero: c > 0 and
    x(t0) >= 1 give x(t) >= 0.4 on the whole interval in both directions (alpha c + sigma / sigma0 (x0 - alpha0 c), and the reverse form)."""
    net, init, kw = small_case(dev, 3, seed=5)
    init = 1 + 0.5 * init.abs()
    with torch.no_grad():
        net.linear.weight.zero_()
        net.linear.bias.copy_(torch.tensor([0.7, 1.3, 0.4]))
    c = net.linear.bias.detach().double().cpu().reshape(1, 1, 1, 3)
    s = _sampler()
    grid = [0.05, 0.2, 0.5, 0.775, 0.95]
    rtol, atol = 1e-3, 1e-6
    res = s.run_dopri_device(net, init, grid, rtol, atol, reverse, kw)
    acc = s.last_ode_stats["accepted"]
    assert acc >= 3 and res.shape == (5,) + init.shape
    for j, t in enumerate(grid):
        want = exact_solution(c, init.double().cpu(), grid[0], t, reverse)
        assert float(want.abs().min()) >= 0.4
        err = solver_norm(res[j].cpu(), want, rtol, atol)
        print(f"PARITY dopri5.exact.reverse{int(reverse)}.slice{j} measured {err:.3e} bar {acc}")
        assert err <= acc, (j, err, acc)


def test_device_drift_coefficients_of_every_path_and_prediction(dev):
    """(vx, vm) as the kernels evaluate them (lsl_debug_dopri_coeffs) against Transport.velocity_coeffs at the same fp32 times, rounded to
    fp32 as both paths hand them to the state arithmetic: within 2 fp32 ulp (device sin / cos / tan / exp against libm, amplified by the
    cancellation in -k + var sx)."""
    import numpy as np
    from lam_slide_amd import CreateTransport, _lib
    t = torch.linspace(1e-3, 0.999, 97, dtype=torch.float32)
    td = t.to(dev)
    for path in ("Linear", "GVP", "VP"):
        for pred in ("velocity", "data", "noise", "score"):
            tr = CreateTransport(path, pred)()
            out = torch.empty(len(t), 2, dtype=torch.float64, device=dev)
            _lib.call(dev, "lsl_debug_dopri_coeffs", _lib.Dopri.PATHS[tr.path_type.name], _lib.Dopri.PREDICTIONS[tr.model_type.name], td.data_ptr(), len(t),
                      out.data_ptr())
            got = out.cpu().numpy().astype(np.float32)
            want = np.array([tr.velocity_coeffs(float(v)) for v in t], dtype=np.float64).astype(np.float32)
            ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
            print(f"PARITY dopri5.coeffs.{path}.{pred} measured {ulps.max():.1f} bar 2 (fp32 ulp)")
            assert ulps.max() <= 2, (path, pred, ulps.max())


def test_over_enqueued_attempts_and_chunked_passes_change_nothing(small, dev):
    net, init, kw = small(3)
    runs = []
    for poll, chunk in ((1, 0), (7, 0), (7, 0), (3, 2)):  # (the third call replays the graph the second one captured; 2 + 1 trajectories per pass)
        net.set_chunk(chunk)
        s = _sampler(attempts_per_poll=poll)
        res = s.get_sample_fn("ODE", dict(num_steps=5, controller="device"))(init, net, **kw)
        runs.append((res.clone(), s.last_ode_log, s.last_ode_stats, s.last_ode_state))
    net.set_chunk(0)
    for res, log, stats, state in runs[1:]:
        assert torch.equal(res, runs[0][0]) and torch.equal(log, runs[0][1]) and stats == runs[0][2] and torch.equal(state, runs[0][3])
    assert runs[0][2]["accepted"] >= 2


def test_grid_edges_follow_the_host_path(small, dev):
    """Several outputs inside one step (num_steps = 50), repeated output times, a single-point grid, an output time that is a step's end."""
    from lam_slide_amd.transport import dopri5_solve
    net, init, kw = small(1)
    want, got, sh, sd, _ = host_and_device(net, init, kw, dict(num_steps=50))
    assert sd.last_ode_stats == sh.last_ode_stats and sd.last_ode_stats["accepted"] < 49
    assert_close_to_host("dopri5.grid50", want, got, 1e-3, 1e-6)
    assert torch.equal(got[0], init)
    s = _sampler()
    first = sd.last_ode_log[0]
    assert first[3] == 1.0  # (the first attempt was accepted: its end is an output time of the third grid)
    t0, end = float(first[0]), float(first[0] + first[1])  # (the first step depends on the initial time and state alone)
    for name, grid in (("repeated", [1e-3, 1e-3, 0.4, 0.4, 0.4, 0.999, 0.999]), ("single", [0.25]), ("step-end", [t0, end, 0.999])):
        res = s.run_dopri_device(net, init, grid, 1e-3, 1e-6, False, kw)
        ys, stats = dopri5_solve(host_drift(s, net, kw), init, grid, 1e-3, 1e-6)
        assert s.last_ode_stats == stats, name
        assert_close_to_host(f"dopri5.grid.{name}", torch.stack(ys), res, 1e-3, 1e-6)
        assert torch.equal(res[0], init)
        if name == "step-end":
            assert float(s.last_ode_log[0, 0] + s.last_ode_log[0, 1]) == end and s.last_ode_log[0, 3] == 1.0
        if name == "single":
            assert stats == {"nfe": 2, "accepted": 0, "rejected": 0} and res.shape == (1,) + init.shape


def test_graph_replay_matches_eager_bits(dev):
    """The same calls with LSL_GRAPH=0 and with the default (attempts captured on their second appearance and replayed): equal bits.  The
    switch is read once per process, so both arms run in subprocesses."""
    code = (
        "import torch, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_hip_dopri5 import small_case, _sampler\n"
        "dev = torch.device('cuda:0')\n"
        "net, init, kw = small_case(dev, 3)\n"
        "outs = []\n"
        "for i in range(2):\n"
        "    s = _sampler(attempts_per_poll=3)\n"
        "    outs.append(s.get_sample_fn('ODE', dict(num_steps=5, controller='device'))(init + i, net, **kw).cpu())\n"
        "    assert s.last_ode_stats['accepted'] + s.last_ode_stats['rejected'] >= 3\n"
        "torch.save((torch.stack(outs), s.last_ode_log), sys.argv[1])\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for mode in ("0", None):
        path = f"/tmp/lsl_dopri_graph_{mode}_{os.getpid()}.pt"
        env = {k: v for k, v in os.environ.items() if k != "LSL_GRAPH"}
        if mode is not None:
            env["LSL_GRAPH"] = mode
        subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=300)
        res[mode] = torch.load(path)
        os.remove(path)
    assert torch.equal(res["0"][0], res[None][0]) and torch.equal(res["0"][1], res[None][1])
    assert not torch.equal(res["0"][0][0], res["0"][0][1])


def test_attempt_limit_and_non_finite_state_raise(small, dev):
    net, init, kw = small(1)
    s = _sampler(ode_max_steps=2)
    with pytest.raises(RuntimeError, match="max_steps reached"):
        s.get_sample_fn("ODE", dict(num_steps=4, controller="device"))(init, net, **kw)
    assert s.last_ode_stats["accepted"] + s.last_ode_stats["rejected"] == 2 and len(s.last_ode_log) == 2
    bad = init.clone()
    bad[0, 1, 2, 0] = float("nan")
    s = _sampler()
    with pytest.raises(RuntimeError, match="not finite"):
        s.get_sample_fn("ODE", dict(num_steps=4, controller="device"))(bad, net, **kw)
    with pytest.raises(RuntimeError, match="not a lam_slide_amd.LatentSIV3 on a GPU"):
        s.get_sample_fn("ODE", dict(num_steps=4, controller="device"))(init, lambda x, t, **k: x, **kw)
