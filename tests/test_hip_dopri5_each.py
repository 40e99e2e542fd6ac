"""GPU tests of adaptive dopri5 sampling with one step controller per trajectory (``sample_ode(controller="device",
step_control="trajectory")``: lsl_dopri_each_begin / lsl_dopri_each_advance, the per-trajectory forms of csrc/k_dopri5.hip.h).

The defining property: trajectory b of such a call equals the ``controller="device"`` call on ``[b:b+1]`` bit for bit - outputs, log,
counters and final state - although the trajectories take different numbers of attempts.  Around it: every trajectory's log replayed with
the host arithmetic, the host form (``dopri5_solve_each``), chunked passes, sub-batches, hipGraph replay, over-enqueued attempts, K samples
folded into a batch, failures that stay with their trajectory, and the precondition in the network: one time per trajectory.
Shapes: the seeded model of tests/test_hip_dopri5.py (105 elements a trajectory: one workgroup of the error norm and the tail of every
element-wise kernel) at B = 1 and B = 3, and the f4 fixture's model at its shape and batch (several workgroups of the error norm a trajectory).
"""
import os
import subprocess
import sys

import pytest
import torch

from conftest import shape_from
from test_dopri5_controller import solver_norm
from test_hip_dopri5 import _sampler, host_drift, replay, small_case
from test_hip_parity import build_net

pytestmark = pytest.mark.gpu

# Distance of the device solve from the host form (controller="host", step_control="trajectory") on the same network, per trajectory and
# output slice in the solver's norm: the value measured on MI355X.  The bound of the test is ten times this, and
# never above 0.05 - the rule of tests/test_hip_dopri5.py.
EACH_HOST_DISTANCE_MEASURED = 0.0

OPTS = dict(num_steps=6, rtol=1e-3, atol=1e-6, controller="device")
EACH = dict(OPTS, step_control="trajectory")
SCALES = (1.0, 8.0, 0.125)


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


@pytest.fixture(scope="module")
def small(dev):
    cache = {}

    def get(B):
        if B not in cache:
            cache[B] = small_case(dev, B)
        return cache[B]

    return get


def rows(kw, idx):
    """The conditioning of the trajectories idx (a slice or an index list)"""
    return {k: v[idx].contiguous() for k, v in kw.items()}


def solve(net, init, kw, options, path="GVP", pred="data", **attrs):
    s = _sampler(path, pred, **attrs)
    return s.get_sample_fn("ODE", dict(options))(init, net, **kw), s


def scaled(init, on):
    if not on:
        return init
    scale = torch.tensor([SCALES[b % 3] for b in range(init.shape[0])], device=init.device).reshape(-1, 1, 1, 1)
    return (init * scale).contiguous()


def assert_trajectory_is_the_solo_call(b, res, s, solo, s1):
    assert torch.equal(res[:, b], solo[:, 0]), b
    assert torch.equal(s.last_ode_log[b], s1.last_ode_log), b
    assert {k: s.last_ode_stats[k][b] for k in ("nfe", "accepted", "rejected")} == s1.last_ode_stats, b
    assert torch.equal(s.last_ode_state[b], s1.last_ode_state[0]), b


@pytest.mark.parametrize("scale", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("case", ["small-gvp-data", "small-linear-velocity", "f4"])
def test_every_trajectory_equals_its_solo_call_bit_for_bit(case, scale, f4, small, dev):
    net, init, kw = f4 if case == "f4" else small(3)
    path, pred = ("Linear", "velocity") if "linear" in case else ("GVP", "data")
    init = scaled(init, scale)
    B = init.shape[0]
    res, s = solve(net, init, kw, EACH, path, pred)
    assert s.last_path == "dopri5-device-each" and net.last_path == "hip" and res.shape == (6,) + init.shape
    stats = s.last_ode_stats
    attempts = [a + r for a, r in zip(stats["accepted"], stats["rejected"])]
    print(f"dopri5-each.{case}.{'scaled' if scale else 'plain'}: attempts per trajectory {attempts}")
    assert stats["attempts"] == max(attempts) and stats["network_passes"] == 2 + 6 * max(attempts) and [len(g) for g in s.last_ode_log] == attempts
    assert stats["nfe"] == [2 + 6 * a for a in attempts] and min(stats["accepted"]) >= 2
    if B > 1:
        assert len(set(attempts)) > 1, attempts  # (trajectories in step with each other would prove nothing)
    for b in range(B):
        solo, s1 = solve(net, init[b:b + 1], rows(kw, slice(b, b + 1)), OPTS, path, pred)
        assert s1.last_path == "dopri5-device"
        assert_trajectory_is_the_solo_call(b, res, s, solo, s1)
    assert torch.equal(res[0], init)


def test_one_trajectory_is_the_batch_form(small, dev):
    net, init, kw = small(1)
    res, s = solve(net, init, kw, EACH)
    solo, s1 = solve(net, init, kw, OPTS)
    assert s.last_path == "dopri5-device-each" and s1.last_path == "dopri5-device"
    assert_trajectory_is_the_solo_call(0, res, s, solo, s1)
    assert s.last_ode_stats["attempts"] == len(s1.last_ode_log)


@pytest.mark.parametrize("case", ["f4", "small-B3"])
def test_every_trajectorys_log_replays_bit_for_bit(case, f4, small, dev):
    """tests/test_hip_dopri5.py's replay (Linear / velocity: the host arithmetic at the logged (t, dt) is the device's) on every trajectory's
    own log and slice."""
    net, init, kw = f4 if case == "f4" else small(3)
    res, s = solve(net, init, kw, EACH, "Linear", "velocity")
    grid = [float(g) for g in torch.linspace(0, 1, 6)]
    for b in range(init.shape[0]):
        kb = rows(kw, slice(b, b + 1))
        outs, y = replay(s, net, init[b:b + 1], kb, grid, 1e-3, 1e-6, s.last_ode_log[b])
        assert len(outs) == 6
        for j, o in enumerate(outs):
            assert torch.equal(res[j, b:b + 1], o), (b, j)
        assert torch.equal(s.last_ode_state[b:b + 1], y), b


@pytest.mark.parametrize("case", ["f4", "small-B3"])
def test_against_the_host_form_per_trajectory(case, f4, small, dev):
    net, init, kw = f4 if case == "f4" else small(3)
    got, sd = solve(net, init, kw, EACH)
    want, sh = solve(net, init, kw, dict(EACH, controller="host"))
    assert sh.last_path == "dopri5-each" and sd.last_path == "dopri5-device-each"
    bound = min(10 * EACH_HOST_DISTANCE_MEASURED, 0.05)
    errs = [max(solver_norm(got[j, b], want[j, b], 1e-3, 1e-6) for j in range(len(want))) for b in range(init.shape[0])]
    print(f"PARITY dopri5-each.{case}.host measured {max(errs):.3e} bar {bound:.1e} (per trajectory: {' '.join(f'{e:.2e}' for e in errs)})")
    assert {k: sd.last_ode_stats[k] for k in ("nfe", "accepted", "rejected")} == {k: sh.last_ode_stats[k] for k in ("nfe", "accepted", "rejected")}
    assert max(errs) <= bound, (errs, bound)


def test_chunked_passes_sub_batches_and_over_enqueued_attempts_change_nothing(small, dev):
    net, init, kw = small(3)
    res, s = solve(net, init, kw, EACH, attempts_per_poll=1)
    runs = []
    for poll, chunk in ((7, 0), (7, 0), (3, 2)):  # (the second call replays the graph the first one captured; then 2 + 1 trajectories per pass)
        net.set_chunk(chunk)
        runs.append(solve(net, init, kw, EACH, attempts_per_poll=poll))
    net.set_chunk(0)
    for other, so in runs:
        assert torch.equal(other, res) and so.last_ode_stats == s.last_ode_stats and torch.equal(so.last_ode_state, s.last_ode_state)
        assert all(torch.equal(a, b) for a, b in zip(so.last_ode_log, s.last_ode_log))
    pair, sp = solve(net, init[[0, 2]].contiguous(), rows(kw, [0, 2]), EACH)
    for i, b in enumerate((0, 2)):
        assert torch.equal(pair[:, i], res[:, b]) and torch.equal(sp.last_ode_log[i], s.last_ode_log[b]), b
        assert torch.equal(sp.last_ode_state[i], s.last_ode_state[b]), b


def test_log_rows_bound_the_log_not_the_solve(small, dev):
    net, init, kw = small(3)
    res, s = solve(net, init, kw, EACH)
    for rows_kept in (0, 5):
        other, so = solve(net, init, kw, EACH, ode_log_rows=rows_kept)
        assert torch.equal(other, res) and so.last_ode_stats == s.last_ode_stats
        assert all(torch.equal(a, b[:rows_kept]) for a, b in zip(so.last_ode_log, s.last_ode_log))


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
        "    outs.append(s.get_sample_fn('ODE', dict(num_steps=5, controller='device', step_control='trajectory'))(init + i, net, **kw).cpu())\n"
        "    assert s.last_path == 'dopri5-device-each' and s.last_ode_stats['attempts'] >= 3\n"
        "torch.save((torch.stack(outs), s.last_ode_log), sys.argv[1])\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for mode in ("0", None):
        path = f"/tmp/lsl_dopri_each_graph_{mode}_{os.getpid()}.pt"
        env = {k: v for k, v in os.environ.items() if k != "LSL_GRAPH"}
        if mode is not None:
            env["LSL_GRAPH"] = mode
        subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=300)
        res[mode] = torch.load(path)
        os.remove(path)
    assert torch.equal(res["0"][0], res[None][0]) and all(torch.equal(a, b) for a, b in zip(res["0"][1], res[None][1]))
    assert not torch.equal(res["0"][0][0], res["0"][0][1])


def test_k_samples_folded_into_one_call_equal_their_own_calls(small, dev):
    from lam_slide_amd import CreateTransport, SecondStageSampler
    net, init, kw = small(2)
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(2, 5, 7, 3, generator=g).to(dev)
    inits = torch.randn(2, 2, 5, 7, 3, generator=g).to(dev)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 2),
                             sampling_kwargs={"sampling_method": "dopri5", "controller": "device", "step_control": "trajectory"})
    folded = drv.sample_latents_k(lat, 2, inits=inits)
    assert drv.last_sampler.last_path == "dopri5-device-each" and folded.shape == inits.shape
    for k in range(2):
        assert torch.equal(folded[k], drv.sample_latents(lat, init=inits[k])), k


def test_failures_stay_with_their_trajectory(small, dev):
    net, init, kw = small(3)
    res, s = solve(net, init, kw, EACH)
    attempts = [len(g) for g in s.last_ode_log]
    # a NaN in trajectory 1's initial state (a given NaN): that trajectory ends with the non-finite status, the others with their results
    bad = init.clone()
    bad[1, 1, 2, 0] = float("nan")
    sb = _sampler()
    with pytest.raises(RuntimeError, match=r"not finite .*\(trajectories \[1\]\)"):
        sb.get_sample_fn("ODE", dict(EACH))(bad, net, **kw)
    assert sb.last_ode_stats["rejected"][1] == 1 and sb.last_ode_stats["accepted"][1] == 0
    for b in (0, 2):
        assert torch.equal(sb.last_ode_state[b], s.last_ode_state[b]) and torch.equal(sb.last_ode_log[b], s.last_ode_log[b]), b
    # the attempt limit between the slowest trajectory and the others
    slowest = attempts.index(max(attempts))
    limit = sorted(attempts)[-2]
    assert limit < attempts[slowest], attempts
    sl = _sampler(ode_max_steps=limit)
    with pytest.raises(RuntimeError, match=r"max_steps reached \(trajectories \[%d\]\)" % slowest):
        sl.get_sample_fn("ODE", dict(EACH))(init, net, **kw)
    assert [len(g) for g in sl.last_ode_log] == [min(a, limit) for a in attempts]
    for b in range(3):
        if b != slowest:
            assert torch.equal(sl.last_ode_state[b], s.last_ode_state[b]), b
    assert torch.equal(sl.last_ode_log[slowest], s.last_ode_log[slowest][:limit])


@pytest.mark.parametrize("case", ["small", "hidden-256"])
def test_network_takes_one_time_per_trajectory(case, small, dev):
    """The precondition of the feature: LatentSIV3.forward with a different time per trajectory equals the single-trajectory forwards."""
    if case == "small":
        net, x, kw = small(3)
    else:
        from oracle import latent_net
        sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2)
        net = build_net(sh, latent_net.random_params(sh, seed=3), dev)
        g = torch.Generator().manual_seed(0)
        x = torch.randn(3, 12, 24, 32, generator=g).to(dev)
        kw = {"x_cond": torch.randn(3, 12, 24, 32, generator=g).to(dev), "x_cond_mask": (torch.rand(3, 12, 24, generator=g) < 0.3).long().to(dev)}
    t = torch.tensor([0.07, 0.5, 0.93], device=dev)
    with torch.no_grad():
        full = net(x, t, **kw).clone()
        for b in range(3):
            one = net(x[b:b + 1].contiguous(), t[b:b + 1], **rows(kw, slice(b, b + 1)))
            assert torch.equal(one, full[b:b + 1]), b
    assert torch.isfinite(full).all() and not torch.equal(full[0], full[1])
