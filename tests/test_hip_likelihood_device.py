"""GPU tests of ``Sampler.sample_ode_likelihood(controller="device")``: the adaptive solve on the augmented vector ``[x | logp]`` inside the
library (lsl_dopri_logp_begin / lsl_dopri_logp_advance, the augmented forms of csrc/k_dopri5.hip.h).

The defining property: with ``step_control="trajectory"`` trajectory b has the bits of the batch-form device call on ``[b:b+1]`` - logp, z,
log, counters, final state - with a fixed probe and with probes drawn on the device, at any pass size and any number of over-enqueued
attempts.  Around it: every trajectory's log replayed with the host arithmetic, the host each-form, the fp64 oracle, the batch form against
today's host-controller call, failures that stay with their trajectory, the probe draw, the refusals, and the precondition in the tangent
pass (one time per trajectory).
Shapes: the seeded hidden-64 model of tests/test_hip_dopri5.py at T, L, C = 5, 7, 3 (N = 105: the logp element shares the last workgroup)
with B = 1 and B = 3, the same model at 4, 8, 8 (N = 256: the logp element alone in a second workgroup of the error norm), the f4 fixture's
model at its shape, the f1 fixture for the oracle.  Initial states scaled by (1, 8, 0.125): the trajectories take different numbers of attempts."""
import ctypes as C
import math

import pytest
import torch

import jvp_oracle
from conftest import parity, rel_l2, shape_from
from test_dopri5_controller import solver_norm
from test_hip_dopri5 import controller_dt, small_case
from test_hip_dopri5_each import rows, scaled
from test_hip_parity import build_net

pytestmark = pytest.mark.gpu

# Distance of the device solve from the host form on the same network, per trajectory over the augmented vector [z | delta_logp] in the
# solver's norm: the value measured on MI355X.  The bound of the tests is ten times this, and never above 0.05 -
# the rule of tests/test_hip_dopri5.py.
LOGP_HOST_DISTANCE_MEASURED = 0.0

RTOL, ATOL, STEPS = 1e-3, 1e-6, 5
PAIRS = [("Linear", "velocity"), ("GVP", "noise")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def shapes(golden, dev):
    """name -> (net, x, conditioning, fixed probe); built once"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "f4":
                f = golden("f4_sampler.npz")
                net = build_net(shape_from(f.group("shape")), f.group("p"), dev)
                x, kw = f["init"].to(dev), {"x_cond": f["x_cond"].to(dev), "x_cond_mask": f["mask"].to(dev)}
            elif name == "n256":
                net, x, kw = small_case(dev, 3, T=4, L=8, C=8)
            else:
                net, x, kw = small_case(dev, int(name[-1]))
            cache[name] = (net, scaled(x, True), kw, jvp_oracle.rademacher(x.shape, 500 + len(name)).to(dev))
        return cache[name]

    return get


def _sampler(path, pred, **attrs):
    from lam_slide_amd import CreateTransport, Sampler
    s = Sampler(CreateTransport(path, pred)())
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


def solve(net, x, kw, eps, path="Linear", pred="velocity", each=True, controller="device", seeds=None, **attrs):
    s = _sampler(path, pred, **attrs)
    fn = s.sample_ode_likelihood(num_steps=STEPS, rtol=RTOL, atol=ATOL, eps=eps, controller=controller, step_control="trajectory" if each else "batch",
                                 probe_seeds=seeds)
    logp, z = fn(x, net, **kw)
    return logp, z, s


def attempts_of(s):
    return [a + r for a, r in zip(s.last_ode_stats["accepted"], s.last_ode_stats["rejected"])]


def assert_trajectory_is_the_solo_call(b, run, solo, i=0):
    """trajectory b of the per-trajectory run against trajectory i of `solo` (the batch form on one trajectory, or another per-trajectory run)"""
    (logp, z, s), (logp1, z1, s1) = run, solo
    assert torch.equal(logp[b], logp1[i]) and torch.equal(z[b], z1[i]), b
    one = isinstance(s1.last_ode_stats["nfe"], int)
    assert torch.equal(s.last_ode_log[b], s1.last_ode_log if one else s1.last_ode_log[i]), b
    assert {k: s.last_ode_stats[k][b] for k in ("nfe", "accepted", "rejected")} == {k: (s1.last_ode_stats[k] if one else s1.last_ode_stats[k][i])
                                                                                  for k in ("nfe", "accepted", "rejected")}, b
    assert torch.equal(s.last_ode_state[b], s1.last_ode_state[i]) and torch.equal(s.last_ode_logp_state[b], s1.last_ode_logp_state[i]), b


@pytest.mark.parametrize("path,pred", PAIRS)
@pytest.mark.parametrize("case", ["small-B1", "small-B3", "n256", "f4"])
def test_every_trajectory_equals_its_solo_call_bit_for_bit(case, path, pred, shapes, dev):
    net, x, kw, eps = shapes(case)
    B = x.shape[0]
    run = solve(net, x, kw, eps, path, pred)
    s = run[2]
    assert s.last_path == "likelihood-device-solve-each" and run[0].shape == (B,) and run[1].shape == x.shape
    attempts = attempts_of(s)
    print(f"likelihood-each.{case}.{path}.{pred}: attempts per trajectory {attempts}")
    assert s.last_ode_stats["attempts"] == max(attempts) and s.last_ode_stats["network_passes"] == 2 + 6 * max(attempts)
    assert [len(g) for g in s.last_ode_log] == attempts and s.last_ode_stats["nfe"] == [2 + 6 * a for a in attempts] and min(s.last_ode_stats["accepted"]) >= 2
    if B > 1:
        assert len(set(attempts)) > 1, attempts  # (trajectories in step with each other would prove nothing)
    for b in range(B):
        solo = solve(net, x[b:b + 1].contiguous(), rows(kw, slice(b, b + 1)), eps[b:b + 1].contiguous(), path, pred, each=False)
        assert solo[2].last_path == "likelihood-device-solve"
        assert_trajectory_is_the_solo_call(b, run, solo)


def test_device_drawn_probes_do_not_depend_on_the_batch(shapes, dev):
    net, x, kw, _ = shapes("small-B3")
    seeds = [11, 2 ** 63 + 5, 7]
    run = solve(net, x, kw, None, seeds=seeds)
    again = solve(net, x, kw, None, seeds=seeds)
    assert torch.equal(run[0], again[0]) and torch.equal(run[1], again[1])
    other = solve(net, x, kw, None, seeds=[12, 2 ** 63 + 5, 7])
    assert not torch.equal(run[0][0], other[0][0]) and torch.equal(run[0][1:], other[0][1:])
    for b in range(3):
        solo = solve(net, x[b:b + 1].contiguous(), rows(kw, slice(b, b + 1)), None, each=False, seeds=[seeds[b]])
        assert_trajectory_is_the_solo_call(b, run, solo)
    # the default seeds: mix_seed(the call's seed, b)
    from lam_slide_amd.transport import mix_seed
    s = _sampler("Linear", "velocity")
    s.seed = 3
    dflt = s.sample_ode_likelihood(num_steps=STEPS, controller="device", step_control="trajectory")(x, net, **kw)
    want = solve(net, x, kw, None, seeds=[mix_seed(mix_seed(3, 0), b) for b in range(3)])
    assert torch.equal(dflt[0], want[0]) and torch.equal(dflt[1], want[1])


def test_pass_size_sub_batch_polls_and_log_rows_change_nothing(shapes, dev):
    net, x, kw, eps = shapes("small-B3")
    run = solve(net, x, kw, eps, attempts_per_poll=1)
    for poll, chunk in ((3, 0), (7, 0), (3, 2)):  # (the last: 2 + 1 trajectories per pass)
        net.set_chunk(chunk)
        try:
            other = solve(net, x, kw, eps, attempts_per_poll=poll)
        finally:
            net.set_chunk(0)
        for b in range(3):
            assert_trajectory_is_the_solo_call(b, run, other, b)
    pair = solve(net, x[[0, 2]].contiguous(), rows(kw, [0, 2]), eps[[0, 2]].contiguous())
    for i, b in enumerate((0, 2)):
        assert_trajectory_is_the_solo_call(b, run, pair, i)
    for kept in (0, 5):
        other = solve(net, x, kw, eps, ode_log_rows=kept)
        assert torch.equal(other[0], run[0]) and torch.equal(other[1], run[1]) and other[2].last_ode_stats == run[2].last_ode_stats
        assert all(torch.equal(a, b[:kept]) for a, b in zip(other[2].last_ode_log, run[2].last_ode_log))


def replay_augmented(f, y0, grid, log, rtol=RTOL, atol=ATOL):
    """Every attempt of ``log`` again with _RkOps on the flat vector [x | logp] and the right-hand side f (the pattern of
    tests/test_hip_dopri5.py: replay); asserts the logged ratios and decisions; returns (outputs, state)"""
    from lam_slide_amd.transport import _DP_ALPHA, _DP_BETA, _DP_C_ERR, _DP_C_MID, _RkOps
    ops = _RkOps(y0)
    y = y0.contiguous()
    fy = f(grid[0], y)
    outs = [y for g in grid if g <= grid[0]]
    for a, (t, dt, ratio, accepted) in enumerate(log.tolist()):
        k = [fy]
        for al, beta in zip(_DP_ALPHA, _DP_BETA):
            yi = ops.lincomb([(1.0, y)] + [(dt * b, kj) for b, kj in zip(beta, k) if b != 0.0])
            k.append(f(t + al * dt, yi))
        got = ops.error_ratio(y, yi, [(dt * c, kj) for c, kj in zip(_DP_C_ERR, k) if c != 0.0], atol, rtol)
        assert got == ratio, (a, got, ratio)
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


@pytest.mark.parametrize("case", ["small-B3", "n256"])
def test_every_trajectorys_log_replays_bit_for_bit(case, shapes, dev):
    """Linear / velocity: (vx, vm) = (0, 1) exactly, so LatentSIV3.jvp and dot_rows at the logged (t, dt) are the device's right-hand side."""
    from lam_slide_amd.transport import _f32, dot_rows
    net, x, kw, eps = shapes(case)
    logp, z, s = solve(net, x, kw, eps)
    tr = s.transport
    t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False, last_step_size=0.0)
    grid = [float(g) for g in torch.linspace(t0, t1, STEPS)]
    n = x[0].numel()
    for b in range(x.shape[0]):
        kb, eb = rows(kw, slice(b, b + 1)), eps[b:b + 1].contiguous()

        def f(t, state):
            xs = state[:n].reshape(x[b:b + 1].shape).contiguous()
            out, jt = net.jvp(xs, torch.full((1,), _f32(1.0 - t), device=dev), kb["x_cond"], kb["x_cond_mask"], tangent=eb)
            return torch.cat([-out.reshape(-1), dot_rows(eb, jt).float()])

        outs, y = replay_augmented(f, torch.cat([x[b].reshape(-1), torch.zeros(1, device=dev)]), grid, s.last_ode_log[b])
        assert len(outs) == STEPS
        assert torch.equal(outs[-1][:n].reshape(x[b].shape), z[b]), b
        assert torch.equal(s.last_delta_logp[b:b + 1], outs[-1][n:]) and torch.equal(s._prior_logp_rows(z[b:b + 1]) - outs[-1][n:], logp[b:b + 1]), b
        assert torch.equal(y[:n].reshape(x[b].shape), s.last_ode_state[b]) and torch.equal(y[n], s.last_ode_logp_state[b]), b


def test_device_drawn_probes_follow_the_documented_stream(shapes, dev):
    """Independent of the solve's own draw: a device-drawn run replayed with the host arithmetic, where the probe of evaluation e is
    lsl_rademacher(probe_seeds[b], e) - e = 0 for f(t0), 1 for the evaluation of Hairer's rule, 2 + 6 a + s for stage s of attempt a.  The
    logged ratios, the outputs and the final state are bit-equal (Linear / velocity), and the first step size is Hairer's from the
    evaluations 0 and 1 (fp64 pow on the device against Python's: 4 ulp).  A probe that changes with every evaluation makes the right-hand
    side of logp rough, so the controller takes many small steps at the reference's tolerances (170 attempts here); the test runs at
    rtol 1e-2, atol 1e-3 and keeps every attempt's row of the log."""
    from lam_slide_amd import _lib
    from lam_slide_amd.transport import _RkOps, _f32, dot_rows
    net, x, kw, _ = shapes("small-B3")
    seeds = [2 ** 64 - 9, 17, 2 ** 40 + 1]
    rtol, atol = 1e-2, 1e-3
    s = _sampler("Linear", "velocity", ode_log_rows=1000)
    logp, z = s.sample_ode_likelihood(num_steps=STEPS, rtol=rtol, atol=atol, controller="device", step_control="trajectory", probe_seeds=seeds)(x, net, **kw)
    attempts = attempts_of(s)
    print(f"likelihood-each.drawn-probes: attempts per trajectory {attempts}")
    assert [len(g) for g in s.last_ode_log] == attempts and max(attempts) <= 1000 and min(s.last_ode_stats["accepted"]) >= 2
    tr = s.transport
    t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False, last_step_size=0.0)
    grid = [float(g) for g in torch.linspace(t0, t1, STEPS)]
    n = x[0].numel()
    for b in range(3):
        kb, shape = rows(kw, slice(b, b + 1)), x[b:b + 1].shape

        def rhs(t, state, e):
            probe = torch.empty(shape, dtype=torch.float32, device=dev)
            _lib.call(dev, "lsl_rademacher", probe.data_ptr(), n, seeds[b], e)
            out, jt = net.jvp(state[:n].reshape(shape).contiguous(), torch.full((1,), _f32(1.0 - t), device=dev), kb["x_cond"], kb["x_cond_mask"], tangent=probe)
            return torch.cat([-out.reshape(-1), dot_rows(probe, jt).float()])

        calls = [0]

        def f(t, state):  # (replay_augmented evaluates f(t0) once, then six stages per logged attempt, in order)
            c = calls[0]
            calls[0] += 1
            return rhs(t, state, 0 if c == 0 else c + 1)

        y0 = torch.cat([x[b].reshape(-1), torch.zeros(1, device=dev)])
        log = s.last_ode_log[b]
        outs, y = replay_augmented(f, y0, grid, log, rtol, atol)
        assert calls[0] == 1 + 6 * len(log) and len(outs) == STEPS
        assert torch.equal(outs[-1][:n].reshape(x[b].shape), z[b]) and torch.equal(outs[-1][n:], s.last_delta_logp[b:b + 1]), b
        assert torch.equal(y[:n].reshape(x[b].shape), s.last_ode_state[b]) and torch.equal(y[n], s.last_ode_logp_state[b]), b
        # the first step: Hairer's rule from evaluation 0 and evaluation 1 (at t0 + h0 on y0 + h0 f0)
        ops = _RkOps(y0)
        f0 = rhs(grid[0], y0, 0)
        d0, d1 = ops.error_ratio(y0, y0, [(1.0, y0)], atol, rtol), ops.error_ratio(y0, y0, [(1.0, f0)], atol, rtol)
        h0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1
        f1 = rhs(grid[0] + h0, ops.lincomb([(1.0, y0), (h0, f0)]), 1)
        d2 = ops.error_ratio(y0, y0, [(1.0, f1), (-1.0, f0)], atol, rtol) / h0
        want = min(100 * h0, max(1e-6, h0 * 1e-3) if d1 <= 1e-15 and d2 <= 1e-15 else (0.01 / max(d1, d2)) ** (1.0 / 5.0))
        got = log[0, 1].item()
        assert abs(got - want) <= 4 * math.ulp(want), (b, got, want)
        wrong = rhs(grid[0] + h0, ops.lincomb([(1.0, y0), (h0, f0)]), 0)  # (evaluation 1 with evaluation 0's probe is another number)
        assert not torch.equal(wrong[n:], f1[n:])


def augmented_distance(got, want, b):
    """trajectory b's [z | delta_logp] of two runs in the solver's norm"""
    vec = [torch.cat([z[b].double().reshape(-1).cpu(), s.last_delta_logp[b:b + 1].double().cpu()]) for _, z, s in (got, want)]
    return solver_norm(vec[0], vec[1], RTOL, ATOL)


def counters(s):
    return {k: s.last_ode_stats[k] for k in ("nfe", "accepted", "rejected")}


@pytest.mark.parametrize("path,pred", PAIRS)
def test_against_the_host_each_form(path, pred, shapes, dev):
    net, x, kw, eps = shapes("small-B3")
    got = solve(net, x, kw, eps, path, pred)
    want = solve(net, x, kw, eps, path, pred, controller="host")
    assert want[2].last_path == "likelihood-device-each" and got[2].last_path == "likelihood-device-solve-each"
    bound = min(10 * LOGP_HOST_DISTANCE_MEASURED, 0.05)
    errs = [augmented_distance(got, want, b) for b in range(3)]
    print(f"PARITY likelihood-each.{path}.{pred}.host measured {max(errs):.3e} bar {bound:.1e} (per trajectory: {' '.join(f'{e:.2e}' for e in errs)})")
    assert counters(got[2]) == counters(want[2])
    assert max(errs) <= bound, (errs, bound)
    if max(errs) == 0.0:  # (equal solves give equal logp: both forms take the prior through the fixed-order sum)
        assert torch.equal(got[0], want[0])


def test_batch_form_against_todays_host_controller_call(shapes, dev):
    net, x, kw, eps = shapes("small-B3")
    got = solve(net, x, kw, eps, each=False)
    want = solve(net, x, kw, eps, each=False, controller="host")
    assert got[2].last_path == "likelihood-device-solve" and want[2].last_path == "likelihood-device"
    bound = min(10 * LOGP_HOST_DISTANCE_MEASURED, 0.05)
    errs = [augmented_distance(got, want, b) for b in range(3)]
    print(f"PARITY likelihood-batch.host measured {max(errs):.3e} bar {bound:.1e} (per trajectory: {' '.join(f'{e:.2e}' for e in errs)})")
    assert counters(got[2]) == want[2].last_ode_stats
    assert max(errs) <= bound, (errs, bound)
    each = solve(net, x, kw, eps)
    assert all(each[0][b] != got[0][b] for b in range(3))  # (one error norm for the batch: a trajectory's logp depends on its companions)


def test_against_the_fp64_oracle(golden, dev):
    """The f1 shape, a fixed probe: logp and z of every trajectory against the generic path on oracle (a) in fp64, run on that row alone;
    bar = 4 x the error the generic path on oracle (b) shows in the same solve (test_multi_step_likelihood_against_the_generic_path's rule)."""
    from oracle import latent_net
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

    net = build_net(sh, p, dev)
    logp, z, s = solve(net, x.to(dev), dict(x_cond=xc.to(dev), x_cond_mask=mask.to(dev), y=y.to(dev)), eps.to(dev))
    for b in range(x.shape[0]):
        r = slice(b, b + 1)
        ref = {}
        for tag, model in (("a", oracle_a), ("b", oracle_b)):
            fn = _sampler("Linear", "velocity").sample_ode_likelihood(num_steps=STEPS, rtol=RTOL, atol=ATOL, eps=eps[r].double())
            ref[tag] = fn(x[r].double(), model, x_cond=xc[r].double(), x_cond_mask=mask[r], y=y[r].double())
        z_model, logp_model = rel_l2(ref["b"][1], ref["a"][1]), float((ref["b"][0] - ref["a"][0]).abs().max())
        parity(f"likelihood-each.oracle.row{b}.z", rel_l2(z[r].cpu(), ref["a"][1]), 4 * z_model)
        parity(f"likelihood-each.oracle.row{b}.logp", float((logp[r].cpu().double() - ref["a"][0]).abs().max()), 4 * logp_model)


def test_failures_stay_with_their_trajectory(shapes, dev):
    """A NaN given in trajectory 1's state: that trajectory ends with the non-finite status, the others keep their bits."""
    net, x, kw, eps = shapes("small-B3")
    _, _, s = solve(net, x, kw, eps)
    bad = x.clone()
    bad[1, 1, 2, 0] = float("nan")
    sb = _sampler("Linear", "velocity")
    with pytest.raises(RuntimeError, match=r"not finite .*\(trajectories \[1\]\)"):
        sb.sample_ode_likelihood(num_steps=STEPS, rtol=RTOL, atol=ATOL, eps=eps, controller="device", step_control="trajectory")(bad, net, **kw)
    assert sb.last_ode_stats["rejected"][1] == 1 and sb.last_ode_stats["accepted"][1] == 0
    for b in (0, 2):
        assert torch.equal(sb.last_ode_state[b], s.last_ode_state[b]) and torch.equal(sb.last_ode_logp_state[b], s.last_ode_logp_state[b]), b
        assert torch.equal(sb.last_ode_log[b], s.last_ode_log[b]), b


def test_prior_term_does_not_depend_on_the_batch(dev):
    """The prior's sum of squares at a size where a torch reduction may pick its order by the batch (15 360 elements a trajectory): a row alone
    and in the batch, and within the rounding of Transport.prior_logp."""
    s = _sampler("Linear", "velocity")
    z = torch.randn(4, 30, 16, 32, generator=torch.Generator().manual_seed(1)).to(dev) * torch.tensor([1.0, 2.0, 0.5, 1.5], device=dev).reshape(4, 1, 1, 1)
    full = s._prior_logp_rows(z)
    for b in range(4):
        assert torch.equal(s._prior_logp_rows(z[b:b + 1].contiguous())[0], full[b]), b
    want = s.transport.prior_logp(z.double().cpu())
    assert float(((full.double().cpu() - want) / want).abs().max()) <= 2.0 ** -23


def test_rademacher_draws(dev):
    from lam_slide_amd import _lib
    n = 65536

    def draw(seed, e, count=n):
        out = torch.empty(count, dtype=torch.float32, device=dev)
        _lib.call(dev, "lsl_rademacher", out.data_ptr(), count, seed, e)
        return out

    a = draw(2 ** 64 - 3, 4)
    assert bool((a.abs() == 1.0).all())
    assert torch.equal(a, draw(2 ** 64 - 3, 4)) and torch.equal(a[:1001], draw(2 ** 64 - 3, 4, 1001))
    assert not torch.equal(a, draw(2 ** 64 - 3, 5)) and not torch.equal(a, draw(2 ** 64 - 4, 4))
    mean = float(a.double().mean())
    print(f"RADEMACHER mean over {n} entries {mean:.3e} bar {4 / math.sqrt(n):.3e}")
    assert abs(mean) <= 4 / math.sqrt(n)


def test_refusals_enqueue_nothing(shapes, dev):
    """Tail, ln_fuse and linear-attention handles: NotImplementedError from the sampler, -21 from the library, and the output buffers keep
    their sentinel; a callable probe and the fixed-grid methods are refused by the keywords' checks."""
    from oracle import latent_net
    from lam_slide_amd import _lib
    kwn = dict(depth=1, in_dim=8, hidden_size=256, num_heads=8, mlp_ratio=2)
    B, T, L = 2, 4, 5
    g = torch.Generator().manual_seed(3)
    x, xc = torch.randn(B, T, L, 8, generator=g).to(dev), torch.randn(B, T, L, 8, generator=g).to(dev)
    mask = torch.ones(B, T, L, dtype=torch.long, device=dev)
    eps = torch.ones_like(x)
    setters = {"linear": "lsl_model_set_attention_mode", "tail": "lsl_model_set_tail", "ln_fuse": "lsl_model_set_ln_fuse"}
    for form, setter in setters.items():
        sh = latent_net.NetShape(**kwn, attention_mode="linear" if form == "linear" else "scaled_dot_product")
        net = build_net(sh, latent_net.random_params(sh, seed=9), dev)
        if form == "tail":
            net.set_tail(True)
        if form == "ln_fuse":
            net.set_ln_fuse(True)
        net.ensure_packed(dev)
        s = _sampler("Linear", "velocity")
        for each in (False, True):
            with pytest.raises(NotImplementedError):
                s.sample_ode_likelihood(num_steps=3, eps=eps, controller="device", step_control="trajectory" if each else "batch")(
                    x, net, x_cond=xc, x_cond_mask=mask)
            out, out_logp = torch.full((3,) + tuple(x.shape), 7.0, device=dev), torch.full((3, B), 9.0, device=dev)
            io, keep = net.make_io(x, xc, mask, None)
            desc, times = s._dopri_desc([0.0, 0.5, 1.0], RTOL, ATOL, True)
            ws = torch.empty(1 << 26, dtype=torch.uint8, device=dev)
            rc = _lib.load().lsl_dopri_logp_begin(net._handle, C.byref(io), C.byref(desc), times, 3, out.data_ptr(), out_logp.data_ptr(), int(each), 8,
                                                  eps.data_ptr(), None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
            assert rc == -21 and setter in _lib.last_error(), (form, rc, _lib.last_error())
            assert bool((out == 7.0).all()) and bool((out_logp == 9.0).all()), form
            del keep
    net, x, kw, eps = shapes("small-B1")
    s = _sampler("Linear", "velocity")
    with pytest.raises(NotImplementedError, match="callable"):
        s.sample_ode_likelihood(controller="device", eps=lambda shape, d: torch.ones(shape, device=d))
    for method in ("euler", "rk4"):
        for extra in (dict(controller="device"), dict(step_control="trajectory")):
            with pytest.raises(ValueError, match="dopri5"):
                s.sample_ode_likelihood(sampling_method=method, **extra)


@pytest.mark.parametrize("case", ["small", "hidden-256"])
def test_tangent_pass_takes_one_time_per_trajectory(case, dev):
    """The precondition: LatentSIV3.jvp with a different time per trajectory equals the single-trajectory calls bit for bit."""
    if case == "small":
        net, x, kw = small_case(dev, 3)
    else:
        from oracle import latent_net
        sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2)
        net = build_net(sh, latent_net.random_params(sh, seed=3), dev)
        g = torch.Generator().manual_seed(0)
        x = torch.randn(3, 12, 24, 32, generator=g).to(dev)
        kw = {"x_cond": torch.randn(3, 12, 24, 32, generator=g).to(dev), "x_cond_mask": (torch.rand(3, 12, 24, generator=g) < 0.3).long().to(dev)}
    t = torch.tensor([0.07, 0.5, 0.93], device=dev)
    v = jvp_oracle.rademacher(x.shape, 13).to(dev)
    out, out_t = net.jvp(x, t, kw["x_cond"], kw["x_cond_mask"], tangent=v)
    out, out_t = out.clone(), out_t.clone()
    for b in range(3):
        kb = rows(kw, slice(b, b + 1))
        o, ot = net.jvp(x[b:b + 1].contiguous(), t[b:b + 1], kb["x_cond"], kb["x_cond_mask"], tangent=v[b:b + 1].contiguous())
        assert torch.equal(o, out[b:b + 1]) and torch.equal(ot, out_t[b:b + 1]), b
    assert torch.isfinite(out_t).all() and not torch.equal(out_t[0], out_t[1])
