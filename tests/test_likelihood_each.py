"""CPU tests of ``Sampler.sample_ode_likelihood(step_control="trajectory")`` - the host restatement of the per-trajectory augmented solve
(``dopri5_solve_each`` on rows ``[x_b | logp_b]``) -, of the new keywords' dispatch and refusals, and of the binding of ``lsl_dopri_logp_*``
against the header.  The device form is tested in tests/test_hip_likelihood_device.py."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from test_dopri5_each import STIFFNESS, _init, _rows_model, _sampler


def _probe(shape, seed=5, dtype=torch.float32):
    return (torch.randint(2, shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dtype)


def test_a_row_of_the_per_trajectory_call_is_the_solo_call():
    """Rows of different stiffness (model(x, t)[b] = sin(k_b t_b) x_b): logp, z and the counters of row b equal the B = 1 call exactly, in the
    each form and - one trajectory being one vector in both - in today's batch form."""
    x, e = _init().float(), _probe((3, 4, 5))
    s = _sampler()
    logp, z = s.sample_ode_likelihood(num_steps=4, eps=e, step_control="trajectory")(x, _rows_model(STIFFNESS))
    assert s.last_path == "likelihood-generic-each" and logp.shape == (3,) and z.shape == x.shape
    stats, logs = s.last_ode_stats, s.last_ode_log
    attempts = [a + r for a, r in zip(stats["accepted"], stats["rejected"])]
    assert len(set(attempts)) > 1, attempts  # (rows that take the same steps would prove nothing)
    assert [len(g) for g in logs] == attempts and stats["attempts"] == max(attempts) and stats["network_passes"] == 2 + 6 * max(attempts)
    assert s.last_ode_state.shape == x.shape and s.last_ode_logp_state.shape == (3,)
    for b in range(3):
        for kw in (dict(step_control="trajectory"), dict()):
            s1 = _sampler()
            logp1, z1 = s1.sample_ode_likelihood(num_steps=4, eps=e[b:b + 1], **kw)(x[b:b + 1], _rows_model(STIFFNESS[b:b + 1]))
            assert torch.equal(logp1, logp[b:b + 1]) and torch.equal(z1, z[b:b + 1]), (b, kw)
            got = s1.last_ode_stats
            assert {k: (got[k][0] if kw else got[k]) for k in ("nfe", "accepted", "rejected")} == {k: stats[k][b] for k in ("nfe", "accepted", "rejected")}, (b, kw)
    batch_logp, _ = _sampler().sample_ode_likelihood(num_steps=4, eps=e)(x, _rows_model(STIFFNESS))
    assert all(batch_logp[b] != logp[b] for b in range(3))  # one controller for the batch: a trajectory's logp depends on its companions


def test_default_keywords_keep_the_result_bits():
    """The defaults run the path of before the keywords: the flat [x | logp] vector through dopri5_solve, restated here with autograd."""
    from lam_slide_amd.transport import _f32, dopri5_solve
    x, e, model = _init().float(), _probe((3, 4, 5)), _rows_model(STIFFNESS)
    s = _sampler()
    logp, z = s.sample_ode_likelihood(num_steps=4, eps=e)(x, model)
    assert s.last_path == "likelihood-generic" and isinstance(s.last_ode_stats["nfe"], int)
    s2 = _sampler()
    logp2, z2 = s2.sample_ode_likelihood(num_steps=4, eps=e, controller="host", step_control="batch")(x, model)
    assert torch.equal(logp, logp2) and torch.equal(z, z2) and s2.last_ode_stats == s.last_ode_stats
    tr = s.transport
    t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False, last_step_size=0.0)

    def rhs(t, state):
        xs = state[:60].reshape(3, 4, 5)
        tf = _f32(1.0 - t)
        vx, vm = tr.velocity_coeffs(tf)
        with torch.enable_grad():
            xg = xs.detach().requires_grad_(True)
            drift = vx * xg + vm * model(xg, torch.full((3,), tf))
            grad = torch.autograd.grad(torch.sum(drift * e), xg)[0]
        return torch.cat([-drift.detach().reshape(-1), torch.sum(grad * e, dim=(1, 2))])

    ys, stats = dopri5_solve(rhs, torch.cat([x.reshape(-1), torch.zeros(3)]), [float(g) for g in torch.linspace(t0, t1, 4)], 1e-3, 1e-6)
    assert stats == s.last_ode_stats
    assert torch.equal(z, ys[-1][:60].reshape(3, 4, 5)) and torch.equal(logp, tr.prior_logp(z) - ys[-1][60:])


def test_linear_drift_gives_the_trace():
    """Linear / velocity with model(x, t) = a * x (a diagonal Jacobian: every Rademacher probe gives eps . (A eps) = trace A exactly): the
    right-hand side of logp is the constant trace A, which the method integrates exactly; delta_logp = trace A (t1 - t0) within the solver's
    tolerance atol + rtol |delta_logp| (float64: the rounding is far below it)."""
    g = torch.Generator().manual_seed(9)
    a = torch.randn(1, 4, 5, generator=g, dtype=torch.float64)
    x = torch.randn(3, 4, 5, generator=g, dtype=torch.float64) * torch.tensor([1.0, 8.0, 0.125], dtype=torch.float64).reshape(3, 1, 1)
    rtol, atol = 1e-3, 1e-6
    for kw in (dict(step_control="trajectory"), dict()):
        s = _sampler()
        tr = s.transport
        t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False, last_step_size=0.0)
        logp, z = s.sample_ode_likelihood(num_steps=5, rtol=rtol, atol=atol, **kw)(x, lambda xs, t, **k: a * xs)
        delta = tr.prior_logp(z) - logp
        want = float(a.sum()) * (t1 - t0)
        assert float((delta - want).abs().max()) <= atol + rtol * abs(want), (kw, delta, want)


def test_keyword_refusals():
    s = _sampler()
    x, model = _init().float(), _rows_model(STIFFNESS)
    for method in ("euler", "rk4", "midpoint", "heun3"):
        for kw in (dict(step_control="trajectory"), dict(controller="device")):
            with pytest.raises(ValueError, match="dopri5"):
                s.sample_ode_likelihood(sampling_method=method, **kw)
    with pytest.raises(ValueError, match="step_control"):
        s.sample_ode_likelihood(step_control="row")
    with pytest.raises(ValueError, match="controller"):
        s.sample_ode_likelihood(controller="gpu")
    with pytest.raises(NotImplementedError, match="callable"):
        s.sample_ode_likelihood(controller="device", eps=lambda shape, dev: torch.ones(shape))
    with pytest.raises(RuntimeError, match="not a lam_slide_amd.LatentSIV3 on a GPU"):
        s.sample_ode_likelihood(controller="device", step_control="trajectory", num_steps=4)(x, model)


def test_header_macros_and_records_match_the_binding():
    from lam_slide_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    D = _lib.Dopri
    assert int(re.search(r"#define LSL_DOPRI_NEGATED (\d+)", header).group(1)) == D.NEGATED == 2
    m = re.search(r"#define LSL_DOPRI_LOGP_SIDE_OFFSET\(([^)]*)\) (.+)$", header, re.M)
    params = [p.strip() for p in m.group(1).split(",")]
    expr = m.group(2).replace("(size_t)", "").replace("/", "//")
    for state_at in (D.STATE_OFFSET, D.each_state_offset(3, 128), D.each_state_offset(D.EACH_MAX_B, 0)):
        for n in (1, 63, 64, 105, 315, 1536, 2 ** 31 + 5):
            side = int(eval(expr, {}, dict(zip(params, (state_at, n)))))
            assert side == D.logp_side_offset(state_at, n) and side % 256 == 0 and state_at + 4 * n <= side < state_at + 4 * n + 256
    # the records at the head of the workspace are those of lsl_dopri_* / lsl_dopri_each_*: the sizes the offsets count on
    assert C.sizeof(_lib.DopriCtl) == D.EACH_CTL_STRIDE == 128 and C.sizeof(_lib.DopriEachSummary) == 20
    assert {"lsl_dopri_logp_workspace_bytes", "lsl_dopri_logp_begin", "lsl_dopri_logp_advance", "lsl_rademacher"} <= set(_lib.EXPORTED)
    for name in ("lsl_dopri_logp_workspace_bytes", "lsl_dopri_logp_begin", "lsl_dopri_logp_advance", "lsl_rademacher"):
        assert re.search(r"\b%s\(" % name, header), name
