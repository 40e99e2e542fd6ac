"""CPU tests of the adaptive ODE sampler's ``step_control`` keyword (lam_slide_amd/transport.py): the lock-step host solver with one step
controller per trajectory (``dopri5_solve_each``) against ``dopri5_solve`` on every trajectory alone, the keyword's dispatch and errors, the
binding of lsl_dopri_each_* against the header, and the argument checks of the library that need no device."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT

STIFFNESS = (3.0, 40.0, 11.0)  # k_b of the rows: model(x, t)[b] = sin(k_b t[b]) x[b]


def _sampler(path="Linear", pred="velocity"):
    from lam_slide_amd import CreateTransport, Sampler
    return Sampler(CreateTransport(path, pred)())


def _rows_model(ks):
    k = torch.tensor(ks, dtype=torch.float64).reshape(-1, 1, 1)
    return lambda x, t, **kw: torch.sin(k * t.double().reshape(-1, 1, 1)).to(x.dtype) * x


def _init():
    return 1.0 + torch.rand(3, 4, 5, generator=torch.Generator().manual_seed(3), dtype=torch.float64)


def test_lock_step_solve_equals_every_trajectory_solved_alone(monkeypatch):
    """Rows of different stiffness: outputs, counters, every evaluation time and every error ratio of row b equal dopri5_solve on [b:b+1]."""
    from lam_slide_amd.transport import _DP_ALPHA, _RkOps, dopri5_solve, dopri5_solve_each
    y0 = _init()
    grid = [0.0, 0.2, 0.55, 0.55, 1.0]
    rtol, atol = 1e-5, 1e-8
    ks = torch.tensor(STIFFNESS, dtype=torch.float64).reshape(-1, 1, 1)
    ys, stats = dopri5_solve_each(lambda ts, y: torch.sin(ks * torch.tensor(ts, dtype=torch.float64).reshape(-1, 1, 1)) * y, y0, grid, rtol, atol)
    assert stats["passes"] == 2 + 6 * stats["attempts"] and len(ys) == len(grid) and ys[0].shape == y0.shape
    attempts = [a + r for a, r in zip(stats["accepted"], stats["rejected"])]
    assert len(set(attempts)) > 1, attempts  # (rows that take the same steps would prove nothing)
    assert stats["attempts"] == max(attempts) and [len(g) for g in stats["log"]] == attempts
    orig = _RkOps.error_ratio
    for b, kb in enumerate(STIFFNESS):
        times, ratios = [], []
        monkeypatch.setattr(_RkOps, "error_ratio", lambda self, *a: ratios.append(orig(self, *a)) or ratios[-1])
        solo, solo_stats = dopri5_solve(lambda t, y: times.append(t) or torch.sin(torch.tensor(kb * t, dtype=torch.float64)) * y, y0[b:b + 1], grid, rtol, atol)
        monkeypatch.undo()
        for j in range(len(grid)):
            assert torch.equal(ys[j][b:b + 1], solo[j]), (b, j)
        assert {k: stats[k][b] for k in ("nfe", "accepted", "rejected")} == solo_stats, b
        log = stats["log"][b]
        assert times[2:] == [t + a * dt for t, dt, _, _ in log.tolist() for a in _DP_ALPHA], b
        assert ratios[3:] == log[:, 2].tolist() and [float(r <= 1.0) for r in ratios[3:]] == log[:, 3].tolist(), b
        end = log[-1, 0].item() + log[-1, 1].item()  # (the state is the end of the last accepted step, at or past the last output time)
        assert log[-1, 3] == 1.0 and end >= grid[-1] and (end > grid[-1] or torch.equal(stats["state"][b:b + 1], solo[-1])), b
    # one controller for the batch takes other steps: its rows are not the solo results
    batch, batch_stats = dopri5_solve(lambda t, y: torch.sin(ks * t) * y, y0, grid, rtol, atol)
    assert all(not torch.equal(batch[-1][b], ys[-1][b]) for b in range(3)), batch_stats


def test_step_control_keyword_dispatch_on_the_cpu():
    s = _sampler()
    y0, model = _init().float(), _rows_model(STIFFNESS)
    plain = s.get_sample_fn("ODE", dict(num_steps=4))(y0, model)
    assert s.last_path == "dopri5" and isinstance(s.last_ode_stats["nfe"], int)
    batch = s.get_sample_fn("ODE", dict(num_steps=4, step_control="batch"))(y0, model)
    assert s.last_path == "dopri5" and torch.equal(plain, batch)
    each = s.get_sample_fn("ODE", dict(num_steps=4, step_control="trajectory"))(y0, model)
    assert s.last_path == "dopri5-each" and each.shape == plain.shape
    stats, logs = s.last_ode_stats, s.last_ode_log
    assert sorted(stats) == ["accepted", "attempts", "network_passes", "nfe", "rejected"] and len(logs) == 3 and s.last_ode_state.shape == y0.shape
    assert stats["network_passes"] == 2 + 6 * stats["attempts"] and [len(g) for g in logs] == [a + r for a, r in zip(stats["accepted"], stats["rejected"])]
    assert len(set(len(g) for g in logs)) > 1
    for b in range(3):  # through the Sampler too, a trajectory of the call is the batch call on that trajectory alone
        solo = s.get_sample_fn("ODE", dict(num_steps=4))(y0[b:b + 1], _rows_model(STIFFNESS[b:b + 1]))
        assert torch.equal(each[:, b:b + 1], solo), b
        assert s.last_ode_stats == {k: stats[k][b] for k in ("nfe", "accepted", "rejected")}
    assert not torch.equal(each, batch)
    with pytest.raises(ValueError, match="step_control"):
        s.get_sample_fn("ODE", dict(step_control="row"))
    for method in ("euler", "rk4", "midpoint"):
        with pytest.raises(ValueError, match="dopri5"):
            s.get_sample_fn("ODE", dict(step_control="trajectory", sampling_method=method))
    with pytest.raises(RuntimeError, match="not a lam_slide_amd.LatentSIV3 on a GPU"):
        s.get_sample_fn("ODE", dict(controller="device", step_control="trajectory", num_steps=4))(y0, model)


def test_a_row_that_exhausts_the_attempt_limit_is_named():
    """max_steps between the attempts of the rows: the stiff row stops alone, the others finish with their solo results, the call raises."""
    s = _sampler()
    y0, model = _init().float(), _rows_model(STIFFNESS)
    s.get_sample_fn("ODE", dict(num_steps=4, step_control="trajectory"))(y0, model)
    attempts = [len(g) for g in s.last_ode_log]
    assert attempts[1] == max(attempts) and sorted(attempts)[1] < attempts[1], attempts
    free = s.last_ode_state.clone()
    s.ode_max_steps = sorted(attempts)[1]
    with pytest.raises(RuntimeError, match=r"max_steps reached \(trajectories \[1\]\)"):
        s.get_sample_fn("ODE", dict(num_steps=4, step_control="trajectory"))(y0, model)
    assert [len(g) for g in s.last_ode_log] == [attempts[0], s.ode_max_steps, attempts[2]]
    assert torch.equal(s.last_ode_state[0], free[0]) and torch.equal(s.last_ode_state[2], free[2])


def test_header_summary_and_workspace_head_match_the_binding():
    """lsl_dopri_each_summary field for field against its ctypes mirror; the offsets and formulas of the workspace head against ``_lib.Dopri``."""
    from lam_slide_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    body = re.search(r"typedef struct lsl_dopri_each_summary \{(.*?)\} lsl_dopri_each_summary;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"int32_t\s*(.+)", decl, re.S)
        assert m, decl
        fields += [(n.strip(), C.c_int32) for n in m.group(1).split(",")]
    assert fields == list(_lib.DopriEachSummary._fields_)
    D = _lib.Dopri
    assert C.sizeof(_lib.DopriEachSummary) <= D.EACH_CTL_OFFSET - D.EACH_SUMMARY_OFFSET and C.sizeof(_lib.DopriCtl) == D.EACH_CTL_STRIDE

    def macro(name):  # the macro as a Python function of its parameters
        m = re.search(r"#define %s(?:\(([^)]*)\))? (.+)$" % name, header, re.M)
        params = [p.strip() for p in (m.group(1) or "").split(",") if p.strip()]
        expr = m.group(2).replace("(size_t)", "").replace("/", "//")
        expr = re.sub(r"LSL_DOPRI_EACH_LOG_OFFSET\(", "LOG(", expr)
        return lambda *a: int(eval(expr, {"LOG": D.each_log_offset}, dict(zip(params, a))))

    assert (macro("LSL_DOPRI_EACH_SUMMARY_OFFSET")(), macro("LSL_DOPRI_EACH_CTL_OFFSET")()) == (D.EACH_SUMMARY_OFFSET, D.EACH_CTL_OFFSET)
    for B in (1, 2, 3, 255, 4096, D.EACH_MAX_B):
        log = macro("LSL_DOPRI_EACH_LOG_OFFSET")(B)
        assert log == D.each_log_offset(B) and log % 256 == 0 and log >= D.EACH_CTL_OFFSET + D.EACH_CTL_STRIDE * B
        for rows in (0, 1, 7, 128, D.MAX_ATTEMPTS):
            state = macro("LSL_DOPRI_EACH_STATE_OFFSET")(B, rows)
            assert state == D.each_state_offset(B, rows) and state % 256 == 0 and state >= log + 32 * B * rows
    assert {"lsl_dopri_each_workspace_bytes", "lsl_dopri_each_begin", "lsl_dopri_each_advance"} <= set(_lib.EXPORTED)


def test_refused_calls_enqueue_nothing_and_say_why():
    """Argument checks of lsl_dopri_each_* that need no device (the pointers are never dereferenced; the model handle has no weights)."""
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = _lib.load()
    assert lib.lsl_dopri_each_workspace_bytes(None, 1, 1, 1, 1, 0) == 0
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    io = _lib.IO(p, p, p, None, None, None, 2, 2, 3)
    desc = _lib.DopriDesc(1, 1, 0, 10, 1e-3, 1e-6)
    begin = lambda m, grid, rows, size=1 << 30: lib.lsl_dopri_each_begin(m, C.byref(io), C.byref(desc), grid, 2, p, rows, p, size, None)  # noqa: E731
    down, up = (C.c_double * 2)(0.5, 0.25), (C.c_double * 2)(0.25, 0.5)
    assert begin(None, down, 4) == -3 and "non-decreasing" in _lib.last_error()
    desc.max_steps = _lib.Dopri.MAX_ATTEMPTS + 1
    assert begin(None, up, 4) == -3 and "max_steps" in _lib.last_error()
    desc.max_steps = 10
    assert begin(None, up, -1) == -3 and "log_rows" in _lib.last_error()
    assert begin(None, up, _lib.Dopri.MAX_ATTEMPTS + 1) == -3 and "log_rows" in _lib.last_error()
    assert begin(None, up, 4) == -1  # (no model)
    assert lib.lsl_dopri_each_advance(None, C.byref(io), 1, p, 1 << 30, None) == -1
    md = _lib.ModelDesc(3, 64, 4, 16, 16, 128, 1, 0, 0, 10000.0)
    handle = C.c_void_p()
    assert lib.lsl_model_create(C.byref(md), C.byref(handle)) == 0
    try:
        need = lib.lsl_dopri_each_workspace_bytes(handle, 2, 2, 3, 2, 4)
        assert need > _lib.Dopri.each_state_offset(2, 4) + 10 * 4 * 2 * 2 * 3 * 3
        assert lib.lsl_dopri_each_workspace_bytes(handle, 2, 2, 3, 2, 0) < need  # (log_rows = 0 is allowed, and smaller)
        assert lib.lsl_dopri_each_workspace_bytes(handle, 2, 2, 3, 2, -1) == 0 and lib.lsl_dopri_each_workspace_bytes(handle, _lib.Dopri.EACH_MAX_B + 1, 2, 3, 2, 0) == 0
        assert begin(handle, up, 4, need - 1) == -4 and "workspace too small" in _lib.last_error()
        assert begin(handle, up, 4, need) == -2  # (room enough: the next check is the weights, still before any launch)
        assert lib.lsl_dopri_each_advance(handle, C.byref(io), 1, p, need, None) == -3 and "lsl_dopri_each_begin" in _lib.last_error()
    finally:
        lib.lsl_model_destroy(handle)


# ---- the one lock-step loop behind both solvers (lam_slide_amd/ode.py): what differs between the two forms, and what must not ----
def _cos_rhs(bad=None, bad_calls=(), bad_rows=slice(None)):
    """y' = cos(t) per row (independent of y, so a non-finite stage leaves later evaluations finite), as (f_batch, f_each, times): both
    count their calls together and return ``bad`` in ``bad_rows`` on the calls (1-based) in ``bad_calls``; times[i] is call i's time(s)."""
    times = []

    def f_each(ts, y):
        times.append(list(ts))
        out = torch.cos(torch.tensor(ts, dtype=y.dtype)).reshape(-1, 1, 1).expand_as(y).clone()
        if len(times) in bad_calls:
            out[bad_rows] = bad
        return out

    return (lambda t, y: f_each([t] * y.shape[0], y)), f_each, times


def test_batch_form_recovers_from_an_infinite_error_ratio():
    """torchdiffeq's rule, kept by the batch form: +inf in the seventh evaluation of the first attempt (it enters the error estimate alone, so the
    ratio is inf, not nan) is a rejected attempt followed by a step of 0.2 times the first, and the solve finishes."""
    from lam_slide_amd.transport import dopri5_solve
    y0 = torch.tensor([1.0, 2.0], dtype=torch.float64).reshape(2, 1, 1)
    f, _, times = _cos_rhs(bad=float("inf"), bad_calls=(8,))  # calls 1, 2: the initial step; 3 .. 8: the first attempt
    grid = [0.0, 0.4, 1.0]
    ys, stats = dopri5_solve(f, y0, grid, 1e-6, 1e-9)
    assert stats["rejected"] >= 1 and stats["accepted"] >= 1 and stats["nfe"] == len(times) == 2 + 6 * (stats["accepted"] + stats["rejected"])
    # the sixth evaluation of an attempt is at t + dt; both attempts start at t = 0, the second because the first was rejected
    dt_first, dt_second = times[6][0], times[12][0]
    assert dt_first > 0.0 and dt_second == dt_first * 0.2, (dt_first, dt_second)
    assert times[8][0] == dt_second * 0.2  # (alpha_1 = 1 / 5 of the new step, from the old time)
    for t, y in zip(grid, ys):  # y = y0 + sin(t): the controller holds 1e-6 |y| + 1e-9 a step, over a handful of steps
        assert torch.isfinite(y).all() and (y - (y0 + math.sin(t))).abs().max() < 1e-5, t


def test_nan_ends_the_batch_form_at_max_steps_and_stops_one_trajectory_alone():
    """NaN from the first attempt on in row 0, max_steps = 4.  Batch form: every attempt is rejected, "max_steps reached".  Per-trajectory
    form: row 0 stops on its first attempt and is named; row 1 goes on and finishes - its counters, log and state are those of its solo
    solves (a failed call returns no outputs: ``err.stats`` is what it leaves)."""
    from lam_slide_amd.transport import DOPRI_MAX_STEPS_MESSAGE, DOPRI_NON_FINITE_MESSAGE, dopri5_solve, dopri5_solve_each
    y0 = torch.tensor([1.0, 2.0], dtype=torch.float64).reshape(2, 1, 1)
    grid, rtol, atol = [0.0, 0.3, 0.5], 1e-3, 1e-6
    every_attempt = range(3, 1000)
    f, _, times = _cos_rhs(bad=float("nan"), bad_calls=every_attempt, bad_rows=slice(0, 1))
    with pytest.raises(RuntimeError) as batch:
        dopri5_solve(f, y0, grid, rtol, atol, max_steps=4)
    assert str(batch.value) == DOPRI_MAX_STEPS_MESSAGE and len(times) == 2 + 6 * 4
    _, f_each, times = _cos_rhs(bad=float("nan"), bad_calls=every_attempt, bad_rows=slice(0, 1))
    with pytest.raises(RuntimeError) as each:
        dopri5_solve_each(f_each, y0, grid, rtol, atol, max_steps=4)
    assert str(each.value) == f"{DOPRI_NON_FINITE_MESSAGE} (trajectories [0])"
    stats = each.value.stats
    assert (stats["accepted"][0], stats["rejected"][0]) == (0, 1) and math.isnan(stats["log"][0][0, 2]) and torch.equal(stats["state"][0], y0[0])
    f_solo, f_solo_each, _ = _cos_rhs()
    solo, solo_stats = dopri5_solve(f_solo, y0[1:2], grid, rtol, atol, max_steps=4)
    solo_each, solo_each_stats = dopri5_solve_each(f_solo_each, y0[1:2], grid, rtol, atol, max_steps=4)
    assert 1 <= solo_stats["accepted"] + solo_stats["rejected"] <= 4 and stats["attempts"] == solo_each_stats["attempts"]
    assert {k: stats[k][1] for k in ("nfe", "accepted", "rejected")} == solo_stats
    assert torch.equal(stats["log"][1], solo_each_stats["log"][0]) and torch.equal(stats["state"][1:2], solo_each_stats["state"])
    assert all(torch.equal(a, b) for a, b in zip(solo, solo_each))


def test_one_trajectory_solved_each_is_the_batch_solve():
    """B = 1: the two wrappers run the one loop on the same single group - equal outputs bit for bit, equal counters."""
    from lam_slide_amd.transport import dopri5_solve, dopri5_solve_each
    y0 = torch.tensor([[[1.5]]], dtype=torch.float64)
    grid, rtol, atol = [0.0, 0.0, 0.7, 2.0], 1e-7, 1e-9
    k = 6.0
    ys, stats = dopri5_solve(lambda t, y: math.sin(k * t) * y, y0, grid, rtol, atol)
    ys_each, stats_each = dopri5_solve_each(lambda ts, y: math.sin(k * ts[0]) * y, y0, grid, rtol, atol)
    assert len(ys) == len(ys_each) == len(grid) and all(torch.equal(a, b) and a.shape == y0.shape for a, b in zip(ys, ys_each))
    assert stats == {key: stats_each[key][0] for key in ("nfe", "accepted", "rejected")} and stats["rejected"] + stats["accepted"] > 3
    assert stats_each["passes"] == stats["nfe"] and stats_each["attempts"] == len(stats_each["log"][0]) == stats["accepted"] + stats["rejected"]
