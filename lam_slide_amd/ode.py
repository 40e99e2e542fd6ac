"""The ODE solvers behind ``Sampler.sample_ode`` / ``sample_ode_likelihood``: the arithmetic of a Runge-Kutta step on whole states
(:class:`_RkOps`), adaptive Dormand-Prince 5(4) (:func:`dopri5_solve`, :func:`dopri5_solve_each`: two wrappers of ONE lock-step loop)
and torchdiffeq's fixed-grid explicit methods (:func:`fixed_grid_rk_solve`).  Nothing here knows about transports or networks: the cost
- every evaluation of the right-hand side - goes through the caller's ``f``."""
from __future__ import annotations

import ctypes as C
import math
from collections.abc import Sequence
from typing import Any, Callable, Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


# ---- adaptive Dormand-Prince 5(4), the reference's default ODE method (transport.py:486-494: torchdiffeq.odeint(method="dopri5")) ----------
# torchdiffeq is a third-party dependency that is neither vendored in the reference nor installed here (parity unpinned); this
# restates its published algorithm (Dormand-Prince / Shampine tableau, Hairer's initial step, RMS error norm over the whole state, step
# factor clamp(0.9 err^-1/5, 0.2 .. 10), first-same-as-last, 4th-order dense output through the midpoint weights) so that the default
# configuration of the reference runs on the HIP network without it.  The network evaluations - all the cost - go through `f`.
_DP_ALPHA = (1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
_DP_BETA = ((1 / 5,), (3 / 40, 9 / 40), (44 / 45, -56 / 15, 32 / 9), (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
            (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656), (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84))
_DP_C_ERR = (35 / 384 - 1951 / 21600, 0.0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 + 12231 / 42400,
             11 / 84 - 649 / 6300, -1 / 60)
_DP_C_MID = (6025192743 / 30085553152 / 2, 0.0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
             187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2)


def _rms(v: Tensor) -> float:
    return float(v.double().pow(2).mean().sqrt())


class _RkOps:
    """The arithmetic of a Runge-Kutta step on whole states: linear combinations, the controller's error ratio, the quartic dense output.
    fp32 CUDA tensors go through the library (``lsl_rk_lincomb`` / ``lsl_rk_error_ratio`` / ``lsl_rk_dense``: one launch per combination, terms
    added in list order, deterministic reduction); anything else (CPU tensors of the host-logic tests, other dtypes) through torch operations
    in the same order.  ``terms`` = [(coefficient, tensor), ...] with at most 8 entries."""

    def __init__(self, like: Tensor):
        self.hip = like.is_cuda and like.dtype == torch.float32
        if self.hip:
            _lib.load()  # (LibraryMissing is raised here, where Sampler._vel catches it)
            self.dev = like.device
            self.scratch = torch.empty(_lib.RK_SCRATCH_BYTES // 4, dtype=torch.float32, device=like.device)
            self.ratio = torch.empty(1, dtype=torch.float32, device=like.device)

    def _pack(self, terms):
        xs = [x.contiguous() for _, x in terms]
        ptrs = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
        cs = (C.c_float * len(xs))(*[float(c) for c, _ in terms])
        return xs, ptrs, cs

    def lincomb(self, terms) -> Tensor:
        if not self.hip:
            rnd = _f32 if terms[0][1].dtype == torch.float32 else float  # (the kernels take fp32 coefficients)
            acc = terms[0][1] * rnd(terms[0][0])
            for c, x in terms[1:]:
                acc = acc + x * rnd(c)
            return acc
        xs, ptrs, cs = self._pack(terms)
        out = torch.empty_like(xs[0])
        _lib.call(self.dev, "lsl_rk_lincomb", out.data_ptr(), ptrs, cs, len(xs), out.numel())
        return out

    def error_ratio(self, y0: Tensor, y1: Tensor, terms, atol: float, rtol: float) -> float:
        """sqrt(mean((sum_j c_j k_j / (atol + rtol max(|y0|, |y1|)))^2)) as a host scalar (the one device sync of a step)."""
        if not self.hip:
            return _rms(self.lincomb(terms) / (atol + rtol * torch.maximum(y0.abs(), y1.abs())))
        xs, ptrs, cs = self._pack(terms)
        y0, y1 = y0.contiguous(), y1.contiguous()
        _lib.call(self.dev, "lsl_rk_error_ratio", self.ratio.data_ptr(), y0.data_ptr(), y1.data_ptr(), ptrs, cs, len(xs), float(atol), float(rtol),
                  y0.numel(), self.scratch.data_ptr())
        return float(self.ratio.item())

    def poly4(self, a: Tensor, b: Tensor, c: Tensor, d: Tensor, e: Tensor, x: float) -> Tensor:
        if not self.hip:
            xf = _f32(x) if e.dtype == torch.float32 else float(x)
            return e + xf * (d + xf * (c + xf * (b + xf * a)))
        out = torch.empty_like(e)
        _lib.call(self.dev, "lsl_rk_dense", out.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), e.data_ptr(), float(x), out.numel())
        return out


DOPRI_MAX_STEPS_MESSAGE = "dopri5: max_steps reached"
DOPRI_NON_FINITE_MESSAGE = "dopri5: the error ratio is not finite (NaN or Inf in the state or in the network's output)"


def dopri_each_failure(max_steps_rows: Sequence[int], non_finite_rows: Sequence[int]) -> Optional[str]:
    """The message of a per-trajectory solve some of whose trajectories failed (None: none did): the messages of the batch solve, each with
    the indices of its trajectories."""
    parts = [f"{msg} (trajectories {list(rows)})" for msg, rows in ((DOPRI_MAX_STEPS_MESSAGE, max_steps_rows), (DOPRI_NON_FINITE_MESSAGE, non_finite_rows))
             if len(rows)]
    return "; ".join(parts) if parts else None


def _dopri5_lockstep(f: Callable[[Sequence[float], Tensor], Tensor], y0: Tensor, grid: Sequence[float], rtol: float, atol: float, max_steps: int,
                     groups: Sequence[slice], stop_non_finite: bool):
    """The adaptive solve, once: y' = f(times, y) in lock step over ``groups``, slices along axis 0 of the state that together cover it in
    order.  Every group has its own time, step size, accept / reject decision, output cursor, counters and log; ``f`` takes one time per
    group; an attempt evaluates ``f`` once per stage for the whole state, and a group that is finished (or failed) is carried along
    unchanged - ``f`` still sees its state, at its last time.  Steps are chosen by a group's error controller alone and run past the output
    times; outputs are interpolated.  An output time that does not exceed the current time (repeated grid points, a single-point grid)
    returns the current state.  Time arithmetic runs in Python float64 (torchdiffeq keeps t in the dtype of the state's time tensor:
    accepted-step sequences agree in accuracy class, not in the last bit).  A group's state arithmetic of an attempt is ten `_RkOps` calls on
    its slice (six stage states, the error ratio - the one host scalar, and the one device sync - and for an accepted step the mid-point and
    three dense-output coefficients), so with an ``f`` whose groups are independent a group's result does not depend on the others.

    A group stops alone after ``max_steps`` attempts and, with ``stop_non_finite`` (the rule of the library's per-trajectory controller),
    on an error ratio that is not finite.  Without it a non-finite ratio is torchdiffeq's: a rejected attempt, then ``dt * 0.2`` after
    ``inf`` (the solve can recover) and no way out but ``max_steps`` after ``nan``.

    Returns ``(ys, stats, hit_limit, non_finite)``: the outputs at ``grid`` (None when a group failed), per-group lists ``nfe`` /
    ``accepted`` / ``rejected`` / ``log`` beside ``attempts``, ``passes`` and ``state``, and the indices of the groups that stopped early."""
    y0 = y0.contiguous()
    ops = _RkOps(y0)
    grid = [float(g) for g in grid]
    t0 = grid[0]
    G = range(len(groups))

    whole = list(groups) == [slice(None)]  # (the tensor itself then: a view per operand is host time on the network's critical path)

    def part(x, g):
        return x if whole else x[groups[g]]

    def merge(fn, keep, live):  # fn(g) for the live groups, the rows of `keep` for the others (one group: its piece itself, no copy)
        pieces = [fn(g) if live[g] else part(keep, g) for g in G]
        return pieces[0] if len(pieces) == 1 else torch.cat(pieces)

    def norm(g, ya, yb, terms):
        return ops.error_ratio(part(ya, g), part(yb, g), [(c, part(x, g)) for c, x in terms], atol, rtol)

    everyone = [True] * len(groups)
    f0 = f([t0] * len(groups), y0)
    # initial step (Hairer, Norsett, Wanner I, II.4), order 4 estimate; scale = atol + |y0| rtol
    d0, d1 = [norm(g, y0, y0, [(1.0, y0)]) for g in G], [norm(g, y0, y0, [(1.0, f0)]) for g in G]
    h0 = [1e-6 if d0[g] < 1e-5 or d1[g] < 1e-5 else 0.01 * d0[g] / d1[g] for g in G]
    f1 = f([t0 + h for h in h0], merge(lambda g: ops.lincomb([(1.0, part(y0, g)), (h0[g], part(f0, g))]), y0, everyone))
    passes = 2
    d2 = [norm(g, y0, y0, [(1.0, f1), (-1.0, f0)]) / h0[g] for g in G]
    dt = [min(100 * h0[g], max(1e-6, h0[g] * 1e-3) if d1[g] <= 1e-15 and d2[g] <= 1e-15 else (0.01 / max(d1[g], d2[g])) ** (1.0 / 5.0)) for g in G]

    t, t_lo, y, fy = [t0] * len(groups), [t0] * len(groups), y0, f0
    coeff: List[Any] = [None] * len(groups)  # dense output of a group's last accepted step [t_lo, t]
    outs = [[part(y0, g)] for g in G]  # per group: its output slices so far
    nfe, accepted, rejected = [2] * len(groups), [0] * len(groups), [0] * len(groups)
    log: List[List[Tuple[float, float, float, float]]] = [[] for _ in G]
    hit_limit, non_finite = [], []

    def flush(g):  # the output times group g's current step covers; is the group still live?
        while len(outs[g]) < len(grid) and not grid[len(outs[g])] > t[g]:
            if coeff[g] is None or t[g] <= t_lo[g]:  # no accepted step to interpolate: the state itself
                outs[g].append(part(y, g))
            else:
                e, d, c, b, a = coeff[g]
                outs[g].append(ops.poly4(a, b, c, d, e, (grid[len(outs[g])] - t_lo[g]) / (t[g] - t_lo[g])))
        if len(outs[g]) == len(grid):
            return False
        if accepted[g] + rejected[g] >= max_steps:
            hit_limit.append(g)
            return False
        return True

    live = [flush(g) for g in G]
    while any(live):
        k = [fy]
        yi = y
        for a, beta in zip(_DP_ALPHA, _DP_BETA):
            yi = merge(lambda g: ops.lincomb([(1.0, part(y, g))] + [(dt[g] * c, part(kj, g)) for c, kj in zip(beta, k) if c != 0.0]), yi, live)
            k.append(f([t[g] + a * dt[g] if live[g] else t[g] for g in G], yi))
        passes += 6
        y1 = yi  # the last stage IS the 5th-order solution (beta[-1] = c_sol): first same as last
        ratio = [norm(g, y, y1, [(dt[g] * c, kj) for c, kj in zip(_DP_C_ERR, k) if c != 0.0]) if live[g] else 0.0 for g in G]
        take = [live[g] and ratio[g] <= 1.0 for g in G]
        for g in G:
            if not live[g]:
                continue
            nfe[g] += 6
            log[g].append((t[g], dt[g], ratio[g], float(take[g])))
            if take[g]:
                y_mid = ops.lincomb([(1.0, part(y, g))] + [(dt[g] * c, part(kj, g)) for c, kj in zip(_DP_C_MID, k) if c != 0.0])
                yg, y1g, fa, fb, h = part(y, g), part(y1, g), part(k[0], g), part(k[-1], g), dt[g]
                coeff[g] = (yg, ops.lincomb([(h, fa)]),
                            ops.lincomb([(h, fb), (-4 * h, fa), (-11.0, yg), (-5.0, y1g), (16.0, y_mid)]),
                            ops.lincomb([(5 * h, fa), (-3 * h, fb), (18.0, yg), (14.0, y1g), (-32.0, y_mid)]),
                            ops.lincomb([(2 * h, fb), (-2 * h, fa), (-8.0, y1g), (-8.0, yg), (16.0, y_mid)]))
                t_lo[g], t[g] = t[g], t[g] + h
                accepted[g] += 1
            else:
                rejected[g] += 1
        y = merge(lambda g: part(y1, g), y, take)
        fy = merge(lambda g: part(k[-1], g), fy, take)
        for g in G:
            if not live[g]:
                continue
            if stop_non_finite and not math.isfinite(ratio[g]):
                non_finite.append(g)
                live[g] = False
                continue
            dt[g] = dt[g] * 10.0 if ratio[g] == 0.0 else dt[g] * min(10.0, max(0.9 / ratio[g] ** 0.2, 1.0 if ratio[g] < 1.0 else 0.2))
            live[g] = flush(g)
    stats = {"nfe": nfe, "accepted": accepted, "rejected": rejected, "attempts": max(a + r for a, r in zip(accepted, rejected)), "passes": passes,
             "log": log, "state": y}
    ys = None
    if not hit_limit and not non_finite:
        ys = [merge(lambda g: outs[g][j], y, everyone) for j in range(len(grid))]
    return ys, stats, sorted(hit_limit), sorted(non_finite)


def dopri5_solve(f: Callable[[float, Tensor], Tensor], y0: Tensor, grid: Sequence[float], rtol: float, atol: float,
                 max_steps: int = 100000) -> Tuple[List[Tensor], Dict[str, int]]:
    """Solution of y' = f(t, y) at the (increasing) times `grid`, grid[0] being the initial time: [y(grid[0]), ..., y(grid[-1])] and
    counters.  :func:`_dopri5_lockstep` with the whole state (of any rank: the likelihood path's augmented state is one flat vector) as its
    one group - one controller whose RMS error norm runs over everything, torchdiffeq's rule, non-finite ratios included."""
    ys, stats, hit_limit, _ = _dopri5_lockstep(lambda ts, y: f(ts[0], y), y0, grid, rtol, atol, max_steps, [slice(None)], stop_non_finite=False)
    if hit_limit:
        raise RuntimeError(DOPRI_MAX_STEPS_MESSAGE)
    return ys, {"nfe": stats["nfe"][0], "accepted": stats["accepted"][0], "rejected": stats["rejected"][0]}


def dopri5_solve_each(f: Callable[[Sequence[float], Tensor], Tensor], y0: Tensor, grid: Sequence[float], rtol: float, atol: float,
                      max_steps: int = 100000) -> Tuple[List[Tensor], Dict[str, Any]]:
    """:func:`dopri5_solve` with one step controller per trajectory (row of ``y0``): :func:`_dopri5_lockstep` with a group per row, the
    host restatement of the library's ``lsl_dopri_each_*`` loop.  ``f(times, y)`` takes one time per row.  Both functions run the one loop,
    so with an ``f`` whose rows are independent, row ``b`` equals ``dopri5_solve`` on ``y0[b:b+1]`` exactly.  A row stops alone at
    ``max_steps`` attempts or on a non-finite error ratio; the others go on, and the call raises once all have stopped (``err.stats``: the
    stats).  Returns the outputs and ``{"nfe", "accepted", "rejected"}`` as per-row lists, ``"attempts"`` (the largest count), ``"passes"``
    (evaluations of ``f``), ``"log"``: per row a float64 [attempts, 4] tensor of (t, dt, ratio, accepted), and ``"state"``."""
    ys, stats, hit_limit, non_finite = _dopri5_lockstep(f, y0, grid, rtol, atol, max_steps, [slice(b, b + 1) for b in range(int(y0.shape[0]))],
                                                        stop_non_finite=True)
    stats["log"] = [torch.tensor(rows, dtype=torch.float64).reshape(-1, 4) for rows in stats["log"]]
    failure = dopri_each_failure(hit_limit, non_finite)
    if failure:
        err = RuntimeError(failure)
        err.stats = stats
        raise err
    return ys, stats


# ---- torchdiffeq's other fixed-grid explicit methods (integrators.py:119 passes any `method` through) ------------------------------------
# Restated from the published schemes, as torchdiffeq's fixed_grid.py / rk_common.py define them (parity unpinned like dopri5: the package is
# absent): the grid is the output grid itself, one step per interval.  "rk4" is torchdiffeq's default fourth-order step, the 3/8 rule.
FIXED_GRID_RK_METHODS = ("midpoint", "heun3", "rk4")


def fixed_grid_rk_solve(f: Callable[[float, Tensor], Tensor], y0: Tensor, grid: Sequence[float], method: str) -> List[Tensor]:
    """[y(grid[0]), ..., y(grid[-1])] of y' = f(t, y) with one explicit Runge-Kutta step of `method` per grid interval; stage states and
    the update through `_RkOps` (library kernels for fp32 CUDA states)."""
    if method not in FIXED_GRID_RK_METHODS:
        raise NotImplementedError(f"fixed-grid method {method!r}")
    y = y0.contiguous()
    ops = _RkOps(y)
    out = [y]
    ts = [float(g) for g in grid]
    for t0, t1 in zip(ts[:-1], ts[1:]):
        dt = t1 - t0
        k1 = f(t0, y)
        if method == "midpoint":
            k2 = f(t0 + dt / 2, ops.lincomb([(1.0, y), (dt / 2, k1)]))
            y = ops.lincomb([(1.0, y), (dt, k2)])
        elif method == "heun3":
            k2 = f(t0 + dt / 3, ops.lincomb([(1.0, y), (dt / 3, k1)]))
            k3 = f(t0 + 2 * dt / 3, ops.lincomb([(1.0, y), (2 * dt / 3, k2)]))
            y = ops.lincomb([(1.0, y), (dt / 4, k1), (3 * dt / 4, k3)])
        else:  # rk4: 3/8 rule
            k2 = f(t0 + dt / 3, ops.lincomb([(1.0, y), (dt / 3, k1)]))
            k3 = f(t0 + 2 * dt / 3, ops.lincomb([(1.0, y), (dt, k2), (-dt / 3, k1)]))
            k4 = f(t1, ops.lincomb([(1.0, y), (dt, k1), (-dt, k2), (dt, k3)]))
            y = ops.lincomb([(1.0, y), (dt / 8, k1), (3 * dt / 8, k2), (3 * dt / 8, k3), (dt / 8, k4)])
        out.append(y)
    return out
