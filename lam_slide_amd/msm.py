"""The Markov state models of the peptide evaluation, estimated on the device (eval_peptide.py:245-288, modules/analysis.py:47-56).

  active_set             <- ``connectivity='largest'`` of ``estimate_markov_model``: the largest strongly connected set of a count matrix
  estimate_markov_model  <- ``pyemma.msm.estimate_markov_model(dtraj, lag)`` with its default, the reversible maximum-likelihood estimate:
                            ``MarkovModel`` with the transition matrix and the stationary vector embedded in the full index space
                            (``np.eye`` / zeros outside the active set, the way eval_peptide.py:261-271 fills them)
  MarkovModel.restricted <- pyemma's ``active_set`` / ``transition_matrix`` / ``pi`` as numpy arrays (the one read-back)
  MarkovModel.timescales <- ``msm.timescales(k)``
  pcca_assignments       <- ``msm.pcca(m)`` / ``msm.metastable_assignments`` by the inner simplex algorithm of PCCA+ (Deuflhard and Weber), host
                            side numpy.  **pyemma's Nelder-Mead refinement of the rotation is not reproduced**: assignments a real pyemma
                            produced enter ``markov_state_block(metastable_assignments=)`` as an array.
  markov_state_block     <- the Markov-state block of ``analyze_trajectory``: ``ref_metastable_probs``, ``traj_metastable_probs``,
                            ``msm_transition_matrix``, ``msm_pi``, ``traj_transition_matrix``, ``traj_pi`` from the projected reference, the
                            projected trajectory and the microstate centres

The estimator is stated as mathematics (include/lsl_api.h) and checked against a numpy / scipy restatement
(tests/msm_oracle.py).  **Parity with a live pyemma was not checked.**  For one count matrix C (entries <= 0 count as 0, total below 2^53):
the active set A is the largest strongly connected component of the graph ``i -> j`` where ``C[i, j] > 0`` (one state alone only with
``C[i, i] > 0``; equal sizes: the one holding the lowest state; none: empty); ``C~ = C[A, A]``, ``c = C~.sum(1)``, ``K = C~ + C~^T``; from
``x0 = K.sum(1) / K.sum()`` the step ``q = c / x``, ``y_i = sum_{j: K_ij != 0} K_ij / (q_i + q_j)``, ``x' = y / y.sum()`` is counted and
repeated until ``!(max |x - x'| / ((x + x') / 2) > maxerr)`` or ``maxiter`` steps; ``pi = x``, ``T_ij = X_ij / sum_j X_ij`` with
``X_ij = K_ij / (q_i + q_j)``.

The device form is ``lsl_msm_active_set`` / ``lsl_msm_reversible_step`` / ``lsl_msm_transition_matrix`` of liblamslide_hip.so
(csrc/k_msm.hip.h): one resident workgroup per count matrix with K in LDS, the stop test on the device, ``ceil(maxiter / CHUNK)`` step calls
enqueued with no host synchronisation (a finished series leaves at once), nothing read back, no atomics, a series' bits the same alone and
in any batch.  It runs for int64 counts on the GPU with ``ns <= MAX_STATES``; anything else (CPU tensors, more states) takes a numpy
float64 restatement with the same outputs.  ``last_path[name]`` tells which of the two ("fused" / "torch") ran last."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import tica as _tica

MAX_STATES = 128  # LSL_MSM_MAX_STATES (csrc/k_msm.hip.h): fp64 K of a series stays in LDS
MAX_S = 65535  # LSL_MSM_MAX_S: series of one library call; more are chunked
CHUNK = 4096  # steps of one lsl_msm_reversible_step call: bounds the run time of a launch

last_path: Dict[str, str] = {}


def fused_applies(counts: Tensor) -> bool:
    """The dispatch rule: int64 counts [S, ns, ns] on the GPU with ``ns <= MAX_STATES``."""
    return _lib.device_form(counts, dtype=torch.int64) and 1 <= counts.shape[-1] <= MAX_STATES


# ---- the numpy float64 restatement ----
def _active_numpy(C: np.ndarray) -> np.ndarray:
    """C [ns, ns] -> bool [ns]: the rule of the active set by a boolean reachability closure."""
    ns = C.shape[0]
    reach = (C > 0) | np.eye(ns, dtype=bool)
    for k in range(ns):
        reach |= reach[:, k:k + 1] & reach[k:k + 1, :]
    comp = reach & reach.T
    size = comp.sum(axis=1)
    ok = (size >= 2) | (np.diagonal(C) > 0)
    if not ok.any():
        return np.zeros(ns, dtype=bool)
    best = size[ok].max()
    root = int(np.flatnonzero(ok & (size == best))[0])  # (the lowest member of a component is its lowest row)
    return comp[root]


def _estimate_numpy(C: np.ndarray, active: np.ndarray, maxiter: int, maxerr: float):
    """One count matrix and its active flags -> (n_iter, err, converged, T [ns, ns], pi [ns]), T and pi embedded."""
    ns = C.shape[0]
    A = np.flatnonzero(active)
    T, pi = np.eye(ns), np.zeros(ns)
    if len(A) == 0:
        return 0, 0.0, True, T, pi
    if len(A) == 1:
        pi[A] = 1.0
        return 0, 0.0, True, T, pi
    Ct = np.maximum(C[np.ix_(A, A)], 0)
    Ki = Ct + Ct.T
    c, K = Ct.sum(axis=1).astype(np.float64), Ki.astype(np.float64)
    nz = K != 0
    x = Ki.sum(axis=1).astype(np.float64) / float(Ki.sum())

    def flows(x):
        q = c / x
        D = q[:, None] + q[None, :]
        return np.where(nz, K / np.where(nz, D, 1.0), 0.0)

    n, err, conv = 0, 0.0, False
    while n < maxiter:
        y = flows(x).sum(axis=1)
        xn = y / y.sum()
        err = float(np.max(np.abs(x - xn) / (0.5 * (x + xn))))
        x = xn
        n += 1
        if not err > maxerr:
            conv = True
            break
    X = flows(x)
    T[np.ix_(A, A)] = X / X.sum(axis=1)[:, None]
    pi[A] = x
    return n, err, conv, T, pi


class MarkovModel(NamedTuple):
    """``transition_matrix`` float64 [(S,) ns, ns] (the identity with the active block written in), ``pi`` float64 [(S,) ns] (0 outside the
    active set), ``active`` bool [(S,) ns], ``n_active`` int32 [(S)], ``counts`` int64 [(S,) ns, ns], ``n_iter`` int32 [(S)], ``err`` float64
    [(S)] (the last step's), ``converged`` bool [(S)] (the stop test held within ``maxiter``; True with no step for at most one active state),
    all on the counts' device; ``lag`` (or None); ``path`` "fused" or "torch"."""
    transition_matrix: Tensor
    pi: Tensor
    active: Tensor
    n_active: Tensor
    counts: Tensor
    n_iter: Tensor
    err: Tensor
    converged: Tensor
    lag: Optional[int]
    path: str

    def restricted(self, s: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(active set indices, T[A][:, A], pi[A]) of series s as numpy arrays: pyemma's ``active_set`` / ``transition_matrix`` / ``pi``.
        The one read-back of a model."""
        batched = self.active.dim() == 2
        pick = (lambda t: t[s]) if batched else (lambda t: t)
        if not batched and s != 0:
            raise IndexError(f"s = {s}: the model holds one series")
        A = np.flatnonzero(_lib.to_host(pick(self.active)))
        T, pi = _lib.to_host(pick(self.transition_matrix)), _lib.to_host(pick(self.pi))
        return A, T[np.ix_(A, A)].copy(), pi[A].copy()

    def timescales(self, k: Optional[int] = None, s: int = 0) -> np.ndarray:
        """The k slowest implied timescales ``-lag / ln |lambda_i|``, i = 1..k (all of them for k = None), of series s: the eigenvalues of
        ``(S + S^T) / 2`` with ``S = D^{1/2} T D^{-1/2}``, ``D = diag(pi)``, on the active set, in descending order.  Host side."""
        if self.lag is None:
            raise ValueError("timescales need the lag the counts were taken at: pass lag= to estimate_markov_model")
        _, T, pi = self.restricted(s)
        lam = _symmetrised_eigh(T, pi)[0]
        k = len(lam) - 1 if k is None else int(k)
        if not 0 <= k <= len(lam) - 1:
            raise ValueError(f"k = {k} outside 0..{len(lam) - 1} (the active set has {len(lam)} states)")
        with np.errstate(divide="ignore"):
            return -float(self.lag) / np.log(np.abs(lam[1:k + 1]))


def _symmetrised_eigh(T: np.ndarray, pi: np.ndarray):
    """Eigenvalues (descending) and orthonormal eigenvectors (columns) of (S + S^T) / 2, S = D^{1/2} T D^{-1/2}, and sqrt(pi)."""
    d = np.sqrt(np.asarray(pi, dtype=np.float64))
    Sm = d[:, None] * np.asarray(T, dtype=np.float64) / d[None, :]
    lam, V = np.linalg.eigh(0.5 * (Sm + Sm.T))
    order = np.argsort(-lam, kind="stable")
    return lam[order], V[:, order], d


def _as_counts(counts) -> Tensor:
    c = counts.detach() if torch.is_tensor(counts) else torch.as_tensor(np.asarray(counts))
    if c.dim() not in (2, 3) or c.shape[-1] != c.shape[-2] or c.shape[-1] < 1 or c.dtype.is_floating_point or c.dtype == torch.bool or (
            c.dim() == 3 and c.shape[0] < 1):
        raise ValueError(f"expected integer counts [ns, ns] or [S, ns, ns], got {c.dtype} {tuple(c.shape)}")
    return c


def active_set(counts) -> Tuple[Tensor, Tensor]:
    """counts [ns, ns] or [S, ns, ns] (integers) -> (active bool [(S,) ns], n_active int32 [(S)]): the largest strongly connected set of the
    graph ``i -> j`` where ``counts[i, j] > 0`` - ``connectivity='largest'``.  A state alone counts only with a positive diagonal; among
    sets of equal size the one holding the lowest state index wins; no candidate gives an empty set."""
    c = _as_counts(counts)
    v = c if c.dim() == 3 else c[None]
    S, ns = int(v.shape[0]), int(v.shape[1])
    dev = v.device
    if fused_applies(v):
        vc = v.contiguous()
        act = torch.empty(S, ns, dtype=torch.int32, device=dev)
        na = torch.empty(S, dtype=torch.int32, device=dev)
        for s0 in range(0, S, MAX_S):
            s1 = min(S, s0 + MAX_S)
            _lib.call(dev, "lsl_msm_active_set", vc[s0:s1].data_ptr(), s1 - s0, ns, act[s0:s1].data_ptr(), na[s0:s1].data_ptr())
        act = act != 0
        last_path["active_set"] = "fused"
    else:
        a = np.stack([_active_numpy(m) for m in _lib.to_host(v.long())])
        act, na = _lib.to_device(a, dev), _lib.to_device(a.sum(axis=1).astype(np.int32), dev)
        last_path["active_set"] = "torch"
    return (act, na) if c.dim() == 3 else (act[0], na[0])


def _estimate_device(v: Tensor, maxiter: int, maxerr: float):
    S, ns = int(v.shape[0]), int(v.shape[1])
    dev = v.device
    act = torch.empty(S, ns, dtype=torch.int32, device=dev)
    na = torch.empty(S, dtype=torch.int32, device=dev)
    x = torch.empty(S, ns, dtype=torch.float64, device=dev)
    n_iter = torch.empty(S, dtype=torch.int32, device=dev)
    err = torch.empty(S, dtype=torch.float64, device=dev)
    done = torch.empty(S, dtype=torch.int32, device=dev)
    T = torch.empty(S, ns, ns, dtype=torch.float64, device=dev)
    pi = torch.empty(S, ns, dtype=torch.float64, device=dev)
    for s0 in range(0, S, MAX_S):
        s1 = min(S, s0 + MAX_S)
        n = s1 - s0
        cp, ap = v[s0:s1].data_ptr(), act[s0:s1].data_ptr()
        state = (x[s0:s1].data_ptr(), n_iter[s0:s1].data_ptr(), err[s0:s1].data_ptr(), done[s0:s1].data_ptr())
        _lib.call(dev, "lsl_msm_active_set", cp, n, ns, ap, na[s0:s1].data_ptr())
        for launch in range(max(1, -(-maxiter // CHUNK))):  # (the first sets the state from the counts; the ones after convergence return at once)
            _lib.call(dev, "lsl_msm_reversible_step", cp, ap, n, ns, CHUNK, maxiter, maxerr, int(launch == 0), *state)
        _lib.call(dev, "lsl_msm_transition_matrix", cp, ap, x[s0:s1].data_ptr(), n, ns, T[s0:s1].data_ptr(), pi[s0:s1].data_ptr())
    return T, pi, act != 0, na, n_iter, err, done == 1


def estimate_markov_model(dtraj: Optional[Tensor] = None, lag: Optional[int] = None, nstates: Optional[int] = None, *, counts=None,
                          reversible: bool = True, maxiter: int = 1_000_000, maxerr: float = 1e-8) -> MarkovModel:
    """The reversible maximum-likelihood Markov model of ``dtraj`` [n] or [S, n] (integer labels, counted by ``tica.transition_counts(dtraj,
    lag, nstates)``) or of ``counts=`` [ns, ns] or [S, ns, ns] (``lag`` is then only recorded, for ``timescales``); a leading S gives S
    independent models and every field a leading S.  ``maxiter`` steps at most; ``maxerr < 0`` never stops early.  On the device nothing is
    read back.  ``reversible=False`` raises ``NotImplementedError``."""
    if not reversible:
        raise NotImplementedError("only the reversible maximum-likelihood estimate (pyemma's default) is implemented")
    maxiter, maxerr = int(maxiter), float(maxerr)
    if maxiter < 0 or maxerr != maxerr:
        raise ValueError(f"maxiter = {maxiter} must not be negative and maxerr = {maxerr} must be a number")
    if (dtraj is None) == (counts is None):
        raise TypeError("estimate_markov_model takes dtraj, lag, nstates or counts=, not both")
    if counts is None:
        if lag is None or nstates is None:
            raise TypeError("estimate_markov_model(dtraj, lag, nstates): lag and nstates are needed to count")
        c = _tica.transition_counts(dtraj, lag, nstates)
        last_path["transition_counts"] = _tica.last_path["transition_counts"]
    else:
        c = _as_counts(counts)
        if nstates is not None and int(nstates) != c.shape[-1]:
            raise ValueError(f"nstates = {nstates} but counts is {tuple(c.shape)}")
    v = (c if c.dim() == 3 else c[None])
    dev = v.device
    if fused_applies(v):
        res, path = _estimate_device(v.contiguous(), maxiter, maxerr), "fused"
    else:
        host = _lib.to_host(v.long())
        act = np.stack([_active_numpy(m) for m in host])
        out = [_estimate_numpy(m, a, maxiter, maxerr) for m, a in zip(host, act)]
        cols = (np.stack([o[3] for o in out]), np.stack([o[4] for o in out]), act, act.sum(axis=1).astype(np.int32),
                np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.float64), np.array([o[2] for o in out], dtype=bool))
        res, path = tuple(_lib.to_device(a, dev) for a in cols), "torch"
    last_path["estimate_markov_model"] = path
    T, pi, act, na, n_iter, err, conv = res if c.dim() == 3 else tuple(r[0] for r in res)
    return MarkovModel(T, pi, act, na, c, n_iter, err, conv, None if lag is None else int(lag), path)


# ---- PCCA+ by the inner simplex algorithm (host side) ----
def pcca_assignments(T, pi, m: int) -> Tuple[np.ndarray, np.ndarray]:
    """T [na, na], pi [na] (a reversible model on its active set, ``MarkovModel.restricted``), m -> (memberships chi float64 [na, m],
    assignments int64 [na]): the inner simplex algorithm of PCCA+ (Deuflhard and Weber).  R [na, m] = the m dominant right eigenvectors of
    T from the symmetrised matrix ``D^{1/2} T D^{-1/2}`` (pi-orthonormal, the first column exactly ones); the representatives ``idx``: the row
    of largest norm, then repeatedly the row farthest from the span of the chosen ones (Gram-Schmidt on ``R - R[idx_0]``); ``chi = R
    R[idx]^{-1}``: rows sum to one and ``chi[idx]`` is the identity; the assignment is the row's argmax, the lowest index on a tie.  pyemma's
    Nelder-Mead refinement of the rotation is not reproduced."""
    T, pi = np.asarray(T, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    na, m = T.shape[0], int(m)
    if T.shape != (na, na) or pi.shape != (na,):
        raise ValueError(f"expected T [na, na] and pi [na], got {T.shape} and {pi.shape}")
    if not 1 <= m <= na:
        raise ValueError(f"m = {m} metastable sets of {na} active states")
    _, V, d = _symmetrised_eigh(T, pi)
    R = V[:, :m] / d[:, None]
    R[:, 0] = 1.0  # (the eigenvector of eigenvalue 1 is sqrt(pi) up to its sign)
    idx = [int(np.argmax((R * R).sum(axis=1)))]
    Y = R - R[idx[0]]
    for _ in range(1, m):
        norms = np.sqrt((Y * Y).sum(axis=1))
        far = int(np.argmax(norms))
        idx.append(far)
        u = Y[far] / norms[far]
        Y = Y - np.outer(Y @ u, u)
    chi = R @ np.linalg.inv(R[idx])
    return chi, np.argmax(chi, axis=1)


# ---- the Markov-state block of analyze_trajectory ----
def markov_state_block(ref_y: Tensor, traj_y: Tensor, centers, *, metastable_assignments=None, nstates: int = 10, lag: int = 1000, msm_lag: int = 10,
                       traj_msm: bool = True) -> Dict[str, Tensor]:
    """The Markov-state block of ``analyze_trajectory`` (eval_peptide.py:245-288) from the projected reference ``ref_y`` [n, d], the projected
    trajectory ``traj_y`` [m, d] and the microstate ``centers`` [k, d]: the microstate labels of the reference (``assign_centers``), the
    microstate model at ``lag``, its ``metastable_assignments`` [k] (those given - e.g. pyemma's - else :func:`pcca_assignments` into
    ``nstates`` sets; a microstate outside the active set gets -1), both coarse label series (``assign_centers(state_map=)``), the coarse
    model at ``lag`` and the trajectory's model at ``msm_lag`` (``traj_msm=False`` leaves it out, as ``cfg.no_traj_msm``).

    Returns ``ref_metastable_probs`` / ``traj_metastable_probs`` float64 [nstates], ``msm_transition_matrix`` [nstates, nstates], ``msm_pi``
    [nstates], ``traj_transition_matrix``, ``traj_pi`` and ``metastable_assignments`` int32 [k], on ref_y's device.  With assignments given
    nothing is read back; without them the one read is the microstate model going into the host PCCA."""
    nstates, lag, msm_lag = int(nstates), int(lag), int(msm_lag)
    dev = ref_y.device
    k = int(centers.shape[0])
    paths = []

    def model(dtraj, at, ns):
        mod = estimate_markov_model(dtraj, at, ns)
        paths.extend((_tica.last_path["transition_counts"], mod.path))
        return mod

    def coarse(y, smap):
        labels, occ = _tica.assign_centers(y, centers, state_map=smap, nstates=nstates)
        paths.append(_tica.last_path["assign_centers"])
        return labels, occ.double() / torch.full((), float(y.shape[0]), dtype=torch.float64, device=dev)  # (a true division: a scalar divisor is multiplied by its inverse on the GPU)

    micro, _ = _tica.assign_centers(ref_y, centers)
    paths.append(_tica.last_path["assign_centers"])
    msm = model(micro, lag, k)
    if metastable_assignments is None:
        A, T, pi = msm.restricted()
        if len(A) < nstates:
            raise ValueError(f"the microstate model has {len(A)} active states: no {nstates} metastable sets")
        full = np.full(k, -1, dtype=np.int32)
        full[A] = pcca_assignments(T, pi, nstates)[1]
        smap = _lib.to_device(full, dev)
    else:
        smap = (metastable_assignments.detach() if torch.is_tensor(metastable_assignments) else torch.as_tensor(np.asarray(metastable_assignments)))
        smap = smap.to(device=dev, dtype=torch.int32)
        if tuple(smap.shape) != (k,):
            raise ValueError(f"metastable_assignments must be [{k}], got {tuple(smap.shape)}")
    ref_d, ref_p = coarse(ref_y, smap)
    traj_d, traj_p = coarse(traj_y, smap)
    cmsm = model(ref_d, lag, nstates)
    out = {"ref_metastable_probs": ref_p, "traj_metastable_probs": traj_p, "msm_transition_matrix": cmsm.transition_matrix, "msm_pi": cmsm.pi,
           "metastable_assignments": smap}
    if traj_msm:
        tmsm = model(traj_d, msm_lag, nstates)
        out["traj_transition_matrix"], out["traj_pi"] = tmsm.transition_matrix, tmsm.pi
    last_path["markov_state_block"] = "fused" if set(paths) == {"fused"} else "torch"
    return out
