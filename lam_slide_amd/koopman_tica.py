"""Koopman-reweighted TICA on wide feature tables, on the device: ``run_tica`` of the peptide validation (utils/tica_utils.py:42-48) over
``structure_stats.tica_features`` - every pair distance of the C / N / S atoms plus sin / cos of phi, psi and omega, 300 .. 1344 columns for
a tetrapeptide, past the F <= 128 of ``tica.lagged_moments`` / ``TicaModel.transform``.

  weighted_moments    <- sw = sum w_t, sx = sum w_t x_t, sy = sum w_t x_{t+lag}, xx = sum w_t x_t x_t^T, yy = sum w_t x_{t+lag} x_{t+lag}^T,
                         xy = sum w_t x_t x_{t+lag}^T over t < m = n - lag, float64 (``lsl_weighted_moments``, 129 <= F <= 2048)
  koopman_weights     <- ``KoopmanWeightingEstimator(lagtime).fit(x).fetch_model()``: ``KoopmanWeights(u, const)``, w_t = x_t . u + const
                         (``lsl_affine_weights``)
  weighted_covariances, model_from_moments
                      <- the reversible estimator's mean, C0 and C_lag from weighted moments; the model from them
  run_tica            <- ``TICA(lagtime, dim).fit_fetch((x[:-lag], x[lag:], weights))``: a :class:`WideTicaModel`
  WideTicaModel       <- ``TicaModel`` itself: its ``transform`` takes 129 <= F <= 2048 and up to 64 output columns on the device
                         (``lsl_project_wide``); ``tica_histograms`` / ``tica_jsd`` work with it unchanged

The estimator, as mathematics (m = n - lag rows x_t, their partners y_t = x_{t+lag}).

  1. Unweighted, non-reversible moments, no Bessel correction: mu0 = sx / m, mut = sy / m, C00 = xx / m - mu0 mu0^T, C0t = xy / m - mu0 mut^T.
  2. C00 = V diag(s) V^T (symmetric eigendecomposition); eigenvalues with |s| <= epsilon are dropped; R = V diag(s^-1/2), each column's sign
     set so that its entry of largest magnitude is positive.  R^T C00 R = I on the kept subspace.
  3. The Koopman matrix in the whitened basis extended by the constant function: K = [[R^T C0t R, 0], [(mut - mu0)^T R, 1]].
  4. Its left eigenvector for the eigenvalue 1, scaled so that its last component is 1: [v, 1] with (I - (R^T C0t R)^T) v = R^T (mut - mu0).
     deeptime takes "the eigenvector of the largest eigenvalue" of K^T; that is this vector whenever the spectral radius of the upper block
     is below 1 (the upper block's eigenvalues are K's other eigenvalues), which holds for a stationary series up to sampling noise.  Here the
     vector is DEFINED by the linear system - a deliberate deviation, stated so that the result does not depend on which of two near-equal
     eigenvalues a LAPACK call lists first; a singular system raises.
  5. u = R v, const = 1 - mu0 . u; the weights w_t = x_t . u + const have mean exactly 1 over the m rows, may be negative, and make every
     kept whitened direction chi stationary: sum_t w_t (chi(y_t) - chi(x_t)) = 0.
  6. Weighted, reversible moments: mu = (sx + sy) / 2 sw, C0 = (xx + yy) / 2 sw - mu mu^T, Ct = (xy + xy^T) / 2 sw - mu mu^T.
  7. ``tica.solve_tica(C0, Ct, epsilon)``, dim = min(dim, rank), the kinetic map as ``TicaModel``.

Data movement: the moments stay on the device; per fit two F x F matrices (and two F vectors) go to the host twice - (C00, C0t) for steps 2-5,
(C0, Ct) for step 7 - and u, the mean and W come back.  Those copies synchronise; everything else is enqueued only.

The device form is liblamslide_hip.so (csrc/k_wtica.hip.h).  The dispatch rule is ``torsion_stats.fused_applies``: float32 tensors on the
GPU, nothing requires grad, a native shape; anything else takes a torch float64 restatement with the same outputs.  ``last_path[name]``
tells which of the two ("fused" / "torch") ran last.

deeptime was not available where this was written: the estimator above is checked against a brute-force numpy / scipy oracle, parity with a
live deeptime was NOT checked.  A model deeptime fitted enters through ``TicaModel.from_arrays`` / ``WideTicaModel.from_arrays``."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import tica as _tica
from .tica import TicaModel, solve_tica
from .torsion_stats import fused_applies

last_path: Dict[str, str] = {}
# the native form of lsl_weighted_moments / lsl_project_wide, the rows of a segment, the roundings on the longest path to one entry of the moments
MIN_F, MAX_F, PROJ_MAX_D, WMOM_SEG, WMOM_CHAIN = _lib.WMOM_MIN_F, _lib.WMOM_MAX_F, _lib.WPROJ_MAX_D, _lib.WMOM_SEG, _lib.WMOM_CHAIN


_to_host, _to_device = _lib.to_host, _lib.to_device  # the documented synchronising copies of a fit, exempt from the sync debug mode
TicaModel.path_logs.append(last_path)  # (``last_path["transform"]`` is written here as in ``tica``)
WideTicaModel = TicaModel  # one class: ``transform`` chooses lsl_project or lsl_project_wide from (F, dim)


# ---- a. weighted lagged moments ----
def _wmom_torch(x: Tensor, lag: int, w: Optional[Tensor]):
    v = x.double()
    m = v.shape[0] - lag
    a, b = v[:m], v[lag:]
    if w is None:
        wa, wb, sw = a, b, torch.full((), float(m), dtype=torch.float64, device=v.device)
    else:
        w = w.double()
        wa, wb, sw = a * w[:, None], b * w[:, None], w.sum()
    return sw, wa.sum(dim=0), wb.sum(dim=0), wa.T @ a, wb.T @ b, wa.T @ b


def weighted_moments(x: Tensor, lag: int, weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """x [n, F], 1 <= lag < n, weights float64 [m] on x's device (None: all ones), m = n - lag -> (sw [], sx [F], sy [F], xx [F, F],
    yy [F, F], xy [F, F]), float64 on x's device: the sums over t < m of w_t, w_t x_t, w_t x_{t+lag}, w_t x_t x_t^T,
    w_t x_{t+lag} x_{t+lag}^T, w_t x_t x_{t+lag}^T.

    The device form (``MIN_F <= F <= MAX_F``) scales one operand, ``p = w_t * float64(x_a)``, multiplies in float64 and adds by fused
    multiply-adds in ascending t within segments of ``WMOM_SEG`` rows, the segments in order within groups of 1024, the groups in order,
    time splits (a function of (n, lag, F) alone) in order: every entry within ``WMOM_CHAIN * 2^-53 * sum_t |w_t x_a x_b|`` of the exact
    sum, xx and yy bit-symmetric (a <= b is computed and mirrored), the bits a function of (x, w, n, lag, F) alone.  With F <= 128 and no
    weights the sums are ``tica.lagged_moments``' (sw = m); any other case runs the torch float64 restatement."""
    if x.dim() != 2:
        raise ValueError(f"expected x [n, F], got {tuple(x.shape)}")
    n, F = int(x.shape[0]), int(x.shape[1])
    lag = int(lag)
    if F < 1 or n < 2:
        raise ValueError(f"x {tuple(x.shape)}: at least one feature and two steps")
    if not 1 <= lag < n:
        raise ValueError(f"lag = {lag} outside 1..n-1 = {n - 1}: the window has n - lag rows")
    m = n - lag
    if weights is not None and (tuple(weights.shape) != (m,) or weights.dtype != torch.float64 or weights.device != x.device):
        raise ValueError(f"weights must be float64 [{m}] on {x.device}, got {weights.dtype} {tuple(weights.shape)} on {weights.device}")
    dev = x.device
    if fused_applies(x) and MIN_F <= F <= MAX_F and (weights is None or not (torch.is_grad_enabled() and weights.requires_grad)):
        xc = x.detach().contiguous()
        wc = None if weights is None else weights.detach().contiguous()
        need = _lib.load().lsl_weighted_moments_workspace_bytes(n, F, lag)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(1 + 2 * F + 3 * F * F, dtype=torch.float64, device=dev)
        _lib.call(dev, "lsl_weighted_moments", xc.data_ptr(), n, F, lag, None if wc is None else wc.data_ptr(), out.data_ptr(), ws.data_ptr(), need)
        mats = out[1 + 2 * F:].reshape(3, F, F)
        last_path["weighted_moments"] = "fused"
        return out[0], out[1:1 + F], out[1 + F:1 + 2 * F], mats[0], mats[1], mats[2]
    if weights is None and F <= _lib.MOM_MAX_F:
        res = _tica.lagged_moments(x, lag)
        last_path["weighted_moments"] = _tica.last_path["lagged_moments"]
        return (torch.full((), float(m), dtype=torch.float64, device=dev),) + tuple(res)
    last_path["weighted_moments"] = "torch"
    return _wmom_torch(x.detach(), lag, None if weights is None else weights.detach())


# ---- b. the Koopman weights ----
def solve_koopman(mu0, mut, C00, C0t, epsilon: float = 1e-6) -> Tuple[np.ndarray, float]:
    """Steps 2-5 of the module's estimator in numpy float64 on the host: (mu0 [F], mut [F], C00 [F, F], C0t [F, F]) -> (u [F], const).
    Raises ValueError when no eigenvalue of C00 passes ``epsilon``, when a kept one is negative, or when ``I - (R^T C0t R)^T`` is
    singular (the upper block has the eigenvalue 1: the stationary vector is not unique)."""
    mu0, mut = np.asarray(mu0, dtype=np.float64).reshape(-1), np.asarray(mut, dtype=np.float64).reshape(-1)
    C00, C0t = np.asarray(C00, dtype=np.float64), np.asarray(C0t, dtype=np.float64)
    F = mu0.size
    if mut.size != F or C00.shape != (F, F) or C0t.shape != (F, F):
        raise ValueError(f"expected mu0 [F], mut [F], C00 [F, F], C0t [F, F], got {mu0.shape}, {mut.shape}, {C00.shape}, {C0t.shape}")
    s, V = np.linalg.eigh((C00 + C00.T) / 2)
    keep = np.abs(s) > epsilon
    if not keep.any():
        raise ValueError(f"no eigenvalue of C00 above epsilon = {epsilon}")
    if (s[keep] < 0).any():
        raise ValueError(f"C00 has an eigenvalue {s[keep].min():.3e} below -epsilon: not a covariance matrix")
    R = V[:, keep] / np.sqrt(s[keep])
    top = np.abs(R).argmax(axis=0)
    R = R * np.where(R[top, np.arange(R.shape[1])] < 0, -1.0, 1.0)
    M = R.T @ C0t @ R
    A = np.eye(M.shape[0]) - M.T
    try:
        v = np.linalg.solve(A, R.T @ (mut - mu0))
    except np.linalg.LinAlgError as e:
        raise ValueError(f"the Koopman matrix has the eigenvalue 1 twice: no unique stationary vector ({e})") from None
    if not np.isfinite(v).all():
        raise ValueError("the Koopman matrix has the eigenvalue 1 twice: no unique stationary vector")
    u = R @ v
    return u, float(1.0 - mu0 @ u)


class KoopmanWeights:
    """``u`` [F] (numpy float64, on the host) and ``const``: the model of ``KoopmanWeightingEstimator`` - ``weights(x)[t] = x_t . u + const``."""

    def __init__(self, u, const: float) -> None:
        self.u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        self.const = float(const)
        self._on: dict = {}

    def weights(self, x: Tensor) -> Tensor:
        """x [rows, F] -> float64 [rows] on x's device: ``sum_f x[t, f] u[f]`` as a fused float64 chain over f ascending, ``const`` added
        last (``lsl_affine_weights``; F <= MAX_F on the device form)."""
        F = self.u.size
        if x.dim() != 2 or x.shape[1] != F or x.shape[0] < 1:
            raise ValueError(f"expected x [rows, {F}], got {tuple(x.shape)}")
        dev = x.device
        if dev not in self._on:
            self._on[dev] = _to_device(self.u, dev)
        u = self._on[dev]
        rows = int(x.shape[0])
        if fused_applies(x) and F <= MAX_F and rows < 2 ** 31:
            xc = x.detach().contiguous()
            w = torch.empty(rows, dtype=torch.float64, device=dev)
            _lib.call(dev, "lsl_affine_weights", xc.data_ptr(), rows, F, u.data_ptr(), self.const, w.data_ptr())
            last_path["weights"] = "fused"
            return w
        last_path["weights"] = "torch"
        return x.detach().double() @ u + self.const


def koopman_weights(x: Tensor, lag: int, epsilon: float = 1e-6) -> KoopmanWeights:
    """x [n, F] -> :class:`KoopmanWeights`: steps 1-5 of the module's estimator.  The unweighted moments and (mu0, mut, C00, C0t) on x's
    device, one copy of them to the host, :func:`solve_koopman` there."""
    sw, sx, sy, xx, yy, xy = weighted_moments(x, lag, None)
    last_path["koopman_weights"] = last_path["weighted_moments"]
    m = float(int(x.shape[0]) - int(lag))
    mu0, mut = sx / m, sy / m
    C00 = xx / m - mu0[:, None] * mu0[None, :]
    C0t = xy / m - mu0[:, None] * mut[None, :]
    F = int(x.shape[1])
    host = _to_host(torch.cat([torch.stack([C00, C0t]).reshape(-1), mu0, mut]))
    mats = host[:2 * F * F].reshape(2, F, F)
    u, const = solve_koopman(host[2 * F * F:2 * F * F + F], host[2 * F * F + F:], mats[0], mats[1], epsilon)
    return KoopmanWeights(u, const)


# ---- c. the reversible estimator and the model ----
def covariances_from_moments(moments) -> Tuple[Tensor, Tensor, Tensor]:
    """(sw, sx, sy, xx, yy, xy) -> (mean [F], C0 [F, F], Ct [F, F]): ``mean = (sx + sy) / 2 sw``, ``C0 = (xx + yy) / 2 sw - mean mean^T``,
    ``Ct = (xy + xy^T) / 2 sw - mean mean^T``, float64 on the moments' device.  Both matrices are bit-symmetric when xx and yy are."""
    sw, sx, sy, xx, yy, xy = moments
    two = 2.0 * sw
    mean = (sx + sy) / two
    mm = mean[:, None] * mean[None, :]
    return mean, (xx + yy) / two - mm, (xy + xy.T) / two - mm


def weighted_covariances(x: Tensor, lag: int, weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """x [n, F] -> (mean, C0, Ct) of the reversible estimator under the weights (None: all ones - then ``tica.tica_covariances``' values)."""
    out = covariances_from_moments(weighted_moments(x, lag, weights))
    last_path["weighted_covariances"] = last_path["weighted_moments"]
    return out


def model_from_moments(moments, lag: Optional[int] = None, dim: int = 40, epsilon: float = 1e-6, kinetic_map: bool = True) -> WideTicaModel:
    """Steps 6-7: the reversible covariances of (sw, sx, sy, xx, yy, xy) on their device, one copy of (C0, Ct, mean) to the host,
    ``solve_tica`` there, ``dim = min(dim, rank)``."""
    mean, C0, Ct = covariances_from_moments(moments)
    F = int(mean.shape[0])
    host = _to_host(torch.cat([torch.stack([C0, Ct]).reshape(-1), mean]))
    mats = host[:2 * F * F].reshape(2, F, F)
    lam, R = solve_tica(mats[0], mats[1], epsilon)
    return WideTicaModel(host[2 * F * F:], R, lam, min(int(dim), lam.size), kinetic_map, lag)


def run_tica(features: Tensor, lagtime: int = 500, dim: int = 40, epsilon: float = 1e-6, kinetic_map: bool = True) -> WideTicaModel:
    """features [n, F] -> :class:`WideTicaModel`: ``tica_utils.run_tica`` - the Koopman weights of the first m = n - lagtime rows
    (:func:`koopman_weights`), the weighted moments, the reversible estimator, ``solve_tica``, ``dim = min(dim, rank)``.  The two host
    eigenproblems (and the copies to and from them) are the only synchronising steps."""
    if features.dim() != 2:
        raise ValueError(f"expected features [n, F], got {tuple(features.shape)}")
    n, lag = int(features.shape[0]), int(lagtime)
    if not 1 <= lag < n:
        raise ValueError(f"lagtime = {lag} outside 1..n-1 = {n - 1}: the window has n - lagtime rows")
    if int(dim) < 1:
        raise ValueError(f"dim = {dim} must be positive")
    kw = koopman_weights(features, lag, epsilon)
    paths = {last_path["koopman_weights"]}
    w = kw.weights(features[:n - lag])
    paths.add(last_path["weights"])
    moments = weighted_moments(features, lag, w)
    paths.add(last_path["weighted_moments"])
    last_path["run_tica"] = "fused" if paths == {"fused"} else "torch"
    return model_from_moments(moments, lag, dim, epsilon, kinetic_map)
