"""k-means fitting on the device: S independent Lloyd problems ``y [S, n, d]`` -> ``centers [S, k, d]``.

  kmeans_fit      <- ``cluster_kmeans(k=100, max_iter=100, fixed_seed=137)`` of the peptide evaluation (modules/analysis.py:42-44: S = 1,
                     n ~ 10^6 projected reference frames) and ``KMeans(n_clusters=num_runs)`` of the ``post_process`` branch of the NBA /
                     pedestrian ``test_step`` (second_stage/nba.py:202-203, 228-229: one problem per agent over its K final frames)
  nearest_rows    <- ``dis.argmin(dim=1)`` of nba.py:230-233: the sample nearest each centre

The algorithm is fixed here as mathematics and checked against a numpy float64 restatement (tests/kmeans_oracle.py).
**Parity with a live pyemma or torch_kmeans was not checked**: neither their seeding streams nor their restart policies are reproduced, and
``init="kmeans++"`` draws its own stream.  Centres fitted elsewhere enter through ``tica.assign_centers(y, centers, ...)`` or ``init=``.

Per series: *assign* every row to the nearest centre (float64 differences, the sum over j ascending, centres ascending, strict ``<``: ties
to the lowest index; a row that holds a NaN gets -1 and takes no part in anything); *update* every centre to ``float32(sum / count)`` of
its rows, the float64 sum taken in ascending t within segments of ``SEG`` rows and the segments in order (an empty cluster keeps its bits);
the *inertia* J of an iteration is the sum of the winning squared distances of its assignment, against the centres before the update.  A
series is done after an iteration when no label changed, or ``rel_tol > 0`` and ``|J_prev - J| <= rel_tol J_prev`` from the second
iteration on, or ``center_tol > 0`` and ``sum (new - old)^2 <= center_tol^2``.  One last assignment against the final centres fills labels,
counts and inertia.

The device form is ``lsl_kmeans_step`` / ``lsl_kmeans_nearest_rows`` of liblamslide_hip.so (csrc/k_kmeans.hip.h): ``max_iter`` step calls
are enqueued with no host synchronisation, a per-series flag on the device stops a finished series, nothing is read back, no float atomics,
and a series has the same bits alone and inside any batch.  It runs for float32 tensors on the GPU when nothing requires grad and the shape
is native (``k <= MAX_K``, ``d <= MAX_D``, ``k d <= CELLS``); anything else runs a torch float64 restatement with the same outputs and
conventions, usable on the CPU.  ``last_path[name]`` tells which of the two ("fused" / "torch") ran last."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Union

import torch
from torch import Tensor

from . import _lib

MAX_K, MAX_D, CELLS = _lib.ASG_MAX_K, _lib.ASG_MAX_D, _lib.ASG_CELLS  # the centres of a series stay in LDS: the limits of assign_centers
SEG = _lib.KM_SEG  # segment g holds the rows [g * SEG, (g + 1) * SEG)
MAX_S = _lib.KM_MAX_S  # series of one library call; more are chunked

last_path: Dict[str, str] = {}


class KMeansResult(NamedTuple):
    """``centers`` float32 [(S,) k, d], ``labels`` int32 [(S,) n] (-1: a row that holds a NaN), ``counts`` int64 [(S,) k], ``inertia`` float64
    [(S)] (of the final centres), ``n_iter`` int32 [(S)] (Lloyd iterations done), ``converged`` bool [(S)] (a stopping rule held within
    ``max_iter``), all on y's device; ``path`` "fused" or "torch"."""
    centers: Tensor
    labels: Tensor
    counts: Tensor
    inertia: Tensor
    n_iter: Tensor
    converged: Tensor
    path: str


def segments(n: int) -> int:
    """The segment rule of the update: the number of segments of a series of n rows."""
    return -(-int(n) // SEG)


def native_shape(n: int, d: int, k: int) -> bool:
    """Whether ``lsl_kmeans_step`` covers (n, d, k)."""
    return 1 <= n < 2 ** 31 and 1 <= d <= MAX_D and 1 <= k <= MAX_K and k * d <= CELLS


# ---- seeding ----
def kmeanspp_indices(y: Tensor, u: Tensor) -> Tensor:
    """D^2 seeding from given uniform numbers: y [S, n, d], u float64 [S, k] in [0, 1) -> int64 [S, k] row indices.  The first pick is
    ``floor(u_0 n)``; pick i is ``searchsorted(cumsum(D^2), u_i total)`` with D^2 the float64 squared distance of every row to the nearest
    centre picked so far (a row that holds a NaN has weight 0).  torch operations on y's device; this is neither pyemma's nor
    torch_kmeans' stream."""
    S, n, _ = y.shape
    k = int(u.shape[1])
    v = y.detach().double()
    u = u.to(device=y.device, dtype=torch.float64)
    ar = torch.arange(S, device=y.device)
    idx = torch.empty(S, k, dtype=torch.int64, device=y.device)
    pick = torch.floor(u[:, 0] * n).long().clamp_(max=n - 1)
    idx[:, 0] = pick
    d2 = None
    for i in range(1, k):
        new = ((v - v[ar, pick][:, None, :]) ** 2).sum(dim=-1)
        new = torch.where(torch.isnan(new), torch.zeros_like(new), new)
        d2 = new if d2 is None else torch.minimum(d2, new)
        cum = torch.cumsum(d2, dim=1)
        pick = torch.searchsorted(cum, (u[:, i] * cum[:, -1])[:, None]).squeeze(1).clamp_(max=n - 1)
        idx[:, i] = pick
    return idx


def initial_centers(y: Tensor, k: int, init: Union[str, Tensor] = "kmeans++", seed: Optional[int] = None) -> Tensor:
    """y [S, n, d] -> float32-or-y's-dtype [S, k, d]: a tensor [S, k, d] or [k, d] as given; "stride": the rows ``floor(i n / k)``;
    "kmeans++": :func:`kmeanspp_indices` with k uniform numbers per series from a CPU ``torch.Generator`` seeded with ``seed`` (None: a
    fresh seed) - deterministic for a seed on one machine."""
    S, n, d = (int(x) for x in y.shape)
    if torch.is_tensor(init):
        c = init.detach().to(device=y.device, dtype=y.dtype)
        if c.dim() == 2:
            c = c[None].expand(S, -1, -1)
        if tuple(c.shape) != (S, k, d):
            raise ValueError(f"init must be [{S}, {k}, {d}] or [{k}, {d}], got {tuple(init.shape)}")
        return c.contiguous().clone()
    if init == "stride":
        idx = ((torch.arange(k, dtype=torch.int64) * n) // k).to(y.device)[None].expand(S, -1)
    elif init == "kmeans++":
        gen = torch.Generator()
        if seed is None:
            gen.seed()
        else:
            gen.manual_seed(int(seed))
        idx = kmeanspp_indices(y, torch.rand(S, k, generator=gen, dtype=torch.float64))
    else:
        raise ValueError(f"init = {init!r}: a tensor, \"stride\" or \"kmeans++\"")
    return torch.gather(y.detach(), 1, idx[:, :, None].expand(-1, -1, d)).contiguous()


# ---- the torch float64 restatement ----
def _assign_torch(v: Tensor, c: Tensor):
    """v [S, n, d], c [S, k, d] float64 -> (labels int64 [S, n], -1 for a NaN row; the winning squared distances [S, n], 0 for a NaN row)."""
    S, n, d = v.shape
    k = c.shape[1]
    step = max(1, (1 << 22) // max(1, S * k))
    labs, best = [], []
    for r0 in range(0, n, step):
        w = v[:, r0:r0 + step]
        dist = torch.zeros(S, w.shape[1], k, dtype=torch.float64, device=v.device)
        for j in range(d):  # (j ascending, as the kernel and the oracle)
            diff = w[:, :, j, None] - c[:, None, :, j]
            dist = dist + diff * diff
        m, i = dist.min(dim=2)
        nan = torch.isnan(w).any(dim=2)
        labs.append(torch.where(nan, torch.full_like(i, -1), i))
        best.append(torch.where(nan, torch.zeros_like(m), m))
    return torch.cat(labs, dim=1), torch.cat(best, dim=1)


def _sums_torch(v: Tensor, labels: Tensor, k: int):
    """The update's sums [S, k, d] float64 (segments of SEG rows added in order) and counts int64 [S, k]."""
    S, n, d = v.shape
    flat = torch.where(labels >= 0, labels + torch.arange(S, device=v.device)[:, None] * k, torch.full_like(labels, S * k))  # (S k: a dump row)
    sums = torch.zeros(S * k + 1, d, dtype=torch.float64, device=v.device)
    for a in range(0, n, SEG):
        part = torch.zeros_like(sums)
        part.index_add_(0, flat[:, a:a + SEG].reshape(-1), v[:, a:a + SEG].reshape(-1, d))
        sums = sums + part
    counts = torch.bincount(flat.reshape(-1), minlength=S * k + 1)[:S * k].reshape(S, k)
    return sums[:S * k].reshape(S, k, d), counts


def _fit_torch(y: Tensor, c0: Tensor, max_iter: int, rel_tol: float, center_tol: float):
    v = y.detach().double()
    S, n, d = v.shape
    k = c0.shape[1]
    dev = v.device
    centers = c0.detach().float().clone()
    labels = torch.full((S, n), -2, dtype=torch.int64, device=dev)
    done = torch.zeros(S, dtype=torch.bool, device=dev)
    it = torch.zeros(S, dtype=torch.float64, device=dev)
    J = torch.zeros(S, dtype=torch.float64, device=dev)
    for _ in range(max_iter):
        if not v.is_cuda and bool(done.all()):
            break  # (on the CPU the test costs nothing; a finished series is left alone either way)
        lab, best = _assign_torch(v, centers.double())
        Jn = best.sum(dim=1)
        changed = (lab != labels).sum(dim=1)
        sums, counts = _sums_torch(v, lab, k)
        newc = torch.where((counts > 0)[:, :, None], (sums / counts.clamp_min(1)[:, :, None].double()).float(), centers)
        shift = ((newc.double() - centers.double()) ** 2).sum(dim=(1, 2))
        act = ~done
        itn = it + 1
        stop = (changed == 0)
        if rel_tol > 0:
            stop = stop | ((itn >= 2) & ((J - Jn).abs() <= rel_tol * J))
        if center_tol > 0:
            stop = stop | (shift <= center_tol * center_tol)
        centers = torch.where(act[:, None, None], newc, centers)
        labels = torch.where(act[:, None], lab, labels)
        J, it = torch.where(act, Jn, J), torch.where(act, itn, it)
        done = done | (act & stop)
    lab, best = _assign_torch(v, centers.double())
    _, counts = _sums_torch(v, lab, k)
    return centers, lab.to(torch.int32), counts, best.sum(dim=1), it.to(torch.int32), done


# ---- the device form ----
def _fit_device(y: Tensor, c0: Tensor, max_iter: int, rel_tol: float, center_tol: float):
    S, n, d = (int(x) for x in y.shape)
    k = int(c0.shape[1])
    dev = y.device
    centers = c0.contiguous().clone()
    labels = torch.full((S, n), -2, dtype=torch.int32, device=dev)
    counts = torch.zeros(S, k, dtype=torch.int64, device=dev)
    state = torch.zeros(S, 4, dtype=torch.float64, device=dev)
    done = torch.zeros(S, dtype=torch.int32, device=dev)
    need = _lib.load().lsl_kmeans_workspace_bytes(min(S, MAX_S), n, d, k)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for s0 in range(0, S, MAX_S):
        s1 = min(S, s0 + MAX_S)
        args = (y[s0:s1].data_ptr(), s1 - s0, n, d, centers[s0:s1].data_ptr(), k, labels[s0:s1].data_ptr(), counts[s0:s1].data_ptr(),
                state[s0:s1].data_ptr(), done[s0:s1].data_ptr())
        for _ in range(max_iter):
            _lib.call(dev, "lsl_kmeans_step", *args, 1, rel_tol, center_tol, ws.data_ptr(), need)
        _lib.call(dev, "lsl_kmeans_step", *args, 0, rel_tol, center_tol, ws.data_ptr(), need)
    return centers, labels, counts, state[:, 1], state[:, 0].to(torch.int32), done != 0


def kmeans_fit(y: Tensor, k: int, *, init: Union[str, Tensor] = "kmeans++", max_iter: int = 100, rel_tol: float = 1e-5, center_tol: float = 0.0,
               seed: Optional[int] = None) -> KMeansResult:
    """Fit k centres to every series of y [n, d] or [S, n, d] (the leading axis of every result is dropped for a 2-D y).  ``init``: see
    :func:`initial_centers`; ``max_iter`` Lloyd iterations at most; ``rel_tol`` / ``center_tol``: 0 switches that stopping rule off.
    Nothing is read back from the device."""
    if y.dim() not in (2, 3):
        raise ValueError(f"expected y [n, d] or [S, n, d], got {tuple(y.shape)}")
    v = y.detach() if y.dim() == 3 else y.detach()[None]
    S, n, d = (int(x) for x in v.shape)
    k, max_iter, rel_tol, center_tol = int(k), int(max_iter), float(rel_tol), float(center_tol)
    if min(S, n, d) < 1 or k < 1:
        raise ValueError(f"y {tuple(y.shape)}, k = {k}: at least one series, one row, one coordinate and one centre")
    if max_iter < 0 or not rel_tol >= 0 or not center_tol >= 0:
        raise ValueError(f"max_iter = {max_iter}, rel_tol = {rel_tol}, center_tol = {center_tol}: none may be negative")
    c0 = initial_centers(v, k, init, seed)
    if _lib.device_form(v, c0) and native_shape(n, d, k):
        res, path = _fit_device(v.contiguous(), c0, max_iter, rel_tol, center_tol), "fused"
    else:
        res, path = _fit_torch(v, c0, max_iter, rel_tol, center_tol), "torch"
    last_path["kmeans_fit"] = path
    if y.dim() == 2:
        res = tuple(r[0] for r in res)
    return KMeansResult(*res, path)


def nearest_rows(y: Tensor, centers: Tensor) -> Tensor:
    """y [n, d] or [S, n, d], centers [k, d] or [S, k, d] -> int32 [(S,) k]: ``rows[s, c] = argmin_t sum_j (y[s, t, j] - centers[s, c, j])^2``
    (the arithmetic of the assignment; the lowest t on ties; rows that hold a NaN skipped; -1 when the series has no finite row)."""
    if y.dim() not in (2, 3) or centers.dim() != y.dim() or centers.shape[-1] != y.shape[-1] or (y.dim() == 3 and centers.shape[0] != y.shape[0]):
        raise ValueError(f"expected y [n, d] / centers [k, d] or y [S, n, d] / centers [S, k, d], got {tuple(y.shape)} and {tuple(centers.shape)}")
    v, c = (y.detach(), centers.detach()) if y.dim() == 3 else (y.detach()[None], centers.detach()[None])
    S, n, d = (int(x) for x in v.shape)
    k = int(c.shape[1])
    if min(S, n, d, k) < 1:
        raise ValueError(f"empty y {tuple(y.shape)} or centers {tuple(centers.shape)}")
    if _lib.device_form(v, c) and native_shape(n, d, k):
        vc, cc = v.contiguous(), c.contiguous()
        rows = torch.empty(S, k, dtype=torch.int32, device=v.device)
        for s0 in range(0, S, MAX_S):
            s1 = min(S, s0 + MAX_S)
            _lib.call(v.device, "lsl_kmeans_nearest_rows", vc[s0:s1].data_ptr(), s1 - s0, n, d, cc[s0:s1].data_ptr(), k, rows[s0:s1].data_ptr())
        last_path["nearest_rows"] = "fused"
    else:
        v64, c64 = v.double(), c.to(v.device).double()
        nan = torch.isnan(v64).any(dim=2)  # [S, n]
        inf = torch.full((), float("inf"), dtype=torch.float64, device=v.device)
        step = max(1, (1 << 22) // max(1, S * n))
        out = []
        for c0 in range(0, k, step):
            cc = c64[:, c0:c0 + step]
            dist = torch.zeros(S, n, cc.shape[1], dtype=torch.float64, device=v.device)
            for j in range(d):
                diff = v64[:, :, j, None] - cc[:, None, :, j]
                dist = dist + diff * diff
            out.append(torch.where(nan[:, :, None], inf, dist).argmin(dim=1))
        idx = torch.cat(out, dim=1)
        rows = torch.where(nan.all(dim=1)[:, None], torch.full_like(idx, -1), idx).to(torch.int32)
        last_path["nearest_rows"] = "torch"
    return rows if y.dim() == 3 else rows[0]
