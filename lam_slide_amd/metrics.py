"""The evaluation tail of the trajectory models: displacement errors of the decoded positions, on the device.

  displacement_rows     <- ``validation_step`` of md17 / NBA / pedestrian (second_stage/md17.py:82-86, nba.py:100-104, pedestrian.py:88-92):
                           ``norm(true - pred, dim=-1).mean(dim=(1, 2))`` and ``norm(true[:, -1] - pred[:, -1], dim=-1).mean(dim=1)``
                           over the future frames and ALL entities, per sample; and the same two numbers per agent
  displacement_errors   <- ``test_step`` of NBA / pedestrian (nba.py:182-225, pedestrian.py:170-212): best-of-``num_runs`` ADE / FDE of the
                           real agents (``attention_mask[:, -1]``), the two minima taken independently; md17's ``test_step``
                           (md17.py:157-169) is the mean of ``traj_ade`` / ``traj_fde`` over its K = 5 samples
  DisplacementMeter     <- ``on_test_epoch_end`` (nba.py:240-251) and the ``MeanMetric`` s of ``validation_step``: the epoch means,
                           accumulated on the device in float64
  displacement_errors(post_process=True)
                        <- the ``post_process`` branch of ``test_step`` (nba.py:202-203, 228-238; pedestrian.py:191, 217): k-means with
                           ``num_runs`` centres over the K final predicted frames of every agent (``kmeans.kmeans_fit``), the sample
                           nearest each centre (``kmeans.nearest_rows``), ``ades_post`` / ``fdes_post`` from the selection

The device form is two launches of liblamslide_hip.so (``lsl_disp_error_rows`` / ``lsl_disp_error_final``, csrc/k_disperr.hip.h): the
decoder's output [K, B, T, A, D] and the batch's positions [B, T, A, D] are read in place (no permute, no slice, no boolean index, no
host round trip), no atomics, every sum in an order fixed by (A, D, Tf): an agent's or a trajectory's error has the same bits in any
batch or shard.  It runs when the tensors are float32 on the GPU, nothing requires grad and 1 <= D <= 4; otherwise (CPU, D > 4, other
dtypes) a torch restatement of the cited lines runs, with the same outputs and the same NaN conventions.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib


def native_shape(D: int) -> bool:
    """Whether ``lsl_disp_error_rows`` covers [..., A, D] (any A >= 1; an agent's coordinates in registers)."""
    return 1 <= D <= _lib.DISP_MAX_D


def fused_applies(pred: Tensor, target: Tensor) -> bool:
    """The dispatch rule (``_lib.device_form``: float32 on one GPU, nothing requires grad) and a native shape."""
    return _lib.device_form(pred, target) and native_shape(int(pred.shape[-1]))


def _layout(pred: Tensor, target: Tensor, first_frame: int) -> Tuple[Tensor, int, int]:
    """pred as [K, B, T, A, D]; the first future frame of the target; the number of future frames."""
    if pred.dim() == 4:
        pred = pred.unsqueeze(0)
    if pred.dim() != 5 or target.dim() != 4:
        raise ValueError(f"expected pred [K, B, T, A, D] or [B, T, A, D] and target [B, T', A, D], got {tuple(pred.shape)} and {tuple(target.shape)}")
    K, B, T, A, D = pred.shape
    first_frame = int(first_frame)
    Tf = T - first_frame
    if first_frame < 0 or Tf < 1:
        raise ValueError(f"first_frame = {first_frame} leaves no future frame of T = {T}")
    if (target.shape[0], target.shape[2], target.shape[3]) != (B, A, D) or target.shape[1] not in (T, Tf):
        raise ValueError(f"target {tuple(target.shape)} is neither [B, T, A, D] = {(B, T, A, D)} nor [B, T - first_frame, A, D] = {(B, Tf, A, D)}")
    if min(K, B, A, D) < 1:
        raise ValueError(f"empty pred {tuple(pred.shape)}")
    return pred, (first_frame if target.shape[1] == T else 0), Tf


def _rows_torch(pred: Tensor, target: Tensor, first_frame: int, t0t: int, Tf: int) -> Tuple[Tensor, Tensor]:
    """The cited lines on [K, B, T, A, D] / [B, T', A, D] in the tensors' own dtype, on Tf frames from ``first_frame`` / ``t0t`` on."""
    err = torch.norm(target[None, :, t0t:t0t + Tf] - pred[:, :, first_frame:first_frame + Tf], dim=-1)  # [K, B, Tf, A]
    rows = torch.stack((err.mean(dim=2), err[:, :, -1]), dim=-1)                        # the rows of _compute_errors, before the minimum
    traj = torch.stack((err.mean(dim=(2, 3)), err[:, :, -1].mean(dim=2)), dim=-1)       # validation_step's ade / fde
    return rows, traj


@torch.no_grad()
def displacement_rows(pred: Tensor, target: Tensor, *, first_frame: int = 0) -> Tuple[Tensor, Tensor]:
    """(rows [K, B, A, 2], traj [K, B, 2]): per sample the (ADE, FDE) of every agent, and the unmasked means over all agents that
    ``validation_step`` logs, of frames ``first_frame:``.  pred [K, B, T, A, D] or [B, T, A, D] (K = 1) as the decoder left it; target
    the batch's full ``pos`` [B, T, A, D] (read from ``first_frame`` on) or the future frames alone [B, T - first_frame, A, D]."""
    pred, t0t, Tf = _layout(pred, target, first_frame)
    if not fused_applies(pred, target):
        return _rows_torch(pred, target, int(first_frame), t0t, Tf)
    K, B, T, A, D = pred.shape
    p, t = pred.detach().contiguous(), target.detach().contiguous()
    dev = p.device
    rows = torch.empty(K, B, A, 2, dtype=torch.float32, device=dev)
    traj = torch.empty(K, B, 2, dtype=torch.float32, device=dev)
    _lib.call(dev, "lsl_disp_error_rows", p.data_ptr(), t.data_ptr(), K, B, T, int(first_frame), t.shape[1], t0t, Tf, A, D, rows.data_ptr(),
              traj.data_ptr())
    return rows, traj


class DisplacementErrors:
    """What :func:`displacement_errors` returns.  ``ade`` / ``fde`` [B, A]: best-of-``num_runs``, NaN where the agent is masked out;
    ``traj_ade`` / ``traj_fde`` [K, B]: the unmasked per-sample means of ``validation_step``; ``totals`` float64 [5] = (sum of ``ade``,
    sum of ``fde``, number of real agents, sum of ``traj_ade[:num_runs]``, sum of ``traj_fde[:num_runs]``): totals of several batches
    or shards add before the division (:class:`DisplacementMeter`).  ``path`` is "fused" (two HIP launches) or "torch".  With
    ``post_process=True`` also ``ade_post`` / ``fde_post`` [B, A] (the minima over the samples nearest the ``num_runs`` k-means centres
    of the agent's final frames; NaN where masked), ``totals_post`` float64 [2] (their sums over the real agents), ``post_rows`` int32
    [B, A, num_runs] (the selected samples) and ``post_fit`` (the :class:`~lam_slide_amd.kmeans.KMeansResult`); None otherwise."""

    def __init__(self, ade: Tensor, fde: Tensor, traj_ade: Tensor, traj_fde: Tensor, totals: Tensor, agent_mask: Optional[Tensor], num_runs: int,
                 path: str) -> None:
        self.ade, self.fde, self.traj_ade, self.traj_fde, self.totals = ade, fde, traj_ade, traj_fde, totals
        self.agent_mask, self.num_runs, self.path = agent_mask, num_runs, path
        self.ade_post = self.fde_post = self.totals_post = self.post_rows = self.post_fit = None

    @property
    def n_trajectories(self) -> int:
        """How many trajectory means ``totals[3:]`` add (known from the shapes: no synchronisation)."""
        return self.num_runs * self.traj_ade.shape[1]

    def real(self) -> Tuple[Tensor, Tensor]:
        """(ADE, FDE) of the real agents, one row each in (scene, agent) order: what ``best_of_k_errors`` returns.  The boolean index
        makes this the only member that waits for the device."""
        if self.agent_mask is None:
            return self.ade.reshape(-1), self.fde.reshape(-1)
        keep = self.agent_mask.reshape(-1)
        return self.ade.reshape(-1)[keep], self.fde.reshape(-1)[keep]

    def real_post(self) -> Tuple[Tensor, Tensor]:
        """(``ade_post``, ``fde_post``) of the real agents, in the order of :meth:`real`."""
        if self.ade_post is None:
            raise ValueError("no post_process results: call displacement_errors(..., post_process=True)")
        if self.agent_mask is None:
            return self.ade_post.reshape(-1), self.fde_post.reshape(-1)
        keep = self.agent_mask.reshape(-1)
        return self.ade_post.reshape(-1)[keep], self.fde_post.reshape(-1)[keep]


def post_process_errors(rows: Tensor, finals: Tensor, num_runs: int, keep: Optional[Tensor] = None, post_kmeans: Optional[dict] = None,
                        centers: Optional[Tensor] = None):
    """The ``post_process`` selection (nba.py:228-238) from the per-sample rows.  rows [K, B, A, 2] (ADE, FDE of every sample and agent),
    finals [K, B, A, D] (the final predicted frame) -> (post [B, A, 2], totals_post float64 [2], sel int32 [B, A, num_runs], fit):
    ``kmeans_fit`` with ``num_runs`` centres over the K final frames of every agent (``post_kmeans``: its keyword arguments; or
    ``centers`` [B A, num_runs, D] fitted elsewhere, then ``fit`` is None), the sample nearest each centre, and the minimum of ADE and of
    FDE, each on its own, over the selected samples.  A gather and a ``min``: no synchronisation.  NaN for a masked agent."""
    from . import kmeans
    K, B, A, D = finals.shape
    yk = finals.detach().permute(1, 2, 0, 3).reshape(B * A, K, D).contiguous()
    fit = None
    if centers is None:
        fit = kmeans.kmeans_fit(yk, int(num_runs), **(post_kmeans or {}))
        centers = fit.centers
    sel = kmeans.nearest_rows(yk, centers.to(yk.dtype))  # [B A, R]
    per_agent = rows.permute(1, 2, 0, 3).reshape(B * A, K, 2)
    picked = torch.gather(per_agent, 1, sel.clamp_min(0).long()[:, :, None].expand(-1, -1, 2))  # [B A, R, 2]
    nan = torch.full((), float("nan"), dtype=rows.dtype, device=rows.device)
    picked = torch.where((sel >= 0)[:, :, None], picked, nan)
    post = picked.min(dim=1).values.reshape(B, A, 2)  # (torch.min keeps a NaN)
    if keep is not None:
        post = torch.where(keep[..., None], post, nan)
        kept = torch.where(keep[..., None], post, torch.zeros((), dtype=post.dtype, device=post.device))
    else:
        kept = post
    return post, kept.double().sum(dim=(0, 1)), sel.reshape(B, A, -1), fit


@torch.no_grad()
def displacement_errors(pred: Tensor, target: Tensor, agent_mask: Optional[Tensor] = None, *, first_frame: int = 0,
                        num_runs: Optional[int] = None, post_process: bool = False, post_kmeans: Optional[dict] = None) -> DisplacementErrors:
    """Best-of-``num_runs`` ADE / FDE per agent (the minima over the first ``num_runs`` of the K samples, each on its own; default all
    K), the per-sample trajectory means, and the float64 sums of both.  pred / target / first_frame as :func:`displacement_rows`;
    agent_mask [B, A] (``attention_mask[:, -1]``; nonzero = real agent) or None for all.  A NaN in any of the ``num_runs`` samples of
    an agent makes that agent's minimum NaN, like ``torch.min``.  ``post_process=True`` adds the reference's ``post_process`` branch
    (:func:`post_process_errors` over all K samples, ``post_kmeans`` = keyword arguments of ``kmeans_fit``: pass a ``seed`` for a
    repeatable seeding); the default leaves every other member as it is."""
    pred5, t0t, Tf = _layout(pred, target, first_frame)
    K, B, T, A, D = pred5.shape
    R = K if num_runs is None else int(num_runs)
    if not 1 <= R <= K:
        raise ValueError(f"num_runs = {R} outside 1..K = {K}")
    keep = None
    if agent_mask is not None:
        if tuple(agent_mask.shape) != (B, A):
            raise ValueError(f"agent_mask must be [B, A] = {(B, A)}, got {tuple(agent_mask.shape)}")
        if agent_mask.device != pred5.device:
            raise RuntimeError(f"Expected all tensors to be on the same device, pred is on {pred5.device}, agent_mask on {agent_mask.device}")
        keep = agent_mask if agent_mask.dtype == torch.bool else agent_mask != 0
    rows, traj = displacement_rows(pred5, target, first_frame=first_frame)
    if fused_applies(pred5, target):
        dev = rows.device
        m8 = None if keep is None else keep.contiguous().view(torch.uint8)
        agents = torch.empty(B, A, 2, dtype=torch.float32, device=dev)
        totals = torch.empty(5, dtype=torch.float64, device=dev)
        _lib.call(dev, "lsl_disp_error_final", rows.data_ptr(), traj.data_ptr(), None if m8 is None else m8.data_ptr(), K, R, B, A,
                  agents.data_ptr(), totals.data_ptr())
        path = "fused"
    else:
        agents = rows[:R].min(dim=0).values  # (torch.min keeps a NaN)
        real = torch.ones(B, A, dtype=torch.bool, device=rows.device) if keep is None else keep
        agents = torch.where(real[..., None], agents, torch.full((), float("nan"), dtype=agents.dtype, device=agents.device))
        kept = torch.where(real[..., None], agents, torch.zeros((), dtype=agents.dtype, device=agents.device)).double()
        totals = torch.cat((kept.sum(dim=(0, 1)), real.sum().double()[None], traj[:R].double().sum(dim=(0, 1))))
        path = "torch"
    res = DisplacementErrors(agents[..., 0], agents[..., 1], traj[..., 0], traj[..., 1], totals, keep, R, path)
    if post_process:
        post, res.totals_post, res.post_rows, res.post_fit = post_process_errors(rows, pred5[:, :, T - 1], R, keep, post_kmeans)
        res.ade_post, res.fde_post = post[..., 0], post[..., 1]
    return res


class DisplacementMeter:
    """The epoch means of the evaluation loops: ``update(result)`` adds a batch's ``totals`` into a float64 buffer on the result's
    device (no synchronisation), ``compute()`` divides once - the one place that waits for the device.  ``scale`` is the dataset's
    (``first_stage_model.hparams.scale``): the reference multiplies the errors by it before it averages.

    ``compute()`` -> {"ade", "fde"}: scale x the mean best-of-K ADE / FDE over all real agents of all batches (``on_test_epoch_end``);
    {"traj_ade", "traj_fde"}: scale x the mean over all trajectories of all batches of the unmasked means (the ``MeanMetric`` s of
    ``validation_step``; md17's ``test_step``); {"ade_post", "fde_post"}: scale x the means of the ``post_process`` errors over the real
    agents of the batches that carried them - present only when an update carried them.  Python floats; an empty meter gives NaN, like
    the mean of an empty tensor."""

    def __init__(self, scale: float = 1.0) -> None:
        self.scale = float(scale)
        self.reset()

    def reset(self) -> None:
        self.sums: Optional[Tensor] = None
        self.sums_post: Optional[Tensor] = None  # (sum of ade_post, sum of fde_post, real agents) of the updates that carried them
        self.n_trajectories = 0

    def update(self, result: DisplacementErrors) -> None:
        totals = result.totals.detach().to(torch.float64)
        self.sums = totals.clone() if self.sums is None else self.sums + totals.to(self.sums.device)
        self.n_trajectories += result.n_trajectories
        if getattr(result, "totals_post", None) is not None:
            post = torch.cat((result.totals_post.detach().to(torch.float64), totals[2:3].to(result.totals_post.device)))
            self.sums_post = post if self.sums_post is None else self.sums_post + post.to(self.sums_post.device)

    def compute(self) -> Dict[str, float]:
        nan = float("nan")
        if self.sums is None:
            return {"ade": nan, "fde": nan, "traj_ade": nan, "traj_fde": nan}
        if self.sums_post is None:
            s = self.sums.tolist()  # the one synchronisation
        else:
            s = torch.cat((self.sums, self.sums_post.to(self.sums.device))).tolist()
        n, nt = s[2], float(self.n_trajectories)
        out = {"ade": self.scale * s[0] / n if n else nan, "fde": self.scale * s[1] / n if n else nan,
               "traj_ade": self.scale * s[3] / nt if nt else nan, "traj_fde": self.scale * s[4] / nt if nt else nan}
        if self.sums_post is not None:
            out["ade_post"] = self.scale * s[5] / s[7] if s[7] else nan
            out["fde_post"] = self.scale * s[6] / s[7] if s[7] else nan
        return out
