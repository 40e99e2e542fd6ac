"""The rest of ``model_step``: the losses ``Loss.forward`` of the reference's trajectory models computes behind the SI term when
``calc_additional_losses`` is set (second_stage/md17.py:194-257, nba.py:266-330, pedestrian.py:254-318 - the same code three times).

  geom_loss_sums, geom_losses   <- MaskedMSELoss, MaskedNormLoss, InterDistanceLoss (modules/losses.py:5-13, 27-34, 126-134) in two
                                   launches of liblamslide_hip.so (``lsl_geom_loss_sums`` / ``lsl_geom_loss_final``, csrc/k_geomloss.hip.h):
                                   no ``torch.cdist`` matrix, no atomics, a frame's sums have the same bits in any batch or shard
  Loss                          <- the three ``Loss`` classes, as a ``_target_`` drop-in: the device form when it applies, otherwise the
                                   given loss modules (or torch restatements of the three defaults) exactly as the reference calls them

The peptide ``Loss`` (frame-local, torsion and atom37 terms, second_stage/peptide.py) is ``PeptideLoss`` of peptide_loss.py.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from .transport import ModelType

SUM_COLUMNS = ("s_mse", "s_norm", "n", "s_pair", "n_pair")


def _frames(pred: Tensor, target: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """[..., A, D] / [..., A] -> contiguous float32 [F, A, D] x 2 and uint8 [F, A] on pred's device (``si_reduce`` refuses what is not
    contiguous; these inputs come out of rearranges and slices, so they are made contiguous instead)."""
    shape = lambda: (f"expected pred and target [..., A, D] and mask [..., A], got {tuple(pred.shape)}, {tuple(target.shape)} and "  # noqa: E731
                     f"{tuple(mask.shape)}")
    device = lambda: (f"Expected all tensors to be on the same device, pred is on {pred.device}, target on {target.device}, "  # noqa: E731
                      f"mask on {mask.device}")
    if pred.dim() < 2:
        raise ValueError(shape())
    lead, (A, D) = tuple(pred.shape[:-2]), pred.shape[-2:]
    return tuple(_lib.flat(x, lead, trailing, dtype, pred.device, shape, device)
                 for x, trailing, dtype in ((pred, (A, D), torch.float32), (target, (A, D), torch.float32), (mask, (A,), torch.uint8)))


def native_shape(A: int, D: int) -> bool:
    """Whether ``lsl_geom_loss_sums`` covers [.., A, D]: both positions and the mask of one frame in LDS."""
    return 1 <= A <= _lib.GEOM_MAX_A and 1 <= D <= _lib.GEOM_MAX_D


@torch.no_grad()
def geom_loss_sums(pred: Tensor, target: Tensor, mask: Tensor) -> Tensor:
    """float32 [F, 5]: per frame (s_mse, s_norm, n, s_pair, n_pair) of ``lsl_geom_loss_sums`` (include/lsl_api.h) for pred / target
    [..., A, D] and mask [..., A] (nonzero = real entity), leading axes flattened to F frames.  Rows of different shards may be concatenated
    and finished by ``geom_losses(sums=...)``.  GPU only; A > 2048 or D > 4 raise ``ValueError``."""
    if not pred.is_cuda:
        raise RuntimeError("geom_loss_sums runs on the GPU (HIP kernel); there is no CPU fallback")
    p, t, m = _frames(pred, target, mask)
    F_, A, D = p.shape
    if F_ == 0:
        raise ValueError("no frames")
    sums = torch.empty(F_, 5, dtype=torch.float32, device=p.device)
    _lib.call(p.device, "lsl_geom_loss_sums", p.data_ptr(), t.data_ptr(), m.data_ptr(), F_, A, D, sums.data_ptr())
    return sums


@torch.no_grad()
def geom_losses(pred: Optional[Tensor] = None, target: Optional[Tensor] = None, mask: Optional[Tensor] = None, *,
                sums: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """{"pos_loss", "dist", "inter_dist_loss"} as 0-dim float32 tensors: the reference's MaskedMSELoss, MaskedNormLoss and
    InterDistanceLoss of (pred, target, mask), or of ``sums`` [F, 5] from :func:`geom_loss_sums`.  The frames are added in index order in
    fp64 and each quotient is rounded once; a batch without a real entity gives NaN like the reference."""
    out = _lib.loss_from_sums("geom_losses", "lsl_geom_loss_final", (5,), 3, sums, (pred, target, mask), (),
                              lambda: geom_loss_sums(pred, target, mask), "(pred, target, mask)")
    return {"pos_loss": out[0], "dist": out[1], "inter_dist_loss": out[2]}


# ---- torch restatements of the three default modules (modules/losses.py), called on the reference's flattened layouts ----
def masked_mse(input: Tensor, target: Tensor, mask: Tensor) -> Tensor:  # [(B T L), D] x 2, [(B T L)]
    return (((input - target) ** 2).mean(dim=1) * mask).sum() / mask.sum()


def masked_norm(input: Tensor, target: Tensor, mask: Tensor) -> Tensor:  # [(B T L), D] x 2, [(B T L)]
    return (torch.norm(input - target, dim=-1) * mask).sum() / mask.sum()


def inter_distance(preds: Tensor, targets: Tensor, mask: Tensor) -> Tensor:  # [(B T), L, D] x 2, [(B T), L]
    diag_att = mask.unsqueeze(-1) * mask.unsqueeze(-2)
    dist = (torch.cdist(preds, preds) - torch.cdist(targets, targets)) * diag_att
    return (dist ** 2).sum() / diag_att.sum()


_DEFAULTS = {"loss_pos": ("MaskedMSELoss", masked_mse), "loss_inter_dist": ("InterDistanceLoss", inter_distance),
             "loss_norm": ("MaskedNormLoss", masked_norm)}


def _is_default(module: Optional[nn.Module], name: str) -> bool:
    if module is None:
        return True
    if type(module).__name__ != name or not isinstance(module, nn.Module):
        return False
    return next(module.parameters(), None) is None and next(module.buffers(), None) is None


class Loss(nn.Module):
    """Drop-in for ``src.models.composites.second_stage.{md17,nba,pedestrian}.Loss`` (``model.loss._target_=lam_slide_amd.Loss``): same
    keywords, same ``forward(model, batch) -> (losses, pred_latent)``, same keys, same arithmetic of ``losses["loss"]``.  ``None`` for a
    loss module means the reference's default (MaskedMSELoss / InterDistanceLoss / MaskedNormLoss).

    ``last_path`` says what computed the three geometry losses of the last call: "fused" (``geom_losses``: two HIP launches) when the
    decoded and the target positions are float32 on the GPU, nothing requires grad, A <= 2048 and D <= 4, and every loss module is ``None`` or a
    parameter-free instance named like its default; "generic" (the modules themselves, torch) otherwise - training with gradients,
    CPU tensors, a Huber variant, ...; ``None`` when ``calc_additional_losses`` is off."""

    def __init__(self, weight_si_loss: float = 1.0, weight_pos_loss: float = 0.0, weight_inter_dist_loss: float = 0.0,
                 weight_norm_loss: float = 0.0, loss_pos: Optional[nn.Module] = None, loss_inter_dist: Optional[nn.Module] = None,
                 loss_norm: Optional[nn.Module] = None, calc_additional_losses: bool = False) -> None:
        super().__init__()
        self.weight_si_loss = weight_si_loss
        self.weight_pos_loss = weight_pos_loss
        self.weight_inter_dist_loss = weight_inter_dist_loss
        self.weight_norm_loss = weight_norm_loss  # (stored and never used, as in the reference)
        self.loss_pos = loss_pos
        self.loss_inter_dist = loss_inter_dist
        self.loss_norm = loss_norm
        self.calc_additional_losses = calc_additional_losses
        self.last_path: Optional[str] = None

    def default_modules(self) -> bool:
        return all(_is_default(getattr(self, attr), name) for attr, (name, _) in _DEFAULTS.items())

    def fused_applies(self, pred_pos: Tensor, target_pos: Tensor) -> bool:
        # (tensors on two GPUs stay on this path: ``_frames`` raises the reference-style device error)
        if not _lib.device_form(pred_pos, target_pos, same_device=False) or pred_pos.dim() < 2:
            return False
        return native_shape(int(pred_pos.shape[-2]), int(pred_pos.shape[-1])) and self.default_modules()

    def _call(self, attr: str, *args: Tensor) -> Tensor:
        module = getattr(self, attr)
        return _DEFAULTS[attr][1](*args) if module is None else module(*args)

    def forward(self, model: nn.Module, batch: Dict[str, Tensor]):
        out = model.si.training_losses(model=model, x1=batch["x1"], model_kwargs=batch["model_kwargs"])
        pred_latent = out["pred"]
        si_loss = out["loss"].mean()
        losses = {"si_loss": si_loss, "loss": si_loss * self.weight_si_loss}
        self.last_path = None
        if self.calc_additional_losses:
            assert model.si.model_type == ModelType.DATA, "Additional losses are currently only supported for DATA model"
            pred_latent, entities = (x.reshape(x.shape[0] * x.shape[1], *x.shape[2:]) for x in (pred_latent, batch["entities"]))
            pred = model.decode(pred_latent, entities)
            pred_pos, target_pos, mask = pred["pos"], batch["pos"], batch["attention_mask"]  # [B, T, L, D] x 2, [B, T, L]
            if self.fused_applies(pred_pos, target_pos):
                self.last_path = "fused"
                geo = geom_losses(pred_pos, target_pos, mask)
                pos_loss, dist, inter_dist_loss = geo["pos_loss"], geo["dist"], geo["inter_dist_loss"]
            else:
                self.last_path = "generic"
                D = pred_pos.shape[-1]
                mask_flat = mask.reshape(-1)
                pos_loss = self._call("loss_pos", pred_pos.reshape(-1, D), target_pos.reshape(-1, D), mask_flat)
                dist = self._call("loss_norm", pred_pos.reshape(-1, D), target_pos.reshape(-1, D), mask_flat)
                frames = lambda x: x.reshape(x.shape[0] * x.shape[1], *x.shape[2:])  # noqa: E731
                inter_dist_loss = self._call("loss_inter_dist", frames(pred_pos), frames(target_pos), frames(mask))
            losses["pos_loss"] = pos_loss
            losses["inter_dist_loss"] = inter_dist_loss
            losses["dist"] = dist
            losses["loss"] = losses["loss"] + self.weight_pos_loss * pos_loss
            losses["loss"] = losses["loss"] + self.weight_inter_dist_loss * inter_dist_loss
        return losses, pred_latent
