"""First-stage validation on the MI355X: what ``first_stage/{md17,pedestrian,nba,peptide}.py`` of the reference run as ``model_step`` /
``validation_step`` - encode -> quant -> post_quant -> decode (every head) -> ``Loss`` - on the frozen autoencoder.

  Stage1Autoencoder               <- ``BackboneBase.forward / encode / decode`` (lightning_base.py:33-44) over a Stage1Encoder and a
                                     Stage1Decoder built from one state dict; ``prepare_inputs`` stays the caller's
  class_loss_sums, class_losses   <- MaskedCrossEntropyLoss (modules/losses.py:62-72) and nn.CrossEntropyLoss in two launches of
                                     liblamslide_hip.so (``lsl_class_loss_sums`` / ``lsl_class_loss_final``, csrc/k_classloss.hip.h): no float
                                     atomics, a frame's sums have the same bits in any batch or shard
  ClassMeter                      <- accuracy / precision / recall of ``validation_step`` (first_stage/nba.py:174-189) from a confusion matrix
                                     the same kernel accumulates on the device
  MD17Loss, PedestrianLoss,       <- the four first-stage ``Loss`` classes as ``_target_`` drop-ins: the device form of every term whose
  NBALoss, PeptideLoss               module is the default the YAMLs name, the given module (torch) for any other
"""
from __future__ import annotations

from typing import Callable, Dict, Mapping, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from . import _lib, losses as _geo, peptide_loss as _pep
from .decoder import Stage1Decoder
from .encoder import Stage1Encoder

MAX_K, IGNORE_INDEX = _lib.CLS_MAX_K, _lib.CLS_IGNORE  # the classes of one lsl_class_loss_sums call, the target of an ignored row
SUM_COLUMNS = ("s_ce", "n")


# ---- the autoencoder ----
class Stage1Autoencoder:
    """``BackboneBase`` of the reference (lightning_base.py:17-48) on the device, inference only: ``encode(batch)`` =
    quant(Encoder(prepare_inputs(batch), batch["entities"], mask)), ``decode(z, entities)`` = every head of Decoder(post_quant(z), entities),
    ``__call__(batch)`` = decode(encode(batch), batch["entities"]).  ``encoder`` / ``decoder`` are the keyword dicts of Stage1Encoder /
    Stage1Decoder (head counts and widths, ``act``, ``max_norm``); ``prepare_inputs(batch) -> x [F, A, dim_input]`` is the dataset-specific
    embedding of the first stage (typically ``first_stage.backbone.prepare_inputs``) and stays the caller's.  ``mask=False`` passes no
    entity mask to the encoder, as the peptide backbone does (first_stage/peptide.py:77-80).  ``output_shapes`` gives a head's last axis
    a shape: ``{"atom14_pos": (14, 3)}`` turns the peptide decoder's [F, R, 42] into the [F, R, 14, 3] its Loss reads.  ``shift`` /
    ``scale`` are the wrapper's hyper-parameters the Loss classes read (``dist = norm_loss * model.scale``)."""

    def __init__(self, state_dict: Dict[str, Tensor], *, encoder: dict, decoder: dict, prepare_inputs: Callable[[Dict[str, Tensor]], Tensor],
                 shift: float = 0.0, scale: float = 1.0, mask: bool = True, output_shapes: Optional[Mapping[str, Sequence[int]]] = None):
        sd = {k.replace("_orig_mod.", ""): v for k, v in state_dict.items()}
        sd = {(k[len("backbone."):] if k.startswith("backbone.") else k): v for k, v in sd.items()}
        heads = [k.split(".")[2] for k in sd if k.startswith("decoder.output_layers.") and k.endswith(".2.weight")]
        if not heads:
            raise KeyError("decoder.output_layers.*")
        dec_kw = dict(decoder)
        dec_kw.setdefault("output", "pos" if "pos" in heads else heads[0])
        self.encoder = Stage1Encoder(sd, **encoder)
        self.decoder = Stage1Decoder(sd, **dec_kw)
        self.prepare_inputs = prepare_inputs
        self.shift, self.scale, self.mask = shift, scale, bool(mask)
        self.output_shapes = {k: tuple(int(n) for n in v) for k, v in (output_shapes or {}).items()}

    @torch.no_grad()
    def encode(self, batch: Dict[str, Tensor]) -> Tensor:
        x = self.prepare_inputs(batch)
        return self.encoder.encode(x, batch["entities"], batch["attention_mask"] if self.mask else None)

    @torch.no_grad()
    def decode(self, z: Tensor, entities: Tensor) -> Dict[str, Tensor]:
        out = self.decoder.decode_heads(z, entities)
        for k, shape in self.output_shapes.items():
            if k in out:
                out[k] = out[k].reshape(*out[k].shape[:-1], *shape)
        return out

    def __call__(self, batch: Dict[str, Tensor]) -> Dict[str, Tensor]:
        return self.decode(self.encode(batch), batch["entities"])

    forward = __call__


# ---- class losses ----
def _rows(logits: Tensor, target: Tensor, mask: Optional[Tensor]) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """[..., A, K] / [..., A] -> contiguous float32 [F, A, K], int64 [F, A] and uint8 [F, A] (or None) on the logits' device."""
    shape = lambda: (f"expected logits [..., A, K], target [..., A] and mask [..., A] or None, got {tuple(logits.shape)}, "  # noqa: E731
                     f"{tuple(target.shape)} and {None if mask is None else tuple(mask.shape)}")
    device = lambda: (f"Expected all tensors to be on the same device, logits are on {logits.device}, target on {target.device}"  # noqa: E731
                      + ("" if mask is None else f", mask on {mask.device}"))
    if logits.dim() < 2:
        raise ValueError(shape())
    lead, (A, K) = tuple(logits.shape[:-2]), logits.shape[-2:]
    if target.is_floating_point() or target.dtype == torch.bool:
        raise ValueError(f"target must hold class indices (integers), got {target.dtype}")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"K = {K} outside the native form (1..{MAX_K} classes)")
    if A < 1 or logits.numel() == 0:
        raise ValueError("no rows")
    return tuple(None if x is None else _lib.flat(x, lead, trailing, dtype, logits.device, shape, device)
                 for x, trailing, dtype in ((logits, (A, K), torch.float32), (target, (A,), torch.int64), (mask, (A,), torch.uint8)))


def native_classes(K: int) -> bool:
    """Whether ``lsl_class_loss_sums`` covers K classes."""
    return 1 <= K <= MAX_K


@torch.no_grad()
def class_loss_sums(logits: Tensor, target: Tensor, mask: Optional[Tensor] = None, label_smoothing: float = 0.0,
                    confusion: Optional[Tensor] = None) -> Tensor:
    """float32 [F, 2]: per frame (s_ce, n) of ``lsl_class_loss_sums`` (include/lsl_api.h) for logits [..., A, K], target [..., A] (class
    indices; -100 = ignored) and mask [..., A] (nonzero = counted) or ``None``, leading axes flattened to F frames.  With a mask n counts the
    masked-in rows (MaskedCrossEntropyLoss), without one the rows whose target is not -100 (nn.CrossEntropyLoss).  A counted target outside
    0..K-1 makes its frame's two sums NaN.  ``confusion``: int64 [K, K] on the same device, added to in place (cell [target, argmax]).  Rows
    of different shards may be concatenated and finished by ``class_losses(sums=...)``.  GPU only; K > 128 raises ``ValueError``."""
    lg, tg, mk = _rows(logits, target, mask)
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError(f"label_smoothing = {label_smoothing} outside [0, 1)")
    F_, A, K = lg.shape
    if confusion is not None and (confusion.dtype != torch.int64 or tuple(confusion.shape) != (K, K) or not confusion.is_contiguous()
                                  or confusion.device != lg.device):
        raise ValueError(f"confusion must be a contiguous int64 [{K}, {K}] tensor on {lg.device}")
    if not lg.is_cuda:
        raise RuntimeError("class_loss_sums runs on the GPU (HIP kernel); there is no CPU fallback")
    sums = torch.empty(F_, 2, dtype=torch.float32, device=lg.device)
    _lib.call(lg.device, "lsl_class_loss_sums", lg.data_ptr(), tg.data_ptr(), None if mk is None else mk.data_ptr(), F_, A, K,
              float(label_smoothing), sums.data_ptr(), None if confusion is None else confusion.data_ptr())
    return sums


@torch.no_grad()
def class_losses(logits: Optional[Tensor] = None, target: Optional[Tensor] = None, mask: Optional[Tensor] = None, label_smoothing: float = 0.0,
                 confusion: Optional[Tensor] = None, *, sums: Optional[Tensor] = None) -> Tensor:
    """0-dim float32: MaskedCrossEntropyLoss(label_smoothing)(logits, target, mask) of the reference - or, without a mask,
    nn.CrossEntropyLoss(label_smoothing=...)(logits, target) - for logits [..., A, K], or of ``sums`` [F, 2] from :func:`class_loss_sums`.
    The frames are added in index order in fp64 and the quotient is rounded once; no counted row gives NaN like the reference."""
    return _lib.loss_from_sums("class_losses", "lsl_class_loss_final", (2,), 1, sums, (logits, target), (mask,),
                               lambda: class_loss_sums(logits, target, mask, label_smoothing, confusion), "(logits, target[, mask])")[0]


class ClassMeter:
    """Classification metrics of an epoch from a confusion matrix C [K, K] (rows = target, columns = argmax of the logits, lowest index
    among equal maxima) that ``lsl_class_loss_sums`` accumulates on the device with integer atomics.  ``update(logits, target, mask=None)``
    adds a batch (rows that are masked out, carry target -100 or hold a NaN logit are not counted); nothing synchronises with the host
    before ``compute()``, which returns device tensors:

        accuracy            = sum_c C[c, c] / sum_tp C[t, p]                  (micro)
        precision_per_class = C[c, c] / sum_t C[t, c],   precision = mean_c   (macro)
        recall_per_class    = C[c, c] / sum_p C[c, p],   recall    = mean_c   (macro)

    with 0 / 0 -> 0.  These are the textbook definitions; torchmetrics is not installed where this was written, so parity with a live
    ``torchmetrics.{Accuracy, Precision, Recall}`` (whose ``average`` default has changed between versions) was NOT checked.  AUROC needs
    the scores, not the argmax, and stays the caller's."""

    def __init__(self, num_classes: int):
        if not native_classes(int(num_classes)):
            raise ValueError(f"num_classes = {num_classes} outside 1..{MAX_K}")
        self.num_classes = int(num_classes)
        self.confusion: Optional[Tensor] = None

    def update(self, logits: Tensor, target: Tensor, mask: Optional[Tensor] = None) -> None:
        if int(logits.shape[-1]) != self.num_classes:
            raise ValueError(f"expected logits [..., {self.num_classes}], got {tuple(logits.shape)}")
        if self.confusion is None or self.confusion.device != logits.device:
            if self.confusion is not None:
                raise RuntimeError(f"ClassMeter holds counts on {self.confusion.device}, got logits on {logits.device}")
            self.confusion = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=logits.device)
        class_loss_sums(logits, target, mask, 0.0, self.confusion)

    def reset(self) -> None:
        self.confusion = None

    @staticmethod
    def formulas(confusion: Tensor) -> Dict[str, Tensor]:
        c = confusion.double()
        diag = c.diagonal()
        div = lambda a, b: torch.where(b > 0, a / b.clamp_min(1.0), torch.zeros_like(a))  # noqa: E731  (0 / 0 -> 0)
        prec, rec = div(diag, c.sum(0)), div(diag, c.sum(1))
        return {"accuracy": div(diag.sum(), c.sum()), "precision": prec.mean(), "recall": rec.mean(), "precision_per_class": prec,
                "recall_per_class": rec}

    def compute(self) -> Dict[str, Tensor]:
        if self.confusion is None:
            raise RuntimeError("ClassMeter.compute() before any update()")
        return self.formulas(self.confusion)


# ---- torch restatements of the two class-loss modules, called on the reference's flattened layouts ----
def masked_cross_entropy(logits: Tensor, target: Tensor, mask: Tensor, label_smoothing: float = 0.0) -> Tensor:  # [(B S), K], [(B S)] x 2
    loss = nn.functional.cross_entropy(logits, target, reduction="none", label_smoothing=label_smoothing)
    return (loss * mask).sum() / mask.sum()


def cross_entropy(logits: Tensor, target: Tensor) -> Tensor:  # [(B S), K], [(B S)]
    return nn.functional.cross_entropy(logits, target)


def _smoothing(module: Optional[nn.Module], name: str) -> Optional[float]:
    """The label smoothing of a class-loss module the device form computes, else ``None``: ``None`` itself (the reference's default,
    smoothing 0), a parameter-free MaskedCrossEntropyLoss, or an nn.CrossEntropyLoss with mean reduction, ignore_index -100 and no weights."""
    if module is None:
        return 0.0
    if not _geo._is_default(module, name):
        return None
    ce = getattr(module, "cross_entropy_loss", None) if name == "MaskedCrossEntropyLoss" else module
    want = "none" if name == "MaskedCrossEntropyLoss" else "mean"
    if not isinstance(ce, nn.CrossEntropyLoss) or ce.weight is not None or ce.ignore_index != IGNORE_INDEX or ce.reduction != want:
        return None
    eps = float(ce.label_smoothing)
    return eps if 0.0 <= eps < 1.0 else None


_GEOM = {"loss_pos": ("MaskedMSELoss", _geo.masked_mse, "pos_loss"), "loss_inter_distance": ("InterDistanceLoss", _geo.inter_distance, "inter_dist_loss"),
         "loss_norm": ("MaskedNormLoss", _geo.masked_norm, "dist")}


class _TrajectoryLoss(nn.Module):
    """What MD17Loss, PedestrianLoss and NBALoss share: the three geometric terms of ``preds["pos"]`` against ``batch["pos"]`` under
    ``batch["attention_mask"]`` and the class terms of the other heads, each from the device (``geom_losses`` / ``class_losses``) when its
    module is ``None`` or a parameter-free instance of the class the YAML names and the tensors are float32 on the GPU in the native
    shape, and from the given module - called exactly as the reference calls it - otherwise.  ``last_paths`` maps every term of the last
    call to "fused" or "generic"."""

    def __init__(self) -> None:
        super().__init__()
        self.last_paths: Dict[str, str] = {}

    def _geometry(self, pos_preds: Tensor, pos_targets: Tensor, mask: Tensor) -> Dict[str, Tensor]:
        fused = {a for a, (name, _, _) in _GEOM.items() if _geo._is_default(getattr(self, a), name)}
        native = (pos_preds.dim() == 3 and _lib.device_form(pos_preds, pos_targets, same_device=False)
                  and _geo.native_shape(int(pos_preds.shape[-2]), int(pos_preds.shape[-1])))
        geo = _geo.geom_losses(pos_preds, pos_targets, mask) if fused and native else None
        D = pos_preds.shape[-1]
        flat = (pos_preds.reshape(-1, D), pos_targets.reshape(-1, D), mask.reshape(-1))
        args = {"loss_pos": flat, "loss_inter_distance": (pos_preds, pos_targets, mask), "loss_norm": (pos_preds, pos_targets, mask)}
        out = {}
        for attr, (_, restated, key) in _GEOM.items():
            if geo is not None and attr in fused:
                out[attr], self.last_paths[attr] = geo[key], "fused"
            else:
                module = getattr(self, attr)
                out[attr], self.last_paths[attr] = (restated if module is None else module)(*args[attr]), "generic"
        return out

    def _class_term(self, attr: str, name: str, masked: bool, logits: Tensor, target: Tensor, mask: Optional[Tensor]) -> Tensor:
        module, eps = getattr(self, attr), _smoothing(getattr(self, attr), name)
        if eps is not None and logits.dim() == 3 and _lib.device_form(logits) and native_classes(int(logits.shape[-1])):
            self.last_paths[attr] = "fused"
            return class_losses(logits, target, mask if masked else None, eps)
        self.last_paths[attr] = "generic"
        lf, tf = logits.reshape(-1, logits.shape[-1]), target.reshape(-1)
        if masked:
            return masked_cross_entropy(lf, tf, mask.reshape(-1)) if module is None else module(logits=lf, target=tf, mask=mask.reshape(-1))
        return cross_entropy(lf, tf) if module is None else module(lf, tf)


class MD17Loss(_TrajectoryLoss):
    """Drop-in for ``src.models.composites.first_stage.md17.Loss`` (``model.loss._target_=lam_slide_amd.first_stage.MD17Loss``): same
    keywords, same ``forward(model, batch) -> (losses, preds)``, same keys, same weighted total.  ``None`` for a loss module means the
    reference's default (MaskedMSELoss / MaskedCrossEntropyLoss / InterDistanceLoss / MaskedNormLoss)."""

    def __init__(self, loss_pos_weight: float = 1.0, loss_atom_type_weight: float = 0.0, loss_inter_distance_weight: float = 1.0,
                 loss_norm_weight: float = 0.0, loss_pos: Optional[nn.Module] = None, loss_atom_type: Optional[nn.Module] = None,
                 loss_inter_distance: Optional[nn.Module] = None, loss_norm: Optional[nn.Module] = None) -> None:
        super().__init__()
        self.loss_pos_weight = loss_pos_weight
        self.loss_atom_type_weight = loss_atom_type_weight
        self.loss_inter_distance_weight = loss_inter_distance_weight
        self.loss_norm_weight = loss_norm_weight
        self.loss_pos = loss_pos
        self.loss_atom_type = loss_atom_type
        self.loss_inter_distance = loss_inter_distance
        self.loss_norm = loss_norm

    def forward(self, model, batch: Dict[str, Tensor]):
        preds = model(batch)
        mask = batch["attention_mask"]
        self.last_paths = {}
        g = self._geometry(preds["pos"], batch["pos"], mask)
        loss_pos, loss_inter_distance, loss_norm = g["loss_pos"], g["loss_inter_distance"], g["loss_norm"]
        loss_atom_type = self._class_term("loss_atom_type", "MaskedCrossEntropyLoss", True, preds["atom"], batch["atom"], mask)
        loss_total = (self.loss_pos_weight * loss_pos + self.loss_inter_distance_weight * loss_inter_distance
                      + self.loss_atom_type_weight * loss_atom_type + self.loss_norm_weight * loss_norm)
        return {"loss": loss_total, "pos_loss": loss_pos, "inter_distance_loss": loss_inter_distance, "atom_type_loss": loss_atom_type,
                "norm_loss": loss_norm, "dist": loss_norm * model.scale}, preds


class PedestrianLoss(_TrajectoryLoss):
    """Drop-in for ``src.models.composites.first_stage.pedestrian.Loss`` (``_target_=lam_slide_amd.first_stage.PedestrianLoss``)."""

    def __init__(self, loss_pos_weight: float = 1.0, loss_inter_distance_weight: float = 1.0, loss_norm_weight: float = 0.0,
                 loss_pos: Optional[nn.Module] = None, loss_inter_distance: Optional[nn.Module] = None, loss_norm: Optional[nn.Module] = None) -> None:
        super().__init__()
        self.loss_pos_weight = loss_pos_weight
        self.loss_inter_distance_weight = loss_inter_distance_weight
        self.loss_norm_weight = loss_norm_weight
        self.loss_pos = loss_pos
        self.loss_inter_distance = loss_inter_distance
        self.loss_norm = loss_norm

    def forward(self, model, batch: Dict[str, Tensor]):
        preds = model(batch)
        self.last_paths = {}
        g = self._geometry(preds["pos"], batch["pos"], batch["attention_mask"])
        loss_pos, loss_inter_distance, loss_norm = g["loss_pos"], g["loss_inter_distance"], g["loss_norm"]
        loss_total = self.loss_pos_weight * loss_pos + self.loss_inter_distance_weight * loss_inter_distance + self.loss_norm_weight * loss_norm
        return {"loss": loss_total, "pos_loss": loss_pos, "inter_distance_loss": loss_inter_distance, "norm_loss": loss_norm,
                "dist": loss_norm * model.scale}, preds


class NBALoss(_TrajectoryLoss):
    """Drop-in for ``src.models.composites.first_stage.nba.Loss`` (``_target_=lam_slide_amd.first_stage.NBALoss``); ``loss_team`` /
    ``loss_group`` default to nn.CrossEntropyLoss() over ALL players, padded ones included, as the reference calls them."""

    def __init__(self, loss_pos_weight: float = 1.0, loss_inter_distance_weight: float = 1.0, loss_norm_weight: float = 0.0,
                 loss_team_weight: float = 0.01, loss_group_weight: float = 0.01, loss_pos: Optional[nn.Module] = None,
                 loss_inter_distance: Optional[nn.Module] = None, loss_norm: Optional[nn.Module] = None, loss_team: Optional[nn.Module] = None,
                 loss_group: Optional[nn.Module] = None) -> None:
        super().__init__()
        self.loss_pos_weight = loss_pos_weight
        self.loss_inter_distance_weight = loss_inter_distance_weight
        self.loss_norm_weight = loss_norm_weight
        self.loss_team_weight = loss_team_weight
        self.loss_group_weight = loss_group_weight
        self.loss_pos = loss_pos
        self.loss_inter_distance = loss_inter_distance
        self.loss_norm = loss_norm
        self.loss_team = loss_team
        self.loss_group = loss_group

    def forward(self, model, batch: Dict[str, Tensor]):
        mask = batch["attention_mask"]
        preds = model(batch)
        self.last_paths = {}
        g = self._geometry(preds["pos"], batch["pos"], mask)
        loss_pos, loss_inter_distance, loss_norm = g["loss_pos"], g["loss_inter_distance"], g["loss_norm"]
        loss_team = self._class_term("loss_team", "CrossEntropyLoss", False, preds["team"], batch["team"], mask)
        loss_group = self._class_term("loss_group", "CrossEntropyLoss", False, preds["group"], batch["group"], mask)
        loss_total = (self.loss_pos_weight * loss_pos + self.loss_inter_distance_weight * loss_inter_distance + self.loss_norm_weight * loss_norm
                      + self.loss_team_weight * loss_team + self.loss_group_weight * loss_group)
        return {"loss": loss_total, "pos_loss": loss_pos, "inter_distance_loss": loss_inter_distance, "norm_loss": loss_norm,
                "team_loss": loss_team, "group_loss": loss_group, "dist": loss_norm * model.scale}, preds


class PeptideLoss(_TrajectoryLoss):
    """Drop-in for ``src.models.composites.first_stage.peptide.Loss`` (``_target_=lam_slide_amd.first_stage.PeptideLoss``): same keywords
    (``scale`` included: stored, ``dist`` reads ``model.scale`` as the reference does), same ``forward``, keys and weighted total.
    ``preds["atom14_pos"]`` is read as [B, R, 14, 3] (``Stage1Autoencoder(output_shapes={"atom14_pos": (14, 3)})``).  The five geometric
    terms come from ``peptide_losses`` (the device form of the second-stage PeptideLoss, same rule: MaskedMSELoss x 2, MaskedNormLoss,
    InterDistanceLoss, MaskedCosineLoss / V2), ``res_type_loss`` from ``class_losses``; any other module takes the torch path of its
    group.  ``residue_tables`` as for the second-stage PeptideLoss."""

    def __init__(self, loss_pos_weight: float = 1.0, loss_pos_frame_weight: float = 0.0, loss_res_type_weight: float = 0.0,
                 loss_norm_weight: float = 0.0, loss_torsion_weight: float = 0.0, loss_inter_distance_weight: float = 0.0,
                 loss_pos: Optional[nn.Module] = None, loss_pos_frame: Optional[nn.Module] = None, loss_res_type: Optional[nn.Module] = None,
                 loss_norm: Optional[nn.Module] = None, loss_torsion: Optional[nn.Module] = None, loss_inter_distance: Optional[nn.Module] = None,
                 scale: float = 1.0, *, residue_tables: Union[None, _pep.ResidueTables, Mapping[str, object]] = None) -> None:
        super().__init__()
        self.loss_pos_weight = loss_pos_weight
        self.loss_pos_frame_weight = loss_pos_frame_weight
        self.loss_res_type_weight = loss_res_type_weight
        self.loss_norm_weight = loss_norm_weight
        self.loss_torsion_weight = loss_torsion_weight
        self.loss_inter_distance_weight = loss_inter_distance_weight
        self.loss_pos = loss_pos
        self.loss_pos_frame = loss_pos_frame
        self.loss_res_type = loss_res_type
        self.loss_norm = loss_norm
        self.loss_torsion = loss_torsion
        self.loss_inter_distance = loss_inter_distance
        self.scale = scale
        self._tables = residue_tables

    tables = _pep.PeptideLoss.tables
    torsion_kind = _pep.PeptideLoss.torsion_kind  # (one copy of the rule: it reads the five module slots alone)
    _call = _pep.PeptideLoss._call

    def forward(self, model, batch: Dict[str, Tensor]):
        preds = model(batch)
        _ = batch["attention_mask"]  # (read and unused, as in the reference: every peptide of the dataset has the same length)
        self.last_paths = {}
        pos, target = preds["atom14_pos"], batch["atom14_pos"]  # [B, R, 14, 3] x 2
        target_frame, tors_target = batch["atom14_pos_frame"], batch["torsions"]
        tors_mask, aatype, atom14_mask = batch["torsions_mask"], batch["aatype"], batch["atom14_mask"]
        kind = self.torsion_kind()
        if kind is not None and _lib.device_form(pos, target, target_frame, tors_target, same_device=False) and _pep.native_shape(pos.shape):
            self.last_paths["geometry"] = "fused"
            got = _pep.peptide_losses(pos, target, target_frame, atom14_mask, tors_target, tors_mask, aatype, kind=kind, residue_tables=self.tables)
        else:
            self.last_paths["geometry"] = "generic"
            got = _pep.generic_terms(self, 1, pos, target, target_frame, atom14_mask, tors_target, tors_mask, aatype)
        res = self._class_term("loss_res_type", "CrossEntropyLoss", False, preds["aatype"], aatype, None)
        loss_total = (self.loss_pos_weight * got["pos_loss"] + self.loss_pos_frame_weight * got["pos_frame_loss"]
                      + self.loss_inter_distance_weight * got["inter_distance_loss"] + self.loss_res_type_weight * res
                      + self.loss_norm_weight * got["norm_loss"] + self.loss_torsion_weight * got["torsion_loss"])
        return {"loss": loss_total, "pos_loss": got["pos_loss"], "pos_frame_loss": got["pos_frame_loss"],
                "inter_distance_loss": got["inter_distance_loss"], "norm_loss": got["norm_loss"], "res_type_loss": res,
                "torsion_loss": got["torsion_loss"], "dist": got["norm_loss"] * model.scale}, preds
