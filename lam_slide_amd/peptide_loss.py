"""The peptide ``model_step``: the five losses ``Loss.forward`` of the reference's peptide model computes behind the SI term when
``calc_additional_losses`` is set (second_stage/peptide.py:293-378, the shipped configs/model/peptide/second-stage.yaml) - position,
frame-local position, inter-distance, norm and torsion loss of the decoded atom14 positions.

  peptide_loss_sums, peptide_losses  <- three launches of liblamslide_hip.so: ``lsl_geom_loss_sums`` with entities = (residue, atom)
                                        (MaskedMSELoss, MaskedNormLoss, InterDistanceLoss; csrc/k_geomloss.hip.h), ``lsl_peptide_loss_sums``
                                        (backbone frames, atom37 gather, seven torsion frames per residue, MaskedMSELoss in the frame and
                                        MaskedCosineLoss / V2; csrc/k_peptloss.hip.h) and ``lsl_peptide_loss_final``.  No atomics: a frame's
                                        sums have the same bits in any batch or shard
  backbone_local, atom37_positions,  <- the same geometry in torch, differentiable, any dtype and device (modules/geometry.py:212-227,
  torsion_angles, torsion_mask          peptide.py:147-168 and :170-286, utils/rigid_utils.py:1093-1134)
  PeptideLoss                        <- ``second_stage/peptide.py:Loss`` as a ``_target_`` drop-in: the device form when it applies, otherwise
                                        the given loss modules (or torch restatements of the constructor's defaults) on the torch geometry

The residue tables (atom37 -> atom14 index and mask per residue type, the chi atoms, the chi mask) are the host application's: they are
handed over as ``residue_tables=`` or imported from ``src.utils.residue_constants`` / ``src.modules.geometry`` when first needed.
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor, nn

from . import _lib
from .losses import _is_default, geom_loss_sums, masked_mse, masked_norm
from .transport import ModelType

SUM_COLUMNS = ("s_frame", "n", "s_tors", "n_tors")
LOSS_KEYS = ("pos_loss", "pos_frame_loss", "inter_distance_loss", "norm_loss", "torsion_loss")  # the order of ``lsl_peptide_loss_final``
TABLE_KEYS = ("restype_atom37_to_atom14", "restype_atom37_mask", "chi_atom_indices", "chi_angles_mask")
KIND_COSINE, KIND_COSINE_V2 = 0, 1
MAX_R = _lib.GEOM_MAX_A // 14  # 146: the frame's R * 14 atoms are the entities of lsl_geom_loss_sums


class ResidueTables:
    """The four tables of the reference as arrays: ``restype_atom37_to_atom14`` [21, 37] (residue_constants.RESTYPE_ATOM37_TO_ATOM14),
    ``restype_atom37_mask`` [21, 37] (RESTYPE_ATOM37_MASK), ``chi_atom_indices`` [21, 4, 4] (geometry.get_chi_atom_indices()) and
    ``chi_angles_mask`` [20 or 21, 4] (residue_constants.chi_angles_mask; the unknown type's row of zeros is appended when missing, as
    peptide.py:218-220 does).  ``restab`` is what ``lsl_peptide_loss_sums`` reads; tensors are cached per device."""

    def __init__(self, tables: Mapping[str, object]) -> None:
        missing = [k for k in TABLE_KEYS if k not in tables]
        if missing:
            raise KeyError(f"residue_tables lacks {missing}; expected the keys {TABLE_KEYS}")
        get = lambda k: tables[k].detach().cpu().numpy() if torch.is_tensor(tables[k]) else np.asarray(tables[k])  # noqa: E731
        self.a37to14 = get(TABLE_KEYS[0]).astype(np.int64)
        self.m37 = get(TABLE_KEYS[1]).astype(np.float64)
        self.chi_idx = get(TABLE_KEYS[2]).astype(np.int64)
        chi_mask = get(TABLE_KEYS[3]).astype(np.float64)
        if chi_mask.shape == (20, 4):
            chi_mask = np.concatenate([chi_mask, np.zeros((1, 4))])
        self.chi_mask = chi_mask
        shapes = (self.a37to14.shape, self.m37.shape, self.chi_idx.shape, self.chi_mask.shape)
        if shapes != ((21, 37), (21, 37), (21, 4, 4), (21, 4)):
            raise ValueError(f"residue tables of shapes {shapes}, expected [21, 37], [21, 37], [21, 4, 4] and [20 or 21, 4]")
        if self.a37to14.min() < 0 or self.a37to14.max() > 13 or self.chi_idx.min() < 0 or self.chi_idx.max() > 36:
            raise ValueError("residue tables hold an atom14 index outside 0..13 or an atom37 index outside 0..36")
        # restab [21, 20]: per residue type the atom14 index of atom37 slots 0, 1, 2, 4 and of the 16 chi atoms; -1 where the atom37 mask is 0
        slots = np.concatenate([np.broadcast_to(np.array([0, 1, 2, 4]), (21, 4)), self.chi_idx.reshape(21, 16)], axis=1)
        rows = np.arange(21)[:, None]
        self.restab = np.where(self.m37[rows, slots] != 0, self.a37to14[rows, slots], -1).astype(np.int8)
        self._on: Dict[Tuple[torch.device, torch.dtype], Dict[str, Tensor]] = {}

    def on(self, device: torch.device, dtype: torch.dtype = torch.float32) -> Dict[str, Tensor]:
        key = (torch.device(device), dtype)
        if key not in self._on:
            dev = key[0]
            self._on[key] = {"a37to14": torch.from_numpy(self.a37to14).to(dev), "m37": torch.from_numpy(self.m37).to(dev, dtype),
                             "chi_idx": torch.from_numpy(self.chi_idx).to(dev), "chi_mask": torch.from_numpy(self.chi_mask).to(dev, dtype),
                             "restab": torch.from_numpy(self.restab).to(dev)}
        return self._on[key]


_host_tables: Optional[ResidueTables] = None


def residue_tables(tables: Union[None, ResidueTables, Mapping[str, object]] = None) -> ResidueTables:
    """``ResidueTables`` of a dict of the four arrays, or - ``None`` - of the host application's own modules (imported once)."""
    global _host_tables
    if isinstance(tables, ResidueTables):
        return tables
    if tables is not None:
        return ResidueTables(tables)
    if _host_tables is None:
        try:
            from src.modules.geometry import get_chi_atom_indices
            from src.utils import residue_constants as rc
        except ImportError as e:
            raise ImportError("the peptide losses need the residue tables: pass residue_tables={" + ", ".join(f"'{k}': ..." for k in TABLE_KEYS)
                              + "} or make the host application's src.utils.residue_constants and src.modules.geometry importable") from e
        _host_tables = ResidueTables({TABLE_KEYS[0]: rc.RESTYPE_ATOM37_TO_ATOM14, TABLE_KEYS[1]: rc.RESTYPE_ATOM37_MASK,
                                      TABLE_KEYS[2]: get_chi_atom_indices(), TABLE_KEYS[3]: rc.chi_angles_mask})
    return _host_tables


# ---- the geometry in torch: differentiable, any dtype and device ----
FRAME_DTYPE = torch.float32  # the reference's Rotation / Rigid hold rotation and translation in float32 whatever went in (rigid_utils.py:302-306, :806-807)


def _dot(a: Tensor, b: Tensor) -> Tensor:  # (the three products added left to right, as rot_vec_mul writes them out: rigid_utils.py:62-80)
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def gram_schmidt(p_neg_x: Tensor, origin: Tensor, p_xy: Tensor, eps: float = 1e-8) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(e0, e1, e2, origin), each [..., 3], of ``Rigid.from_3_points`` (utils/rigid_utils.py:1093-1134): the rotation's columns and the
    translation, computed in the dtype of the points and then held in float32 like the reference's ``Rigid`` - nothing changes for float32
    points; for float64 points it is what the reference computes too."""
    e0 = origin - p_neg_x
    e0 = e0 / torch.sqrt(_dot(e0, e0) + eps)[..., None]
    e1 = p_xy - origin
    e1 = e1 - e0 * _dot(e0, e1)[..., None]
    e1 = e1 / torch.sqrt(_dot(e1, e1) + eps)[..., None]
    e2 = torch.stack([e0[..., 1] * e1[..., 2] - e0[..., 2] * e1[..., 1], e0[..., 2] * e1[..., 0] - e0[..., 0] * e1[..., 2],
                      e0[..., 0] * e1[..., 1] - e0[..., 1] * e1[..., 0]], dim=-1)
    return e0.to(FRAME_DTYPE), e1.to(FRAME_DTYPE), e2.to(FRAME_DTYPE), origin.to(FRAME_DTYPE)


def backbone_local(atom14: Tensor) -> Tensor:
    """[..., R, 14, 3] -> every atom in its residue's backbone frame (``atom14_to_frames(x).unsqueeze(-1).invert_apply(x)``,
    modules/geometry.py:212-227 and peptide.py:330-336): from_3_points(C, CA, N) with the x and z axes flipped, origin CA."""
    e0, e1, e2, ca = gram_schmidt(atom14[..., 2:3, :], atom14[..., 1:2, :], atom14[..., 0:1, :])
    d = atom14 - ca
    return torch.stack([-_dot(e0, d), _dot(e1, d), -_dot(e2, d)], dim=-1)


def atom37_positions(atom14: Tensor, aatype: Tensor, tables: ResidueTables) -> Tensor:
    """[..., R, 14, 3], [..., R] -> [..., R, 37, 3]: the atom14 -> atom37 gather times the atom37 mask of the type (peptide.py:147-168)."""
    t = tables.on(atom14.device, atom14.dtype)
    idx = t["a37to14"][aatype]  # [..., R, 37]
    pos = torch.gather(atom14, -2, idx[..., None].expand(*idx.shape, 3))
    return pos * t["m37"][aatype][..., None]


def torsion_angles(atom14: Tensor, aatype: Tensor, tables: ResidueTables) -> Tensor:
    """[..., R, 14, 3], [..., R] -> (sin, cos) [..., R, 7, 2] of pre-omega, phi, psi, chi1..4 (``calc_torsions``, peptide.py:170-291)."""
    a37 = atom37_positions(atom14, aatype, tables)
    prev = torch.cat([torch.zeros_like(a37[..., :1, :, :]), a37[..., :-1, :, :]], dim=-3)  # the residue before residue 0: zeros
    chi = tables.on(atom14.device, atom14.dtype)["chi_idx"][aatype]  # [..., R, 4, 4]
    chi_pos = torch.gather(a37, -2, chi.reshape(*chi.shape[:-2], 16)[..., None].expand(*chi.shape[:-2], 16, 3)).reshape(*chi.shape, 3)
    four = torch.cat([torch.stack([prev[..., 1, :], prev[..., 2, :], a37[..., 0, :], a37[..., 1, :]], dim=-2)[..., None, :, :],
                      torch.stack([prev[..., 2, :], a37[..., 0, :], a37[..., 1, :], a37[..., 2, :]], dim=-2)[..., None, :, :],
                      torch.stack([a37[..., 0, :], a37[..., 1, :], a37[..., 2, :], a37[..., 4, :]], dim=-2)[..., None, :, :],
                      chi_pos], dim=-3)  # [..., R, 7, 4, 3]
    _, e1, e2, o = gram_schmidt(four[..., 1, :], four[..., 2, :], four[..., 0, :])
    # (z, y) of the fourth atom in the frame, as ``frames.invert().apply(p)`` forms them: R^T p - (R^T o), the second term a float32 of its own
    sc = torch.stack([_dot(e2, four[..., 3, :]) - _dot(e2, o), _dot(e1, four[..., 3, :]) - _dot(e1, o)], dim=-1)
    sc = sc / torch.sqrt((sc * sc).sum(-1, keepdim=True) + 1e-8)
    sign = sc.new_tensor([1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0])
    return sc * sign[:, None]


def torsion_mask(aatype: Tensor, tables: ResidueTables, dtype: torch.dtype = torch.float32) -> Tensor:
    """[..., R] -> [..., R, 7]: where all four atoms of a torsion exist and, for chi, the type has that angle (peptide.py:184-253 with the
    atom37 mask of the type as ``all_atom_mask``) - the ``torsions_mask`` the dataset stores."""
    t = tables.on(aatype.device, dtype)
    m = t["m37"][aatype]  # [..., R, 37]
    pm = torch.cat([torch.zeros_like(m[..., :1, :]), m[..., :-1, :]], dim=-2)
    bb = m[..., 0] * m[..., 1] * m[..., 2]
    chi = t["chi_idx"][aatype]
    chi_atoms = torch.gather(m, -1, chi.reshape(*chi.shape[:-2], 16)).reshape(chi.shape).prod(-1)
    return torch.cat([(pm[..., 1] * pm[..., 2] * m[..., 0] * m[..., 1])[..., None], (pm[..., 2] * bb)[..., None], (bb * m[..., 4])[..., None],
                      t["chi_mask"][aatype] * chi_atoms], dim=-1)


# ---- torch restatements of the two torsion modules (modules/losses.py:75-92) ----
def masked_cosine(preds: Tensor, targets: Tensor, mask: Tensor) -> Tensor:  # [(B T R 7), 2] x 2, [(B T R 7)]
    return ((1 - nn.functional.cosine_similarity(preds, targets, dim=-1)) * mask).sum() / mask.sum()


def masked_cosine_v2(preds: Tensor, targets: Tensor, mask: Tensor) -> Tensor:
    return ((1 - (preds * targets).sum(dim=-1)) * mask).sum() / mask.sum()


# ---- the device form ----
def native_shape(shape) -> bool:
    """Whether ``lsl_peptide_loss_sums`` covers positions of this shape: [.., R, 14, 3] with 1 <= R <= 146."""
    return len(shape) >= 3 and tuple(shape[-2:]) == (14, 3) and 1 <= int(shape[-3]) <= MAX_R


def _peptide_frames(pred: Tensor, target_frame: Tensor, atom14_mask: Tensor, tors_target: Tensor, tors_mask: Tensor, aatype: Tensor):
    if pred.dim() < 3 or tuple(pred.shape[-2:]) != (14, 3):
        raise ValueError(f"expected pred [..., R, 14, 3], got {tuple(pred.shape)}")
    lead, R = tuple(pred.shape[:-3]), int(pred.shape[-3])
    specs = (("pred", pred, (R, 14, 3), torch.float32), ("target_frame", target_frame, (R, 14, 3), torch.float32),
             ("atom14_mask", atom14_mask, (R, 14), torch.uint8), ("tors_target", tors_target, (R, 7, 2), torch.float32),
             ("tors_mask", tors_mask, (R, 7), torch.uint8), ("aatype", aatype, (R,), torch.int64))
    if aatype.is_floating_point() or aatype.dtype == torch.bool:
        raise ValueError(f"aatype must hold integers, got {aatype.dtype}")
    return tuple(_lib.flat(x, lead, trailing, dtype, pred.device,
                           lambda: f"expected {name} {list(lead + trailing)} for pred {tuple(pred.shape)}, got {tuple(x.shape)}",
                           lambda: f"Expected all tensors to be on the same device, pred is on {pred.device}, {name} on {x.device}")
                 for name, x, trailing, dtype in specs)


@torch.no_grad()
def peptide_loss_sums(pred: Tensor, target_frame: Tensor, atom14_mask: Tensor, tors_target: Tensor, tors_mask: Tensor, aatype: Tensor, *,
                      kind: int = KIND_COSINE_V2, residue_tables: Union[None, ResidueTables, Mapping[str, object]] = None) -> Tensor:
    """float32 [F, 4]: per frame (s_frame, n, s_tors, n_tors) of ``lsl_peptide_loss_sums`` (include/lsl_api.h) for pred / target_frame
    [..., R, 14, 3], atom14_mask [..., R, 14], tors_target [..., R, 7, 2], tors_mask [..., R, 7] (nonzero = counted) and aatype [..., R],
    leading axes flattened to F frames.  kind 0 = MaskedCosineLoss, 1 = MaskedCosineLossV2.  A frame with an aatype outside 0..20 gets four
    NaN.  Rows of different shards may be concatenated and finished by ``peptide_losses(sums=...)``.  GPU only; R > 146 raises
    ``ValueError``."""
    if not pred.is_cuda:
        raise RuntimeError("peptide_loss_sums runs on the GPU (HIP kernel); there is no CPU fallback")
    p, tf, am, tt, tm, aa = _peptide_frames(pred, target_frame, atom14_mask, tors_target, tors_mask, aatype)
    F_, R = p.shape[:2]
    if F_ == 0:
        raise ValueError("no frames")
    dev = p.device
    restab = residue_tables_on(residue_tables, dev)
    sums = torch.empty(F_, 4, dtype=torch.float32, device=dev)
    _lib.call(dev, "lsl_peptide_loss_sums", p.data_ptr(), tf.data_ptr(), am.data_ptr(), tt.data_ptr(), tm.data_ptr(), aa.data_ptr(), restab.data_ptr(),
              F_, R, int(kind), sums.data_ptr())
    return sums


def residue_tables_on(tables, device) -> Tensor:
    """int8 [21, 20] ``restab`` on ``device`` (cached per device by the ``ResidueTables``)."""
    return residue_tables(tables).on(device)["restab"]


@torch.no_grad()
def peptide_losses(pred: Optional[Tensor] = None, target: Optional[Tensor] = None, target_frame: Optional[Tensor] = None,
                   atom14_mask: Optional[Tensor] = None, tors_target: Optional[Tensor] = None, tors_mask: Optional[Tensor] = None,
                   aatype: Optional[Tensor] = None, *, kind: int = KIND_COSINE_V2,
                   residue_tables: Union[None, ResidueTables, Mapping[str, object]] = None,
                   sums: Optional[Tuple[Tensor, Tensor]] = None) -> Dict[str, Tensor]:
    """{"pos_loss", "pos_frame_loss", "inter_distance_loss", "norm_loss", "torsion_loss"} as 0-dim float32 tensors: the reference's
    MaskedMSELoss (global and frame-local), InterDistanceLoss, MaskedNormLoss and MaskedCosineLoss / V2 of the decoded atom14 positions
    ``pred`` against ``target`` [..., R, 14, 3] and the dataset's ``target_frame`` / ``tors_target`` - three launches - or of
    ``sums = (geom_sums [F, 5], peptide_sums [F, 4])`` from ``geom_loss_sums`` (entities = R * 14 atoms, mask = atom14_mask) and
    :func:`peptide_loss_sums` - one launch.  Frames are added in index order in fp64, each quotient is rounded once; 0 / 0 is NaN like the
    reference."""
    def both_sums():
        if not pred.is_cuda:
            raise RuntimeError("peptide_losses runs on the GPU (HIP kernel); there is no CPU fallback")
        pept = peptide_loss_sums(pred, target_frame, atom14_mask, tors_target, tors_mask, aatype, kind=kind, residue_tables=residue_tables)
        if tuple(target.shape) != tuple(pred.shape):
            raise ValueError(f"expected target {tuple(pred.shape)}, got {tuple(target.shape)}")
        A = int(pred.shape[-3]) * 14
        return geom_loss_sums(pred.reshape(-1, A, 3), target.reshape(-1, A, 3), atom14_mask.reshape(-1, A)), pept

    out = _lib.loss_from_sums("peptide_losses", "lsl_peptide_loss_final", (5, 4), 5, sums,
                              (pred, target, target_frame, atom14_mask, tors_target, tors_mask, aatype), (), both_sums,
                              "(pred, target, target_frame, atom14_mask, tors_target, tors_mask, aatype)", "the tensors")
    return {k: out[i] for i, k in enumerate(LOSS_KEYS)}


# slot -> (name of the reference constructor's default, its torch restatement)   (second_stage/peptide.py:115-119)
_DEFAULTS = {"loss_pos": ("MaskedMSELoss", masked_mse), "loss_pos_frame": ("MaskedMSELoss", masked_mse), "loss_norm": ("MaskedNormLoss", masked_norm),
             "loss_torsion": ("MaskedCosineLoss", masked_cosine), "loss_inter_distance": ("MaskedMSELoss", masked_mse)}
_TORSION_KINDS = {"MaskedCosineLoss": KIND_COSINE, "MaskedCosineLossV2": KIND_COSINE_V2}


def generic_terms(loss: nn.Module, lead: int, pos: Tensor, target: Tensor, target_frame: Tensor, atom14_mask: Tensor, tors_target: Tensor,
                  tors_mask: Tensor, aatype: Tensor) -> Dict[str, Tensor]:
    """The five terms from the modules of ``loss`` (``loss._call``: the module of a slot or the torch restatement of its default) on the
    torch geometry of this file, each called on the layout the reference rearranges to.  pos [..., R, 14, 3] with ``lead`` leading axes -
    (B, T) in the second stage, (B) in the first - flattened to frames."""
    R = int(pos.shape[lead])
    flat3 = lambda x: x.reshape(-1, 3)  # noqa: E731  "... R A D -> (... R A) D"
    mask_flat = atom14_mask.reshape(-1)
    frames = pos.reshape(-1, R, 14, 3)
    return {"pos_loss": loss._call("loss_pos", flat3(pos), flat3(target), mask_flat),
            "pos_frame_loss": loss._call("loss_pos_frame", flat3(backbone_local(frames)), flat3(target_frame), mask_flat),
            "inter_distance_loss": loss._call("loss_inter_distance", pos.reshape(-1, R * 14, 3), target.reshape(-1, R * 14, 3),
                                              atom14_mask.reshape(-1, R * 14)),
            "norm_loss": loss._call("loss_norm", flat3(pos), flat3(target), mask_flat),
            "torsion_loss": loss._call("loss_torsion", preds=torsion_angles(frames, aatype.reshape(-1, R), loss.tables).reshape(-1, 2),
                                       targets=tors_target.reshape(-1, 2), mask=tors_mask.reshape(-1))}


class PeptideLoss(nn.Module):
    """Drop-in for ``src.models.composites.second_stage.peptide.Loss`` (``model.loss._target_=lam_slide_amd.PeptideLoss``): same keywords
    and defaults, same ``forward(model, batch) -> (losses, pred_latent)``, same keys, same arithmetic of ``losses["loss"]``.  ``None`` for a
    loss module means the reference constructor's default for that slot (MaskedMSELoss for ``loss_inter_distance`` too, as odd as that is:
    the shipped YAML names every module).  ``residue_tables``: the four tables as a dict, or ``None`` to take them from the host
    application when first needed.

    ``last_path`` says what computed the five losses of the last call: "fused" (``peptide_losses``: three HIP launches) when the decoded
    positions and the batch's float targets are float32 on the GPU, nothing requires grad, the shape is [.., R <= 146, 14, 3], and the
    modules are parameter-free instances named MaskedMSELoss (``loss_pos``, ``loss_pos_frame``; or ``None``), MaskedNormLoss (or ``None``),
    InterDistanceLoss, and MaskedCosineLoss (or ``None``) / MaskedCosineLossV2; "generic" (the modules themselves on the torch geometry of
    this file) otherwise - training with gradients, CPU tensors, other modules; ``None`` when ``calc_additional_losses`` is off."""

    def __init__(self, loss_si_weight: float = 1.0, loss_pos_weight: float = 1.0, loss_pos_frame_weight: float = 0.0, loss_norm_weight: float = 0.0,
                 loss_torsion_weight: float = 0.0, loss_inter_distance_weight: float = 0.0, loss_pos: Optional[nn.Module] = None,
                 loss_pos_frame: Optional[nn.Module] = None, loss_norm: Optional[nn.Module] = None, loss_torsion: Optional[nn.Module] = None,
                 loss_inter_distance: Optional[nn.Module] = None, calc_additional_losses: bool = False, *,
                 residue_tables: Union[None, ResidueTables, Mapping[str, object]] = None) -> None:
        super().__init__()
        self.loss_si_weight = loss_si_weight
        self.loss_pos_weight = loss_pos_weight
        self.loss_pos_frame_weight = loss_pos_frame_weight
        self.loss_norm_weight = loss_norm_weight
        self.loss_torsion_weight = loss_torsion_weight
        self.loss_inter_distance_weight = loss_inter_distance_weight
        self.loss_pos = loss_pos
        self.loss_pos_frame = loss_pos_frame
        self.loss_norm = loss_norm
        self.loss_torsion = loss_torsion
        self.loss_inter_distance = loss_inter_distance
        self.calc_additional_losses = calc_additional_losses
        self._tables = residue_tables
        self.last_path: Optional[str] = None

    @property
    def tables(self) -> ResidueTables:
        if not isinstance(self._tables, ResidueTables):
            self._tables = residue_tables(self._tables)
        return self._tables

    def torsion_kind(self) -> Optional[int]:
        """0 / 1 when the five modules are what the device form computes (``loss_torsion`` picks the kind), else ``None``."""
        named = all(_is_default(getattr(self, attr), _DEFAULTS[attr][0]) for attr in ("loss_pos", "loss_pos_frame", "loss_norm"))
        inter = self.loss_inter_distance
        if not named or inter is None or not _is_default(inter, "InterDistanceLoss"):
            return None
        if self.loss_torsion is None:
            return KIND_COSINE
        kind = _TORSION_KINDS.get(type(self.loss_torsion).__name__)
        return kind if kind is not None and _is_default(self.loss_torsion, type(self.loss_torsion).__name__) else None

    def fused_applies(self, pred_pos: Tensor, *float_targets: Tensor) -> bool:
        # (tensors on two GPUs stay on this path: ``_peptide_frames`` raises the reference-style device error)
        return (_lib.device_form(pred_pos, *float_targets, same_device=False) and native_shape(pred_pos.shape)
                and self.torsion_kind() is not None)

    def _call(self, attr: str, *args: Tensor, **kwargs: Tensor) -> Tensor:
        module = getattr(self, attr)
        return _DEFAULTS[attr][1](*args, **kwargs) if module is None else module(*args, **kwargs)

    def calc_torsions(self, atom14_pos: Tensor, aatype: Tensor) -> Tensor:
        return torsion_angles(atom14_pos, aatype, self.tables)

    def forward(self, model: nn.Module, batch: Dict[str, Tensor]):
        out = model.si.training_losses(model=model, x1=batch["x1"], model_kwargs=batch["model_kwargs"])
        pred_latent = out["pred"]
        si_loss = out["loss"].mean()
        losses = {"si_loss": si_loss, "loss": si_loss * self.loss_si_weight}
        self.last_path = None
        if self.calc_additional_losses:
            assert model.si.model_type == ModelType.DATA, "Additional losses are currently only supported for DATA model"
            pred_latent, entities = (x.reshape(x.shape[0] * x.shape[1], *x.shape[2:]) for x in (pred_latent, batch["entities"]))
            pred = model.decode(pred_latent, entities)
            _ = batch["attention_mask"]  # (read and unused, as in the reference: every peptide of the dataset has the same length)
            pos, target = pred["atom14_pos"], batch["atom14_pos"]  # [B, T, R, 14, 3] x 2
            target_frame, tors_target = batch["atom14_pos_frame"], batch["torsions"]
            tors_mask, aatype, atom14_mask = batch["torsions_mask"], batch["aatype"], batch["atom14_mask"]
            if self.fused_applies(pos, target, target_frame, tors_target):
                self.last_path = "fused"
                got = peptide_losses(pos, target, target_frame, atom14_mask, tors_target, tors_mask, aatype, kind=self.torsion_kind(),
                                     residue_tables=self.tables)
            else:
                self.last_path = "generic"
                got = generic_terms(self, 2, pos, target, target_frame, atom14_mask, tors_target, tors_mask, aatype)
            for k in LOSS_KEYS:
                losses[k] = got[k]
            losses["loss"] = losses["loss"] + self.loss_pos_weight * got["pos_loss"]
            losses["loss"] = losses["loss"] + self.loss_pos_frame_weight * got["pos_frame_loss"]
            losses["loss"] = losses["loss"] + self.loss_inter_distance_weight * got["inter_distance_loss"]
            losses["loss"] = losses["loss"] + self.loss_norm_weight * got["norm_loss"]
            losses["loss"] = losses["loss"] + self.loss_torsion_weight * got["torsion_loss"]
        return losses, pred_latent
