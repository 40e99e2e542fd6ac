"""Rigid superposition of a sampled trajectory on the device: the step the reference runs through mdtraj between a sampled peptide
trajectory and its numbers (``eval_peptide.py:347`` ``traj_pred.superpose(traj_pred)``; ``utils/traj_utils.py:54-60`` ``create_trajectory``
= ``center_coordinates()`` then ``superpose(traj, 0)``), from the positions ``RolloutSampler.sample_rollout`` leaves there.

  center_coordinates  <- ``traj.center_coordinates()``: every frame minus the centroid of its (selected) atoms
  superpose           <- ``traj.superpose(reference, frame, atom_indices)``: the Kabsch fit of every frame onto one reference frame (or onto
                         its own frame of a second trajectory), applied to all atoms
  rmsd                <- ``md.rmsd(traj, reference, frame, atom_indices)``: the minimal root-mean-square deviation after that fit
  rmsf                <- ``md.rmsf`` without its own superposition: per atom ``sqrt(mean_f |x_fa - mean_f x_fa|^2)``, and the mean structure
  superpose_atom14    <- the same on atom14 positions [F, R, 14, 3]: fitted on the heavy atoms ``atom14_to_mdtraj`` puts into the topology
                         (``torsion_stats.topology_atoms``), the padding slots left exactly as they are
  create_trajectory   <- ``traj_utils.create_trajectory``: centred on those atoms, then superposed on frame 0

Stated as mathematics.  For a frame x and its reference y over the selected atoms: cx, cy the centroids, ``S = sum_i (x_i - cx)(y_i - cy)^T``,
R the proper rotation (det +1, never a reflection) minimising ``sum_i |R (x_i - cx) - (y_i - cy)|^2``, ``out_a = R (x_a - cx) + cy`` for every
atom, ``rmsd = sqrt(sum_i |R (x_i - cx) - (y_i - cy)|^2 / n)``.  ``S = 0`` exactly (one selected atom, coincident atoms) gives R = 1; where the
optimum is not unique (two atoms, collinear atoms) the RMSD is the minimum and R one of the minimisers.  A frame holding NaN gives NaN
for that frame only.  All arithmetic is float64 on the exact float32 inputs; each output is rounded once.

The device form is liblamslide_hip.so (``lsl_superpose`` / ``lsl_atom_rmsf``, csrc/k_superpose.hip.h): Horn's quaternion form with a fixed
number of Jacobi sweeps, every sum in a fixed order (a frame has the same bits alone and inside any batch, an atom the same bits at any
A).  The dispatch rule is ``_lib.device_form``: float32 tensors on one GPU, nothing requires grad, 1 <= A <= 2044; anything else (CPU
tensors, float64, tensors requiring grad, larger frames) takes the same mathematics in torch float64 (``torch.linalg.eigh`` of Horn's
matrix) with the same outputs and conventions.  ``last_path[name]`` tells which of the two ("fused" / "torch") the last call took.

mdtraj was not available where this was written: it fits in float32 by the QCP polynomial, so its coordinates differ from these in the
last float32 digits; parity with a live mdtraj was not checked.  Not here: mdtraj I/O, ``ref_atom_indices`` other than ``atom_indices``,
mass weighting, a pairwise RMSD matrix."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .torsion_stats import _index_table, fused_applies, topology_atoms

last_path: Dict[str, str] = {}
MAX_A = _lib.TORS_MAX_A  # atoms of a frame of lsl_superpose: a frame in LDS
RMSF_SEG = 128  # LSL_RMSF_SEG: frames of one segment of lsl_atom_rmsf
CENTER_ONLY = 1  # LSL_SUP_CENTER_ONLY


# ---- arguments ----
def _frames(pos: Tensor, name: str = "pos") -> Tensor:
    if pos.dim() != 3 or pos.shape[-1] != 3 or pos.shape[0] < 1 or pos.shape[1] < 1:
        raise ValueError(f"expected {name} [F, A, 3], got {tuple(pos.shape)}")
    return pos


def _selection(atom_indices, A: int) -> Tuple[Optional[np.ndarray], Optional[Tensor]]:
    """(host int32 [n], its device copy or None) of ``atom_indices``: None (all atoms), a host array / list / tensor of indices (a device
    tensor is copied back), or a pair ``(host table, device table)`` - the device table is then used as it is, nothing is copied."""
    if atom_indices is None:
        return None, None
    dev = None
    if isinstance(atom_indices, tuple) and len(atom_indices) == 2 and torch.is_tensor(atom_indices[1]):
        atom_indices, dev = atom_indices
    a = atom_indices.detach().cpu().numpy() if torch.is_tensor(atom_indices) else np.asarray(atom_indices)
    host = _index_table(a.reshape(-1, 1) if a.ndim == 1 else a, 1, "atom_indices").reshape(-1)
    if host.min() < 0 or host.max() >= A:
        raise ValueError(f"atom_indices holds an index outside the frame's atoms 0..{A - 1}")
    if dev is not None and (dev.dtype != torch.int32 or dev.numel() != host.size or not dev.is_contiguous()):
        raise ValueError(f"the device table of atom_indices must be contiguous int32 [{host.size}], got {dev.dtype} {tuple(dev.shape)}")
    return host, dev


def _reference(pos: Tensor, reference: Optional[Tensor], frame: int) -> Tensor:
    F, A = int(pos.shape[0]), int(pos.shape[1])
    if reference is None:
        if not -F <= int(frame) < F:
            raise ValueError(f"frame = {frame} outside the trajectory's {F} frames")
        return pos[int(frame)][None]
    ref = reference[None] if reference.dim() == 2 else reference
    if ref.dim() != 3 or tuple(ref.shape[1:]) != (A, 3) or ref.shape[0] not in (1, F):
        raise ValueError(f"expected reference [{A}, 3] or [{F}, {A}, 3], got {tuple(reference.shape)}")
    if ref.device != pos.device:
        raise ValueError(f"reference on {ref.device}, pos on {pos.device}")
    return ref


def _overlap(a: Tensor, b: Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


# ---- the restatement in torch float64 ----
def _rotation_torch(S: Tensor) -> Tensor:
    """S float64 [F, 3, 3] = sum x y^T -> the proper rotations [F, 3, 3] minimising sum |R x - y|^2: the top eigenvector of Horn's matrix.
    S == 0: the identity.  A frame with a NaN: NaN."""
    bad = ~torch.isfinite(S).all(dim=(1, 2))
    zero = (S == 0).all(dim=(1, 2))
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (torch.where(bad, torch.zeros_like(S[:, 0, 0]), S[:, i, j]) for i in range(3) for j in range(3))
    K = torch.stack([torch.stack([Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], dim=-1),
                     torch.stack([Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz], dim=-1),
                     torch.stack([Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy], dim=-1),
                     torch.stack([Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz], dim=-1)], dim=-2)
    q = torch.linalg.eigh(K).eigenvectors[..., -1]  # (ascending eigenvalues: the last column)
    unit = torch.zeros_like(q)
    unit[:, 0] = 1.0
    q = torch.where((zero | bad)[:, None], unit, q)
    q = q / torch.linalg.norm(q, dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([torch.stack([(w * w + x * x) - (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], dim=-1),
                     torch.stack([2 * (x * y + w * z), (w * w - x * x) + (y * y - z * z), 2 * (y * z - w * x)], dim=-1),
                     torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), (w * w - x * x) - (y * y - z * z)], dim=-1)], dim=-2)
    return torch.where(bad[:, None, None], torch.full_like(R, float("nan")), R)


def _fit_torch(pos: Tensor, ref: Optional[Tensor], sel: Optional[Tensor], fixed: Optional[Tensor]):
    """(out [F, A, 3], rmsd [F] or None, rot [F, 3, 3], trans [F, 3]), all float64; ref None: centring only."""
    x = pos.double()
    xs = x if sel is None else x[:, sel]
    n = xs.shape[1]
    cx = xs.sum(dim=1, keepdim=True) / n
    eye = torch.eye(3, dtype=torch.float64, device=x.device).expand(x.shape[0], 3, 3)
    if ref is None:
        out, rms, R, trans = x - cx, None, eye, -cx[:, 0]
    else:
        y = ref.double().expand(x.shape[0], -1, -1)
        ys = y if sel is None else y[:, sel]
        cy = ys.sum(dim=1, keepdim=True) / n
        dx, dy = xs - cx, ys - cy
        R = _rotation_torch(torch.einsum("fia,fib->fab", dx, dy))
        res = torch.einsum("fab,fib->fia", R, dx) - dy
        rms = torch.sqrt((res * res).sum(dim=(1, 2)) / n)
        out = torch.einsum("fab,fib->fia", R, x - cx) + cy
        trans = cy[:, 0] - torch.einsum("fab,fb->fa", R, cx[:, 0])
    if fixed is not None:
        out = torch.where(fixed[None, :, None], x, out)
    return out, rms, R, trans


# ---- the device form ----
def _fit_fused(pos: Tensor, ref: Optional[Tensor], sel_host: Optional[np.ndarray], sel_dev: Optional[Tensor], fixed: Optional[Tensor],
               out: Optional[Tensor], want_out: bool, want_rmsd: bool, want_transform: bool):
    dev, F, A = pos.device, int(pos.shape[0]), int(pos.shape[1])
    p = pos.detach().contiguous()
    if sel_host is not None and sel_dev is None:
        sel_dev = torch.from_numpy(sel_host).to(dev)
    n_sel = A if sel_host is None else int(sel_host.size)
    if want_out and out is None:
        out = torch.empty_like(p)
    r = None
    if ref is not None:
        r = ref.detach().contiguous()
        if out is not None and _overlap(out, r):  # (superposing in place on one of the trajectory's own frames: the reference is copied)
            r = r.clone()
    rms = torch.empty(F, dtype=torch.float32, device=dev) if want_rmsd else None
    rot = torch.empty(F, 3, 3, dtype=torch.float64, device=dev) if want_transform else None
    trans = torch.empty(F, 3, dtype=torch.float64, device=dev) if want_transform else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.call(dev, "lsl_superpose", p.data_ptr(), ptr(r), 1 if r is None else int(r.shape[0]), ptr(sel_dev),
              None if sel_host is None else sel_host.ctypes.data, n_sel, ptr(fixed), F, A, CENTER_ONLY if r is None else 0, ptr(out), ptr(rms),
              ptr(rot), ptr(trans))
    return out, rms, rot, trans


def _fit(name: str, pos: Tensor, ref: Optional[Tensor], atom_indices, fixed, out: Optional[Tensor], want_out: bool, want_rmsd: bool,
         want_transform: bool):
    """The one path of every function here: ``ref`` None centres only.  Returns (out, rmsd, rot, trans), the ones not asked for None."""
    F, A = int(pos.shape[0]), int(pos.shape[1])
    sel_host, sel_dev = _selection(atom_indices, A)
    fx = None
    if fixed is not None:
        fx = torch.as_tensor(fixed, device=pos.device)
        if fx.shape != (A,):
            raise ValueError(f"fixed must be [{A}], got {tuple(fx.shape)}")
        fx = (fx != 0).contiguous()
    if out is not None and (out.shape != pos.shape or out.dtype != pos.dtype or out.device != pos.device or not out.is_contiguous()):
        raise ValueError(f"out must be contiguous {pos.dtype} {tuple(pos.shape)} on {pos.device}")
    tensors = (pos,) if ref is None else (pos, ref)
    if fused_applies(*tensors) and 1 <= A <= MAX_A and (sel_host is None or sel_host.size <= MAX_A):
        last_path[name] = "fused"
        return _fit_fused(pos, ref, sel_host, sel_dev, None if fx is None else fx.to(torch.uint8), out, want_out, want_rmsd, want_transform)
    last_path[name] = "torch"
    sel = None if sel_host is None else torch.from_numpy(sel_host.astype(np.int64)).to(pos.device)
    o, rms, rot, trans = _fit_torch(pos, ref, sel, fx)
    o = o.to(pos.dtype)
    if out is not None:
        out.copy_(o)
        o = out
    return (o if want_out else None, rms.to(torch.float32) if want_rmsd else None, rot if want_transform else None,
            trans if want_transform else None)


# ---- the functions ----
def center_coordinates(pos: Tensor, atom_indices=None, out: Optional[Tensor] = None) -> Tensor:
    """pos [F, A, 3] -> [F, A, 3]: every frame minus the centroid of its atoms (``atom_indices``: of those atoms; all are moved) -
    ``traj.center_coordinates()``.  The centroid and the difference in float64, rounded once to pos's dtype.  ``out=pos`` works in place."""
    return _fit("center_coordinates", _frames(pos), None, atom_indices, None, out, True, False, False)[0]


def superpose(pos: Tensor, reference: Optional[Tensor] = None, frame: int = 0, atom_indices=None, fixed=None, out: Optional[Tensor] = None,
              return_rmsd: bool = False, return_transform: bool = False):
    """pos [F, A, 3] -> the frames fitted onto the reference, [F, A, 3] in pos's dtype - ``traj.superpose(reference, frame, atom_indices)``.

    ``reference`` None: ``pos[frame]`` (mdtraj's ``traj.superpose(traj, frame)``); [A, 3]: one frame for all; [F, A, 3]: frame f onto
    ``reference[f]``.  ``atom_indices`` [n]: the atoms the fit is computed on (a host array, a list or a tensor; or a pair ``(host table,
    int32 device table)``, which uploads nothing); every atom is moved.  ``fixed`` [A] (nonzero: the atom is copied through unchanged - the
    zeroed padding slots of an atom14 frame).  ``out``: where to write (``out=pos`` superposes in place; a reference inside ``out`` is
    copied first).  ``return_rmsd``: also the RMSD of the fit, float32 [F]; ``return_transform``: also ``rot`` float64 [F, 3, 3] and
    ``trans`` float64 [F, 3] with ``out = rot @ x + trans``.  Returns the frames, or the tuple (frames, [rmsd], [rot, trans])."""
    pos = _frames(pos)
    o, rms, rot, trans = _fit("superpose", pos, _reference(pos, reference, frame), atom_indices, fixed, out, True, return_rmsd, return_transform)
    extra = ((rms,) if return_rmsd else ()) + ((rot, trans) if return_transform else ())
    return (o,) + extra if extra else o


def rmsd(pos: Tensor, reference: Optional[Tensor] = None, frame: int = 0, atom_indices=None) -> Tensor:
    """pos [F, A, 3] -> float32 [F]: the root-mean-square deviation of the selected atoms after the optimal fit onto the reference
    (``reference`` / ``frame`` / ``atom_indices`` as :func:`superpose`) - ``md.rmsd``.  From the float64 residuals: a frame against itself
    gives 0.  Nothing is written back."""
    pos = _frames(pos)
    return _fit("rmsd", pos, _reference(pos, reference, frame), atom_indices, None, None, False, True, False)[1]


def rmsf(pos: Tensor, atom_indices=None, return_mean: bool = False):
    """pos [F, A, 3] -> float32 [A] (``atom_indices``: [n], those atoms): ``sqrt(mean_f |x_fa - mean_f x_fa|^2)`` of the frames as they are
    (superpose them first: ``md.rmsf`` does it itself).  ``return_mean``: also the mean structure, float64 [A, 3] (or [n, 3])."""
    pos = _frames(pos)
    F, A = int(pos.shape[0]), int(pos.shape[1])
    sel_host, sel_dev = _selection(atom_indices, A)
    if fused_applies(pos) and F <= 65535 * RMSF_SEG:
        dev = pos.device
        p = pos.detach().contiguous()
        need = int(_lib.load().lsl_atom_rmsf_workspace_bytes(F, A))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        fl = torch.empty(A, dtype=torch.float32, device=dev)
        mean = torch.empty(A, 3, dtype=torch.float64, device=dev) if return_mean else None
        _lib.call(dev, "lsl_atom_rmsf", p.data_ptr(), F, A, None if mean is None else mean.data_ptr(), fl.data_ptr(), ws.data_ptr(), need)
        last_path["rmsf"] = "fused"
    else:
        x = pos.double()
        mean = x.sum(dim=0) / F
        d = x - mean
        fl = torch.sqrt((d * d).sum(dim=(0, 2)) / F).to(torch.float32)
        last_path["rmsf"] = "torch"
    if sel_host is not None:
        idx = sel_dev.long() if sel_dev is not None else torch.from_numpy(sel_host.astype(np.int64)).to(pos.device)
        fl, mean = fl[idx], (mean[idx] if return_mean else None)
    return (fl, mean) if return_mean else fl


# ---- atom14 positions ----
def _atom14(pos14: Tensor, aatype, tables):
    """(frames [F, R * 14, 3], (host, device) selection of the topology's heavy atoms, fixed bool [R * 14] on the device)."""
    from .structure_stats import _tables_of
    if pos14.dim() != 4 or tuple(pos14.shape[-2:]) != (14, 3) or pos14.shape[0] < 1:
        raise ValueError(f"expected pos14 [F, R, 14, 3], got {tuple(pos14.shape)}")
    st = _tables_of(aatype, tables)
    if st.R != pos14.shape[1]:
        raise ValueError(f"aatype holds {st.R} residues, pos14 {pos14.shape[1]}")
    on = st.on(pos14.device)
    return pos14.reshape(pos14.shape[0], -1, 3), (st.topology, on["topology"]), on["padding"]


def superpose_atom14(pos14: Tensor, aatype, reference: Optional[Tensor] = None, frame: int = 0, tables=None, out: Optional[Tensor] = None,
                     return_rmsd: bool = False):
    """pos14 [F, R, 14, 3], aatype [R] (or a ``StructureTables`` of it, which keeps the index tables on the device) -> [F, R, 14, 3]:
    :func:`superpose` fitted on ``torsion_stats.topology_atoms(aatype)`` - the heavy atoms ``atom14_to_mdtraj`` puts into the topology, all
    mdtraj ever sees - with every other slot ``fixed``: padding stays exactly as it is (zero).  ``reference``: None (``pos14[frame]``),
    [R, 14, 3] or [F, R, 14, 3].  ``eval_peptide.py:347`` is ``superpose_atom14(pos14, aatype)``."""
    x, sel, padding = _atom14(pos14, aatype, tables)
    ref = None if reference is None else reference.reshape(*reference.shape[:-3], -1, 3)
    o = None if out is None else out.view(x.shape)
    res = superpose(x, ref, frame, sel, padding, o, return_rmsd=return_rmsd)
    last_path["superpose_atom14"] = last_path["superpose"]
    return (res[0].reshape(pos14.shape), res[1]) if return_rmsd else res.reshape(pos14.shape)


def create_trajectory(pos14: Tensor, aatype, tables=None) -> Tensor:
    """pos14 [F, R, 14, 3] -> [F, R, 14, 3]: ``utils/traj_utils.py:create_trajectory`` - ``center_coordinates()`` on the topology's heavy
    atoms, then ``superpose(traj, 0)``; the padding slots stay as they are."""
    x, sel, padding = _atom14(pos14, aatype, tables)
    c = _fit("center_coordinates", x, None, sel, padding, None, True, False, False)[0]
    o = superpose(c, None, 0, sel, padding, c)
    last_path["create_trajectory"] = "fused" if {last_path["center_coordinates"], last_path["superpose"]} == {"fused"} else "torch"
    return o.reshape(pos14.shape)
