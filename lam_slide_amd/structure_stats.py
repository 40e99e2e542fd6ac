"""The structure statistics of the peptide validation: what ``SIAtom14SampleCallback.log_metrics`` logs per peptide on every validation
epoch through ``utils/traj_utils.py:traj_analysis``, on the device, from the atom14 positions ``RolloutSampler.sample_rollout`` leaves there.

  ca_atoms, ca_pair_table, backbone_torsion_quads, tica_atom_selection, triu_pairs, StructureTables
                      <- the index tables mdtraj's topology queries give the reference (``select("name CA")``, ``compute_phi`` / ``psi`` /
                         ``omega``, ``select("symbol == C or symbol == N or symbol == S")``), from the residue tables alone
  pair_distances      <- ``np.linalg.norm(xyz[:, i] - xyz[:, j], axis=-1)`` of a general table of atom pairs (``compute_pairwise_distances``,
                         ``tica_utils.distances``)
  ca_frame_stats      <- ``md.compute_rg`` of the C-alpha atoms, ``compute_validity``'s clash / bond-break test per frame and its tallies,
                         ``compute_contact_matrix`` as integer contact counts
  tica_features       <- ``tica_utils.tica_features``: [triu distances | sin phi | cos phi | sin psi | cos psi | sin omega | cos omega]
  column_edges        <- ``np.linspace(ref_col.min(), ref_col.max(), bins)`` of every column, on the device
  histogram_columns   <- ``np.histogram(x[:, q], bins=edges[q])[0]`` with one edge table per column
  js_distance_density <- ``jensenshannon`` of two ``density=True`` histograms with ``discretize_features``' pseudo-count
  density_js          <- ``compute_js_distance``;  joint_density_js <- ``compute_joint_js_distance``
  traj_analysis       <- the seven numbers: ramachandran_js, pwd_js, rg_js, tic_js, tic2d_js, val_ca, rmse_contact

The device form is liblamslide_hip.so (``lsl_pair_distances`` / ``lsl_ca_frame_stats`` / ``lsl_histogram_columns`` /
``lsl_js_distance_density``, csrc/k_structstat.hip.h; the angles are ``lsl_dihedral_angles``, the 2-D counts ``lsl_histogram``'s pair form):
counts are integers (exact), every float is a sum in a fixed order (a frame has the same bits alone and in any batch).  The dispatch rule is
``_lib.device_form``: float32 tensors (counts: int64, edges and cell sizes: float64) on the GPU, nothing requires grad, a native shape;
anything else takes a numpy / torch restatement with the same outputs and the same NaN conventions.  ``last_path[name]`` tells which of
the two ("fused" / "torch") the last call of a function took.

Not here.  Plots and mdtraj I/O.  Every metric here is invariant under rigid motion; superposition, RMSD and RMSF of the same positions
are ``lam_slide_amd.superpose``.  ``run_tica``'s Koopman-reweighted
estimate over ``tica_features`` is ``koopman_tica.run_tica`` (``traj_analysis(..., tica_lagtime=)``); projections from any other model
enter ``traj_analysis`` as ``tics_ref`` / ``tics_model``.  Neither mdtraj nor deeptime was available where this was
written: the statements below are checked against numpy / scipy, parity with a live mdtraj was not checked."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import torsion_stats as _ts
from .peptide_loss import residue_tables
from .torsion_stats import _aatype_list, _index_table, fused_applies

last_path: Dict[str, str] = {}
MAX_P, MAX_R = _lib.PAIR_MAX_P, _lib.CA_MAX_R  # pairs of one call of lsl_pair_distances, selected atoms of a frame
PSEUDO_COUNT = 1e-6  # discretize_features' pseudo_count
# residue_constants.atom_types: the names of the 37 atom37 slots (the first letter is the element atom14_to_mdtraj gives the atom)
ATOM37_NAMES = ("N", "CA", "C", "CB", "O", "CG", "CG1", "CG2", "OG", "OG1", "SG", "CD", "CD1", "CD2", "ND1", "ND2", "OD1", "OD2", "SD", "CE", "CE1",
                "CE2", "CE3", "NE", "NE1", "NE2", "OE1", "OE2", "CH2", "NH1", "NH2", "OH", "CZ", "CZ2", "CZ3", "NZ", "OXT")


# ---- index tables: all index a frame [R * 14, 3] of atom14 positions ----
def ca_atoms(aatype, tables=None) -> np.ndarray:
    """int64 [R]: the index ``r * 14 + slot`` of each residue's C-alpha (atom37 slot 1) - ``topology.select("name CA")``."""
    t = residue_tables(tables)
    return np.asarray([r * 14 + int(t.a37to14[aa, 1]) for r, aa in enumerate(_aatype_list(aatype))], dtype=np.int64)


def ca_pair_table(R: int, offset: int = 3) -> np.ndarray:
    """int64 [P, 2]: the residue pairs (i, j) with j >= i + offset + 1, i major - the column order of ``compute_pairwise_distances``.
    ``ca_atoms(aatype)[ca_pair_table(R)]`` indexes a frame.  Empty ([0, 2]) for R <= offset + 1: every tetrapeptide."""
    return np.asarray([(i, j) for i in range(int(R)) for j in range(i + int(offset) + 1, int(R))], dtype=np.int64).reshape(-1, 2)


class BackboneQuads(NamedTuple):
    phi: np.ndarray
    psi: np.ndarray
    omega: np.ndarray


def backbone_torsion_quads(aatype, tables=None) -> BackboneQuads:
    """(phi, psi, omega), int32 [R - 1, 4] each, in residue order as ``md.compute_phi`` / ``compute_psi`` / ``compute_omega`` return them:
    phi of residues 1..R-1 (C of the residue before, N, CA, C), psi of residues 0..R-2 (N, CA, C, N of the next residue), omega of residues
    0..R-2 (CA, C, N and CA of the next residue).  None across a residue of the unknown type, which has no atoms."""
    t = residue_tables(tables)
    aa = _aatype_list(aatype)
    at = lambda r, slot37: r * 14 + int(t.a37to14[aa[r], slot37])  # noqa: E731  (N, CA, C are atom37 slots 0, 1, 2)
    backbone = [all(t.m37[a, s] != 0 for s in (0, 1, 2)) for a in aa]
    phi, psi, omega = [], [], []
    for i in range(len(aa) - 1):
        if backbone[i] and backbone[i + 1]:
            phi.append((at(i, 2), at(i + 1, 0), at(i + 1, 1), at(i + 1, 2)))
            psi.append((at(i, 0), at(i, 1), at(i, 2), at(i + 1, 0)))
            omega.append((at(i, 1), at(i, 2), at(i + 1, 0), at(i + 1, 1)))
    return BackboneQuads(*(np.asarray(q, dtype=np.int32).reshape(-1, 4) for q in (phi, psi, omega)))


def tica_atom_selection(aatype, tables=None) -> np.ndarray:
    """int64 [n]: the atoms of ``atom14_to_mdtraj``'s topology (``torsion_stats.topology_atoms``: residues in order, the set atom37 slots in
    atom37 order) whose atom37 name does not start with ``O`` - ``select("symbol == C or symbol == N or symbol == S")`` there, where an
    atom's element is the first letter of its name."""
    t = residue_tables(tables)
    out = []
    for r, aa in enumerate(_aatype_list(aatype)):
        out.extend(r * 14 + int(t.a37to14[aa, s]) for s in range(37) if t.m37[aa, s] != 0 and not ATOM37_NAMES[s].startswith("O"))
    return np.asarray(out, dtype=np.int64)


def triu_pairs(idx) -> np.ndarray:
    """int64 [k (k - 1) / 2, 2]: (idx[m], idx[n]) for m < n in ``np.triu_indices(k, 1)`` order - the columns of ``tica_utils.distances``."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    m, n = np.triu_indices(idx.size, k=1)
    return np.stack([idx[m], idx[n]], axis=1).reshape(-1, 2)


class StructureTables:
    """The index tables of one peptide, built once (host int32 arrays) and put on a device once (``on(device)``): ``ca`` [R],
    ``ca_pairs`` [P, 2] (frame indices of ``ca_pair_table``, P may be 0), ``quads`` [3 (R - 1), 4] = phi | psi | omega with ``n_tors``
    rows each, ``rama`` [2, 4] = the first phi and the first psi, ``tica_pairs`` = ``triu_pairs(tica_atom_selection(aatype))``, ``topology``
    [n] = ``topology_atoms(aatype)`` (the heavy atoms ``superpose.superpose_atom14`` fits on) and ``padding`` bool [R * 14] = every other slot.  Pass it
    where a function takes ``aatype`` to keep the tables on the device between calls: with it, ``traj_analysis`` uploads nothing."""

    def __init__(self, aatype, tables=None, offset: int = 3) -> None:
        i32 = lambda a, w: np.ascontiguousarray(np.asarray(a).reshape(-1, w).astype(np.int32)) if w else np.ascontiguousarray(np.asarray(a, dtype=np.int32))  # noqa: E731
        self.aatype = _aatype_list(aatype)
        self.R = len(self.aatype)
        ca = ca_atoms(self.aatype, tables)
        bb = backbone_torsion_quads(self.aatype, tables)
        self.n_tors = int(bb.phi.shape[0])
        self.ca = i32(ca, 0)
        self.ca_pairs = i32(ca[ca_pair_table(self.R, offset)], 2)
        self.quads = i32(np.concatenate(bb), 4)
        self.rama = i32(np.concatenate([bb.phi[:1], bb.psi[:1]]), 4)
        self.tica_pairs = i32(triu_pairs(tica_atom_selection(self.aatype, tables)), 2)
        self.topology = i32(_ts.topology_atoms(self.aatype, tables), 0)
        self.padding = np.ones(self.R * 14, dtype=bool)
        self.padding[self.topology] = False
        self._on: dict = {}

    def on(self, device) -> Dict[str, Tensor]:
        device = torch.device(device)
        if device not in self._on:
            names = ("ca", "ca_pairs", "quads", "rama", "tica_pairs", "topology", "padding")
            self._on[device] = {k: torch.from_numpy(getattr(self, k)).to(device) for k in names}
            if device.type == "cuda":
                _ts._pair01_on(device)  # (joint_density_js' pair table: with the tables on the device, nothing is uploaded later)
        return self._on[device]


def _tables_of(aatype, tables=None) -> StructureTables:
    return aatype if isinstance(aatype, StructureTables) else StructureTables(aatype, tables)


def _frames(pos: Tensor, name: str = "pos") -> Tensor:
    if pos.dim() == 4 and pos.shape[-2:] == (14, 3):
        pos = pos.reshape(pos.shape[0], -1, 3)  # [n, R, 14, 3] -> [n, R * 14, 3]
    if pos.dim() != 3 or pos.shape[-1] != 3 or pos.shape[0] < 1 or pos.shape[1] < 1:
        raise ValueError(f"expected {name} [n, R, 14, 3] or [n, A, 3], got {tuple(pos.shape)}")
    return pos


# ---- a. pair distances ----
def _pairs_torch(pos: Tensor, pairs: Tensor) -> Tensor:
    d = pos[..., pairs[:, 0], :] - pos[..., pairs[:, 1], :]
    return torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _pairs_fused(pos: Tensor, pairs_host: np.ndarray, pairs_dev: Tensor) -> Tensor:
    A, P = int(pos.shape[-2]), int(pairs_host.shape[0])
    p = pos.detach().contiguous()
    F = p.numel() // (A * 3)
    parts = []
    for p0 in range(0, P, MAX_P):  # (a column's bits do not depend on the columns beside it)
        k = min(MAX_P, P - p0)
        part = torch.empty(F, k, dtype=torch.float32, device=p.device)
        host = pairs_host[p0:p0 + k]
        _lib.call(p.device, "lsl_pair_distances", p.data_ptr(), pairs_dev[p0:p0 + k].data_ptr(), host.ctypes.data, F, A, k, part.data_ptr())
        parts.append(part)
    out = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
    return out.reshape(*p.shape[:-2], P)


def _pairs(pos: Tensor, pairs_host: np.ndarray, pairs_dev: Optional[Tensor], name: str = "pair_distances") -> Tensor:
    A = int(pos.shape[-2])
    if pairs_host.min() < 0 or pairs_host.max() >= A:
        raise ValueError(f"pairs holds an index outside the frame's atoms 0..{A - 1}")
    if fused_applies(pos) and 1 <= A <= _lib.TORS_MAX_A and pos.numel() > 0:
        last_path[name] = "fused"
        return _pairs_fused(pos, pairs_host, pairs_dev if pairs_dev is not None else torch.from_numpy(pairs_host).to(pos.device))
    last_path[name] = "torch"
    return _pairs_torch(pos.detach(), torch.from_numpy(pairs_host.astype(np.int64)).to(pos.device))


def pair_distances(pos: Tensor, pairs) -> Tensor:
    """[..., A, 3], pairs [P, 2] (atom slots 0..A-1 of a frame; a host array, a list or a tensor) -> distances [..., P]:
    ``sqrt((dx dx + dy dy) + dz dz)`` of ``d = pos[.., pairs[p][0], :] - pos[.., pairs[p][1], :]``, float32 with every operation rounded on
    its own: ``np.linalg.norm(.., axis=-1)``.  An index outside the frame raises ValueError on either path.  Each call on the device form
    copies the table to the device (which waits for the stream); ``StructureTables`` keeps its tables there between calls."""
    if pos.dim() < 2 or pos.shape[-1] != 3:
        raise ValueError(f"expected pos [..., A, 3], got {tuple(pos.shape)}")
    return _pairs(pos, _index_table(pairs, 2, "pairs"), None)


# ---- b. per-frame statistics of the selected atoms ----
class CaFrameStats(NamedTuple):
    """``rg`` float32 [n]; ``flags`` int32 [n] (bit 0: a clash, bit 1: a broken bond; 0: a valid frame); ``tally`` int64 [4] = (frames, frames
    with a clash, frames with a broken bond, valid frames); ``contacts`` int64 [R, R], cell (i, j), i < j: the frames with d_ij below the
    contact threshold, the other cells 0."""
    rg: Tensor
    flags: Tensor
    tally: Tensor
    contacts: Tensor


def _f32(v) -> float:
    return float(np.float32(v))  # (the reference compares float32 distances with the threshold as a float32)


def _ca_stats_torch(pos: Tensor, sel: Tensor, clash: float, brk: float, contact: float) -> CaFrameStats:
    x = pos[:, sel]  # [n, R, 3]
    n, R = int(x.shape[0]), int(x.shape[1])
    x64 = x.double()
    c = x64 - x64.sum(dim=1, keepdim=True) / R
    rg = torch.sqrt((c * c).sum(dim=(1, 2)) / R).float()
    d = x[:, :, None, :] - x[:, None, :, :]
    d = torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])  # [n, R, R]
    upper = torch.ones(R, R, dtype=torch.bool, device=x.device).triu(1)
    has_clash = ((d < clash) & upper).flatten(1).any(dim=1)
    i = torch.arange(R - 1, device=x.device)
    has_break = (d[:, i, i + 1] > brk).any(dim=1) if R > 1 else torch.zeros(n, dtype=torch.bool, device=x.device)
    flags = has_clash.int() + 2 * has_break.int()
    tally = torch.stack([torch.full((), n, dtype=torch.int64, device=x.device), has_clash.sum(), has_break.sum(), (flags == 0).sum()])
    return CaFrameStats(rg, flags, tally, ((d < contact) & upper).sum(dim=0))


def _ca_stats(pos: Tensor, sel_host: np.ndarray, sel_dev: Optional[Tensor], clash: float, brk: float, contact: float) -> CaFrameStats:
    n, A, R = int(pos.shape[0]), int(pos.shape[1]), int(sel_host.shape[0])
    if R < 1 or sel_host.min() < 0 or sel_host.max() >= A:
        raise ValueError(f"sel must hold at least one index of the frame's atoms 0..{A - 1}")
    clash, brk, contact = _f32(clash), _f32(brk), _f32(contact)
    if fused_applies(pos) and R <= MAX_R:
        dev = pos.device
        p = pos.detach().contiguous()
        sd = sel_dev if sel_dev is not None else torch.from_numpy(sel_host).to(dev)
        rg, flags = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        tally, contacts = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(R, R, dtype=torch.int64, device=dev)
        _lib.call(dev, "lsl_ca_frame_stats", p.data_ptr(), sd.data_ptr(), sel_host.ctypes.data, n, A, R, clash, brk, contact, rg.data_ptr(),
                  flags.data_ptr(), tally.data_ptr(), contacts.data_ptr())
        last_path["ca_frame_stats"] = "fused"
        return CaFrameStats(rg, flags, tally, contacts)
    last_path["ca_frame_stats"] = "torch"
    return _ca_stats_torch(pos.detach(), torch.from_numpy(sel_host.astype(np.int64)).to(pos.device), clash, brk, contact)


def ca_frame_stats(pos: Tensor, sel, clash_threshold: float = 0.3, bond_break_threshold: float = 0.419, contact_threshold: float = 1.0) -> CaFrameStats:
    """pos [n, A, 3] (or [n, R, 14, 3]), sel [R'] (atom slots of a frame: ``ca_atoms(aatype)``) -> :class:`CaFrameStats` of the selected
    atoms.  ``rg`` = ``sqrt(mean_i |x_i - mean_j x_j|^2)`` in float64 from the float32 coordinates, rounded once (``md.compute_rg``, unit
    masses); a clash is some pair i < j closer than ``clash_threshold``, a broken bond some consecutive pair farther than
    ``bond_break_threshold`` (``compute_validity``: NaN compares false on both); distances are those of :func:`pair_distances`.  The
    positions are in the units of the thresholds - the reference's are nanometres.  ``tally[3] / tally[0]`` is ``val_ca``,
    ``contacts / n`` the upper triangle of ``compute_contact_matrix``; tallies and contacts of chunks add exactly."""
    pos = _frames(pos)
    s = sel.detach().cpu().numpy() if torch.is_tensor(sel) else np.asarray(sel)
    if s.ndim != 1 or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"sel must be integers [R], got {s.dtype} {tuple(s.shape)}")
    return _ca_stats(pos, np.ascontiguousarray(s.astype(np.int32)), None, clash_threshold, bond_break_threshold, contact_threshold)


# ---- the TICA features ----
def _angles(pos: Tensor, quads_host: np.ndarray, quads_dev: Optional[Tensor]) -> Tuple[Tensor, str]:
    A = int(pos.shape[-2])
    if quads_host.min() < 0 or quads_host.max() >= A:
        raise ValueError(f"the torsion table holds an index outside the frame's atoms 0..{A - 1}")
    if fused_applies(pos) and A <= _lib.TORS_MAX_A and quads_host.shape[0] <= _lib.TORS_MAX_Q:
        qd = quads_dev if quads_dev is not None else torch.from_numpy(quads_host).to(pos.device)
        return _ts._dihedral_fused(pos, quads_host, qd), "fused"
    return _ts._dihedral_torch(pos.detach(), torch.from_numpy(quads_host.astype(np.int64)).to(pos.device)), "torch"


def tica_features(pos: Tensor, aatype, tables=None) -> Tensor:
    """pos [n, R, 14, 3] (or [n, R * 14, 3]), aatype [R] (or a :class:`StructureTables`) -> float32 [n, k (k - 1) / 2 + 6 (R - 1)]:
    ``tica_utils.tica_features`` - the distances of all pairs of the k atoms of :func:`tica_atom_selection` in ``np.triu_indices`` order,
    then sin phi | cos phi | sin psi | cos psi | sin omega | cos omega, each block in residue order.  Distances by
    :func:`pair_distances`, angles by ``dihedral_angles``, sine and cosine in torch."""
    st = _tables_of(aatype, tables)
    pos = _frames(pos)
    if st.n_tors < 1 or st.tica_pairs.shape[0] < 1:
        raise ValueError("tica_features needs at least two residues with backbone atoms")
    on = st.on(pos.device) if pos.is_cuda else {}
    d = _pairs(pos, st.tica_pairs, on.get("tica_pairs"), "tica_features")
    ang, path = _angles(pos, st.quads, on.get("quads"))
    if path != "fused":
        last_path["tica_features"] = "torch"
    k = st.n_tors
    phi, psi, omega = ang[:, :k], ang[:, k:2 * k], ang[:, 2 * k:]
    return torch.cat([d, torch.sin(phi), torch.cos(phi), torch.sin(psi), torch.cos(psi), torch.sin(omega), torch.cos(omega)], dim=-1)


# ---- c. histograms with one edge table per column ----
def column_edges(ref: Tensor, bins: int = 50) -> Tensor:
    """ref [n, Q] (or [n]) -> float64 [Q, bins] on its device with the bits of ``np.linspace(col.min(), col.max(), bins)`` of every column
    (the column's extremes taken to float64 first): ``i * step`` then ``+ lo`` as two roundings, ``step = (hi - lo) / (bins - 1)``, the last
    edge set to ``hi``; a zero step takes numpy's other branch, ``i / (bins - 1) * (hi - lo)``.  These are ``bins`` EDGES: the
    histograms built on them have ``bins - 1`` bins, as the reference's.  Nothing is read back."""
    bins = int(bins)
    if bins < 2:
        raise ValueError(f"bins = {bins}: at least two edges")
    x = ref.detach()
    x = x[:, None] if x.dim() == 1 else x
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"expected ref [n, Q], got {tuple(ref.shape)}")
    lo, hi = x.amin(dim=0).double(), x.amax(dim=0).double()
    div = torch.full((), bins - 1, dtype=torch.float64, device=x.device)  # (a tensor divisor: a true division, not a reciprocal)
    delta = hi - lo
    step = delta / div
    i = torch.arange(bins, dtype=torch.float64, device=x.device)
    e = torch.where((step == 0)[:, None], (i / div)[None, :] * delta[:, None], i[None, :] * step[:, None])
    e = e + lo[:, None]
    e[:, bins - 1] = hi
    return e


def _hist_columns_numpy(x: Tensor, edges: Tensor) -> Tensor:
    v, e = x.detach().cpu().double().numpy(), edges.detach().cpu().double().numpy()
    return torch.from_numpy(np.stack([np.histogram(v[:, q], bins=e[q])[0] for q in range(v.shape[1])]).astype(np.int64)).to(x.device)


def histogram_columns(x: Tensor, edges: Tensor, counts: Optional[Tensor] = None) -> Tensor:
    """x [n, Q], edges float64 [Q, cells + 1] (one ascending table per column) -> int64 [Q, cells]: column q's
    ``np.histogram(x[:, q], bins=edges[q])[0]`` - the last bin closed on the right, values outside the table and NaN dropped; equal to
    numpy's on the same values as integers.  ``counts`` (int64 [Q, cells] on x's device) is added to in place and returned: chunks of a
    trajectory accumulate exactly."""
    if x.dim() != 2 or edges.dim() != 2 or edges.shape[0] != x.shape[1] or edges.shape[1] < 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"expected x [n, Q] and edges [Q, cells + 1], got {tuple(x.shape)} and {tuple(edges.shape)}")
    n, Q, cells = int(x.shape[0]), int(x.shape[1]), int(edges.shape[1]) - 1
    if counts is None:
        counts = torch.zeros(Q, cells, dtype=torch.int64, device=x.device)
    elif counts.shape != (Q, cells) or counts.dtype != torch.int64 or counts.device != x.device or not counts.is_contiguous():
        raise ValueError(f"counts must be contiguous int64 [{Q}, {cells}] on {x.device}")
    tiles = -(-Q // max(1, min(Q, 4096 // (cells + 1))))
    if fused_applies(x) and fused_applies(edges, dtype=torch.float64) and edges.device == x.device and cells <= _lib.HIST_MAX_BINS and n < 2 ** 31 and tiles <= 65535:
        xc, ec = x.detach().contiguous(), edges.detach().contiguous()
        _lib.call(x.device, "lsl_histogram_columns", xc.data_ptr(), n, Q, ec.data_ptr(), cells, counts.data_ptr())
        last_path["histogram_columns"] = "fused"
    else:
        counts += _hist_columns_numpy(x, edges)
        last_path["histogram_columns"] = "torch"
    return counts


# ---- d. the Jensen-Shannon distance of density histograms ----
def _density(counts: Tensor, measure: Tensor, pseudo: float) -> Tensor:
    c = counts.double()
    return c / measure / c.sum(dim=-1, keepdim=True) + pseudo


def js_distance_density(counts_a: Tensor, counts_b: Tensor, measure: Tensor, pseudo: float = PSEUDO_COUNT) -> Tensor:
    """counts [..., cells] x 2 (int64), measure float64 [..., cells] (the cell sizes: ``np.diff(edges)``, or the flattened outer product of
    two of them for a 2-D table) -> float64 [...]: ``jensenshannon(h_a, h_b)`` with ``h = counts / measure / counts.sum() + pseudo`` -
    numpy's ``density=True`` histogram plus ``discretize_features``' pseudo-count.  A row without a count on either side, or with a cell of
    size zero, gives NaN, as the reference's arithmetic does."""
    if counts_a.shape != counts_b.shape or counts_a.shape != measure.shape or counts_a.dim() < 1 or counts_a.shape[-1] < 1:
        raise ValueError(f"expected two count tables and the cell sizes [..., cells] of one shape, got {tuple(counts_a.shape)}, "
                         f"{tuple(counts_b.shape)} and {tuple(measure.shape)}")
    cells = int(counts_a.shape[-1])
    if (fused_applies(counts_a, counts_b, dtype=torch.int64) and fused_applies(measure, dtype=torch.float64) and measure.device == counts_a.device
            and 0 < counts_a.numel() // cells < 2 ** 31):
        a, b, m = counts_a.contiguous(), counts_b.contiguous(), measure.detach().contiguous()
        out = torch.empty(a.shape[:-1], dtype=torch.float64, device=a.device)
        _lib.call(a.device, "lsl_js_distance_density", a.data_ptr(), b.data_ptr(), m.data_ptr(), a.numel() // cells, cells, float(pseudo), out.data_ptr())
        last_path["js_distance_density"] = "fused"
        return out
    last_path["js_distance_density"] = "torch"
    m = measure.detach().double().to(counts_a.device)
    return _ts._js_torch(_density(counts_a.detach(), m, float(pseudo)), _density(counts_b.detach().to(counts_a.device), m, float(pseudo)))


def density_js(ref: Tensor, model: Tensor, bins: int = 50) -> Tuple[Tensor, Tensor]:
    """ref [n, Q], model [m, Q] (or [n], [m]) -> (float64 [Q], their mean, float64 0-d): ``compute_js_distance`` - per column the
    Jensen-Shannon distance of the two density histograms on ``np.linspace(ref_col.min(), ref_col.max(), bins)`` (``bins - 1`` bins; model
    values outside the reference's range are dropped), pseudo-count 1e-6.  A constant reference column (every cell of size zero) gives
    NaN.  Nothing is read back."""
    r, m = (v[:, None] if v.dim() == 1 else v for v in (ref, model))
    if r.dim() != 2 or m.dim() != 2 or r.shape[1] != m.shape[1] or m.device != r.device:
        raise ValueError(f"expected ref [n, Q] and model [m, Q] on one device, got {tuple(ref.shape)} on {ref.device} and {tuple(model.shape)} on {model.device}")
    edges = column_edges(r, bins)
    cr = histogram_columns(r, edges)
    paths = {last_path["histogram_columns"]}
    cm = histogram_columns(m, edges)
    js = js_distance_density(cr, cm, torch.diff(edges, dim=1))
    last_path["density_js"] = "fused" if paths | {last_path["histogram_columns"], last_path["js_distance_density"]} == {"fused"} else "torch"
    return js, js.mean()


def _joint_counts(a: Tensor, b: Tensor, ea: Tensor, eb: Tensor) -> Tuple[Tensor, str]:
    """np.histogram2d(a, b, bins=(ea, eb))[0] as int64 [cells, cells] on a's device: ``lsl_histogram``'s pair form with one pair."""
    x = torch.stack([a.detach(), b.detach()], dim=1).contiguous()
    n, cells, dev = int(x.shape[0]), int(ea.numel()) - 1, x.device
    if fused_applies(x) and fused_applies(ea, eb, dtype=torch.float64) and ea.device == dev and cells <= _lib.HIST2_MAX_BINS and n < 2 ** 31:
        eac, ebc = ea.contiguous(), eb.contiguous()
        own = torch.zeros(2, cells, dtype=torch.int64, device=dev)  # (the 1-D counts the call also makes: not used)
        counts2 = torch.zeros(cells, cells, dtype=torch.int64, device=dev)
        _ts._hist_pair01(x, eac, own, eac, ebc, counts2)
        return counts2, "fused"
    v = x.cpu().double().numpy()
    c2 = np.histogram2d(v[:, 0], v[:, 1], bins=(ea.cpu().numpy(), eb.cpu().numpy()))[0]
    return torch.from_numpy(c2.astype(np.int64)).to(dev), "torch"


def joint_density_js(a_ref: Tensor, b_ref: Tensor, a_model: Tensor, b_model: Tensor, bins: int = 50) -> Tensor:
    """Four series [n], [n], [m], [m] -> float64 0-d: ``compute_joint_js_distance`` - the Jensen-Shannon distance of the two 2-D density
    histograms of (a, b) on ``np.linspace`` tables between the reference's extremes (``bins`` edges, ``(bins - 1)^2`` cells), pseudo-count
    1e-6.  bins - 1 <= 90 on the device form."""
    for v in (a_ref, b_ref, a_model, b_model):
        if v.dim() != 1 or v.shape[0] < 1 or v.device != a_ref.device:
            raise ValueError("expected four series [n], [n], [m], [m] on one device")
    if a_ref.shape != b_ref.shape or a_model.shape != b_model.shape:
        raise ValueError(f"the two coordinates of a side differ in length: {tuple(a_ref.shape)}, {tuple(b_ref.shape)}, {tuple(a_model.shape)}, {tuple(b_model.shape)}")
    edges = column_edges(torch.stack([a_ref.detach(), b_ref.detach()], dim=1), bins)
    cr, p1 = _joint_counts(a_ref, b_ref, edges[0], edges[1])
    cm, p2 = _joint_counts(a_model, b_model, edges[0], edges[1])
    measure = (torch.diff(edges[0])[:, None] * torch.diff(edges[1])[None, :]).reshape(1, -1)
    js = js_distance_density(cr.reshape(1, -1), cm.reshape(1, -1), measure)[0]
    last_path["joint_density_js"] = "fused" if {p1, p2, last_path["js_distance_density"]} == {"fused"} else "torch"
    return js


# ---- the seven numbers ----
def contact_rmse(contacts_ref: Tensor, n_ref: int, contacts_model: Tensor, n_model: int) -> Tensor:
    """Two contact-count tables [R, R] (``CaFrameStats.contacts``) and their frame counts -> float64 0-d:
    ``sqrt(2 / (R (R - 1)) sum (c_ref - c_model)^2)`` of the contact rates ``contacts / n``; 0 for R < 2, as the reference's ``except`` gives
    (its division by zero raises)."""
    R = int(contacts_ref.shape[-1])
    if contacts_ref.shape != (R, R) or contacts_model.shape != (R, R) or int(n_ref) < 1 or int(n_model) < 1:
        raise ValueError(f"expected two tables [R, R] and positive frame counts, got {tuple(contacts_ref.shape)}, {tuple(contacts_model.shape)}, {n_ref}, {n_model}")
    if R < 2:
        return torch.zeros((), dtype=torch.float64, device=contacts_ref.device)
    diff = contacts_ref.double() / float(n_ref) - contacts_model.double() / float(n_model)
    return torch.sqrt(2.0 / (R * (R - 1)) * (diff * diff).sum())


def traj_analysis(pos_model: Tensor, pos_ref: Tensor, aatype, tics_ref: Optional[Tensor] = None, tics_model: Optional[Tensor] = None,
                  bins: int = 50, tables=None, *, tica_lagtime: Optional[int] = None, tica_dim: int = 40) -> Dict[str, Tensor]:
    """``utils/traj_utils.py:traj_analysis`` behind the TICA model: pos_model [m, R, 14, 3], pos_ref [n, R, 14, 3] (atom14 positions in
    nanometres, or [.., R * 14, 3]), aatype [R] or a :class:`StructureTables` of it -> {name: float64 0-d tensor on the positions' device}:

      ramachandran_js  ``compute_joint_js_distance`` of (phi[:, 0], psi[:, 0]) of the reference and the model
      pwd_js, rg_js    ``compute_js_distance`` of the C-alpha distances of :func:`ca_pair_table` and of the radius of gyration.  The
                       reference computes both in one ``try``: with no C-alpha pair (R <= 4: every tetrapeptide) ``np.stack([])`` raises
                       and BOTH become 0.  That is reproduced here - an empty pair table gives pwd_js = rg_js = 0; ``density_js`` on
                       ``ca_frame_stats(...).rg`` gives the distance itself.
      val_ca           the model's valid frames over its frames: ``tally[3] / tally[0]``
      rmse_contact     ``sqrt(2 / (R (R - 1)) sum (c_ref - c_model)^2)`` of the contact rates, from the integer tables; 0 for R < 2, as the
                       reference's ``except`` gives
      tic_js, tic2d_js ``compute_js_distance`` of the first two TIC columns and ``compute_joint_js_distance`` of the two.  From the caller's
                       projections when ``tics_ref`` [n, >= 2] and ``tics_model`` [m, >= 2] are given (float32 on the device, from any
                       model); else, when ``tica_lagtime`` is given, from positions alone as the reference does: ``tica_features`` of both
                       trajectories, ``koopman_tica.run_tica(ref_features, tica_lagtime, tica_dim)``, both projected with that model
                       (``tica_lagtime >= n`` raises ValueError).  With neither the two keys are absent.

    On the device form nothing is read back and, when ``aatype`` is a :class:`StructureTables` already ``on`` the device, nothing is
    uploaded: no host synchronisation - except, with ``tica_lagtime``, the two host eigenproblems of ``run_tica`` (the Koopman step and
    ``solve_tica``) with their copies (``koopman_tica._to_host`` / ``_to_device``).  ``tables``: the residue tables, for building the
    index tables from a plain ``aatype``."""
    st = _tables_of(aatype, tables)
    pm, pr = _frames(pos_model, "pos_model"), _frames(pos_ref, "pos_ref")
    dev, R = pm.device, st.R
    if pr.device != dev or pm.shape[1] != R * 14 or pr.shape[1] != R * 14:
        raise ValueError(f"expected both trajectories [.., {R} * 14, 3] on one device, got {tuple(pos_model.shape)} on {dev} and {tuple(pos_ref.shape)} on {pr.device}")
    if st.rama.shape[0] != 2:
        raise ValueError("ramachandran_js needs two consecutive residues with backbone atoms (the reference reads phi[:, 0] and psi[:, 0])")
    if (tics_ref is None) != (tics_model is None):
        raise ValueError("give both tics_ref and tics_model, or neither")
    on = st.on(dev) if dev.type == "cuda" else {}
    paths = set()
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    out: Dict[str, Tensor] = {}

    ar, p = _angles(pr, st.rama, on.get("rama"))
    paths.add(p)
    am, p = _angles(pm, st.rama, on.get("rama"))
    paths.add(p)
    out["ramachandran_js"] = joint_density_js(ar[:, 0], ar[:, 1], am[:, 0], am[:, 1], bins)
    paths.add(last_path["joint_density_js"])

    sr = _ca_stats(pr, st.ca, on.get("ca"), 0.3, 0.419, 1.0)
    paths.add(last_path["ca_frame_stats"])
    sm = _ca_stats(pm, st.ca, on.get("ca"), 0.3, 0.419, 1.0)
    paths.add(last_path["ca_frame_stats"])
    if st.ca_pairs.shape[0] == 0:
        out["pwd_js"], out["rg_js"] = zero, zero.clone()
    else:
        dr = _pairs(pr, st.ca_pairs, on.get("ca_pairs"))
        paths.add(last_path["pair_distances"])
        dm = _pairs(pm, st.ca_pairs, on.get("ca_pairs"))
        paths.add(last_path["pair_distances"])
        out["pwd_js"] = density_js(dr, dm, bins)[1]
        paths.add(last_path["density_js"])
        out["rg_js"] = density_js(sr.rg, sm.rg, bins)[1]
        paths.add(last_path["density_js"])
    if tics_ref is None and tica_lagtime is not None:
        from . import koopman_tica
        if not 1 <= int(tica_lagtime) < int(pr.shape[0]):
            raise ValueError(f"tica_lagtime = {tica_lagtime} outside 1..n_ref-1 = {int(pr.shape[0]) - 1}: the window has n_ref - tica_lagtime rows")
        fr, fm = tica_features(pr, st), tica_features(pm, st)
        model = koopman_tica.run_tica(fr, int(tica_lagtime), int(tica_dim))
        paths.add(koopman_tica.last_path["run_tica"])
        if model.dim < 2:
            raise ValueError(f"the fitted TICA model has {model.dim} component: tic2d_js needs two (tica_dim = {tica_dim})")
        tics_ref = model.transform(fr)
        paths.add(koopman_tica.last_path["transform"])
        tics_model = model.transform(fm)
        paths.add(koopman_tica.last_path["transform"])
    if tics_ref is not None:
        if tics_ref.dim() != 2 or tics_model.dim() != 2 or tics_ref.shape[1] < 2 or tics_model.shape[1] < 2:
            raise ValueError(f"expected tics_ref [n, >= 2] and tics_model [m, >= 2], got {tuple(tics_ref.shape)} and {tuple(tics_model.shape)}")
        tr, tm = tics_ref[:, :2], tics_model[:, :2]
        out["tic_js"] = density_js(tr, tm, bins)[1]
        paths.add(last_path["density_js"])
        out["tic2d_js"] = joint_density_js(tr[:, 0], tr[:, 1], tm[:, 0], tm[:, 1], bins)
        paths.add(last_path["joint_density_js"])
    out["val_ca"] = sm.tally[3].double() / sm.tally[0].double()
    out["rmse_contact"] = contact_rmse(sr.contacts, int(pr.shape[0]), sm.contacts, int(pm.shape[0]))
    last_path["traj_analysis"] = "fused" if paths == {"fused"} else "torch"
    keys = ("ramachandran_js", "pwd_js", "rg_js", "tic_js", "tic2d_js", "val_ca", "rmse_contact")  # the reference's order
    return {k: out[k] for k in keys if k in out}
