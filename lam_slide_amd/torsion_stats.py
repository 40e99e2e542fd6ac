"""The evaluation tail of the peptide family: torsion statistics of a sampled trajectory, on the device.

  dihedral_angles     <- the torsion features ``analysis.get_featurized_traj`` reads back through pyemma / mdtraj: the four-point
                         dihedral of a general table of atom quadruples (``topology_atoms`` maps a featurizer's own ``angle_indexes``
                         to it; ``eval_torsion_quads`` builds phi / psi / chi tables from the residue tables for callers without pyemma)
  angle_histograms    <- ``np.histogram(x, range=, bins=100)`` of every torsion and ``np.histogram2d(.., bins=50)`` of chosen pairs
                         (eval_peptide.py:114-129); with a caller-given ``range`` the same call serves ``TICA-0`` / ``TICA-0,1``
  js_distance         <- ``scipy.spatial.distance.jensenshannon`` of two count tables, row by row (``out["JSD"]``)
  lagged_products     <- ``statsmodels.tsa.stattools.acovf(x, demean=False, adjusted=True, nlag=)``
  decorrelation       <- ``(acovf(sin) + acovf(cos) - baseline) / (1 - baseline)`` (eval_peptide.py:138-182), float32
  TorsionStats        <- the accumulation over rollouts: ``update(pos)`` adds a chunk of frames' counts on the device, ``jsd(reference)``
                         returns the ``out["JSD"]`` dict, ``summary_metrics`` the BB / SC / ALL means of ``calc_summary_metrics``

The device form is liblamslide_hip.so (``lsl_dihedral_angles`` / ``lsl_histogram`` / ``lsl_lag_products`` / ``lsl_js_distance``,
csrc/k_torsstat.hip.h): counts are integers (exact, equal to numpy's on the same float32 values), every float is a sum in a fixed order
(the same bits in any batch).  Each primitive runs it when its tensors are float32 (counts: integers) on the GPU, nothing requires grad
and the shape is native; otherwise a numpy / torch restatement runs, with the same outputs and the same NaN conventions.
``last_path[name]`` tells which of the two ("fused" / "torch") the last call of a primitive took.  The TICA model, its projection and
the state statistics behind it are ``lam_slide_amd.tica``.
"""
from __future__ import annotations

import math
from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .peptide_loss import ResidueTables, residue_tables

PI = math.pi
last_path: Dict[str, str] = {}
LAG_WORKSPACE_BYTES = 256 << 20  # lagged_products splits the channels of a call so that the fp64 segment sums stay below this


# ---- quadruple tables ----
def _aatype_list(aatype) -> List[int]:
    a = aatype.detach().cpu().numpy() if torch.is_tensor(aatype) else np.asarray(aatype)
    a = a.reshape(-1).astype(np.int64)
    if a.size < 1 or a.min() < 0 or a.max() > 20:
        raise ValueError("aatype must hold residue types 0..20 of one peptide [R]")
    return [int(v) for v in a]


def topology_atoms(aatype, tables=None) -> np.ndarray:
    """For each atom of the heavy-atom topology that the reference's ``atom14_to_mdtraj`` (modules/sampling.py) builds - residues in
    order, within a residue the atom37 slots whose mask is set, in atom37 order - its index ``r * 14 + slot`` into a frame [R * 14, 3]
    of atom14 positions.  int64 [n_atoms]: ``topology_atoms(...)[featurizer.active_features[i].angle_indexes]`` is a ``quads`` table
    whose features and order are pyemma's by construction."""
    t = residue_tables(tables)
    out = []
    for r, aa in enumerate(_aatype_list(aatype)):
        out.extend(r * 14 + int(t.a37to14[aa, s]) for s in range(37) if t.m37[aa, s] != 0)
    return np.asarray(out, dtype=np.int64)


def eval_torsion_quads(aatype, tables=None, sidechains: bool = True) -> Tuple[np.ndarray, List[str]]:
    """(quads int32 [Q, 4], labels) of the evaluation's torsions from the residue tables alone: phi of residues 1..R-1 (C of the residue
    before, N, CA, C) and psi of residues 0..R-2 (N, CA, C, N of the next residue), interleaved (phi 1, psi 0, phi 2, psi 1, ...; none
    across a residue of the unknown type, which has no atoms), then - ``sidechains`` - chi1..chi4 of each residue in residue order,
    where the chi mask of the type counts it and the atom37 mask holds its four atoms.  Labels are "PHI r" / "PSI r" / "CHIk r"
    (``summary_metrics`` groups by these words).

    This is the set pyemma's backbone and side-chain torsion features describe (psi from the next residue's N, not from O as the seven
    torsions of ``PeptideLoss``).  Neither pyemma nor mdtraj was available where this was written: the ORDER was not compared against
    ``feats.describe()``.  Where it matters (a stored MD reference in pyemma's order), build ``quads`` from the featurizer's own
    ``angle_indexes`` with :func:`topology_atoms`."""
    t = residue_tables(tables)
    aa = _aatype_list(aatype)
    R = len(aa)
    at = lambda r, slot37: r * 14 + int(t.a37to14[aa[r], slot37])  # noqa: E731  (N, CA, C are atom37 slots 0, 1, 2)
    backbone = [all(t.m37[a, s] != 0 for s in (0, 1, 2)) for a in aa]  # (the unknown type has no atoms: no torsion through it)
    quads, labels = [], []
    for i in range(R - 1):
        if not (backbone[i] and backbone[i + 1]):
            continue
        quads.append((at(i, 2), at(i + 1, 0), at(i + 1, 1), at(i + 1, 2)))
        labels.append(f"PHI {i + 1}")
        quads.append((at(i, 0), at(i, 1), at(i, 2), at(i + 1, 0)))
        labels.append(f"PSI {i}")
    if sidechains:
        for r in range(R):
            for k in range(4):
                slots = [int(s) for s in t.chi_idx[aa[r], k]]
                if t.chi_mask[aa[r], k] != 0 and all(t.m37[aa[r], s] != 0 for s in slots):
                    quads.append(tuple(at(r, s) for s in slots))
                    labels.append(f"CHI{k + 1} {r}")
    return np.asarray(quads, dtype=np.int32).reshape(-1, 4), labels


# ---- dispatch ----
def fused_applies(*tensors: Tensor, dtype: torch.dtype = torch.float32) -> bool:
    """The dispatch rule: every tensor of ``dtype`` on the same GPU, nothing requires grad; each function adds its own limits."""
    return _lib.device_form(*tensors, dtype=dtype)


def _index_table(table, width: int, name: str) -> np.ndarray:
    """An index table as a contiguous host int32 array [rows, width] (a device tensor is copied back: pass a host table to avoid it)."""
    a = table.detach().cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
    if a.ndim != 2 or a.shape[1] != width or a.shape[0] < 1:
        raise ValueError(f"{name} must be [rows, {width}], got {tuple(a.shape)}")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must hold integers, got {a.dtype}")
    return np.ascontiguousarray(a.astype(np.int32))


def _edges(lo_hi, bins: int, name: str = "range") -> np.ndarray:
    lo, hi = float(lo_hi[0]), float(lo_hi[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"{name} = ({lo}, {hi}) must be finite and ascending")
    if int(bins) < 1:
        raise ValueError(f"bins = {bins} must be positive")
    return np.linspace(lo, hi, int(bins) + 1)  # (float64: the edge table np.histogram builds for range=)


# ---- a. dihedral angles ----
def _dihedral_torch(pos: Tensor, quads: Tensor) -> Tensor:
    p = pos[..., quads, :]  # [..., Q, 4, 3]
    b1, b2, b3 = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 1, :], p[..., 3, :] - p[..., 2, :]
    c1, c2 = torch.linalg.cross(b2, b3), torch.linalg.cross(b1, b2)
    return torch.atan2((b1 * c1).sum(-1) * torch.linalg.norm(b2, dim=-1), (c1 * c2).sum(-1))


def _dihedral_fused(pos: Tensor, quads_host: np.ndarray, quads_dev: Tensor) -> Tensor:
    A, Q = int(pos.shape[-2]), int(quads_host.shape[0])
    p = pos.detach().contiguous()
    out = torch.empty(*p.shape[:-2], Q, dtype=torch.float32, device=p.device)
    _lib.call(p.device, "lsl_dihedral_angles", p.data_ptr(), quads_dev.data_ptr(), quads_host.ctypes.data, p.numel() // (A * 3), A, Q, out.data_ptr())
    return out


def dihedral_angles(pos: Tensor, quads) -> Tensor:
    """[..., A, 3], quads [Q, 4] (atom slots 0..A-1 of a frame; a host array, a list or a tensor) -> angles [..., Q] in radians in
    [-pi, pi]: ``atan2((b1 . c1) |b2|, c1 . c2)``, b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, c1 = b2 x b3, c2 = b1 x b2.  An index outside
    the frame raises ValueError on either path.  Each call on the device form copies the table to the device (a small pageable upload,
    which waits for the stream); ``TorsionStats`` keeps its tables on the device between calls."""
    if pos.dim() < 2 or pos.shape[-1] != 3:
        raise ValueError(f"expected pos [..., A, 3], got {tuple(pos.shape)}")
    qh = _index_table(quads, 4, "quads")
    A = int(pos.shape[-2])
    if qh.min() < 0 or qh.max() >= A:
        raise ValueError(f"quads holds an index outside the frame's atoms 0..{A - 1}")
    if fused_applies(pos) and 1 <= A <= _lib.TORS_MAX_A and qh.shape[0] <= _lib.TORS_MAX_Q and pos.numel() > 0:
        last_path["dihedral_angles"] = "fused"
        return _dihedral_fused(pos, qh, torch.from_numpy(qh).to(pos.device))
    last_path["dihedral_angles"] = "torch"
    return _dihedral_torch(pos, torch.from_numpy(qh.astype(np.int64)).to(pos.device))


# ---- b. histograms ----
def _hist_numpy(x: Tensor, edges: np.ndarray, pairs: Optional[np.ndarray], ea: Optional[np.ndarray], eb: Optional[np.ndarray]):
    """numpy on the host, on the values as they are (float64 holds every float32): [S, n, Q] -> int64 [S, Q, bins], [S, P, b2, b2]."""
    v = x.detach().cpu().double().numpy()
    S, n, Q = v.shape
    counts = np.stack([np.stack([np.histogram(v[s, :, q], bins=edges)[0] for q in range(Q)]) for s in range(S)]).astype(np.int64)
    counts2 = None
    if pairs is not None:
        counts2 = np.stack([np.stack([np.histogram2d(v[s, :, a], v[s, :, b], bins=(ea, eb))[0] for a, b in pairs]) for s in range(S)]).astype(np.int64)
    return counts, counts2


def _hist_add(x: Tensor, edges, pairs, ea, eb, counts: Tensor, counts2: Optional[Tensor], cache: Optional[dict] = None) -> str:
    """Add the counts of x [S, n, Q] to ``counts`` [S, Q, bins] (and ``counts2``) in place, on x's device; returns the path taken.
    edges / ea / eb host float64, pairs host int32 [P, 2] or None; ``cache`` keeps their device copies between calls."""
    bins, P = len(edges) - 1, 0 if pairs is None else int(pairs.shape[0])
    bins2 = 0 if pairs is None else len(ea) - 1
    S, n, Q = (int(v) for v in x.shape)
    native = (bins <= _lib.HIST_MAX_BINS and bins2 <= _lib.HIST2_MAX_BINS and S <= 65535 and P <= 65535 and n >= 1
              and -(-Q // max(1, min(Q, 8192 // bins))) <= 65535)
    if fused_applies(x) and native:
        dev = x.device
        key = ("hist", dev)
        if cache is None or key not in cache:
            on = {"edges": torch.from_numpy(edges).to(dev)}
            if pairs is not None:
                on.update(pairs=torch.from_numpy(pairs).to(dev), ea=torch.from_numpy(ea).to(dev), eb=torch.from_numpy(eb).to(dev))
            if cache is not None:
                cache[key] = on
        else:
            on = cache[key]
        xc = x.detach().contiguous()
        _lib.call(dev, "lsl_histogram", xc.data_ptr(), S, n, Q, on["edges"].data_ptr(), bins, counts.data_ptr(),
                  on["pairs"].data_ptr() if P else None, pairs.ctypes.data if P else None, P,
                  on["ea"].data_ptr() if P else None, on["eb"].data_ptr() if P else None, bins2, counts2.data_ptr() if P else None)
        return "fused"
    c, c2 = _hist_numpy(x, edges, pairs, ea, eb)
    counts += torch.from_numpy(c).to(counts.device)
    if c2 is not None:
        counts2 += torch.from_numpy(c2).to(counts2.device)
    return "torch"


_PAIR01 = np.array([[0, 1]], dtype=np.int32)
_pair01_dev: dict = {}


def _pair01_on(dev) -> Tensor:
    """The pair table [[0, 1]] on ``dev``: uploaded once per device (a caller that must not upload later asks for it ahead)."""
    if dev not in _pair01_dev:
        _pair01_dev[dev] = torch.from_numpy(_PAIR01).to(dev)
    return _pair01_dev[dev]


def _hist_pair01(x: Tensor, edges: Tensor, counts: Tensor, ea: Optional[Tensor] = None, eb: Optional[Tensor] = None,
                 counts2: Optional[Tensor] = None) -> None:
    """``lsl_histogram`` of one series with the one pair (0, 1), every table already on the device: x float32 [n, Q] contiguous, ``counts``
    int64 [Q, bins] += np.histogram of each column on ``edges`` (float64 [bins + 1]); with ``ea`` / ``eb`` (float64 [bins2 + 1]) also
    ``counts2`` int64 [bins2, bins2] += np.histogram2d(x[:, 0], x[:, 1], bins=(ea, eb))[0].  The caller has checked the native form."""
    two, dev = ea is not None, x.device
    _lib.call(dev, "lsl_histogram", x.data_ptr(), 1, int(x.shape[0]), int(x.shape[1]), edges.data_ptr(), edges.numel() - 1, counts.data_ptr(),
              _pair01_on(dev).data_ptr() if two else None, _PAIR01.ctypes.data if two else None, 1 if two else 0,
              ea.data_ptr() if two else None, eb.data_ptr() if two else None, ea.numel() - 1 if two else 0, counts2.data_ptr() if two else None)


def _hist_setup(Q: int, bins, pairs, bins2, range, range2):
    edges = _edges(range, bins)
    if pairs is None:
        return edges, None, None, None
    ph = _index_table(pairs, 2, "pairs")
    if ph.min() < 0 or ph.max() >= Q:
        raise ValueError(f"pairs holds a column outside 0..{Q - 1}")
    ra, rb = (range, range) if range2 is None else range2
    return edges, ph, _edges(ra, bins2, "range2[0]"), _edges(rb, bins2, "range2[1]")


def angle_histograms(angles: Tensor, bins: int = 100, pairs=None, bins2: int = 50, range: Tuple[float, float] = (-PI, PI),
                     range2: Optional[Tuple[Tuple[float, float], Tuple[float, float]]] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """angles [n, Q] or [S, n, Q] -> (counts int64 [(S,) Q, bins], counts2 int64 [(S,) P, bins2, bins2] or None): column q's
    ``np.histogram(angles[:, q], range=range, bins=bins)[0]`` and, for ``pairs`` [P, 2] of columns, ``np.histogram2d(angles[:, a],
    angles[:, b], range=range2 or (range, range), bins=bins2)[0]``.  numpy's semantics exactly: float64 edges ``np.linspace(lo, hi,
    bins + 1)``, the last bin closed on the right, values outside the range and NaN dropped, a pair dropped when either coordinate is;
    the counts equal numpy's on the same values as integers.  Each call copies the edge and pair tables to the device (``TorsionStats``
    keeps them there between calls)."""
    if angles.dim() not in (2, 3):
        raise ValueError(f"expected angles [n, Q] or [S, n, Q], got {tuple(angles.shape)}")
    x = angles if angles.dim() == 3 else angles[None]
    S, n, Q = x.shape
    if n < 1 or Q < 1 or S < 1:
        raise ValueError(f"empty angles {tuple(angles.shape)}")
    edges, ph, ea, eb = _hist_setup(Q, bins, pairs, bins2, range, range2)
    counts = torch.zeros(S, Q, len(edges) - 1, dtype=torch.int64, device=x.device)
    counts2 = None if ph is None else torch.zeros(S, ph.shape[0], len(ea) - 1, len(eb) - 1, dtype=torch.int64, device=x.device)
    last_path["angle_histograms"] = _hist_add(x, edges, ph, ea, eb, counts, counts2)
    if angles.dim() == 2:
        return counts[0], None if counts2 is None else counts2[0]
    return counts, counts2


# ---- d. Jensen-Shannon distance ----
def _js_torch(a: Tensor, b: Tensor) -> Tensor:
    a, b = a.double(), b.double()
    p, q = a / a.sum(-1, keepdim=True), b / b.sum(-1, keepdim=True)
    m = (p + q) / 2
    nan = torch.full((), float("nan"), dtype=torch.float64, device=a.device)
    rel_entr = lambda v: torch.where(v > 0, v * torch.log(v / m), torch.where(v == 0, torch.zeros_like(v), nan))  # noqa: E731  (0 where v = 0, NaN where v is)
    left, right = rel_entr(p), rel_entr(q)
    js = left.sum(-1) + right.sum(-1)
    return torch.sqrt(torch.where(js < 0, torch.zeros_like(js), js) / 2)


def js_distance(counts_a: Tensor, counts_b: Tensor) -> Tensor:
    """[..., bins] x 2 (non-negative counts; flatten a 2-D table into a row first) -> float64 [...]:
    ``scipy.spatial.distance.jensenshannon(counts_a[r], counts_b[r])`` of every row - both rows over their sums, m = (p + q) / 2,
    ``sqrt((sum rel_entr(p, m) + sum rel_entr(q, m)) / 2)``, natural log.  A row that is all zero on either side gives NaN, as scipy."""
    if counts_a.shape != counts_b.shape or counts_a.dim() < 1 or counts_a.shape[-1] < 1:
        raise ValueError(f"expected two tables [..., bins] of one shape, got {tuple(counts_a.shape)} and {tuple(counts_b.shape)}")
    ints = (torch.int64, torch.int32)
    if (counts_a.is_cuda and counts_b.is_cuda and counts_a.device == counts_b.device and counts_a.dtype in ints and counts_b.dtype in ints
            and counts_a.numel() > 0 and counts_a.numel() // counts_a.shape[-1] < 2 ** 31):
        a, b = counts_a.to(torch.int64).contiguous(), counts_b.to(torch.int64).contiguous()
        dev, bins = a.device, int(a.shape[-1])
        out = torch.empty(a.shape[:-1], dtype=torch.float64, device=dev)
        _lib.call(dev, "lsl_js_distance", a.data_ptr(), b.data_ptr(), a.numel() // bins, bins, out.data_ptr())
        last_path["js_distance"] = "fused"
        return out
    last_path["js_distance"] = "torch"
    return _js_torch(counts_a.detach(), counts_b.detach().to(counts_a.device))


# ---- c. lagged products ----
def _lag_torch(x: Tensor, nlag: int) -> Tensor:
    """The direct sum in float64, rounded to x's dtype: [S, n, C] -> [S, C, nlag + 1]."""
    v = x.double()
    n = v.shape[1]
    out = torch.stack([(v[:, :n - k] * v[:, k:]).sum(dim=1) / (n - k) for k in np.arange(nlag + 1)], dim=-1)
    return out.to(x.dtype if x.dtype.is_floating_point else torch.float64)


def lagged_products(x: Tensor, nlag: int) -> Tensor:
    """x [n, C] or [S, n, C] -> [(S,) C, nlag + 1] with ``ac[k] = (sum_{t < n - k} x_t x_{t+k}) / (n - k)``: statsmodels'
    ``acovf(x, demean=False, adjusted=True, nlag=nlag)`` of every channel.  0 <= nlag < n.  The device form adds a lag's terms in t order, at
    most 448 in float32 behind one another, everything above in float64: within ``456 * 2^-24`` of the exact value for |x| <= 1, and
    the same bits for a series alone and inside a batch."""
    if x.dim() not in (2, 3):
        raise ValueError(f"expected x [n, C] or [S, n, C], got {tuple(x.shape)}")
    v = x if x.dim() == 3 else x[None]
    S, n, C = (int(d) for d in v.shape)
    nlag = int(nlag)
    if min(S, n, C) < 1:
        raise ValueError(f"empty x {tuple(x.shape)}")
    if not 0 <= nlag < n:
        raise ValueError(f"nlag = {nlag} outside 0..n-1 = {n - 1}: lag k has n - k terms")
    if fused_applies(v) and nlag + 1 <= _lib.LAG_MAX_LAGS and S <= _lib.LAG_MAX_ROWS:
        dev = v.device
        per_channel = _lib.load().lsl_lag_products_workspace_bytes(S, n, 1, nlag)
        step = max(1, min(C, LAG_WORKSPACE_BYTES // per_channel, _lib.LAG_MAX_ROWS // S))
        ws = torch.empty(per_channel * step, dtype=torch.uint8, device=dev)
        parts = []
        for c0 in np.arange(0, C, step):  # (a channel's bits do not depend on the channels beside it)
            vc = v.detach()[:, :, c0:c0 + step].contiguous()
            part = torch.empty(S, vc.shape[2], nlag + 1, dtype=torch.float32, device=dev)
            _lib.call(dev, "lsl_lag_products", vc.data_ptr(), S, n, vc.shape[2], nlag, part.data_ptr(), ws.data_ptr(), ws.numel())
            parts.append(part)
        out = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        last_path["lagged_products"] = "fused"
    else:
        out = _lag_torch(v.detach(), nlag)
        last_path["lagged_products"] = "torch"
    return out if x.dim() == 3 else out[0]


def decorrelation(angles: Tensor, nlag: int) -> Tensor:
    """angles [n, Q] or [S, n, Q] -> float32 [(S,) Q, nlag + 1]: ``(ac_sin + ac_cos - baseline) / (1 - baseline)`` with ac_* the lagged
    products of sin / cos of each torsion and ``baseline = mean(sin)^2 + mean(cos)^2`` (eval_peptide.py:138-155; the float16 cast the
    reference stores the curves through stays the caller's choice).  The means and the last line are float64."""
    if angles.dim() not in (2, 3):
        raise ValueError(f"expected angles [n, Q] or [S, n, Q], got {tuple(angles.shape)}")
    a = angles.detach() if angles.dim() == 3 else angles.detach()[None]
    Q = a.shape[2]
    sc = torch.cat([torch.sin(a), torch.cos(a)], dim=2)  # [S, n, 2Q]
    ac = lagged_products(sc, nlag).double()
    last_path["decorrelation"] = last_path["lagged_products"]
    mean = sc.double().mean(dim=1)
    base = (mean[:, :Q] ** 2 + mean[:, Q:] ** 2)[..., None]
    out = ((ac[:, :Q] + ac[:, Q:] - base) / (1 - base)).float()
    return out if angles.dim() == 3 else out[0]


# ---- the accumulator ----
class TorsionStats:
    """Torsion histograms of a trajectory that arrives in chunks (rollouts come one at a time; counts add exactly), in the spirit of
    ``DisplacementMeter``.  ``quads`` [Q, 4] and ``labels`` as :func:`eval_torsion_quads` returns them (or from pyemma's ``angle_indexes``
    and ``describe()``); ``pairs`` the columns of the joint histograms - the reference's ``i in [1, 3]``: columns (1, 2) and (3, 4);
    pairs beyond the Q columns are left out.

    ``update(pos)`` -> the chunk's angles [n, Q]; adds its counts to ``counts`` int64 [Q, bins] / ``counts2`` int64 [P, bins2, bins2] on
    ``pos``'s device - no synchronisation, no host round trip (the index and edge tables are put on the device once).
    ``jsd(reference)`` -> {label: distance, ..., "a|b": distance of the joint histograms}: the reference's ``out["JSD"]``; the one place
    that waits for the device.  ``path``: "fused" / "torch" of the last update."""

    def __init__(self, quads, labels: Sequence[str], bins: int = 100, pairs=((1, 2), (3, 4)), bins2: int = 50,
                 range: Tuple[float, float] = (-PI, PI)) -> None:
        self.quads = _index_table(quads, 4, "quads")
        self.labels = [str(s) for s in labels]
        Q = self.quads.shape[0]
        if len(self.labels) != Q:
            raise ValueError(f"{len(self.labels)} labels for {Q} quadruples")
        if self.quads.min() < 0:
            raise ValueError("quads holds a negative index")
        kept = [tuple(int(v) for v in p) for p in (pairs or ()) if max(p) < Q]
        self.edges, self.pairs, self.edges2a, self.edges2b = _hist_setup(Q, bins, kept or None, bins2, range, None)
        self.bins, self.bins2 = int(bins), int(bins2)
        self._on: dict = {}
        self.reset()

    def reset(self) -> None:
        self.counts: Optional[Tensor] = None
        self.counts2: Optional[Tensor] = None
        self.n_frames = 0
        self.path: Optional[str] = None

    @property
    def pair_labels(self) -> List[str]:
        return [] if self.pairs is None else ["|".join((self.labels[a], self.labels[b])) for a, b in self.pairs]

    def update(self, pos: Tensor) -> Tensor:
        if pos.dim() == 4:
            pos = pos.reshape(pos.shape[0], -1, 3)  # [n, R, 14, 3] -> [n, R * 14, 3]
        if pos.dim() != 3 or pos.shape[-1] != 3 or pos.shape[0] < 1:
            raise ValueError(f"expected pos [n, R, 14, 3] or [n, A, 3], got {tuple(pos.shape)}")
        A, Q, dev = int(pos.shape[1]), self.quads.shape[0], pos.device
        if self.quads.max() >= A:
            raise ValueError(f"quads holds an index outside the frame's atoms 0..{A - 1}")
        if self.counts is None:
            self.counts = torch.zeros(Q, self.bins, dtype=torch.int64, device=dev)
            self.counts2 = None if self.pairs is None else torch.zeros(self.pairs.shape[0], self.bins2, self.bins2, dtype=torch.int64, device=dev)
        elif self.counts.device != dev:
            raise RuntimeError(f"TorsionStats holds counts on {self.counts.device}, pos is on {dev}")
        if fused_applies(pos) and A <= _lib.TORS_MAX_A and Q <= _lib.TORS_MAX_Q:
            if ("quads", dev) not in self._on:
                self._on[("quads", dev)] = torch.from_numpy(self.quads).to(dev)
            angles = _dihedral_fused(pos, self.quads, self._on[("quads", dev)])
        else:
            angles = _dihedral_torch(pos.detach(), torch.from_numpy(self.quads.astype(np.int64)).to(dev))
        c2 = None if self.counts2 is None else self.counts2[None]
        self.path = _hist_add(angles[None], self.edges, self.pairs, self.edges2a, self.edges2b, self.counts[None], c2, self._on)
        self.n_frames += int(pos.shape[0])
        return angles

    def _tables(self, ref) -> Tuple[Tensor, Optional[Tensor]]:
        if isinstance(ref, TorsionStats):
            c, c2 = ref.counts, ref.counts2
        elif isinstance(ref, Mapping):
            c, c2 = ref["counts"], ref.get("counts2")
        else:
            c, c2 = ref
        as_t = lambda v: None if v is None else (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)))  # noqa: E731
        return as_t(c), as_t(c2)

    def jsd(self, reference) -> Dict[str, float]:
        """``reference``: the MD side's counts - another ``TorsionStats``, ``(counts, counts2)`` or {"counts", "counts2"} (tensors or
        arrays of this object's shapes; counts2 may be None when there are no pairs).  jensenshannon(reference, own), as the reference."""
        if self.counts is None:
            raise RuntimeError("jsd() before any update()")
        rc, rc2 = self._tables(reference)
        if rc is None or tuple(rc.shape) != tuple(self.counts.shape):
            raise ValueError(f"reference counts must be {tuple(self.counts.shape)}, got {None if rc is None else tuple(rc.shape)}")
        dev = self.counts.device
        out = dict(zip(self.labels, js_distance(rc.to(dev), self.counts).tolist()))
        if self.counts2 is not None:
            if rc2 is None or tuple(rc2.shape) != tuple(self.counts2.shape):
                raise ValueError(f"reference counts2 must be {tuple(self.counts2.shape)}, got {None if rc2 is None else tuple(rc2.shape)}")
            P = self.counts2.shape[0]
            out.update(zip(self.pair_labels, js_distance(rc2.to(dev).reshape(P, -1), self.counts2.reshape(P, -1)).tolist()))
        return out

    @staticmethod
    def summary_metrics(jsd_dicts: Sequence[Mapping[str, float]]) -> Dict[str, float]:
        """BB / SC / ALL of ``calc_summary_metrics`` (eval_peptide.py:378-404) over the ``jsd`` dicts of several peptides: the mean distance
        of the keys holding "PHI" or "PSI" (not the "a|b" joint ones), of the keys holding "CHI", and of all three kinds without the
        joint ones; "TICA-0" / "TICA-0,1" the means of those keys when every dict has them (``tica.tica_jsd`` returns them: merge its
        dict into ``jsd``'s).  An empty group gives NaN, like the mean of an empty list."""
        bb, sc, al = [], [], []
        for d in jsd_dicts:
            bb += [v for k, v in d.items() if ("PHI" in k or "PSI" in k) and "|" not in k]
            sc += [v for k, v in d.items() if "CHI" in k]
            al += [v for k, v in d.items() if ("PHI" in k or "PSI" in k or "CHI" in k) and "|" not in k]
        mean = lambda v: float(np.mean(v)) if len(v) else float("nan")  # noqa: E731
        out = {"BB": mean(bb), "SC": mean(sc), "ALL": mean(al)}
        for key in ("TICA-0", "TICA-0,1"):
            if len(jsd_dicts) and all(key in d for d in jsd_dicts):
                out[key] = mean([d[key] for d in jsd_dicts])
        return out


summary_metrics = TorsionStats.summary_metrics
