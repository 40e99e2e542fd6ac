"""The oracle of the structure-statistics tests (test_structure_stats.py, test_hip_structure_stats.py), written out in numpy / scipy
float64: pair distances, the radius of gyration, ``compute_validity``'s flags, the contact counts, ``compute_js_distance`` /
``compute_joint_js_distance`` through ``np.histogram(density=True)`` / ``np.histogram2d(density=True)`` and
``scipy.spatial.distance.jensenshannon``, the seven numbers of ``traj_analysis`` from given features - and a seeded chain generator.
Not a test module."""
import numpy as np
from scipy.spatial.distance import jensenshannon

CASES = ((1, 4, 0), (1, 5, 1), (257, 5, 2), (300, 9, 3), (1025, 12, 4), (2000, 20, 5))  # (n, R, seed)
CLASH, BREAK, CONTACT = 0.3, 0.419, 1.0  # compute_validity's and compute_contact_matrix's thresholds, nanometres
PSEUDO = 1e-6
NEAR = 2.0 ** -20  # a frame with a distance this close (relative) to a threshold may fall on either side in float32


def aatype(R):
    """A fixed mix of the twenty residue types, R long (restypes order A R N D C Q E G H I L K M F P S T W Y V)."""
    return [(3 * i + 1) % 20 for i in range(R)]


def chain(n, R, seed):
    """float32 [n, R, 14, 3], nanometres.  The C-alpha trace is a persistent random walk: step_0 a unit Gaussian direction, step_k =
    normalize(step_{k-1} + 0.9 g_k), bond lengths 0.38 + 0.02 z; C-alpha is slot 1, every other slot C-alpha + 0.15 Gaussian.  All from one
    ``default_rng(seed)`` in the order g [n, R - 1, 3], lengths [n, R - 1], offsets [n, R, 14, 3].  Frames clash (a walk that turns
    back), break (z > 1.95) and are valid, side by side.  Checked in float64 at CASES: every case with n > 1 holds clashing, broken
    and valid frames (58 / 57 / 196 of 300 at R = 9), contact rates run from 0.05 to 1, every C-alpha distance column four or more
    residues apart has a range above 1, and no C-alpha distance lies within 9.9e-7 (relative) of one of the three thresholds -
    outside NEAR, and three times the float32 error bound of a distance."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, max(R - 1, 0), 3))
    length = 0.38 + 0.02 * rng.standard_normal((n, max(R - 1, 0)))
    offsets = 0.15 * rng.standard_normal((n, R, 14, 3))
    ca = np.zeros((n, R, 3))
    step = None
    for k in range(R - 1):
        step = g[:, k] if k == 0 else step + 0.9 * g[:, k]
        step = step / np.linalg.norm(step, axis=-1, keepdims=True)
        ca[:, k + 1] = ca[:, k] + length[:, k, None] * step
    pos = ca[:, :, None, :] + offsets
    pos[:, :, 1] = ca
    return pos.astype(np.float32)


def dist64(pos, pairs):
    """|pos[:, a] - pos[:, b]| in float64 of the values as they are: pos [n, A, 3], pairs [P, 2] -> [n, P]."""
    p = np.asarray(pos, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    d = p[:, pairs[:, 0]] - p[:, pairs[:, 1]]
    return np.sqrt((d * d).sum(axis=-1))


def ca_stats64(pos, sel, clash=CLASH, brk=BREAK, contact=CONTACT):
    """(rg [n], flags [n], tally [4], contacts [R, R] int64, near [n] bool) of the selected atoms of pos [n, A, 3] in float64.  The
    thresholds are taken to float32 first (numpy compares a float32 distance with the threshold as a float32).  ``near``: the frames with a
    distance within NEAR (relative) of a threshold it is compared with."""
    x = np.asarray(pos, dtype=np.float64)[:, np.asarray(sel, dtype=np.int64)]
    n, R = x.shape[:2]
    clash, brk, contact = (float(np.float32(v)) for v in (clash, brk, contact))
    c = x - x.mean(axis=1, keepdims=True)
    rg = np.sqrt((c * c).sum(axis=(1, 2)) / R)
    d = np.sqrt(((x[:, :, None] - x[:, None, :]) ** 2).sum(axis=-1))
    i, j = np.triu_indices(R, k=1)
    du = d[:, i, j]  # [n, pairs]
    da = d[:, np.arange(R - 1), np.arange(1, R)] if R > 1 else np.zeros((n, 0))
    has_clash, has_break = (du < clash).any(axis=1), (da > brk).any(axis=1)
    flags = has_clash.astype(np.int32) + 2 * has_break.astype(np.int32)
    tally = np.array([n, has_clash.sum(), has_break.sum(), (flags == 0).sum()], dtype=np.int64)
    contacts = np.zeros((R, R), dtype=np.int64)
    contacts[i, j] = (du < contact).sum(axis=0)
    near = ((np.abs(du - clash) <= NEAR * clash).any(axis=1) | (np.abs(du - contact) <= NEAR * contact).any(axis=1)
            | (np.abs(da - brk) <= NEAR * brk).any(axis=1))
    return rg, flags, tally, contacts, near


def edges_np(ref, bins=50):
    """float64 [Q, bins]: np.linspace between the extremes of every column of ref [n, Q], the extremes taken to float64 first."""
    r = np.asarray(ref)
    r = r[:, None] if r.ndim == 1 else r
    return np.stack([np.linspace(np.float64(r[:, q].min()), np.float64(r[:, q].max()), bins) for q in range(r.shape[1])])


def density(values, edges):
    """discretize_features: np.histogram(density=True) + the pseudo-count, on the float64 copies of the values."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.histogram(np.asarray(values, dtype=np.float64), bins=edges, density=True)[0] + PSEUDO


def density_js_np(ref, model, edges):
    """compute_js_distance on given edge tables: ref [n, Q], model [m, Q], edges [Q, bins] -> (float64 [Q], their mean)."""
    ref, model = (np.asarray(v)[:, None] if np.asarray(v).ndim == 1 else np.asarray(v) for v in (ref, model))
    with np.errstate(divide="ignore", invalid="ignore"):
        js = np.array([jensenshannon(density(ref[:, q], edges[q]), density(model[:, q], edges[q])) for q in range(ref.shape[1])])
    return js, js.mean()


def density2(a, b, ea, eb):
    """discretize_features2d."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.histogram2d(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), bins=(ea, eb), density=True)[0] + PSEUDO


def joint_js_np(a_ref, b_ref, a_model, b_model, ea, eb):
    """compute_joint_js_distance on given edge tables."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(jensenshannon(density2(a_ref, b_ref, ea, eb).flatten(), density2(a_model, b_model, ea, eb).flatten()))


def rmse_contact_np(contacts_ref, n_ref, contacts_model, n_model):
    R = contacts_ref.shape[0]
    if R < 2:
        return 0.0
    return float(np.sqrt(2 / (R * (R - 1)) * np.sum((contacts_ref / n_ref - contacts_model / n_model) ** 2)))


def _square(d32):
    """float32 [n, R (R - 1) / 2] in np.triu_indices(R, 1) order -> the symmetric [n, R, R] with a zero diagonal, as torch.cdist's."""
    n, k = d32.shape
    R = int(round((1 + np.sqrt(1 + 8 * k)) / 2))
    assert R * (R - 1) // 2 == k
    d = np.zeros((n, R, R), dtype=np.float32)
    i, j = np.triu_indices(R, k=1)
    d[:, i, j] = d32
    d[:, j, i] = d32
    return d


def validity_np(d32, clash=CLASH, brk=BREAK):
    """compute_validity from the float32 C-alpha distances, line by line (the comparisons are float32 ones)."""
    distances = _square(np.asarray(d32, dtype=np.float32))
    num_atoms = distances.shape[1]
    has_clash = np.sum(distances < np.float32(clash), axis=(1, 2)) - num_atoms > 0
    adjacent = distances[:, np.arange(num_atoms - 1), np.arange(1, num_atoms)]
    has_bond_break = np.sum(adjacent > np.float32(brk), axis=1) > 0
    return float(np.mean(~(has_clash | has_bond_break)))


def contacts_np(d32, contact=CONTACT):
    """compute_contact_matrix's upper triangle as integer counts, from the float32 C-alpha distances."""
    distances = _square(np.asarray(d32, dtype=np.float32))
    R = distances.shape[1]
    out = np.zeros((R, R), dtype=np.int64)
    for i in range(R):
        for j in range(i + 1, R):
            out[i, j] = np.sum(distances[:, i, j] < np.float32(contact))
    return out


def traj_analysis_np(feat_ref, feat_model, bins=50):
    """The seven numbers from given features of the two sides - dicts with ``phi0``, ``psi0`` [n], ``pwd`` [n, P] (P may be 0), ``rg`` [n],
    ``ca_dist`` float32 [n, R (R - 1) / 2] (all C-alpha pairs, np.triu_indices order; R >= 2) and optionally ``tics`` [n, 2]:
    utils/traj_utils.py:traj_analysis line by line, the edge tables built from the reference's values as given."""
    r, m = feat_ref, feat_model
    e = edges_np(np.stack([r["phi0"], r["psi0"]], axis=1), bins)
    out = {"ramachandran_js": joint_js_np(r["phi0"], r["psi0"], m["phi0"], m["psi0"], e[0], e[1])}
    if r["pwd"].shape[1] == 0:
        out["pwd_js"] = out["rg_js"] = 0.0  # np.stack([]) raises inside the reference's try: both fall to the except
    else:
        out["pwd_js"] = float(density_js_np(r["pwd"], m["pwd"], edges_np(r["pwd"], bins))[1])
        out["rg_js"] = float(density_js_np(r["rg"], m["rg"], edges_np(r["rg"], bins))[1])
    if "tics" in r:
        tr, tm = r["tics"][:, :2], m["tics"][:, :2]
        et = edges_np(tr, bins)
        out["tic_js"] = float(density_js_np(tr, tm, et)[1])
        out["tic2d_js"] = joint_js_np(tr[:, 0], tr[:, 1], tm[:, 0], tm[:, 1], et[0], et[1])
    out["val_ca"] = validity_np(m["ca_dist"])
    out["rmse_contact"] = rmse_contact_np(contacts_np(r["ca_dist"]), len(r["ca_dist"]), contacts_np(m["ca_dist"]), len(m["ca_dist"]))
    return out


def tics(n, seed):
    """Seeded two-column float32 projections: two Gaussian clusters along the first, a slow drift along the second."""
    rng = np.random.default_rng(seed)
    a = np.where(rng.random(n) < 0.6, -1.0, 1.5) + 0.4 * rng.standard_normal(n)
    b = 0.5 * a + np.linspace(-1.0, 1.0, n) + 0.3 * rng.standard_normal(n)
    return np.stack([a, b], axis=1).astype(np.float32)
