"""The float64 oracle of tests/test_superpose.py and tests/test_hip_superpose.py: Kabsch by SVD with the determinant fix in numpy, on the
float32 inputs widened to float64, the seeded inputs, and the bars.

Inputs (the issue's): a random reference frame (scale 3); every frame a random proper rotation of it plus 0.3 * noise plus a shift of
about 10.  For these the relative gap (l1 - l2) / l1 of Horn's matrix is >= 0.19 at every size, so the optimal rotation is well
conditioned and the quaternion form and the SVD form agree to ~1e-14.

Bars, derived: the arithmetic under test is float64 on exact inputs, the one float32 rounding is the output.
  coordinates  |out - oracle| <= 2^-23 * max |oracle out of that frame|   (half an ulp for the rounding, doubled; the float64 error is about
               1e-16 / gap <= 1e-13 relative)
  rmsd         |rmsd - oracle| <= 2^-23 * oracle + 1e-12 * m, m the largest input magnitude of the frame; rmsf and the mean likewise
  rot, trans   |rot - oracle| <= 1e-10, trans the same scaled by m: the eigenvector error eps / gap with three orders of margin at
               gap >= 1e-3"""
import numpy as np

LDS_ATOMS, MAX_A, RMSF_SEG = 2048, 2044, 128  # LSL_TORS_LDS_ATOMS, LSL_TORS_MAX_A, LSL_RMSF_SEG
SIZES = (1, 3, 4, 56, 65, 364, 2044)  # atoms of a frame: 65 is one atom past a wave


def fpb(A):
    """Frames per workgroup of k_superpose at A atoms."""
    return LDS_ATOMS // A


def frame_counts(A):
    n = fpb(A)
    return sorted({F for F in (1, n - 1, n, n + 1, 3 * n + 2) if F >= 1})


def rotations(rng, n):
    """n random proper rotations, float64 [n, 3, 3]."""
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    return q * np.linalg.det(q)[:, None, None]


def trajectory(A, F, seed, variant=0):
    """(reference float32 [A, 3], frames float32 [F, A, 3]); another ``variant`` gives other frames of the same reference."""
    ref = 3.0 * np.random.default_rng(seed).standard_normal((A, 3))
    rng = np.random.default_rng([seed, variant + 1])
    pos = np.einsum("fab,ib->fia", rotations(rng, F), ref) + 0.3 * rng.standard_normal((F, A, 3)) + 10.0 * rng.standard_normal((F, 1, 3))
    return ref.astype(np.float32), pos.astype(np.float32)


def kabsch(pos, ref, sel=None, fixed=None):
    """pos [F, A, 3], ref [A, 3] or [F, A, 3] -> dict of float64 arrays: out [F, A, 3], rmsd [F], rot [F, 3, 3], trans [F, 3], gap [F] (the
    relative gap of Horn's matrix; NaN where S = 0), zero [F] (S = 0 exactly: the rotation is the identity by convention)."""
    x = np.asarray(pos, dtype=np.float64)
    y = np.broadcast_to(np.asarray(ref, dtype=np.float64), x.shape)
    sel = np.arange(x.shape[1]) if sel is None else np.asarray(sel)
    xs, ys = x[:, sel], y[:, sel]
    cx, cy = xs.mean(axis=1, keepdims=True), ys.mean(axis=1, keepdims=True)
    S = np.einsum("fia,fib->fab", xs - cx, ys - cy)
    U, s, Vt = np.linalg.svd(S)
    V = np.swapaxes(Vt, 1, 2)
    d = np.sign(np.linalg.det(V @ np.swapaxes(U, 1, 2)))
    d[d == 0] = 1.0
    D = np.zeros_like(S)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = V @ D @ np.swapaxes(U, 1, 2)
    zero = ~S.any(axis=(1, 2))
    R[zero] = np.eye(3)
    out = np.einsum("fab,fib->fia", R, x - cx) + cy
    res = np.einsum("fab,fib->fia", R, xs - cx) - (ys - cy)
    if fixed is not None:
        out[:, np.asarray(fixed) != 0] = x[:, np.asarray(fixed) != 0]
    top = s[:, 0] + s[:, 1] + d * s[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = 2.0 * (s[:, 1] + d * s[:, 2]) / top
    return {"out": out, "rmsd": np.sqrt((res * res).sum(axis=(1, 2)) / len(sel)), "rot": R, "trans": cy[:, 0] - np.einsum("fab,fb->fa", R, cx[:, 0]),
            "gap": gap, "zero": zero}


def magnitude(pos, ref):
    """m [F]: the largest input magnitude of each frame and its reference."""
    x = np.abs(np.asarray(pos, dtype=np.float64)).reshape(len(pos), -1).max(axis=1)
    y = np.abs(np.broadcast_to(np.asarray(ref, dtype=np.float64), np.shape(pos))).reshape(len(pos), -1).max(axis=1)
    return np.maximum(x, y)


def check_fit(want, pos, ref, out=None, rmsd=None, rot=None, trans=None, coordinates=True):
    """Assert the outputs given against the oracle's at the bars above; returns the worst ratio error / bar seen.  Coordinates (and the
    transform) are compared on every frame, and every such frame must have gap >= 1e-3 or S = 0."""
    worst = 0.0
    m = magnitude(pos, ref)

    def ratio(err, bar):
        nonlocal worst
        assert np.all(err <= bar), float((err / bar).max())
        worst = max(worst, float((err / bar).max()))

    if coordinates and (out is not None or rot is not None):
        assert np.all(want["zero"] | (want["gap"] >= 1e-3)), want["gap"].min()
    if out is not None and coordinates:
        o = np.asarray(out, dtype=np.float64)
        ratio(np.abs(o - want["out"]).reshape(len(o), -1).max(axis=1), 2.0 ** -23 * np.abs(want["out"]).reshape(len(o), -1).max(axis=1))
    if rmsd is not None:
        ratio(np.abs(np.asarray(rmsd, dtype=np.float64) - want["rmsd"]), 2.0 ** -23 * want["rmsd"] + 1e-12 * m)
    if rot is not None and coordinates:
        ratio(np.abs(np.asarray(rot) - want["rot"]).reshape(-1, 9).max(axis=1), np.full(len(m), 1e-10))
        ratio(np.abs(np.asarray(trans) - want["trans"]).max(axis=1), 1e-10 * m)
    return worst


def is_proper_rotation(rot, tol=1e-12):
    rot = np.asarray(rot, dtype=np.float64)
    return bool(np.all(np.abs(np.linalg.det(rot) - 1.0) <= tol) and np.all(np.abs(rot @ np.swapaxes(rot, -1, -2) - np.eye(3)) <= tol))


def rmsf(pos):
    """(rmsf [A], mean [A, 3]) in float64."""
    x = np.asarray(pos, dtype=np.float64)
    mean = x.mean(axis=0)
    return np.sqrt(((x - mean) ** 2).sum(axis=2).mean(axis=0)), mean


def subset(A, seed=5):
    """An unsorted subset of the atoms: about half, at least min(A, 3)."""
    rng = np.random.default_rng(seed)
    return rng.permutation(A)[:max(min(A, 3), A // 2)]


def peptide(tables, F, seed=4):
    """(aatype, pos14 float32 [F, 4, 14, 3] with the padding slots zero, the topology's atoms) of ALA-ARG-GLY-SER."""
    from lam_slide_amd import topology_atoms
    aa = [0, 1, 7, 15]  # residue_constants.restypes order: A R N D C Q E G H I L K M F P S T W Y V
    top = topology_atoms(aa, tables)
    _, heavy = trajectory(len(top), F, seed)
    pos = np.zeros((F, 56, 3), dtype=np.float32)
    pos[:, top] = heavy
    return aa, pos.reshape(F, 4, 14, 3), top
