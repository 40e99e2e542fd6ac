"""The oracle of the torsion-statistics tests (test_torsion_stats.py, test_hip_torsion_stats.py), written out in numpy / scipy: the
four-point dihedral component by component in a chosen precision, the direct float64 lagged sum, seeded AR(1) trajectories around a
fixture geometry, and values planted on and around histogram edges.  Not a test module."""
import numpy as np
import scipy.signal

PI = np.pi


def ar1_frames(base, n, seed, rho=0.95, sigma=0.05):
    """float32 [n, A, 3]: ``base`` [A, 3] plus, per atom and coordinate, a stationary AR(1) Gaussian series (correlation ``rho`` from
    frame to frame, standard deviation ``sigma`` - a few percent of the fixture's ~2-unit bond lengths): torsions move smoothly, their
    decorrelation curves are not flat and no four atoms come near a line."""
    base = np.asarray(base, dtype=np.float64).reshape(-1, 3)
    e = np.random.default_rng(seed).standard_normal((n,) + base.shape)
    e[1:] *= np.sqrt(1.0 - rho * rho)
    z = scipy.signal.lfilter([1.0], [1.0, -rho], e, axis=0)
    return (base[None] + sigma * z).astype(np.float32)


def dihedral_np(pos, quads, dtype):
    """angle = atan2((b1 . c1) |b2|, c1 . c2) of pos [..., A, 3] at quads [Q, 4], every operation in ``dtype``, left to right."""
    p = np.asarray(pos).astype(dtype)[..., np.asarray(quads, dtype=np.int64), :]  # [..., Q, 4, 3]
    b1, b2, b3 = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 1, :], p[..., 3, :] - p[..., 2, :]
    x_, y_, z_ = (lambda v: v[..., 0]), (lambda v: v[..., 1]), (lambda v: v[..., 2])
    cross = lambda a, b: (y_(a) * z_(b) - z_(a) * y_(b), z_(a) * x_(b) - x_(a) * z_(b), x_(a) * y_(b) - y_(a) * x_(b))  # noqa: E731
    c1, c2 = cross(b2, b3), cross(b1, b2)
    nb2 = np.sqrt((x_(b2) * x_(b2) + y_(b2) * y_(b2)) + z_(b2) * z_(b2))
    y = ((x_(b1) * c1[0] + y_(b1) * c1[1]) + z_(b1) * c1[2]) * nb2
    x = (c1[0] * c2[0] + c1[1] * c2[1]) + c1[2] * c2[2]
    out = np.arctan2(y, x)
    assert out.dtype == dtype
    return out


def wrapped_diff(a, b):
    """|a - b| on the circle, float64."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return np.minimum(d, 2 * PI - d)


def lag64(x, nlag):
    """x [..., n, C] (any float) -> float64 [..., C, nlag + 1]: ac[k] = sum_{t < n - k} x_t x_{t+k} / (n - k), the direct sum in float64
    (statsmodels' acovf(x, demean=False, adjusted=True, nlag=nlag))."""
    v = np.asarray(x, dtype=np.float64)
    n = v.shape[-2]
    return np.stack([(v[..., :n - k, :] * v[..., k:, :]).sum(axis=-2) / (n - k) for k in range(nlag + 1)], axis=-1)


def decorrelation64(angles, nlag):
    """angles [n, Q] -> float64 [Q, nlag + 1]: (acovf(sin) + acovf(cos) - baseline) / (1 - baseline), and the baselines [Q]."""
    a = np.asarray(angles, dtype=np.float64)
    s, c = np.sin(a), np.cos(a)
    base = s.mean(axis=0) ** 2 + c.mean(axis=0) ** 2
    return (lag64(s, nlag) + lag64(c, nlag) - base[:, None]) / (1 - base[:, None]), base


def planted_angles(n, Q, seed, bins=100, lo=-PI, hi=PI, bins2=50):
    """float32 [n, Q] uniform a little beyond [lo, hi], with - where n allows - values planted on ``np.float32`` of the range's ends and
    of interior edges of the ``bins`` and ``bins2`` tables, on the float32 neighbours of the ends on both sides, NaN and +-inf.  With a
    range and a bin width that float32 holds exactly (lo = -1, hi = 2.5, widths 0.25 / 0.5) the planted values ARE the float64 edges:
    v == edges[0], v == edges[bins] (the last bin is closed on the right) and v == edges[i] (bin i, not i - 1).  +-pi is not a float32:
    there ``np.float32(hi)`` lies just outside and its neighbour just inside."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo - 0.05, hi + 0.05, size=(n, Q)).astype(np.float32)
    f32 = np.float32
    special = [f32(lo), f32(hi), np.nextafter(f32(lo), f32(hi)), np.nextafter(f32(hi), f32(lo)), np.nextafter(f32(lo), f32(-9)),
               np.nextafter(f32(hi), f32(9)), f32(np.nan), f32(np.inf), f32(-np.inf), f32(0.0), f32(-0.0)]
    for b in (bins, bins2):
        edges = np.linspace(lo, hi, b + 1)
        special += [f32(edges[i]) for i in sorted({1 % (b + 1), 2 % (b + 1), b // 4, b // 2, b // 2 + 1, max(b - 2, 0), b - 1})]
    special = np.asarray(special, dtype=np.float32)
    if n >= 4 * len(special):
        rows = rng.choice(n, size=len(special), replace=False)  # the same rows in every column: pairs see (edge, edge) combinations
        for q in range(Q):
            x[rows, q] = np.roll(special, q)
        x[rows[0], :] = f32(hi)  # one row with every coordinate on the right end, one on the left: the corner cells of the joint tables
        x[rows[1], :] = f32(lo)
    return x


def hist_np(x, bins, lo, hi):
    """np.histogram(range=) of every column of x [n, Q] -> int64 [Q, bins] (the float32 values held in float64, so that numpy's edge table
    is the float64 ``np.linspace`` whatever its promotion rules do with a float32 array)."""
    v = np.asarray(x).astype(np.float64)
    return np.stack([np.histogram(v[:, q], bins=bins, range=(lo, hi))[0] for q in range(v.shape[1])]).astype(np.int64)


def hist2_np(x, pairs, bins2, lo, hi):
    v = np.asarray(x).astype(np.float64)
    return np.stack([np.histogram2d(v[:, a], v[:, b], bins=bins2, range=((lo, hi), (lo, hi)))[0] for a, b in pairs]).astype(np.int64)
