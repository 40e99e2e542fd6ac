"""The oracle of the TICA / state-statistics tests (test_tica.py, test_hip_tica.py), written out in numpy / scipy float64: the lagged second
moments as direct sums with the absolute sums their error bars are made of, the reversible covariances, the generalised eigenproblem
through ``scipy.linalg.eigh(Ct, C0)``, the projection, the nearest centre with the gap between the two smallest distances, the transition
counts through ``np.add.at``, and a seeded synthetic series with slow and fast processes.  Not a test module."""
import numpy as np
import scipy.linalg
import scipy.signal

AR_COEFFICIENTS = (0.999, 0.995, 0.98, 0.93, 0.8, 0.5)
CASES = ((4000, 5, 10), (20000, 12, 50), (20000, 33, 100))  # (n, F, lag): the well-conditioned models (C0 condition numbers ~20..120)


def series(n, F, seed):
    """float32 [n, F]: 6 independent stationary unit-variance AR(1) processes (coefficients ``AR_COEFFICIENTS``), mixed into F columns by a
    seeded Gaussian matrix over sqrt(6), plus 0.3 x white noise, scaled to max |x| = 1."""
    rng = np.random.default_rng(seed)
    rho = np.asarray(AR_COEFFICIENTS)
    e = rng.standard_normal((n, rho.size))
    e[1:] *= np.sqrt(1.0 - rho * rho)
    z = np.stack([scipy.signal.lfilter([1.0], [1.0, -r], e[:, i]) for i, r in enumerate(rho)], axis=1)
    x = z @ (rng.standard_normal((rho.size, F)) / np.sqrt(rho.size)) + 0.3 * rng.standard_normal((n, F))
    return (x / np.abs(x).max()).astype(np.float32)


def moments64(x, lag):
    """x [n, F] -> ((sx, sy, xx, yy, xy), (the same five sums of absolute values)): direct sums over t < n - lag.  Blocks of 256 rows in
    float64 (the products of float32 values are exact; a block's own rounding stays below 256 * 2^-53 of its absolute sum), the blocks
    added in extended precision."""
    v = np.asarray(x, dtype=np.float64)
    m = v.shape[0] - lag
    pad = (-m) % 256

    def five(a, b):
        a = np.concatenate([a, np.zeros((pad, a.shape[1]))]).reshape(-1, 256, a.shape[1])
        b = np.concatenate([b, np.zeros((pad, b.shape[1]))]).reshape(-1, 256, b.shape[1])
        at, bt = a.transpose(0, 2, 1), b.transpose(0, 2, 1)
        total = lambda blocks: blocks.astype(np.longdouble).sum(axis=0).astype(np.float64)  # noqa: E731
        return total(a.sum(axis=1)), total(b.sum(axis=1)), total(at @ a), total(bt @ b), total(at @ b)

    return five(v[:m], v[lag:]), five(np.abs(v[:m]), np.abs(v[lag:]))


def covariances64(x, lag):
    """The reversible estimator: (mean, C0, Ct) from the moments, no Bessel correction."""
    (sx, sy, xx, yy, xy), _ = moments64(x, lag)
    two_m = 2.0 * (np.asarray(x).shape[0] - lag)
    mean = (sx + sy) / two_m
    mm = np.outer(mean, mean)
    return mean, (xx + yy) / two_m - mm, (xy + xy.T) / two_m - mm


def sign_fixed(R):
    """Each column's sign set so that its entry of largest magnitude is positive."""
    top = np.abs(R).argmax(axis=0)
    return R * np.where(R[top, np.arange(R.shape[1])] < 0, -1.0, 1.0)


def eigh_scipy(C0, Ct):
    """(eigenvalues descending, sign-fixed eigenvectors with R^T C0 R = I) of Ct r = lambda C0 r by scipy's generalised solver."""
    lam, R = scipy.linalg.eigh(Ct, C0)
    order = np.argsort(-lam, kind="stable")
    return lam[order], sign_fixed(R[:, order])


def dimension(lam, var_cutoff=0.95):
    lam2 = np.asarray(lam) ** 2
    return int(np.searchsorted(np.cumsum(lam2) / lam2.sum(), var_cutoff)) + 1


def project64(x, mean, W):
    """(y64 [n, d], the sum over f of |(x_f - mean_f) W_fj| [n, d]): the projection in float64 and the sum its error bar is made of."""
    c = np.asarray(x, dtype=np.float64) - mean
    return c @ W, np.abs(c) @ np.abs(W)


def assign64(y, centers):
    """(argmin [n] (-1 for a row with NaN), the smallest distance [n], the gap to the second smallest distance [n]; inf when k = 1)."""
    y64, c64 = np.asarray(y, dtype=np.float64), np.asarray(centers, dtype=np.float64)
    dist = ((y64[:, None, :] - c64[None]) ** 2).sum(-1)
    nan = np.isnan(y64).any(axis=1)
    dist[nan] = 0.0
    idx = dist.argmin(axis=1)
    srt = np.sort(dist, axis=1)
    gap = srt[:, 1] - srt[:, 0] if dist.shape[1] > 1 else np.full(len(idx), np.inf)
    return np.where(nan, -1, idx), srt[:, 0], gap


def transitions_np(dtraj, lag, ns):
    """int64 [ns, ns] by np.add.at over the pairs (d_t, d_{t+lag}) with both labels in 0..ns-1."""
    d = np.asarray(dtraj, dtype=np.int64)
    c = np.zeros((ns, ns), dtype=np.int64)
    if lag < d.size:
        a, b = d[:d.size - lag], d[lag:]
        ok = (a >= 0) & (a < ns) & (b >= 0) & (b < ns)
        np.add.at(c, (a[ok], b[ok]), 1)
    return c


def labels(n, ns, seed, holes=0.02):
    """int32 [n] seeded labels in 0..ns-1 that dwell (a label stays with probability 0.9), with about ``holes`` of them -1."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, ns, size=n)
    stay = rng.random(n) < 0.9
    for t in range(1, n):
        if stay[t]:
            d[t] = d[t - 1]
    d[rng.random(n) < holes] = -1
    return d.astype(np.int32)
