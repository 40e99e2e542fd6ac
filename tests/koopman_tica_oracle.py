"""The oracle of the Koopman-TICA tests (test_koopman_tica.py, test_hip_koopman_tica.py), written out in numpy / scipy float64 (and x87
extended precision where an "exact" sum is needed): seeded series, weighted lagged moments, the brute-force Koopman weights through
``scipy.linalg.eig`` of the transposed Koopman matrix, the reversible weighted covariances, the sequential projection.  Not a test module."""
import numpy as np
import scipy.linalg

U = 2.0 ** -53


def ar_series(n=4000, seed=0):
    """float32 [n, 6]: five AR(1) coordinates with coefficients 0.99 .. 0.5 mixed by a seeded matrix and shifted, and a sixth column that
    is exactly 2 * column 0 (a power of two: exact in float32), so C00 has one eigenvalue that is zero up to rounding and the epsilon cut
    drops it."""
    rng = np.random.default_rng(seed)
    phi = np.array([0.99, 0.95, 0.9, 0.7, 0.5])
    z = np.zeros((n, 5))
    z[0] = rng.standard_normal(5)
    g = rng.standard_normal((n, 5)) * np.sqrt(1 - phi ** 2)
    for t in range(1, n):
        z[t] = phi * z[t - 1] + g[t]
    x5 = (z @ (np.eye(5) + 0.3 * rng.standard_normal((5, 5))) + np.array([1.0, -2.0, 0.5, 0.0, 3.0])).astype(np.float32)
    return np.concatenate([x5, 2.0 * x5[:, :1]], axis=1)


def planted(n=6000, F=150, seed=0, dwell=200, noise=1.0, dwell2=None):
    """(x float32 [n, F], s float64 [n]): s a two-state coordinate (+-1) that switches with probability 1 / dwell per step, mixed into every
    column with seeded loadings of size ~1 next to white noise of size ``noise`` and a constant offset per column.  ``dwell2``: a second,
    independent two-state coordinate of that dwell with loadings of its own (not returned): a second slow process below the first."""
    rng = np.random.default_rng(seed)
    flips = rng.random(n) < 1.0 / dwell
    s = np.where(np.cumsum(flips) % 2 == 0, 1.0, -1.0)
    load = rng.standard_normal(F)
    x = s[:, None] * load[None, :] + noise * rng.standard_normal((n, F)) + rng.standard_normal(F)[None, :]
    if dwell2 is not None:
        s2 = np.where(np.cumsum(rng.random(n) < 1.0 / dwell2) % 2 == 0, 1.0, -1.0)
        x = x + s2[:, None] * rng.standard_normal(F)[None, :]
    return x.astype(np.float32), s


PROJ_F, PROJ_D, PROJ_ROWS = (129, 1344, 2048), (1, 40, 64), (1, 65, 1000)


def projection_case(F, d, seed=0):
    """(x float32 [1000, F], mean float64 [F], W float64 [F, d], u float64 [F], c): seeded Gaussian rows around per-column offsets, a mean
    two below the offsets and positive loadings of size 1 / F - so the sums do not cancel and sum |terms| is close to |sum|: few values
    lie near a float32 rounding boundary on the scale of the float64 chain's error."""
    rng = np.random.default_rng(1000 * F + d + seed)
    off = rng.standard_normal(F)
    x = (rng.standard_normal((1000, F)) * (0.25 + 0.5 * rng.random(F)) + off).astype(np.float32)
    return x, off - 2.0, (0.5 + rng.random((F, d))) / F, (0.5 + rng.random(F)) / F, 0.75


def gaussian(n, F, seed):
    """float32 [n, F]: seeded Gaussian columns with a column-dependent scale and offset (so the means matter)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, F)) * (0.5 + rng.random(F)) + rng.standard_normal(F)).astype(np.float32)


def signed_weights(m, seed):
    """float64 [m]: seeded weights of both signs, mean about 1 (what Koopman weights look like, exaggerated)."""
    rng = np.random.default_rng(seed)
    return 1.0 + 1.5 * rng.standard_normal(m)


def moments64(x, lag, w=None):
    """(sw, sx, sy, xx, yy, xy) in float64 (BLAS) from the float32 values as they are."""
    v = np.asarray(x, dtype=np.float64)
    m = v.shape[0] - lag
    a, b = v[:m], v[lag:]
    w = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
    wa, wb = a * w[:, None], b * w[:, None]
    return w.sum(), wa.sum(axis=0), wb.sum(axis=0), wa.T @ a, wb.T @ b, wa.T @ b


def abs_moments64(x, lag, w=None):
    """The same six sums of the absolute values of the terms: sum |w_t|, sum |w_t x_a|, .., sum |w_t x_a x_b| - what the error bound scales with."""
    w = None if w is None else np.abs(np.asarray(w, dtype=np.float64))
    return moments64(np.abs(np.asarray(x, dtype=np.float64)), lag, w)


def moment_rows_exact(x, lag, w, rows):
    """Rows ``rows`` of (xx, yy, xy) and the entries ``rows`` of (sx, sy), and sw, in x87 extended precision (64-bit significand: the sum of
    m <= 4096 terms is within m 2^-64 sum |terms| < 2^-53 sum |terms| of exact - two thousandths of the bound it referees), returned as
    longdouble: (sw, sx [k], sy [k], xx [k, F], yy [k, F], xy [k, F])."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs x87 extended precision"
    v = np.asarray(x, dtype=np.longdouble)
    m = v.shape[0] - lag
    a, b = v[:m], v[lag:]
    wl = np.ones(m, dtype=np.longdouble) if w is None else np.asarray(w, dtype=np.longdouble)
    wa, wb = a[:, rows] * wl[:, None], b[:, rows] * wl[:, None]
    return wl.sum(), wa.sum(axis=0), wb.sum(axis=0), wa.T @ a, wb.T @ b, wa.T @ b


def koopman_inputs(x, lag):
    """(mu0, mut, C00, C0t) of the unweighted, non-reversible estimator, float64."""
    m = x.shape[0] - lag
    sw, sx, sy, xx, yy, xy = moments64(x, lag)
    mu0, mut = sx / m, sy / m
    return mu0, mut, xx / m - np.outer(mu0, mu0), xy / m - np.outer(mu0, mut)


def whitening(C00, epsilon=1e-6):
    s, V = np.linalg.eigh((C00 + C00.T) / 2)
    keep = np.abs(s) > epsilon
    R = V[:, keep] / np.sqrt(s[keep])
    top = np.abs(R).argmax(axis=0)
    return R * np.where(R[top, np.arange(R.shape[1])] < 0, -1.0, 1.0)


def koopman_brute(x, lag, epsilon=1e-6):
    """(u [F], const, R [F, r]) by brute force: K = [[R^T C0t R, 0], [(mut - mu0)^T R, 1]], ``scipy.linalg.eig(K.T)``, the eigenvector of
    the eigenvalue nearest 1 scaled to last component 1, u = R v, const = 1 - mu0 . u."""
    mu0, mut, C00, C0t = koopman_inputs(x, lag)
    R = whitening(C00, epsilon)
    r = R.shape[1]
    K = np.zeros((r + 1, r + 1))
    K[:r, :r] = R.T @ C0t @ R
    K[r, :r] = (mut - mu0) @ R
    K[r, r] = 1.0
    lam, vec = scipy.linalg.eig(K.T)
    i = int(np.argmin(np.abs(lam - 1.0)))
    assert abs(lam[i] - 1.0) < 1e-9 and np.abs(vec[:, i].imag).max() < 1e-12
    v = vec[:, i].real
    v = v / v[r]
    u = R @ v[:r]
    return u, float(1.0 - mu0 @ u), R


def reversible64(moments):
    """(mean, C0, Ct) of the reversible estimator from (sw, sx, sy, xx, yy, xy)."""
    sw, sx, sy, xx, yy, xy = moments
    mean = (sx + sy) / (2 * sw)
    mm = np.outer(mean, mean)
    return mean, (xx + yy) / (2 * sw) - mm, (xy + xy.T) / (2 * sw) - mm


def run_tica64(x, lag, epsilon=1e-6):
    """(eigenvalues descending, R [F, r] with R^T C0 R = I, mean) of the whole estimator in float64: brute-force Koopman weights, weighted
    reversible covariances, ``scipy.linalg.eigh`` in the whitened basis."""
    u, const, _ = koopman_brute(x, lag, epsilon)
    m = x.shape[0] - lag
    w = np.asarray(x[:m], dtype=np.float64) @ u + const
    mean, C0, Ct = reversible64(moments64(x, lag, w))
    L = whitening(C0, epsilon)
    M = L.T @ Ct @ L
    lam, Um = scipy.linalg.eigh((M + M.T) / 2)
    order = np.argsort(-lam, kind="stable")
    return lam[order], L @ Um[:, order], mean


def project_sequential(x, mean, W):
    """(acc float64 [n, d], mag float64 [n, d]): acc[t, j] = sum_f (x[t, f] - mean[f]) W[f, j] evaluated sequentially over f ascending in
    float64 (a rounded product and a rounded addition per step: within F 2^-53 mag of the fused chain), mag = sum_f |(x - mean) W|."""
    xd = np.asarray(x, dtype=np.float64) - np.asarray(mean, dtype=np.float64)[None, :]
    W = np.asarray(W, dtype=np.float64)
    acc = np.zeros((xd.shape[0], W.shape[1]))
    mag = np.zeros_like(acc)
    for f in range(xd.shape[1]):
        term = xd[:, f, None] * W[f][None, :]
        acc = acc + term
        mag += np.abs(term)
    return acc, mag


def fp32_rounding_is_decided(acc, slack):
    """bool [..]: float32(v) is the same for every v within ``slack`` of ``acc`` - acc is not that close to a float32 rounding boundary."""
    lo, hi = (acc - slack).astype(np.float32), (acc + slack).astype(np.float32)
    return lo == hi
