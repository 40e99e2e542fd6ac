"""A numpy float64 restatement of the Lloyd iteration of ``lam_slide_amd.kmeans``, one series at a time, with exactly
its rules: the assignment in float64 (differences, the sum over j ascending, centres ascending, strict ``<``; -1 for a row that holds a
NaN), the update ``float32(sum / count)`` with the sum taken in ascending t within segments of SEG rows and the segments in order (an empty
cluster keeps its bits), the inertia of an iteration against the centres before the update, the three stopping rules and the final
assignment.  It also returns the relative gap between the best and the second-best distance of every row: a label may differ from another
correct float64 evaluation only where that gap is at rounding level."""
import numpy as np

SEG = 2048


def distances(y, c):
    """y [n, d], c [k, d] -> float64 [n, k], the sum over j ascending."""
    y64, c64 = np.asarray(y, dtype=np.float64), np.asarray(c, dtype=np.float64)
    dist = np.zeros((y64.shape[0], c64.shape[0]))
    for j in range(y64.shape[1]):
        diff = y64[:, j, None] - c64[None, :, j]
        dist += diff * diff
    return dist


def _gap(best, second):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(second > 0, (second - best) / second, np.where(np.isfinite(second), 0.0, np.inf))


def assign(y, c):
    """-> (labels int64 [n], -1 for a NaN row; winning distances [n], 0 for a NaN row; relative gap to the second best [n], inf for a NaN
    row or k = 1)."""
    dist = distances(y, c)
    nan = np.isnan(np.asarray(y, dtype=np.float64)).any(axis=1)
    dist = np.where(nan[:, None], 0.0, dist)
    lab = dist.argmin(axis=1)  # (the first minimum: the lowest index)
    best = dist[np.arange(len(lab)), lab]
    if dist.shape[1] > 1:
        second = np.partition(dist, 1, axis=1)[:, 1]
        gap = _gap(best, second)
    else:
        gap = np.full(len(lab), np.inf)
    return np.where(nan, -1, lab), np.where(nan, 0.0, best), np.where(nan, np.inf, gap)


def sums_counts(y, labels, k):
    """The update's float64 sums [k, d] (rows ascending within a segment, the segments in order) and the integer counts [k]."""
    y64 = np.asarray(y, dtype=np.float64)
    n, d = y64.shape
    sums = np.zeros((k, d))
    for a in range(0, n, SEG):
        part = np.zeros((k, d))
        lab = labels[a:a + SEG]
        ok = lab >= 0
        np.add.at(part, lab[ok], y64[a:a + SEG][ok])  # (unbuffered: in index order)
        sums += part
    return sums, np.bincount(labels[labels >= 0], minlength=k)[:k]


def update(y, labels, centers):
    """-> (new centres float32 [k, d], counts [k])."""
    c = np.asarray(centers, dtype=np.float32)
    sums, counts = sums_counts(y, labels, c.shape[0])
    new = c.copy()
    live = counts > 0
    new[live] = (sums[live] / counts[live, None].astype(np.float64)).astype(np.float32)
    return new, counts


def step(y, centers, prev_labels=None):
    """One iteration -> dict(labels, best, gap, J, changed, counts, centers (new), shift)."""
    lab, best, gap = assign(y, centers)
    prev = np.full(len(lab), -2) if prev_labels is None else np.asarray(prev_labels)
    new, counts = update(y, lab, centers)
    shift = float(((new.astype(np.float64) - np.asarray(centers, dtype=np.float32).astype(np.float64)) ** 2).sum())
    return dict(labels=lab, best=best, gap=gap, J=float(best.sum()), changed=int((lab != prev).sum()), counts=counts, centers=new, shift=shift)


def fit(y, init, max_iter=100, rel_tol=1e-5, center_tol=0.0):
    """-> dict(centers, labels, counts, inertia, n_iter, converged, history: J of every iteration, min_gap: the smallest gap met)."""
    c = np.asarray(init, dtype=np.float32).copy()
    prev, J_prev, done, n_iter, hist, min_gap = None, 0.0, False, 0, [], np.inf
    for it in range(1, max_iter + 1):
        s = step(y, c, prev)
        hist.append(s["J"])
        min_gap = min(min_gap, float(s["gap"].min()))
        c, prev, n_iter = s["centers"], s["labels"], it
        done = (s["changed"] == 0 or (rel_tol > 0 and it >= 2 and abs(J_prev - s["J"]) <= rel_tol * J_prev)
                or (center_tol > 0 and s["shift"] <= center_tol * center_tol))
        J_prev = s["J"]
        if done:
            break
    lab, best, gap = assign(y, c)
    counts = np.bincount(lab[lab >= 0], minlength=c.shape[0])
    return dict(centers=c, labels=lab, counts=counts, inertia=float(best.sum()), n_iter=n_iter, converged=bool(done), history=hist,
                min_gap=min(min_gap, float(gap.min())))


def nearest(y, centers):
    """-> (rows int64 [k]: the lowest t of the smallest distance, NaN rows skipped, -1 without a finite row; the relative gap [k])."""
    dist = distances(y, centers)  # [n, k]
    nan = np.isnan(np.asarray(y, dtype=np.float64)).any(axis=1)
    k = dist.shape[1]
    if nan.all():
        return np.full(k, -1), np.full(k, np.inf)
    dist = np.where(nan[:, None], np.inf, dist)
    rows = dist.argmin(axis=0)
    best = dist[rows, np.arange(k)]
    gap = _gap(best, np.partition(dist, 1, axis=0)[1]) if dist.shape[0] > 1 else np.full(k, np.inf)
    return rows, gap


def kmeanspp_indices(y, u):
    """y [n, d], u [k] -> the picks of ``kmeans.kmeanspp_indices`` for one series."""
    y64 = np.asarray(y, dtype=np.float64)
    n = y64.shape[0]
    idx = [min(int(np.floor(u[0] * n)), n - 1)]
    d2 = None
    for i in range(1, len(u)):
        new = np.nan_to_num(((y64 - y64[idx[-1]]) ** 2).sum(axis=1), nan=0.0)
        d2 = new if d2 is None else np.minimum(d2, new)
        cum = np.cumsum(d2)
        idx.append(min(int(np.searchsorted(cum, u[i] * cum[-1])), n - 1))
    return np.array(idx)


def blobs(n, k, d, seed, spread=1.0, sep=3.0):
    """A seeded Gaussian mixture, float32 [n, d]: k components with centres ~ sep * N(0, 1) and standard deviation ``spread``, rows in
    random component order."""
    rng = np.random.default_rng(seed)
    means = sep * rng.standard_normal((k, d))
    comp = rng.integers(0, k, size=n)
    return (means[comp] + spread * rng.standard_normal((n, d))).astype(np.float32)


def center_bar(y, labels, centers, counts):
    """The bar of a new centre against the float64 update from the same labels: half a float32 ulp of the centre (one rounding) plus the
    float64 summation error ``(SEG + segments + 2) 2^-53 sum |y| / count``.  [k, d]."""
    y64 = np.abs(np.asarray(y, dtype=np.float64))
    n = y64.shape[0]
    k = centers.shape[0]
    tot = np.zeros((k, y64.shape[1]))
    ok = labels >= 0
    np.add.at(tot, labels[ok], y64[ok])
    chain = SEG + -(-n // SEG) + 2
    half_ulp = 0.5 * np.spacing(np.abs(centers).astype(np.float32)).astype(np.float64)
    return half_ulp + chain * 2.0 ** -53 * tot / np.maximum(counts, 1)[:, None]
