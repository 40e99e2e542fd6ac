"""numpy float64 oracle of ``lam_slide_amd.msm``: the largest strongly connected set through scipy's ``connected_components``, the
reversible maximum-likelihood row-sum iteration with a selectable summation order, the embedded transition matrix, and the inner simplex
algorithm of PCCA+.  Written from the mathematics of include/lsl_api.h, independently of the package's own restatement.

Summation order.  ``perm`` (a permutation of the active set's positions, default ascending) is the order in which the terms of every
``y_i``, of ``sum_i y_i`` and of the row sums of X are added, strictly one after the other (``np.cumsum``): two permutations give two
correct float64 evaluations, and their difference is the yardstick of the tests that have no derived bound."""
import bisect
import functools

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

U = 2.0 ** -53


# ---- inputs ----
@functools.lru_cache(maxsize=None)
def chain(ns, n, seed):
    """A seeded Markov chain of n steps over ns states with a few metastable groups and some rarely visited states: int32 [n]."""
    rng = np.random.default_rng(seed)
    groups = np.arange(ns) % max(1, min(4, ns // 3))
    P = rng.random((ns, ns)) ** 3 * np.where(groups[:, None] == groups[None, :], 1.0, 0.02)
    P[:, rng.random(ns) < 0.15] *= 1e-4  # (columns that are entered rarely: transient or unvisited states)
    P += np.eye(ns) * rng.random(ns)
    cum = [list(np.cumsum(row / row.sum())) for row in P]
    u = rng.random(n).tolist()
    out = np.empty(n, dtype=np.int32)
    s = int(rng.integers(ns))
    for t in range(n):
        out[t] = s
        s = min(bisect.bisect_right(cum[s], u[t]), ns - 1)
    out.setflags(write=False)
    return out


def count_matrix(dtraj, lag, ns):
    """The sliding-window count matrix int64 [ns, ns]; a pair with a label outside 0..ns-1 is skipped."""
    a, b = np.asarray(dtraj[:-lag], dtype=np.int64), np.asarray(dtraj[lag:], dtype=np.int64)
    ok = (a >= 0) & (a < ns) & (b >= 0) & (b < ns)
    return np.bincount(a[ok] * ns + b[ok], minlength=ns * ns).reshape(ns, ns).astype(np.int64)


def chain_counts(ns, n, lag, seed):
    return count_matrix(chain(ns, n, seed), lag, ns)


def slow_matrix(seed=0):
    """12 states in two blocks of 6 with entries in 1..499, joined by C[2, 8] = 1 and C[9, 3] = 40: tens of thousands of iterations."""
    rng = np.random.default_rng(seed)
    C = np.zeros((12, 12), dtype=np.int64)
    C[:6, :6] = rng.integers(1, 500, (6, 6))
    C[6:, 6:] = rng.integers(1, 500, (6, 6))
    C[2, 8], C[9, 3] = 1, 40
    return C


# ---- the active set ----
def active_set(C):
    """bool [ns]: the largest strongly connected component of i -> j where C[i, j] > 0; one state alone only with C[i, i] > 0; equal sizes:
    the component holding the lowest state index; no candidate: empty."""
    C = np.asarray(C)
    ns = C.shape[0]
    _, lab = connected_components(csr_matrix((C > 0).astype(np.int8)), directed=True, connection="strong")
    best, best_size = None, 0
    for state in range(ns):  # (ascending: the first component of a size is the one with the lowest state)
        members = lab == lab[state]
        size = int(members.sum())
        if size == 1 and not C[state, state] > 0:
            continue
        if size > best_size:
            best, best_size = members, size
    return np.zeros(ns, dtype=bool) if best is None else best


# ---- the iteration ----
class Problem:
    """C and its active flags -> A (indices), c [na], K [na, na] float64 (exact integers), x0 [na]."""

    def __init__(self, C, active=None):
        C = np.asarray(C, dtype=np.int64)
        self.ns = C.shape[0]
        self.active = active_set(C) if active is None else np.asarray(active, dtype=bool)
        self.A = np.flatnonzero(self.active)
        Ct = np.maximum(C[np.ix_(self.A, self.A)], 0)
        self.Ct = Ct
        Ki = Ct + Ct.T
        self.c = Ct.sum(axis=1).astype(np.float64)
        self.K = Ki.astype(np.float64)
        self.nz = self.K != 0
        self.na = len(self.A)
        self.x0 = Ki.sum(axis=1).astype(np.float64) / float(Ki.sum()) if self.na else np.zeros(0)

    def flows(self, x):
        q = self.c / x
        D = q[:, None] + q[None, :]
        return np.where(self.nz, self.K / np.where(self.nz, D, 1.0), 0.0)

    def step(self, x, perm=None):
        """One step from x -> (x', err), the sums taken strictly in the order ``perm``."""
        perm = np.arange(self.na) if perm is None else np.asarray(perm)
        y = np.cumsum(self.flows(x)[:, perm], axis=1)[:, -1]
        xn = y / np.cumsum(y[perm])[-1]
        return xn, float(np.max(np.abs(x - xn) / (0.5 * (x + xn))))

    def iterate(self, maxiter, maxerr, perm=None, x=None, keep=()):
        """(x, n_iter, err, converged[, {n: x after n steps for n in keep}]): count the step, then stop when !(err > maxerr) or at maxiter."""
        x = self.x0 if x is None else x
        if self.na <= 1:
            return (np.ones(self.na), 0, 0.0, True) + (({},) if keep else ())
        n, err, conv, kept = 0, 0.0, False, {}
        while n < maxiter:
            x, err = self.step(x, perm)
            n += 1
            if n in keep:
                kept[n] = x
            if not err > maxerr:
                conv = True
                break
        return (x, n, err, conv) + ((kept,) if keep else ())

    def tmatrix(self, x, perm=None):
        """T [na, na] on the active set from x."""
        if self.na == 1:
            return np.ones((1, 1))
        perm = np.arange(self.na) if perm is None else np.asarray(perm)
        X = self.flows(x)
        return X / np.cumsum(X[:, perm], axis=1)[:, -1][:, None]

    def embed(self, T, x):
        """(T_full = eye with the active block written in, pi_full = 0 outside A)."""
        Tf, pf = np.eye(self.ns), np.zeros(self.ns)
        if self.na:
            Tf[np.ix_(self.A, self.A)] = T
            pf[self.A] = x
        return Tf, pf

    def log_likelihood(self, T):
        m = self.Ct > 0
        return float((self.Ct[m] * np.log(T[m])).sum())


def estimate(C, maxiter=1_000_000, maxerr=1e-8, perm=None):
    """C -> dict(active, n_active, T, pi (embedded), T_A, pi_A, n_iter, err, converged)."""
    p = Problem(C)
    x, n, err, conv = p.iterate(maxiter, maxerr, perm)
    TA = p.tmatrix(x, perm) if p.na else np.zeros((0, 0))
    T, pi = p.embed(TA, x)
    return dict(active=p.active, n_active=p.na, T=T, pi=pi, T_A=TA, pi_A=x, n_iter=n, err=err, converged=conv, problem=p)


def reversed_perm(na):
    return np.arange(na)[::-1]


def rel_diff(a, b):
    """max |a - b| / |b| over the entries where b != 0 (where b == 0, a must be 0 too)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.all(a[b == 0] == 0)
    m = b != 0
    return float((np.abs(a[m] - b[m]) / np.abs(b[m])).max()) if m.any() else 0.0


# ---- PCCA+ by the inner simplex algorithm ----
def isa(T, pi, m):
    """(chi [na, m], assignments [na], idx [m]): the m dominant right eigenvectors (pi-orthonormal, the first exactly ones), the inner
    simplex representatives by the textbook loop (the farthest row, subtract it, then orthogonalise against each chosen direction), chi =
    R R[idx]^-1."""
    T, pi = np.asarray(T, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    d = np.sqrt(pi)
    Sm = (T * d[:, None]) / d[None, :]
    lam, V = np.linalg.eigh((Sm + Sm.T) / 2)
    top = np.argsort(lam)[::-1][:m]
    R = V[:, top] / d[:, None]
    R[:, 0] = 1.0
    ortho = R.copy()
    idx = np.zeros(m, dtype=int)
    idx[0] = int(np.argmax(np.linalg.norm(ortho, axis=1)))
    ortho -= ortho[idx[0]].copy()
    for j in range(1, m):
        if j > 1:
            temp = ortho[idx[j - 1]].copy()
            for row in range(len(ortho)):
                ortho[row] -= temp * np.dot(ortho[row], temp)
        dist = np.linalg.norm(ortho, axis=1)
        idx[j] = int(np.argmax(dist))
        ortho /= dist[idx[j]]
    chi = R @ np.linalg.inv(R[idx])
    return chi, np.argmax(chi, axis=1), idx


def planted_blocks(blocks=3, size=4, coupling=1e-3, seed=0):
    """A reversible T of `blocks` blocks of `size` states, weakly coupled, under a random state permutation -> (T, pi, block of each state)."""
    rng = np.random.default_rng(seed)
    n = blocks * size
    X = np.zeros((n, n))
    for b in range(blocks):
        blk = rng.random((size, size)) + 0.5
        X[b * size:(b + 1) * size, b * size:(b + 1) * size] = blk + blk.T
    W = rng.random((n, n))
    X += coupling * (W + W.T)
    order = rng.permutation(n)
    X = X[np.ix_(order, order)]
    member = (np.arange(n) // size)[order]
    return X / X.sum(axis=1)[:, None], X.sum(axis=1) / X.sum(), member


# ---- the cases of the tests (tests/test_msm.py checks on the CPU what the GPU tests rely on) ----
# (ns, n, lag, seed): chain-generated counts; with these seeds the oracle stops at the same count in ascending and in reversed order, and
# after convergence at maxerr = 1e-12 it holds detailed balance within 1e-9 relative
CONVERGED_CASES = ((2, 500, 1, 2), (10, 20000, 10, 0), (33, 5000, 1, 0), (65, 20000, 3, 0), (100, 100000, 100, 0), (128, 60000, 5, 0))
FIXED_CASES = CONVERGED_CASES[1:]  # 64 steps with maxerr = -1
# The largest relative difference between two summation orders of the oracle after 64 steps on FIXED_CASES (ascending against reversed and
# against a seeded random order), measured: 17.6 * 2^-53 on pi, 17.8 * 2^-53 on T (test_msm.py re-measures both against these constants).
# The GPU tests allow 16 times as much.
ORDER_DIFF_PI = 18 * U
ORDER_DIFF_T = 18 * U


def order_differences(case, steps=64):
    """(pi, T): the largest relative difference of the oracle between ascending order and two others after `steps` steps."""
    ns, n, lag, seed = case
    p = Problem(chain_counts(ns, n, lag, seed))
    xa = p.iterate(steps, -1.0)[0]
    Ta = p.tmatrix(xa)
    dp = dt = 0.0
    for perm in (reversed_perm(p.na), np.random.default_rng(5).permutation(p.na)):
        xb = p.iterate(steps, -1.0, perm=perm)[0]
        dp, dt = max(dp, rel_diff(xb, xa)), max(dt, rel_diff(p.tmatrix(xb, perm), Ta))
    return dp, dt


WELLS = np.array([[-2.0, 0.0], [2.0, 0.0], [0.0, 3.0]])


@functools.lru_cache(maxsize=None)
def three_wells(n, seed, stay=0.97):
    """A seeded 2-D series with three wells: a sticky 3-state chain plus Gaussian noise, float32 [n, 2]."""
    rng = np.random.default_rng(seed)
    u, w = rng.random(n), rng.integers(1, 3, n)
    state = np.empty(n, dtype=np.int64)
    s = 0
    for t in range(n):
        state[t] = s
        if u[t] > stay:
            s = (s + int(w[t])) % 3
    y = (WELLS[state] + 0.45 * rng.standard_normal((n, 2))).astype(np.float32)
    y.setflags(write=False)
    return y


def well_centers():
    """12 microstate centres, four around each well, float32 [12, 2] (centre c belongs to well c // 4)."""
    off = 0.4 * np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    return (WELLS[:, None, :] + off[None]).reshape(12, 2).astype(np.float32)


def nearest(y, centers):
    """labels [n]: argmin_c of the float64 squared distance, the lowest index on a tie."""
    d = ((y[:, None, :].astype(np.float64) - centers[None].astype(np.float64)) ** 2).sum(axis=2)
    return d.argmin(axis=1)


def state_block(ref_y, traj_y, centers, assignments, nstates, lag, msm_lag):
    """The block of eval_peptide.py:249-288 from given assignments [k] (-1: outside), everything through this oracle."""
    assignments = np.asarray(assignments)
    out = {}
    coarse = {}
    for name, y in (("ref", ref_y), ("traj", traj_y)):
        d = assignments[nearest(y, centers)]
        coarse[name] = d
        out[name + "_metastable_probs"] = (d == np.arange(nstates)[:, None]).mean(1)
    c = estimate(count_matrix(coarse["ref"], lag, nstates))
    t = estimate(count_matrix(coarse["traj"], msm_lag, nstates))
    out.update(msm_transition_matrix=c["T"], msm_pi=c["pi"], traj_transition_matrix=t["T"], traj_pi=t["pi"])
    return out
