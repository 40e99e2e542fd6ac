"""GPU tests of the Markov state models on the device (``lsl_msm_active_set`` / ``lsl_msm_reversible_step`` / ``lsl_msm_transition_matrix``
behind ``lam_slide_amd.msm``) against the numpy float64 oracle of tests/msm_oracle.py.  U = 2^-53.

Bars.
  active set   exact against scipy's strongly connected components plus the rules.
  one step     from the oracle's iterate after 10 steps: relative 2 (2 na + 5) U per element of x' - q is one rounding, a term two more, a
               chain of at most na positive terms, a normalising sum of na terms and a division; the factor 2 for both sides.  T from a
               given x: 2 (na + 5) U.
  64 steps     (maxerr = -1) no bound is derived across steps: 16 times the largest relative difference the oracle itself shows between two
               summation orders on the same cases - msm_oracle.ORDER_DIFF_PI = ORDER_DIFF_T = 18 U (measured 17.6 U and 17.8 U;
               tests/test_msm.py re-measures them on the CPU).
  converged    (maxerr = 1e-8) |pi - pi_oracle| <= 2 maxerr pi, the same on T, n_iter within one of the oracle's; the seeds are those where
               the oracle's own two orders stop at the same count (checked on the CPU).
  no oracle    rows of T sum to 1 within (na + 2) U; pi sums to 1 within (2 na + 2) U (a division per entry, the device's normalising sum
               and numpy's own sum); detailed balance within 1e-9 relative after convergence at 1e-12 (T is renormalised per row: a
               condition, which the oracle meets on these cases); the likelihood is not below that of 20 random reversible matrices of the
               same sparsity; a symmetric count matrix is its own fixed point.
  bits         split launches, batches, repeats and finished series: bit for bit.
Measured values: profiles/msm_parity.txt."""
import numpy as np
import pytest
import torch

import msm_oracle as orc
from conftest import parity

pytestmark = pytest.mark.gpu

U = orc.U
MAXERR = 1e-8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


class State:
    """The caller's side of the three entry points for count matrices [S, ns, ns] (numpy)."""

    def __init__(self, dev, counts):
        from lam_slide_amd import _lib
        self.lib, self.dev = _lib, dev
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        self.S, self.ns = counts.shape[0], counts.shape[1]
        self.counts = torch.from_numpy(counts).to(dev)
        self.active = torch.zeros(self.S, self.ns, dtype=torch.int32, device=dev)
        self.n_active = torch.zeros(self.S, dtype=torch.int32, device=dev)
        self.x = torch.zeros(self.S, self.ns, dtype=torch.float64, device=dev)
        self.n_iter = torch.zeros(self.S, dtype=torch.int32, device=dev)
        self.err = torch.zeros(self.S, dtype=torch.float64, device=dev)
        self.done = torch.zeros(self.S, dtype=torch.int32, device=dev)
        _lib.call(dev, "lsl_msm_active_set", self.counts.data_ptr(), self.S, self.ns, self.active.data_ptr(), self.n_active.data_ptr())

    def step(self, iters, maxiter=1_000_000, maxerr=MAXERR, restart=0):
        self.lib.call(self.dev, "lsl_msm_reversible_step", self.counts.data_ptr(), self.active.data_ptr(), self.S, self.ns, iters, maxiter, maxerr, restart,
                      self.x.data_ptr(), self.n_iter.data_ptr(), self.err.data_ptr(), self.done.data_ptr())
        return self

    def tmatrix(self):
        T = torch.empty(self.S, self.ns, self.ns, dtype=torch.float64, device=self.dev)
        pi = torch.empty(self.S, self.ns, dtype=torch.float64, device=self.dev)
        self.lib.call(self.dev, "lsl_msm_transition_matrix", self.counts.data_ptr(), self.active.data_ptr(), self.x.data_ptr(), self.S, self.ns, T.data_ptr(),
                      pi.data_ptr())
        return T, pi

    def snapshot(self):
        return tuple(t.clone() for t in (self.x, self.n_iter, self.err, self.done))


# ---- the active set ----
def test_active_set_rules(dev):
    from lam_slide_amd import msm
    C7 = np.zeros((7, 7), dtype=np.int64)
    C7[0, 2] = C7[2, 5] = C7[5, 0] = 3
    C7[1, 4] = C7[4, 1] = 9
    C7[3, 0], C7[6, 6] = 2, 50
    C4 = np.zeros((4, 4), dtype=np.int64)
    C4[0, 1] = C4[1, 0] = C4[2, 3] = C4[3, 2] = 1
    C1 = np.zeros((3, 3), dtype=np.int64)
    C1[1, 1] = 4
    for Cm, want in ((C7, [0, 2, 5]), (C4, [0, 1]), (np.zeros((5, 5), dtype=np.int64), []), (C1, [1]), (-C7, [])):
        act, na = msm.active_set(torch.from_numpy(Cm).to(dev))
        assert msm.last_path["active_set"] == "fused" and act.dtype == torch.bool and na.dtype == torch.int32
        assert act.cpu().numpy().nonzero()[0].tolist() == want and int(na) == len(want)
        assert np.array_equal(orc.active_set(Cm), act.cpu().numpy())


@pytest.mark.parametrize("ns", [1, 2, 33, 64, 65, 128])
def test_active_set_matches_scipy(dev, ns):
    from lam_slide_amd import msm
    mats = []
    for seed in range(3):
        Cm = orc.chain_counts(ns, 3000, 1, 10 + seed)
        mats += [Cm, Cm * (Cm > 2), Cm * (np.random.default_rng(seed).random((ns, ns)) < 0.03)]  # dense, thinned, and a few edges only
    act, na = msm.active_set(torch.from_numpy(np.stack(mats)).to(dev))
    sizes = []
    for s, Cm in enumerate(mats):
        want = orc.active_set(Cm)
        assert np.array_equal(act[s].cpu().numpy(), want) and int(na[s]) == int(want.sum()), (ns, s)
        sizes.append(int(want.sum()))
    print(f"active set ns = {ns}: sizes {sizes}")
    assert ns <= 2 or len(set(sizes)) >= 3  # the cases differ


# ---- one step and T against the oracle ----
@pytest.mark.parametrize("case", orc.CONVERGED_CASES)
def test_one_step_from_the_oracles_iterate(dev, case):
    p = orc.Problem(orc.chain_counts(*case))
    x10 = p.iterate(10, -1.0)[0]
    st = State(dev, orc.chain_counts(*case)[None])
    assert np.array_equal(st.active[0].cpu().numpy() != 0, p.active)
    full = np.zeros(p.ns)
    full[p.A] = x10
    st.x.copy_(torch.from_numpy(full)[None])
    st.n_iter.fill_(10)
    st.step(1, maxerr=-1.0)
    want, want_err = p.step(x10)
    got = st.x[0].cpu().numpy()
    assert int(st.n_iter[0]) == 11 and int(st.done[0]) == 0 and np.all(got[~p.active] == 0)
    parity(f"msm_one_step_ns{case[0]} (units of the bar 2 (2 na + 5) U)", orc.rel_diff(got[p.active], want) / (2 * (2 * p.na + 5) * U), 1.0)
    assert abs(float(st.err[0]) - want_err) <= 4 * (2 * p.na + 5) * U * max(1.0, want_err)
    # T from a given x
    st.x.copy_(torch.from_numpy(full)[None])
    T, pi = st.tmatrix()
    Tw, pw = p.embed(p.tmatrix(x10), x10)
    parity(f"msm_T_from_x_ns{case[0]} (units of the bar 2 (na + 5) U)", orc.rel_diff(T[0].cpu().numpy(), Tw) / (2 * (p.na + 5) * U), 1.0)
    assert np.array_equal(pi[0].cpu().numpy(), pw)


@pytest.mark.parametrize("case", orc.FIXED_CASES)
def test_fixed_64_steps_against_the_oracle(dev, case):
    p = orc.Problem(orc.chain_counts(*case))
    st = State(dev, orc.chain_counts(*case)[None]).step(64, maxerr=-1.0, restart=1)
    x64 = p.iterate(64, -1.0)[0]
    assert int(st.n_iter[0]) == 64 and int(st.done[0]) == 0
    T, pi = st.tmatrix()
    Tw, pw = p.embed(p.tmatrix(x64), x64)
    parity(f"msm_64_steps_pi_ns{case[0]} (units of U)", orc.rel_diff(pi[0].cpu().numpy(), pw) / U, 16 * orc.ORDER_DIFF_PI / U)
    parity(f"msm_64_steps_T_ns{case[0]} (units of U)", orc.rel_diff(T[0].cpu().numpy(), Tw) / U, 16 * orc.ORDER_DIFF_T / U)


# ---- converged runs through the module ----
@pytest.mark.parametrize("case", orc.CONVERGED_CASES)
def test_converged_runs_against_the_oracle(dev, case):
    from lam_slide_amd import msm
    ns, n, lag, seed = case
    mod = msm.estimate_markov_model(torch.from_numpy(orc.chain(ns, n, seed).copy()).to(dev), lag, ns)
    assert mod.path == "fused" == msm.last_path["estimate_markov_model"] and msm.last_path["transition_counts"] == "fused"
    assert all(t.is_cuda for t in (mod.transition_matrix, mod.pi, mod.active, mod.n_active, mod.counts, mod.n_iter, mod.err, mod.converged))
    Cm = orc.chain_counts(*case)
    assert np.array_equal(mod.counts.cpu().numpy(), Cm)
    want = orc.estimate(Cm)
    T, pi = mod.transition_matrix.cpu().numpy(), mod.pi.cpu().numpy()
    assert np.array_equal(mod.active.cpu().numpy(), want["active"]) and int(mod.n_active) == want["n_active"] and bool(mod.converged)
    print(f"msm converged ns = {ns}: n_iter {int(mod.n_iter)} (oracle {want['n_iter']}), err {float(mod.err):.3e}, na {want['n_active']}")
    assert abs(int(mod.n_iter) - want["n_iter"]) <= 1 and not float(mod.err) > MAXERR
    parity(f"msm_converged_pi_ns{ns} (units of 2 maxerr)", orc.rel_diff(pi, want["pi"]) / (2 * MAXERR), 1.0)
    parity(f"msm_converged_T_ns{ns} (units of 2 maxerr)", orc.rel_diff(T, want["T"]) / (2 * MAXERR), 1.0)
    out = ~want["active"]
    assert np.array_equal(T[out], np.eye(ns)[out]) and np.all(pi[out] == 0)
    A, TA, piA = mod.restricted()
    assert np.array_equal(A, want["problem"].A) and np.array_equal(TA, T[np.ix_(A, A)]) and np.array_equal(piA, pi[A])


# ---- properties that need no oracle ----
@pytest.mark.parametrize("case", orc.CONVERGED_CASES)
def test_stochastic_reversible_and_most_likely(dev, case):
    from lam_slide_amd import msm
    Cm = orc.chain_counts(*case)
    mod = msm.estimate_markov_model(counts=torch.from_numpy(Cm).to(dev), maxerr=1e-12)
    A, T, pi = mod.restricted()
    na = len(A)
    assert bool(mod.converged) and na >= 2
    parity(f"msm_row_sums_ns{case[0]} (units of the bar (na + 2) U)", float(np.abs(T.sum(axis=1) - 1).max()) / ((na + 2) * U), 1.0 + 1e-9)
    parity(f"msm_pi_sum_ns{case[0]} (units of the bar (2 na + 2) U)", abs(float(pi.sum()) - 1) / ((2 * na + 2) * U), 1.0 + 1e-9)
    F = pi[:, None] * T
    m = F > 0
    parity(f"msm_detailed_balance_ns{case[0]}", float((np.abs(F - F.T)[m] / F[m]).max()), 1e-9)
    assert np.array_equal(F > 0, F.T > 0) and np.all(T >= 0)
    p = orc.Problem(Cm)
    best = p.log_likelihood(T)
    rng = np.random.default_rng(case[0])
    others = []
    for _ in range(20):
        W = rng.random((na, na)) + 0.05
        X = (W + W.T) * p.nz  # a symmetric positive X of the same sparsity: a reversible T
        others.append(p.log_likelihood(X / X.sum(axis=1)[:, None]))
    print(f"msm log-likelihood ns = {case[0]}: estimate {best:.6f}, best of 20 random reversible matrices {max(others):.6f}")
    assert best >= max(others)
    # a perturbation of the estimate itself along its own sparsity is no better either (the maximum is sharp enough to see)
    Xe = F * (1 + 1e-3 * np.triu(rng.standard_normal((na, na))))
    Xe = np.triu(Xe) + np.triu(Xe, 1).T
    assert best >= p.log_likelihood(Xe / Xe.sum(axis=1)[:, None])


def test_symmetric_counts_are_their_own_fixed_point(dev):
    from lam_slide_amd import msm
    rng = np.random.default_rng(3)
    for ns in (5, 40, 128):
        B = rng.integers(0, 50, (ns, ns)) * (rng.random((ns, ns)) < 0.5)
        Cm = (B + B.T + np.diag(rng.integers(1, 9, ns))).astype(np.int64)
        Cm[0, 1] = Cm[1, 0] = 1
        for i in range(ns - 1):
            Cm[i, i + 1] = Cm[i + 1, i] = max(1, Cm[i, i + 1])  # connected
        mod = msm.estimate_markov_model(counts=torch.from_numpy(Cm).to(dev))
        assert int(mod.n_active) == ns and int(mod.n_iter) == 1 and bool(mod.converged)
        rows = Cm.sum(axis=1).astype(np.float64)
        parity(f"msm_symmetric_T_ns{ns} (units of the bar 2 (na + 5) U)", orc.rel_diff(mod.transition_matrix.cpu().numpy(), Cm / rows[:, None]) / (2 * (ns + 5) * U), 1.0)
        parity(f"msm_symmetric_pi_ns{ns} (units of the bar 2 (2 na + 5) U)", orc.rel_diff(mod.pi.cpu().numpy(), rows / rows.sum()) / (2 * (2 * ns + 5) * U), 1.0)


# ---- the slow matrix ----
@pytest.fixture(scope="module")
def slow():
    Cm = orc.slow_matrix()
    p = orc.Problem(Cm)
    x, n, err, conv, kept = p.iterate(1_000_000, MAXERR, keep=(5,))
    return Cm, p, x, n, conv, kept[5]


def test_slow_matrix_converges_on_the_device(dev, slow):
    from lam_slide_amd import msm
    Cm, p, x, n, conv, x5 = slow
    assert conv and n > 20000 and p.na == 12
    mod = msm.estimate_markov_model(counts=torch.from_numpy(Cm).to(dev))
    print(f"msm slow matrix: n_iter {int(mod.n_iter)} (oracle {n}), err {float(mod.err):.3e}")
    assert bool(mod.converged) and abs(int(mod.n_iter) - n) <= 1
    parity("msm_slow_pi (units of 2 maxerr)", orc.rel_diff(mod.pi.cpu().numpy(), x) / (2 * MAXERR), 1.0)
    cut = msm.estimate_markov_model(counts=torch.from_numpy(Cm).to(dev), maxiter=5)
    assert not bool(cut.converged) and int(cut.n_iter) == 5
    parity("msm_slow_fifth_iterate (units of U)", orc.rel_diff(cut.pi.cpu().numpy(), x5) / U, 16 * orc.ORDER_DIFF_PI / U)


# ---- bits ----
def test_split_launches_batches_and_repeats_have_the_same_bits(dev):
    base = orc.chain_counts(33, 5000, 1, 0)
    thin = base * (base > 5)
    few = base.copy()
    few[20:] = 0  # the last states only receive: another active set
    mats = np.stack([base, thin, few])
    sets = [tuple(orc.active_set(m).nonzero()[0]) for m in mats]
    assert len(set(sets)) == 3  # ns-equal matrices of different active sets
    one = State(dev, mats).step(21, maxerr=-1.0, restart=1)
    three = State(dev, mats).step(7, maxerr=-1.0, restart=1).step(7, maxerr=-1.0).step(7, maxerr=-1.0)
    again = State(dev, mats).step(21, maxerr=-1.0, restart=1)
    for a, b in zip(one.snapshot(), three.snapshot()):
        assert same_bits(a, b)
    for a, b in zip(one.snapshot(), again.snapshot()):
        assert same_bits(a, b)
    assert one.n_iter.tolist() == [21, 21, 21]
    To, po = one.tmatrix()
    for s in range(3):
        alone = State(dev, mats[s:s + 1]).step(21, maxerr=-1.0, restart=1)
        for a, b in zip(alone.snapshot(), one.snapshot()):
            assert same_bits(a[0], b[s]), s
        Ta, pa = alone.tmatrix()
        assert same_bits(Ta[0], To[s]) and same_bits(pa[0], po[s])
    # a series that stops on its own leaves the others running, in any position of the batch
    mixed = State(dev, mats[[1, 0, 2]]).step(4096, restart=1)
    ref = State(dev, mats).step(4096, restart=1)
    assert ref.done.tolist() == [1, 1, 1] and len(set(ref.n_iter.tolist())) >= 2
    for a, b in zip(mixed.snapshot(), ref.snapshot()):
        assert same_bits(a, b[[1, 0, 2]])


def test_a_launch_on_a_finished_series_touches_nothing(dev):
    mats = np.stack([orc.chain_counts(10, 20000, 10, 0), orc.chain_counts(10, 20000, 10, 1)])
    st = State(dev, mats).step(3, maxerr=-1.0, restart=1)
    st.x[0] = float("nan")
    st.x[0, 3] = -7.5
    st.n_iter[0], st.err[0], st.done[0] = 77, 3.5, 1
    before = st.snapshot()
    st.step(5, maxerr=-1.0)
    after = st.snapshot()
    for a, b in zip(before, after):
        assert same_bits(a[0], b[0])
    assert int(st.n_iter[1]) == 8 and int(st.done[1]) == 0
    # maxiter: the count stops there, done says why
    st.step(100, maxiter=12, maxerr=-1.0)
    assert int(st.n_iter[1]) == 12 and int(st.done[1]) == 2 and int(st.n_iter[0]) == 77
    # restart sets the state from the counts whatever it held
    st.step(0, restart=1)
    p = orc.Problem(mats[0])
    full = np.zeros(10)
    full[p.A] = p.x0
    assert np.array_equal(st.x[0].cpu().numpy(), full) and st.n_iter.tolist() == [0, 0] and st.done.tolist() == [0, 0] and st.err.tolist() == [0.0, 0.0]


# ---- the block end to end ----
def test_markov_state_block_end_to_end(dev):
    from lam_slide_amd import msm
    ref, traj, centers = orc.three_wells(20000, 1), orc.three_wells(4000, 2), orc.well_centers()
    asg = np.arange(12) // 4
    asg5 = np.where(asg == 2, 4, asg)  # five coarse states, two of them never seen
    rd, td, cd = (torch.from_numpy(a.copy()).to(dev) for a in (ref, traj, centers))
    ad = torch.from_numpy(asg5.astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # with assignments given nothing is read back
    try:
        out = msm.markov_state_block(rd, td, cd, metastable_assignments=ad, nstates=5, lag=5, msm_lag=2)
        assert msm.last_path["markov_state_block"] == "fused"
        auto = msm.markov_state_block(rd, td, cd, nstates=3, lag=5, msm_lag=2)  # (the one read, through _lib.to_host)
        assert torch.cuda.get_sync_debug_mode() == 2
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert msm.last_path["markov_state_block"] == "fused" and all(v.is_cuda for v in out.values())
    want = orc.state_block(ref, traj, centers, asg5, 5, 5, 2)
    for k in ("ref_metastable_probs", "traj_metastable_probs"):
        assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    for k in ("msm_transition_matrix", "msm_pi", "traj_transition_matrix", "traj_pi"):
        parity(f"msm_block_{k} (units of 2 maxerr)", orc.rel_diff(out[k].cpu().numpy(), want[k]) / (2 * MAXERR), 1.0)
    T = out["msm_transition_matrix"].cpu().numpy()
    assert np.array_equal(T[2:4], np.eye(5)[2:4]) and np.all(out["msm_pi"].cpu().numpy()[2:4] == 0)
    got = auto["metastable_assignments"].cpu().numpy()
    assert np.array_equal(got[:, None] == got[None, :], asg[:, None] == asg[None, :])  # the three wells, up to the names of the sets
    want3 = orc.state_block(ref, traj, centers, got, 3, 5, 2)
    for k in ("msm_transition_matrix", "msm_pi", "traj_transition_matrix", "traj_pi"):
        assert orc.rel_diff(auto[k].cpu().numpy(), want3[k]) <= 2 * MAXERR, k
    assert np.array_equal(auto["ref_metastable_probs"].cpu().numpy(), want3["ref_metastable_probs"])
