"""``lam_slide_amd.msm`` without a GPU: the C ABI (symbols, header, the limit, every refusal before anything touches a GPU), the numpy
restatement against the oracle of tests/msm_oracle.py, PCCA+ by the inner simplex algorithm on a planted matrix, implied timescales, the
Markov-state block's keys and embedding - and the conditions on the oracle itself that the GPU tests (tests/test_hip_msm.py) rely on."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import msm_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lsl_msm_active_set", "lsl_msm_reversible_step", "lsl_msm_transition_matrix")
U = orc.U


# ---- the C ABI ----
def test_library_exports_header_and_limit():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib, msm
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
        assert getattr(lib, s).argtypes is not None
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6
    assert "lsl_msm_active_set, lsl_msm_reversible_step, lsl_msm_transition_matrix added the same way" in header
    src = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_msm.hip.h")).read()
    macro = lambda name: int(re.search(r"^#define " + name + r" (\d+)", src, re.M).group(1))  # noqa: E731
    assert macro("LSL_MSM_MAX_STATES") == msm.MAX_STATES == _lib.TR_MAX_STATES == 128 and macro("LSL_MSM_MAX_S") == msm.MAX_S == 65535
    assert not hasattr(_lib, "MSM_MAX_STATES")  # the mirror lives in the module, as peptide_loss.MAX_R does
    assert not re.search(r"atomic\w*\(", src)  # no atomics at all
    # fp64 K of the widest form and the vectors beside it fit the 160 KiB of LDS
    parts = macro("LSL_MSM_PARTS")  # threads per row: 8 * 128 = 1024 threads at the widest form
    assert parts * msm.MAX_STATES <= 1024
    assert 8 * msm.MAX_STATES ** 2 + 8 * (1 + parts) * msm.MAX_STATES + 32 + 16 * msm.MAX_STATES + 4 * msm.MAX_STATES <= 160 * 1024


def test_entry_points_refuse_before_a_launch():
    from lam_slide_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch

    def active(S=1, ns=10, counts=one, act=one, na=one):
        return lib.lsl_msm_active_set(counts, S, ns, act, na, None)

    def step(S=1, ns=10, iters=8, maxiter=100, maxerr=1e-8, restart=1, **ptr):
        p = {k: ptr.get(k, one) for k in ("counts", "active", "x", "n_iter", "err", "done")}
        return lib.lsl_msm_reversible_step(p["counts"], p["active"], S, ns, iters, maxiter, maxerr, restart, p["x"], p["n_iter"], p["err"], p["done"], None)

    def tmat(S=1, ns=10, **ptr):
        p = {k: ptr.get(k, one) for k in ("counts", "active", "x", "T", "pi")}
        return lib.lsl_msm_transition_matrix(p["counts"], p["active"], p["x"], S, ns, p["T"], p["pi"], None)

    for k in ("counts", "act", "na"):
        assert active(**{k: None}) == -1, k
    for k in ("counts", "active", "x", "n_iter", "err", "done"):
        assert step(**{k: None}) == -1, k
    for k in ("counts", "active", "x", "T", "pi"):
        assert tmat(**{k: None}) == -1, k
    assert b"null" in lib.lsl_last_error()
    for kw in (dict(ns=0), dict(ns=129), dict(ns=-1), dict(S=0), dict(S=65536)):
        for f in (active, step, tmat):
            assert f(**kw) == -3, (f.__name__, kw)
    assert step(ns=129) == -3 and b"ns = 129" in lib.lsl_last_error() and b"LDS" in lib.lsl_last_error()
    assert step(S=65536) == -3 and b"S = 65536" in lib.lsl_last_error()
    assert step(iters=-1) == -3 and b"iters = -1" in lib.lsl_last_error()
    assert step(maxiter=-1) == -3 and step(maxerr=float("nan")) == -3 and b"maxerr" in lib.lsl_last_error()


# ---- the oracle itself: what the GPU tests rely on ----
def test_oracle_active_set_rules():
    C7 = np.zeros((7, 7), dtype=np.int64)
    C7[0, 2] = C7[2, 5] = C7[5, 0] = 3
    C7[1, 4] = C7[4, 1] = 9
    C7[3, 0], C7[6, 6] = 2, 50
    assert orc.active_set(C7).nonzero()[0].tolist() == [0, 2, 5]
    C4 = np.zeros((4, 4), dtype=np.int64)
    C4[0, 1] = C4[1, 0] = C4[2, 3] = C4[3, 2] = 1
    assert orc.active_set(C4).nonzero()[0].tolist() == [0, 1]
    assert not orc.active_set(np.zeros((5, 5), dtype=np.int64)).any()
    C1 = np.zeros((3, 3), dtype=np.int64)
    C1[1, 1] = 4
    assert orc.active_set(C1).nonzero()[0].tolist() == [1]


def test_oracle_conditions_of_the_gpu_cases():
    """The seeds are chosen so that the oracle's two summation orders stop at the same count, the oracle itself holds detailed balance within
    1e-9 after convergence at 1e-12, and the order differences after 64 steps are what msm_oracle.ORDER_DIFF_* say."""
    for case in orc.CONVERGED_CASES:
        Cm = orc.chain_counts(*case)
        a = orc.estimate(Cm)
        b = orc.estimate(Cm, perm=orc.reversed_perm(a["n_active"]))
        assert a["converged"] and a["n_iter"] == b["n_iter"] >= 1 and a["n_active"] >= 2, case
        assert orc.rel_diff(b["pi_A"], a["pi_A"]) <= 2e-8
        fine = orc.estimate(Cm, maxerr=1e-12)
        F = fine["pi_A"][:, None] * fine["T_A"]
        m = F > 0
        assert float((np.abs(F - F.T)[m] / F[m]).max()) <= 1e-9, case
    dp, dt = (max(v) for v in zip(*(orc.order_differences(case) for case in orc.FIXED_CASES)))
    print(f"oracle order differences after 64 steps: pi {dp / U:.1f} * 2^-53, T {dt / U:.1f} * 2^-53")
    assert orc.ORDER_DIFF_PI / 2 <= dp <= orc.ORDER_DIFF_PI and orc.ORDER_DIFF_T / 2 <= dt <= orc.ORDER_DIFF_T
    assert any(orc.Problem(orc.chain_counts(*case)).na < case[0] for case in orc.CONVERGED_CASES)  # some case has states outside A


# ---- the numpy restatement against the oracle ----
def check_model(mod, want, maxerr=1e-8, s=None):
    pick = (lambda t: t.numpy()) if s is None else (lambda t: t[s].numpy())
    assert np.array_equal(pick(mod.active), want["active"]) and int(pick(mod.n_active)) == want["n_active"]
    assert abs(int(pick(mod.n_iter)) - want["n_iter"]) <= 1 and bool(pick(mod.converged)) == want["converged"]
    T, pi = pick(mod.transition_matrix), pick(mod.pi)
    assert np.all(np.abs(pi - want["pi"]) <= 2 * maxerr * want["pi"]) and np.all(np.abs(T - want["T"]) <= 2 * maxerr * want["T"])
    out = ~want["active"]
    assert np.array_equal(T[out], np.eye(len(pi))[out]) and np.array_equal(T[:, out][want["active"]], np.zeros((want["n_active"], int(out.sum()))))
    assert np.all(pi[out] == 0)


@pytest.mark.parametrize("case", orc.CONVERGED_CASES[:4] + ((130, 30000, 2, 0),))
def test_restatement_matches_the_oracle(case):
    from lam_slide_amd import msm
    ns, n, lag, seed = case
    d = torch.from_numpy(orc.chain(ns, n, seed).copy())
    mod = msm.estimate_markov_model(d, lag, ns)
    assert mod.path == "torch" == msm.last_path["estimate_markov_model"] and mod.lag == lag
    assert mod.transition_matrix.dtype == torch.float64 and mod.pi.dtype == torch.float64 and mod.active.dtype == torch.bool
    assert mod.n_active.dtype == torch.int32 and mod.n_iter.dtype == torch.int32 and mod.err.dtype == torch.float64 and mod.converged.dtype == torch.bool
    Cm = orc.chain_counts(*case)
    assert np.array_equal(mod.counts.numpy(), Cm)
    want = orc.estimate(Cm)
    check_model(mod, want)
    A, TA, piA = mod.restricted()
    assert np.array_equal(A, want["problem"].A) and TA.shape == (len(A), len(A)) and abs(piA.sum() - 1) <= 1e-12
    assert np.all(np.abs(TA.sum(axis=1) - 1) <= (len(A) + 2) * U)
    act, na = msm.active_set(torch.from_numpy(Cm))
    assert np.array_equal(act.numpy(), want["active"]) and int(na) == want["n_active"] and msm.last_path["active_set"] == "torch"


def test_batch_special_cases_maxiter_and_arguments():
    from lam_slide_amd import msm
    mats = [orc.chain_counts(10, 20000, 10, 0), np.zeros((10, 10), dtype=np.int64), np.zeros((10, 10), dtype=np.int64), orc.chain_counts(10, 20000, 10, 1)]
    mats[2][4, 4] = 7  # a single self-loop
    mats[3] = mats[3] - 5 * (mats[3] < 5)  # entries <= 0 count as 0
    mod = msm.estimate_markov_model(counts=torch.from_numpy(np.stack(mats)))
    assert mod.transition_matrix.shape == (4, 10, 10) and mod.pi.shape == (4, 10) and mod.n_iter.shape == (4,) and mod.lag is None
    for s, m in enumerate(mats):
        check_model(mod, orc.estimate(m), s=s)
    assert int(mod.n_active[1]) == 0 and int(mod.n_iter[1]) == 0 and bool(mod.converged[1]) and torch.equal(mod.transition_matrix[1], torch.eye(10, dtype=torch.float64))
    assert int(mod.n_active[2]) == 1 and float(mod.pi[2, 4]) == 1.0 and float(mod.pi[2].sum()) == 1.0 and bool(mod.converged[2]) and int(mod.n_iter[2]) == 0
    A, TA, piA = mod.restricted(2)
    assert A.tolist() == [4] and TA.tolist() == [[1.0]] and piA.tolist() == [1.0]
    cut = msm.estimate_markov_model(counts=mats[0], maxiter=5)
    x5, n5, _, conv5 = orc.Problem(mats[0]).iterate(5, 1e-8)
    assert int(cut.n_iter) == 5 == n5 and not bool(cut.converged) and not conv5
    assert orc.rel_diff(cut.pi.numpy()[orc.active_set(mats[0])], x5) <= 16 * orc.ORDER_DIFF_PI
    never = msm.estimate_markov_model(counts=mats[0], maxiter=40, maxerr=-1.0)
    assert int(never.n_iter) == 40 and not bool(never.converged)
    with pytest.raises(NotImplementedError):
        msm.estimate_markov_model(counts=mats[0], reversible=False)
    with pytest.raises(TypeError):
        msm.estimate_markov_model()
    with pytest.raises(TypeError):
        msm.estimate_markov_model(torch.zeros(10, dtype=torch.int32), counts=mats[0])
    with pytest.raises(TypeError):
        msm.estimate_markov_model(torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError):
        msm.estimate_markov_model(counts=np.zeros((3, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        msm.estimate_markov_model(counts=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        msm.estimate_markov_model(counts=mats[0], maxiter=-1)
    with pytest.raises(ValueError):
        mod.timescales(1)  # no lag recorded


# ---- PCCA+ and timescales ----
def test_pcca_recovers_planted_blocks():
    from lam_slide_amd import msm
    for seed in range(4):
        T, pi, member = orc.planted_blocks(3, 4, 1e-3, seed)
        chi, asg = msm.pcca_assignments(T, pi, 3)
        assert chi.shape == (12, 3) and asg.shape == (12,)
        assert np.all(np.abs(chi.sum(axis=1) - 1) <= 1e-12)
        # the blocks: two states share a set exactly when they share a planted block
        assert np.array_equal(asg[:, None] == asg[None, :], member[:, None] == member[None, :]), seed
        want_chi, want_asg, idx = orc.isa(T, pi, 3)
        assert np.all(np.abs(chi[idx] - np.eye(3)) <= 1e-12)
        assert np.array_equal(asg, want_asg) and np.all(np.abs(chi - want_chi) <= 1e-9)
    with pytest.raises(ValueError):
        msm.pcca_assignments(T, pi, 13)
    chi1, asg1 = msm.pcca_assignments(T, pi, 1)
    assert np.array_equal(chi1, np.ones((12, 1))) and not asg1.any()


def test_timescales_of_a_two_state_chain():
    from lam_slide_amd import msm
    Cm = np.array([[900, 100], [150, 350]], dtype=np.int64)
    mod = msm.estimate_markov_model(counts=Cm, lag=7, maxerr=1e-13)
    _, T, pi = mod.restricted()
    ts = mod.timescales(1)
    assert ts.shape == (1,) and abs(ts[0] - (-7.0 / np.log(1.0 - T[0, 1] - T[1, 0]))) <= 1e-9 * ts[0]
    assert np.array_equal(mod.timescales(), ts) and mod.timescales(0).shape == (0,)
    with pytest.raises(ValueError):
        mod.timescales(2)
    # the reversible estimate of two states has pi_0 T_01 = pi_1 T_10 and the symmetrised counts' flows
    assert abs(pi[0] * T[0, 1] - pi[1] * T[1, 0]) <= 1e-12


# ---- the Markov-state block ----
KEYS = {"ref_metastable_probs", "traj_metastable_probs", "msm_transition_matrix", "msm_pi", "traj_transition_matrix", "traj_pi", "metastable_assignments"}


def test_markov_state_block_keys_embedding_and_oracle_chain():
    from lam_slide_amd import msm
    ref, traj, centers = orc.three_wells(6000, 1), orc.three_wells(1500, 2)[:, :].copy(), orc.well_centers()
    traj = traj[orc.nearest(traj, centers) < 8]  # the trajectory never visits the third well
    asg = np.arange(12) // 4
    asg5 = np.where(asg == 2, 4, asg)  # five coarse states, two of them (2 and 3) never seen
    out = msm.markov_state_block(torch.from_numpy(ref.copy()), torch.from_numpy(traj), torch.from_numpy(centers), metastable_assignments=asg5, nstates=5,
                                 lag=5, msm_lag=2)
    assert set(out) == KEYS and msm.last_path["markov_state_block"] == "torch"
    want = orc.state_block(ref, traj, centers, asg5, 5, 5, 2)
    for k in ("ref_metastable_probs", "traj_metastable_probs"):
        assert out[k].dtype == torch.float64 and np.array_equal(out[k].numpy(), want[k]), k
    for k in ("msm_transition_matrix", "msm_pi", "traj_transition_matrix", "traj_pi"):
        assert out[k].dtype == torch.float64 and np.all(np.abs(out[k].numpy() - want[k]) <= 2e-8 * want[k]), k
    T, pi = out["msm_transition_matrix"].numpy(), out["msm_pi"].numpy()
    assert np.array_equal(T[2:4], np.eye(5)[2:4]) and np.array_equal(T[:, 2:4][[0, 1, 4]], np.zeros((3, 2))) and np.all(pi[2:4] == 0) and pi[4] > 0
    Tt, pt = out["traj_transition_matrix"].numpy(), out["traj_pi"].numpy()
    assert np.array_equal(Tt[2:], np.eye(5)[2:]) and np.all(pt[2:] == 0) and abs(pt.sum() - 1) <= 1e-12 and float(out["traj_metastable_probs"][4]) == 0.0
    assert np.array_equal(out["metastable_assignments"].numpy(), asg5) and out["metastable_assignments"].dtype == torch.int32
    # without assignments: the host PCCA finds the three wells (up to the names of the sets)
    auto = msm.markov_state_block(torch.from_numpy(ref.copy()), torch.from_numpy(traj), torch.from_numpy(centers), nstates=3, lag=5, msm_lag=2, traj_msm=False)
    assert set(auto) == KEYS - {"traj_transition_matrix", "traj_pi"}
    got = auto["metastable_assignments"].numpy()
    assert np.array_equal(got[:, None] == got[None, :], asg[:, None] == asg[None, :]) and sorted(set(got.tolist())) == [0, 1, 2]
    assert abs(float(auto["msm_pi"].sum()) - 1) <= 1e-12 and abs(float(auto["ref_metastable_probs"].sum()) - 1) <= 1e-12
    with pytest.raises(ValueError):
        msm.markov_state_block(torch.from_numpy(ref.copy()), torch.from_numpy(traj), torch.from_numpy(centers), metastable_assignments=asg[:5], nstates=3)
    with pytest.raises(ValueError):
        msm.markov_state_block(torch.from_numpy(ref.copy()), torch.from_numpy(traj), torch.from_numpy(centers), nstates=13, lag=5)


def test_package_exports_and_example_runs_on_the_cpu():
    import lam_slide_amd
    for name in ("msm", "MarkovModel", "active_set", "estimate_markov_model", "markov_state_block", "pcca_assignments"):
        assert name in lam_slide_amd.__all__ and hasattr(lam_slide_amd, name), name
    import importlib.util
    spec = importlib.util.spec_from_file_location("peptide_msm_on_device", os.path.join(ROOT, "examples", "peptide_msm_on_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.main(device="cpu", n_ref=4000, n_traj=1000, lag=20, msm_lag=5, k=30)
    assert KEYS <= set(out)
