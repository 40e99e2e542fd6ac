"""``lam_slide_amd.tica`` without a GPU: the numpy / torch restatements of the TICA and state statistics against the oracle of
tests/tica_oracle.py (direct float64 moments, ``scipy.linalg.eigh(Ct, C0)``, the float64 projection, nearest centre, ``np.add.at``),
``linspace_edges`` against ``np.linspace`` bit for bit, the host eigenproblem ``solve_tica``, the model's dimension and kinetic map, and
the C ABI (symbols, header, refusals before anything touches a GPU).

Inputs: the seeded synthetic series of the oracle at its three well-conditioned cases (n, F, lag) = (4000, 5, 10), (20000, 12, 50),
(20000, 33, 100)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.spatial.distance import jensenshannon

import tica_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lsl_lagged_moments_workspace_bytes", "lsl_lagged_moments", "lsl_project", "lsl_assign_centers", "lsl_transition_counts")


@pytest.fixture(scope="module")
def cases():
    """[(x float32 [n, F], lag, (mean, C0, Ct) of the oracle)] of the three cases."""
    out = []
    for i, (n, F, lag) in enumerate(orc.CASES):
        x = orc.series(n, F, seed=100 + i)
        out.append((x, lag, orc.covariances64(x, lag)))
    return out


# ---- the C ABI ----
def test_library_exports_and_header_declare_the_tica_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    exports = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*lsl_\*;", exports) and re.search(r"local:\s*\*;", exports)  # every lsl_ symbol, nothing else
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
        assert re.fullmatch(r"lsl_[a-z_]+", s)
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6 and "lsl_lagged_moments_workspace_bytes, lsl_lagged_moments, lsl_project" in header
    src = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_tica.hip.h")).read()
    macro = lambda name: int(re.search(r"#define " + name + r" (\d+)", src).group(1))  # noqa: E731
    assert macro("LSL_MOM_SEG") == _lib.MOM_SEG == _lib.MOM_CHAIN and macro("LSL_MOM_MAX_F") == _lib.MOM_MAX_F
    assert macro("LSL_PROJ_MAX_D") == _lib.PROJ_MAX_D and macro("LSL_ASG_MAX_K") == _lib.ASG_MAX_K and macro("LSL_ASG_MAX_D") == _lib.ASG_MAX_D
    assert macro("LSL_ASG_CELLS") == _lib.ASG_CELLS and macro("LSL_ASG_MAX_STATES") == _lib.ASG_MAX_STATES
    assert macro("LSL_TR_MAX_STATES") == _lib.TR_MAX_STATES and macro("LSL_TR_MAX_STATES") ** 2 * 4 <= 65536  # int32 counts in 64 KiB of LDS
    seg = _lib.MOM_SEG
    assert _lib.mom_segments(2, 1) == 1 and _lib.mom_segments(seg + 1, 1) == 1 and _lib.mom_segments(seg + 2, 1) == 2
    assert not re.search(r"atomic\w*\([^;]*(float|double)", src)  # integer atomics only


def test_entry_points_validate_arguments_without_gpu():
    from lam_slide_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    mom = lambda x=one, S=1, n=1000, F=12, lag=50, out=one, ws=one, nbytes=1 << 40: lib.lsl_lagged_moments(x, S, n, F, lag, out, ws, nbytes, None)  # noqa: E731
    proj = lambda x=one, n=100, F=12, mean=one, W=one, d=3, y=one, lim=one: lib.lsl_project(x, n, F, mean, W, d, y, lim, None)  # noqa: E731
    asg = lambda y=one, n=100, d=3, c=one, k=100, m=one, ns=10, lab=one, cnt=one: lib.lsl_assign_centers(y, n, d, c, k, m, ns, lab, cnt, None)  # noqa: E731
    trn = lambda dt=one, S=1, n=100, lag=1, ns=10, cnt=one: lib.lsl_transition_counts(dt, S, n, lag, ns, cnt, None)  # noqa: E731
    assert mom(x=None) == -1 and mom(out=None) == -1 and mom(ws=None) == -1
    assert proj(x=None) == -1 and proj(mean=None) == -1 and proj(W=None) == -1 and proj(y=None) == -1
    assert asg(y=None) == -1 and asg(c=None) == -1 and asg(lab=None) == -1
    assert trn(dt=None) == -1 and trn(cnt=None) == -1
    # refused shapes: -3 and a text
    assert mom(lag=1000) == -3 and b"lag" in lib.lsl_last_error()  # lag >= n
    for kw in (dict(lag=0), dict(lag=-1), dict(n=1, lag=1), dict(n=0), dict(F=0), dict(F=129), dict(S=0), dict(S=65536)):
        assert mom(**kw) == -3, kw
    assert mom(nbytes=8) == -4 and b"workspace" in lib.lsl_last_error()
    assert proj(d=17) == -3 and b"d = 17" in lib.lsl_last_error()
    for kw in (dict(d=0), dict(F=0), dict(F=129), dict(n=0), dict(n=-4)):
        assert proj(**kw) == -3, kw
    assert asg(k=1025, d=1) == -3 and b"k = 1025" in lib.lsl_last_error()
    for kw in (dict(k=0), dict(d=0), dict(d=65), dict(k=1024, d=9), dict(n=0), dict(ns=0), dict(ns=1025), dict(ns=0, m=None), dict(ns=0, cnt=None)):
        assert asg(**kw) == -3, kw
    assert trn(ns=129) == -3 and b"nstates = 129" in lib.lsl_last_error()
    for kw in (dict(ns=0), dict(lag=0), dict(lag=-3), dict(n=0), dict(S=0), dict(S=65536)):
        assert trn(**kw) == -3, kw
    # the workspace of the moments: fp64 sums per (series, segment of MOM_SEG steps, entry); 0 for a refused shape
    need = lib.lsl_lagged_moments_workspace_bytes
    E = lambda F: 2 * F + 3 * F * F  # noqa: E731
    assert need(1, 1000, 12, 50) == E(12) * 8 and need(3, 2, 1, 1) == 3 * 5 * 8
    seg = _lib.MOM_SEG
    assert need(2, 3 * seg + 17, 128, seg + 3) == 2 * 3 * E(128) * 8 and need(1, seg + 2, 5, 1) == 2 * E(5) * 8  # m = 2 seg + 14; m = seg + 1
    assert need(1, 1000, 12, 1000) == 0 and need(1, 1000, 129, 1) == 0
    assert need(1, 2 ** 31 - 1, 1, 1) == _lib.mom_segments(2 ** 31 - 1, 1) * 5 * 8
    with pytest.raises(ValueError):
        _lib.check(-3)


# ---- linspace_edges ----
def test_linspace_edges_has_numpy_linspace_bits():
    from lam_slide_amd import linspace_edges
    rng = np.random.default_rng(11)
    checked = 0
    for i in range(200):
        bins = (1, 2, 50, 100)[i % 4]
        scale = 10.0 ** rng.integers(-3, 4)
        lo = np.float32(rng.standard_normal() * scale)
        hi = np.float32(float(lo) + abs(rng.standard_normal()) * scale + 1e-3 * scale)
        assert hi > lo
        want = np.linspace(float(lo), float(hi), bins + 1)
        got = linspace_edges(torch.tensor(lo), torch.tensor(hi), bins)  # (float32 0-dim tensors: what the joint range is)
        assert got.dtype == torch.float64 and got.shape == (bins + 1,)
        assert np.array_equal(got.numpy().view(np.int64), want.view(np.int64)), (lo, hi, bins)
        assert np.array_equal(want, np.histogram_bin_edges(np.zeros(1), bins=bins, range=(float(lo), float(hi))))
        checked += 1
    assert checked == 200
    for v, bins in ((0.0, 100), (1.5, 50), (-3.25, 1), (1e6, 2)):  # lo == hi: np.histogram widens the range by +-0.5
        want = np.histogram_bin_edges(np.zeros(1), bins=bins, range=(v, v))
        got = linspace_edges(torch.tensor(v), torch.tensor(v), bins).numpy()
        assert np.array_equal(got.view(np.int64), want.view(np.int64)) and got[0] == v - 0.5 and got[-1] == v + 0.5
    assert np.array_equal(linspace_edges(-1.0, 2.5, 14).numpy(), np.linspace(-1.0, 2.5, 15))  # python floats work too
    with pytest.raises(ValueError):
        linspace_edges(0.0, 1.0, 0)


# ---- the host eigenproblem ----
def test_solve_tica_against_scipy_generalised_eigh(cases):
    from lam_slide_amd import solve_tica, tica_dimension
    for (x, lag, (mean, C0, Ct)), want_dim in zip(cases, (3, 3, 2)):
        F = x.shape[1]
        lam, R = solve_tica(C0, Ct, 1e-6)
        lam_s, R_s = orc.eigh_scipy(C0, Ct)
        dim = tica_dimension(lam, 0.95)
        s = np.linalg.eigvalsh(C0)
        print(f"F = {F}: cond(C0) = {s[-1] / s[0]:.1f}, smallest eigenvalue {s[0]:.2e}, gaps {np.diff(-lam[:dim + 1])}, dim = {dim}")
        assert s[0] > 1e-3 and lam.shape == (F,) and R.shape == (F, F)  # the epsilon cut drops nothing
        assert dim == want_dim == orc.dimension(lam_s) and float(np.diff(-lam[:dim + 1]).min()) >= 0.07
        assert float(np.abs(lam - lam_s).max()) <= 1e-12
        assert float(np.abs(R[:, :dim] - R_s[:, :dim]).max()) <= 1e-10
        assert float(np.abs(R.T @ C0 @ R - np.eye(F)).max()) <= 1e-12
        assert np.all(np.diff(lam) <= 0) and np.all(R[np.abs(R).argmax(axis=0), np.arange(F)] > 0)
    # a rank-deficient C0: the duplicated column's direction is dropped by the epsilon cut
    x, lag, _ = cases[0]
    xd = np.concatenate([x, x[:, :1]], axis=1)
    _, C0, Ct = orc.covariances64(xd, lag)
    lam, R = solve_tica(C0, Ct, 1e-6)
    assert lam.shape == (5,) and R.shape == (6, 5) and float(np.abs(lam - solve_tica(*cases[0][2][1:])[0]).max()) <= 1e-10
    with pytest.raises(ValueError):
        solve_tica(np.zeros((3, 3)), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        solve_tica(np.eye(3), np.eye(4))


def test_dimension_and_kinetic_map_scaling():
    from lam_slide_amd import TicaModel, tica_dimension
    lam = np.array([0.9, 0.5, 0.1, 0.05])
    cum = np.cumsum(lam ** 2) / (lam ** 2).sum()
    assert tica_dimension(lam, 0.95) == 2 and cum[0] < 0.95 <= cum[1]
    assert tica_dimension(lam, 0.5) == 1 and tica_dimension(lam, 0.99) == 3 and tica_dimension(lam, 1.0) == 4 and tica_dimension(lam[:1]) == 1
    R = np.random.default_rng(3).standard_normal((6, 4))
    mean = np.arange(6.0)
    km = TicaModel.from_arrays(mean, R, lam, dim=2)
    plain = TicaModel.from_arrays(mean, R, lam, dim=2, kinetic_map=False)
    assert km.W.shape == (6, 2) and np.array_equal(plain.W, R[:, :2]) and np.array_equal(km.W, R[:, :2] * lam[:2])
    assert TicaModel.from_arrays(mean, R, lam).dim == 4  # dim None: every column
    for bad in (dict(dim=0), dict(dim=5)):
        with pytest.raises(ValueError):
            TicaModel.from_arrays(mean, R, lam, **bad)
    with pytest.raises(ValueError):
        TicaModel.from_arrays(mean[:5], R, lam)


# ---- the torch path of every public function ----
def test_features_moments_and_covariances_restatements(cases):
    from lam_slide_amd import cossin_features, lagged_moments, tica, tica_covariances
    ang = torch.from_numpy(np.random.default_rng(5).uniform(-np.pi, np.pi, size=(2, 7, 3)))
    f = cossin_features(ang)
    assert f.shape == (2, 7, 6) and torch.equal(f[..., 0::2], torch.cos(ang)) and torch.equal(f[..., 1::2], torch.sin(ang))
    for x, lag, (mean, C0, Ct) in cases[:2]:
        want, absum = orc.moments64(x, lag)
        got = lagged_moments(torch.from_numpy(x), lag)
        assert tica.last_path["lagged_moments"] == "torch" and all(g.dtype == torch.float64 for g in got)
        for g, w, a in zip(got, want, absum):
            assert g.shape == w.shape and float((np.abs(g.numpy() - w) / a).max()) <= 64 * 2.0 ** -53  # (blocked float64 sums of either side)
        m, c0, ct = tica_covariances(torch.from_numpy(x), lag)
        assert float(np.abs(m.numpy() - mean).max()) <= 1e-15 and float(np.abs(c0.numpy() - C0).max()) <= 1e-15
        assert float(np.abs(ct.numpy() - Ct).max()) <= 1e-15 and torch.equal(c0, c0.T) and torch.equal(ct, ct.T)
    x, lag, _ = cases[0]
    xs = torch.from_numpy(np.stack([x, x[::-1].copy()]))
    batched = lagged_moments(xs, lag)
    assert batched[0].shape == (2, 5) and batched[4].shape == (2, 5, 5)
    assert float((batched[2][0] - lagged_moments(xs[0], lag)[2]).abs().max()) <= 1e-12
    assert float((batched[4][1] - batched[4][0].T).abs().max()) <= 1e-9  # the reversed series: xy transposed
    two = lagged_moments(torch.tensor([[2.0, 1.0], [3.0, -1.0]]), 1)  # n = 2: one term
    assert two[0].tolist() == [2.0, 1.0] and two[1].tolist() == [3.0, -1.0] and two[4].tolist() == [[6.0, -2.0], [3.0, -1.0]]
    for bad in (0, -1, 4000, 9000):
        with pytest.raises(ValueError, match="lag"):
            lagged_moments(torch.from_numpy(x), bad)
    with pytest.raises(ValueError):
        lagged_moments(torch.from_numpy(x)[0], 1)


def test_model_fit_transform_and_round_trip(cases):
    from lam_slide_amd import TicaModel, tica
    for (x, lag, (mean, C0, Ct)), want_dim in zip(cases, (3, 3, 2)):
        xt = torch.from_numpy(x)
        model = TicaModel.fit(xt, lag=lag)
        lam_s, R_s = orc.eigh_scipy(C0, Ct)
        assert tica.last_path["fit"] == "torch" and model.dim == want_dim and model.lag == lag and model.kinetic_map
        assert float(np.abs(model.eigenvalues - lam_s).max()) <= 1e-10 and float(np.abs(model.mean - mean).max()) <= 1e-15
        assert float(np.abs(model.W - R_s[:, :want_dim] * lam_s[:want_dim]).max()) <= 1e-9
        lim = torch.tensor([[np.inf] * want_dim, [-np.inf] * want_dim], dtype=torch.float32)
        y = model.transform(xt, lim)
        y64, absum = orc.project64(x, model.mean, model.W)
        assert tica.last_path["transform"] == "torch" and y.dtype == torch.float32 and y.shape == (x.shape[0], want_dim)
        bar = 2.0 ** -24 * np.abs(y64) + 2.0 ** -149 + (x.shape[1] + 2) * 2.0 ** -53 * absum
        assert np.all(np.abs(y.double().numpy() - y64) <= bar)
        assert np.array_equal(lim.numpy(), np.stack([y.numpy().min(0), y.numpy().max(0)]))
        # the kinetic map: the variance of component j is eigenvalue_j^2 (the reversible estimate normalises R^T C0 R = I)
        var = ((y64[:x.shape[0] - lag] ** 2).sum(0) + (y64[lag:] ** 2).sum(0)) / (2.0 * (x.shape[0] - lag))
        assert float(np.abs(var - model.eigenvalues[:want_dim] ** 2).max()) <= 1e-9
        again = TicaModel.from_arrays(model.mean, model.eigenvectors, model.eigenvalues, dim=model.dim, kinetic_map=model.kinetic_map)
        assert np.array_equal(again.W, model.W) and torch.equal(again.transform(xt), y)
        assert torch.equal(model.transform(xt[None].expand(2, -1, -1))[1], y)  # a leading batch dimension
    model = TicaModel.fit(torch.from_numpy(cases[0][0]), lag=10, kinetic_map=False, var_cutoff=0.3)
    assert model.dim == 1 and np.array_equal(model.W, model.eigenvectors[:, :1])
    xt = torch.from_numpy(cases[0][0][:50].copy())
    xt[7, 2] = float("nan")
    lim = torch.tensor([[0.25], [-0.25]])
    y = model.transform(xt, lim)  # a NaN row is ignored by the limits; the limits given are kept
    ok = y[~torch.isnan(y[:, 0]), 0]
    assert torch.isnan(y[7, 0]) and float(lim[0, 0]) == min(0.25, float(ok.min())) and float(lim[1, 0]) == max(-0.25, float(ok.max()))
    for bad in (torch.zeros(2, 2), torch.zeros(2, 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="lim"):
            model.transform(xt, bad)
    with pytest.raises(ValueError):
        model.transform(xt[:, :4])


def test_tica_jsd_restatement_is_numpy_and_scipy(cases):
    from lam_slide_amd import TicaModel, summary_metrics, tica, tica_autocovariance, tica_histograms, tica_jsd
    x, lag, _ = cases[1]
    ref, traj = torch.from_numpy(x), torch.from_numpy(orc.series(2000, x.shape[1], seed=7))
    model = TicaModel.fit(ref, lag=lag)
    h = tica_histograms(model, ref, traj)
    assert tica.last_path["tica_histograms"] == "torch" and h.ref_counts.shape == (100,) and h.traj_counts2.shape == (50, 50)
    yr, yt = h.y_ref.numpy().astype(np.float64), h.y_traj.numpy().astype(np.float64)
    lo, hi = np.minimum(yr.min(0), yt.min(0)), np.maximum(yr.max(0), yt.max(0))
    assert np.array_equal(h.lim.numpy().astype(np.float64), np.stack([lo, hi]))
    assert np.array_equal(h.edges.numpy(), np.linspace(lo[0], hi[0], 101)) and np.array_equal(h.edges2b.numpy(), np.linspace(lo[1], hi[1], 51))
    want = {}
    for name, y, c, c2 in (("ref", yr, h.ref_counts, h.ref_counts2), ("traj", yt, h.traj_counts, h.traj_counts2)):
        want[name] = (np.histogram(y[:, 0], range=(lo[0], hi[0]), bins=100)[0],
                      np.histogram2d(y[:, 0], y[:, 1], range=((lo[0], hi[0]), (lo[1], hi[1])), bins=50)[0])
        assert np.array_equal(c.numpy(), want[name][0]) and np.array_equal(c2.numpy(), want[name][1]) and int(c.sum()) == len(y) == int(c2.sum())
    d = tica_jsd(model, ref, traj)
    assert list(d) == ["TICA-0", "TICA-0,1"] and tica.last_path["tica_jsd"] == "torch"
    assert abs(d["TICA-0"] ** 2 - jensenshannon(want["ref"][0], want["traj"][0]) ** 2) <= 100 * 2.0 ** -50
    assert abs(d["TICA-0,1"] ** 2 - jensenshannon(want["ref"][1].reshape(-1), want["traj"][1].reshape(-1)) ** 2) <= 2500 * 2.0 ** -50
    assert 0.0 < d["TICA-0"] < math.sqrt(math.log(2)) and tica_jsd(model, ref, ref) == {"TICA-0": 0.0, "TICA-0,1": 0.0}
    merged = {"PHI 1": 0.1, "CHI1 0": 0.3, **d}
    out = summary_metrics([merged, merged])
    assert out["TICA-0"] == pytest.approx(d["TICA-0"]) and out["TICA-0,1"] == pytest.approx(d["TICA-0,1"]) and out["ALL"] == pytest.approx(0.2)
    one = TicaModel.from_arrays(model.mean, model.eigenvectors, model.eigenvalues, dim=1)
    assert list(tica_jsd(one, ref, traj)) == ["TICA-0"] and tica_jsd(one, ref, traj)["TICA-0"] == d["TICA-0"]
    ac = tica_autocovariance(h.y_traj, 20)
    y0 = yt[:, 0]
    assert ac.shape == (21,) and float(np.abs(ac.double().numpy() - [np.dot(y0[:len(y0) - k], y0[k:]) / (len(y0) - k) for k in range(21)]).max()) <= 2.0 ** -24


def test_assign_centers_and_metastable_jsd_restatements():
    from lam_slide_amd import assign_centers, metastable_jsd, tica
    rng = np.random.default_rng(9)
    y = rng.standard_normal((500, 3)).astype(np.float32)
    centers = rng.standard_normal((20, 3)).astype(np.float32)
    centers[13] = centers[4]  # an exact duplicate: the lowest index wins
    y[17, 1] = np.nan
    want, _, _ = orc.assign64(y, centers)
    labels, counts = assign_centers(torch.from_numpy(y), centers)
    assert tica.last_path["assign_centers"] == "torch" and labels.dtype == torch.int32 and counts.dtype == torch.int64 and counts.shape == (20,)
    assert np.array_equal(labels.numpy(), want) and want[17] == -1 and (want == 4).any() and not (want == 13).any()
    assert np.array_equal(counts.numpy(), np.bincount(want[want >= 0], minlength=20)) and int(counts.sum()) == 499
    smap = rng.integers(0, 5, size=20)
    smap[2] = 7  # outside 0..nstates-1
    labels2, counts2 = assign_centers(torch.from_numpy(y), torch.from_numpy(centers), state_map=smap, nstates=5)
    want2 = np.where(want >= 0, smap[np.maximum(want, 0)], -1)
    want2[want2 >= 5] = -1
    assert np.array_equal(labels2.numpy(), want2) and (want == 2).any() and np.array_equal(counts2.numpy(), np.bincount(want2[want2 >= 0], minlength=5))
    assert assign_centers(torch.from_numpy(y), centers, state_map=torch.from_numpy(smap))[1].shape == (8,)  # nstates = max + 1
    ref = torch.from_numpy(np.bincount(rng.integers(0, 5, size=4000), minlength=5))
    d = metastable_jsd(ref, counts2)
    assert d.dtype == torch.float64 and d.shape == () and abs(float(d) ** 2 - jensenshannon(ref.numpy(), counts2.numpy()) ** 2) <= 5 * 2.0 ** -50
    assert float(metastable_jsd(ref, ref)) == 0.0
    for bad in (dict(centers=centers[:, :2]), dict(centers=centers, state_map=smap[:5]), dict(centers=centers, nstates=0)):
        with pytest.raises(ValueError):
            assign_centers(torch.from_numpy(y), **bad)


def test_transition_counts_restatement_is_add_at():
    from lam_slide_amd import tica, transition_counts
    d = orc.labels(3000, 10, seed=4)
    assert (d == -1).sum() > 10
    for lag in (1, 7, 2999):
        got = transition_counts(torch.from_numpy(d), lag, 10)
        assert tica.last_path["transition_counts"] == "torch" and got.dtype == torch.int64 and got.shape == (10, 10)
        assert np.array_equal(got.numpy(), orc.transitions_np(d, lag, 10))
    both = transition_counts(torch.from_numpy(np.stack([d, d[::-1].copy()])).long(), 7, 10)
    assert both.shape == (2, 10, 10) and torch.equal(both[1], both[0].T) and int(both[0].sum()) < 2993  # (pairs with a -1 are skipped)
    assert int(transition_counts(torch.from_numpy(d), 3000, 10).sum()) == 0 and int(transition_counts(torch.from_numpy(d), 1, 4).sum()) < 1500
    for bad in (dict(lag=0), dict(nstates=0)):
        with pytest.raises(ValueError):
            transition_counts(torch.from_numpy(d), **{"lag": 1, "nstates": 10, **bad})
    with pytest.raises(ValueError):
        transition_counts(torch.from_numpy(d).float(), 1, 10)
