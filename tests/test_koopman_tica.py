"""``lam_slide_amd.koopman_tica`` without a GPU: the C ABI of the three new entry points (symbols, header, limits, refusals before anything
touches a GPU), the Koopman weights against the brute-force oracle of tests/koopman_tica_oracle.py (``scipy.linalg.eig`` of the transposed
Koopman matrix), their defining stationarity property, the reversible covariances with unit weights against ``tica.tica_covariances``,
a planted slow coordinate recovered by ``run_tica``, and ``traj_analysis(..., tica_lagtime=)`` against the same projections passed in.

deeptime is not installed where these tests run: they check the estimator as the module states it, not parity with a live deeptime."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import koopman_tica_oracle as orc
import structstat_oracle as sorc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lsl_weighted_moments_workspace_bytes", "lsl_weighted_moments", "lsl_affine_weights", "lsl_project_wide")


@pytest.fixture(scope="module")
def tables(golden):
    from lam_slide_amd.peptide_loss import residue_tables
    return residue_tables(golden("f18_peptide_loss.npz").group("tables"))


# ---- the C ABI ----
def test_library_exports_and_header_declare_the_entry_points_and_limits():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib, koopman_tica as kt
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6 and ", ".join(SYMBOLS) in header
    src = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_wtica.hip.h")).read()
    defines = dict(re.findall(r"^#define (LSL_\w+)[ \t]+([^\n]*?)[ \t]*(?://[^\n]*)?$", src, re.M))

    def macro(name):
        expr = re.sub(r"LSL_\w+", lambda m: str(macro(m.group(0))), defines[name])
        assert re.fullmatch(r"[\d\s()*/+-]+", expr), (name, expr)
        return eval(expr)  # (digits, brackets and integer operators only)

    assert (macro("LSL_WMOM_MIN_F"), macro("LSL_WMOM_MAX_F"), macro("LSL_WPROJ_MAX_D")) == (kt.MIN_F, kt.MAX_F, kt.PROJ_MAX_D) == (129, 2048, 64)
    assert macro("LSL_WMOM_SEG") == kt.WMOM_SEG and macro("LSL_WMOM_CHAIN") == kt.WMOM_CHAIN
    assert kt.MIN_F == _lib.MOM_MAX_F + 1
    # the derivation of the chain: the scaling, a segment, a group of segments, the groups of n < 2^31 (+ 1: a split starts inside a group), the splits
    groups = -(-(2 ** 31 // macro("LSL_WMOM_SEG")) // macro("LSL_WMOM_SEG1"))
    assert kt.WMOM_CHAIN == 1 + macro("LSL_WMOM_SEG") + macro("LSL_WMOM_SEG1") + groups + 1 + macro("LSL_WMOM_MAX_SPLITS") <= 4200
    assert f"{kt.WMOM_CHAIN}" in header
    assert not re.search(r"atomic\w*\([^;]*(float|double)", src)  # integer atomics only
    # the limits live in the binding beside the others; the module's names are aliases of them
    assert (kt.MIN_F, kt.MAX_F, kt.PROJ_MAX_D, kt.WMOM_SEG, kt.WMOM_CHAIN) == (_lib.WMOM_MIN_F, _lib.WMOM_MAX_F, _lib.WPROJ_MAX_D, _lib.WMOM_SEG, _lib.WMOM_CHAIN)


def test_entry_points_validate_arguments_without_gpu():
    from lam_slide_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    mom = lambda x=one, n=1000, F=300, lag=50, w=None, out=one, ws=one, nbytes=1 << 40: lib.lsl_weighted_moments(x, n, F, lag, w, out, ws, nbytes, None)  # noqa: E731
    aff = lambda x=one, m=100, F=300, u=one, c=1.0, w=one: lib.lsl_affine_weights(x, m, F, u, c, w, None)  # noqa: E731
    proj = lambda x=one, n=100, F=300, mean=one, W=one, d=40, y=one, lim=one: lib.lsl_project_wide(x, n, F, mean, W, d, y, lim, None)  # noqa: E731
    assert mom(x=None) == -1 and mom(out=None) == -1 and mom(ws=None) == -1
    assert aff(x=None) == -1 and aff(u=None) == -1 and aff(w=None) == -1
    assert proj(x=None) == -1 and proj(mean=None) == -1 and proj(W=None) == -1 and proj(y=None) == -1
    assert mom(F=128) == -3 and b"F = 128" in lib.lsl_last_error() and b"lsl_lagged_moments" in lib.lsl_last_error()
    assert mom(F=2049) == -3 and b"F = 2049" in lib.lsl_last_error()
    assert mom(lag=0) == -3 and b"lag" in lib.lsl_last_error()
    assert mom(lag=1000) == -3 and b"lag = 1000" in lib.lsl_last_error()  # lag = n
    assert mom(n=1, lag=1) == -3 and b"n = 1" in lib.lsl_last_error()
    assert mom(lag=-2) == -3 and mom(n=0) == -3
    assert mom(nbytes=8) == -4 and b"workspace" in lib.lsl_last_error()
    assert proj(d=65) == -3 and b"d = 65" in lib.lsl_last_error()
    for kw in (dict(d=0), dict(F=128), dict(F=2049), dict(n=0), dict(n=-4)):
        assert proj(**kw) == -3 and lib.lsl_last_error(), kw
    for kw in (dict(F=0), dict(F=2049), dict(m=0)):
        assert aff(**kw) == -3 and lib.lsl_last_error(), kw
    # the workspace: splits * 3 (F + 1)^2 doubles, the splits a function of (n, lag, F) alone and at most 32; bounded independently of n
    need = lib.lsl_weighted_moments_workspace_bytes
    part = lambda F: 3 * (F + 1) ** 2 * 8  # noqa: E731
    assert need(1000, 128, 1) == 0 and need(1000, 2049, 1) == 0 and need(1000, 300, 1000) == 0 and need(1, 300, 1) == 0
    assert need(2, 129, 1) == part(129)  # one segment: one split
    assert need(2 ** 31 - 1, 129, 1) == 32 * part(129)  # 21 jobs: 32 splits
    assert need(100000, 1344, 1000) == 2 * part(1344) and need(2 ** 31 - 1, 2048, 1) == part(2048) <= 512 << 20
    assert max(need(2 ** 31 - 1, F, 1) for F in range(129, 2049, 13)) <= 512 << 20


# ---- the estimator ----
@pytest.fixture(scope="module")
def ar():
    x = orc.ar_series(4000, seed=3)
    return x, 25


def test_koopman_weights_match_the_brute_force_eigenvector(ar):
    from lam_slide_amd import koopman_tica as kt
    x, lag = ar
    u_b, c_b, R = orc.koopman_brute(x, lag)
    assert R.shape == (6, 5)  # the collinear column: one direction dropped by the epsilon cut
    kw = kt.koopman_weights(torch.from_numpy(x), lag)
    assert kt.last_path["koopman_weights"] == "torch"
    assert np.abs(kw.u - u_b).max() <= 1e-9 * np.abs(u_b).max() and abs(kw.const - c_b) <= 1e-9 * abs(c_b)
    # the module's restatement on the oracle's inputs gives the same vector
    u_s, c_s = kt.solve_koopman(*orc.koopman_inputs(x, lag))
    assert np.abs(u_s - u_b).max() <= 1e-9 * np.abs(u_b).max() and abs(c_s - c_b) <= 1e-9 * abs(c_b)
    with pytest.raises(ValueError):
        kt.solve_koopman(np.zeros(3), np.zeros(3), np.zeros((3, 3)), np.zeros((3, 3)))  # nothing above epsilon
    with pytest.raises(ValueError):
        kt.solve_koopman(np.zeros(2), np.zeros(2), np.eye(2), np.eye(2))  # the upper block has the eigenvalue 1: singular


def test_koopman_weights_are_stationary_and_average_to_one(ar):
    from lam_slide_amd import koopman_tica as kt
    x, lag = ar
    m = x.shape[0] - lag
    u_b, c_b, R = orc.koopman_brute(x, lag)
    kw = kt.koopman_weights(torch.from_numpy(x), lag)
    w = kw.weights(torch.from_numpy(x[:m])).numpy()
    assert kt.last_path["weights"] == "torch" and w.dtype == np.float64 and w.shape == (m,)
    x64 = x.astype(np.float64)
    w_b = x64[:m] @ u_b + c_b
    assert abs(w.mean() - 1.0) <= 1e-12
    chi0, chit = x64[:m] @ R, x64[lag:] @ R  # every kept whitened direction
    res = np.abs(((chit - chi0) * w[:, None]).sum(axis=0))
    res_b = np.abs(((chit - chi0) * w_b[:, None]).sum(axis=0))
    floor = 1e-12 * np.abs(w).sum() * np.maximum(np.abs(chi0).max(axis=0), np.abs(chit).max(axis=0))
    assert (res <= np.maximum(10 * res_b, floor)).all(), (res, res_b, floor)
    assert w.min() < 1.0 < w.max()


def test_unit_weights_give_the_covariances_of_tica(ar):
    from lam_slide_amd import koopman_tica as kt, tica
    x, lag = ar
    xt = torch.from_numpy(x)
    m = x.shape[0] - lag
    want = tica.tica_covariances(xt, lag)
    for weights in (None, torch.ones(m, dtype=torch.float64)):
        got = kt.weighted_covariances(xt, lag, weights)
        for g, w_ in zip(got, want):
            assert g.dtype == torch.float64 and (g - w_).abs().max() <= 1e-13 * w_.abs().max()
    wide = torch.from_numpy(orc.gaussian(500, 140, seed=1))  # past lagged_moments' width: the torch restatement of the wide path
    got = kt.weighted_covariances(wide, 7, None)
    assert kt.last_path["weighted_covariances"] == "torch"
    for g, w_ in zip(got, orc.reversible64(orc.moments64(wide.numpy(), 7))):
        assert np.abs(g.numpy() - w_).max() <= 1e-13 * np.abs(w_).max()
    sw, sx, sy, xx, yy, xy = kt.weighted_moments(wide, 7, torch.from_numpy(orc.signed_weights(493, 2)))
    for g, w_ in zip((sw, sx, sy, xx, yy, xy), orc.moments64(wide.numpy(), 7, orc.signed_weights(493, 2))):
        assert np.abs(g.numpy() - w_).max() <= 1e-12 * np.abs(w_).max()
    with pytest.raises(ValueError):
        kt.weighted_moments(wide, 500)
    with pytest.raises(ValueError):
        kt.weighted_moments(wide, 7, torch.ones(492, dtype=torch.float64))


# ---- planted structure ----
def test_run_tica_recovers_a_planted_slow_coordinate():
    from lam_slide_amd import koopman_tica as kt
    x, s = orc.planted(6000, 150, seed=5, dwell=200)
    lag = 50
    # the float64 oracle itself reaches the bar on this data
    lam, R, mean = orc.run_tica64(x, lag)
    r_orc = abs(np.corrcoef((x.astype(np.float64) - mean) @ R[:, 0], s)[0, 1])
    assert r_orc >= 0.95 and lam[0] - lam[1] > 0.05, (r_orc, lam[:3])
    model = kt.run_tica(torch.from_numpy(x), lagtime=lag, dim=40)
    assert isinstance(model, kt.WideTicaModel) and model.dim == 40 and model.lag == lag and kt.last_path["run_tica"] == "torch"
    y = model.transform(torch.from_numpy(x))
    assert y.shape == (6000, 40) and y.dtype == torch.float32 and kt.last_path["transform"] == "torch"
    r = abs(np.corrcoef(y[:, 0].numpy().astype(np.float64), s)[0, 1])
    assert r >= 0.95, r
    assert abs(model.eigenvalues[0] - lam[0]) <= 1e-8 and abs(model.eigenvalues[1] - lam[1]) <= 1e-8
    assert kt.run_tica(torch.from_numpy(x[:400, :20]), lagtime=10, dim=40).dim == 20  # dim = min(dim, rank)
    with pytest.raises(ValueError):
        kt.run_tica(torch.from_numpy(x[:100]), lagtime=100)


# ---- what the GPU tests rely on, checked with the oracle alone ----
def test_oracle_projection_values_rarely_sit_on_a_float32_rounding_boundary():
    """tests/test_hip_koopman_tica.py excepts an entry from the bitwise comparison when the sequential float64 value lies within
    (F + 2) 2^-53 sum |terms| of a float32 rounding boundary, and allows 1 entry in 10^4: the seeded cases stay inside that."""
    total = 0
    for F in orc.PROJ_F:
        for d in orc.PROJ_D:
            x, mean, W, u, c = orc.projection_case(F, d)
            acc, mag = orc.project_sequential(x, mean, W)
            near = ~orc.fp32_rounding_is_decided(acc, (F + 2) * orc.U * mag)
            entries = sum(rows * d for rows in orc.PROJ_ROWS)
            excepted = sum(int(near[:rows].sum()) for rows in orc.PROJ_ROWS)
            assert excepted * 10 ** 4 <= entries, (F, d, excepted, entries)
            total += excepted
    assert total <= 3


def test_oracle_eigenvalue_gaps_of_the_end_to_end_case():
    """The planted data of the GPU end-to-end test (two slow two-state coordinates in 300 columns): the float64 oracle separates the two
    leading eigenvalues from each other and from the third by more than 0.05, and its TIC-0 is the first planted coordinate."""
    x, s = orc.planted(6000, 300, seed=11, dwell=400, dwell2=120)
    lam, R, mean = orc.run_tica64(x, 50)
    assert lam[0] - lam[1] > 0.05 and lam[1] - lam[2] > 0.05, lam[:4]
    assert abs(np.corrcoef((x.astype(np.float64) - mean) @ R[:, 0], s)[0, 1]) >= 0.95


# ---- traj_analysis ----
def test_traj_analysis_from_positions_alone(tables):
    from lam_slide_amd import StructureTables, koopman_tica as kt, tica_features, traj_analysis
    n, R, seed = sorc.CASES[3]
    assert (n, R) == (300, 9)
    st = StructureTables(sorc.aatype(R), tables)
    ref = torch.from_numpy(sorc.chain(n, R, seed).reshape(n, R * 14, 3))
    model = torch.from_numpy(sorc.chain(n, R, seed + 100).reshape(n, R * 14, 3))
    keys7 = ["ramachandran_js", "pwd_js", "rg_js", "tic_js", "tic2d_js", "val_ca", "rmse_contact"]
    got = traj_analysis(model, ref, st, tica_lagtime=20)
    assert list(got) == keys7 and all(v.dtype == torch.float64 and v.shape == () for v in got.values())
    assert all(np.isfinite(float(v)) for v in got.values())
    fr, fm = tica_features(ref, st), tica_features(model, st)
    assert fr.shape[1] > 128
    tm = kt.run_tica(fr, 20, 40)
    want = traj_analysis(model, ref, st, tm.transform(fr), tm.transform(fm))
    assert list(want) == keys7
    for k in keys7:
        assert float(got[k]) == float(want[k]), k
    # without the keyword nothing changes: today's five keys, the same values
    plain = traj_analysis(model, ref, st)
    assert list(plain) == [k for k in keys7 if not k.startswith("tic")]
    for k in plain:
        assert float(plain[k]) == float(got[k]), k
    assert list(traj_analysis(model, ref, st, tica_lagtime=20, tica_dim=2)) == keys7
    for bad in (300, 301, 0):
        with pytest.raises(ValueError):
            traj_analysis(model, ref, st, tica_lagtime=bad)
