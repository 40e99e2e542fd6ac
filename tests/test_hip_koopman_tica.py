"""GPU tests of the Koopman-reweighted TICA on wide feature tables (``lsl_weighted_moments`` / ``lsl_affine_weights`` / ``lsl_project_wide``
behind ``lam_slide_amd.koopman_tica``) against the numpy / scipy oracle of tests/koopman_tica_oracle.py.

Bars.
  moments      every entry: |device - oracle| <= WMOM_CHAIN * 2^-53 * sum_t |w_t x_a x_b| over the entry's own window (sx / sy: sum_t |w_t x_a|,
               sw: sum_t |w_t|), WMOM_CHAIN = 4130 derived from the summation order (csrc/k_wtica.hip.h), not measured.  Twice: every entry
               against float64 BLAS sums, and whole rows of every matrix (the tile edges 0, 63, 64, F - 1 and seeded others) against sums in
               x87 extended precision, whose own error (m 2^-64 of the same sum) is below a thousandth of the bar.  xx and yy bit-symmetric,
               a repeated call gives the same bits, a NaN reaches only the entries of its own column.
  weights      |w - w64| <= (F + 2) * 2^-53 * (sum_f |x_f u_f| + |c|) against the sequential float64 sum.
  projection   y EQUALS float32(the sequential float64 sum) wherever that sum is farther than (F + 2) * 2^-53 * sum_f |(x_f - mean_f) W_fj|
               from a float32 rounding boundary; the entries nearer are counted, at most 1 in 10^4 (test_koopman_tica.py checks on the CPU
               that the oracle's values allow that).  The limits equal numpy's minimum / maximum of the device's own y; NaN rows are
               ignored.
  end to end   each stage is fed the device's own previous output: the eigenvalues of the model from device moments within 1e-10 of the
               model from oracle moments under the device's weights; histogram counts equal numpy's on the device's own projections and
               device-built edges; both distances within bins * 2^-50 in d^2 of scipy on those counts (the bars of test_hip_tica.py).
  no sync      ``traj_analysis(..., tica_lagtime=20)`` runs under ``torch.cuda.set_sync_debug_mode("error")``: the two host eigenproblems of
               ``run_tica`` (the Koopman step's and ``solve_tica``'s copies down, ``u``, the mean and ``W`` back up) are the documented
               exceptions, wrapped by ``koopman_tica._to_host`` / ``_to_device`` alone.
Measured values: profiles/koopman_tica_parity.txt."""
import numpy as np
import pytest
import torch
from scipy.spatial.distance import jensenshannon

import koopman_tica_oracle as orc
import structstat_oracle as sorc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MOMENT_SHAPES = ((2, 129, 1), (40, 130, 7), (1100, 200, 1050), (2049, 257, 1), (3000, 1344, 1000), (64, 2048, 3))  # (n, F, lag)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def worst(err, bar):
    """max err / bar over the entries (an entry whose bar is 0 must be exact)."""
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    assert np.all(err[bar == 0] == 0)
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0


# ---- moments ----
@pytest.fixture(scope="module")
def moment_inputs():
    """{case: (x float32 [n, F], the signed weights)}, each made once."""
    return {i: (orc.gaussian(n, F, seed=40 + i), orc.signed_weights(n - lag, seed=60 + i)) for i, (n, F, lag) in enumerate(MOMENT_SHAPES)}


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("case", range(len(MOMENT_SHAPES)))
def test_weighted_moments_against_the_float64_sums(dev, moment_inputs, case, weighted):
    from lam_slide_amd import koopman_tica as kt
    n, F, lag = MOMENT_SHAPES[case]
    x, w = moment_inputs[case]
    w = w if weighted else None
    xd = torch.from_numpy(x).to(dev)
    wd = None if w is None else torch.from_numpy(w).to(dev)
    got = kt.weighted_moments(xd, lag, wd)
    assert kt.last_path["weighted_moments"] == "fused"
    again = kt.weighted_moments(xd, lag, wd)
    assert all(same_bits(a, b) for a, b in zip(got, again))
    assert same_bits(got[3], got[3].T) and same_bits(got[4], got[4].T)
    assert [tuple(g.shape) for g in got] == [(), (F,), (F,), (F, F), (F, F), (F, F)] and all(g.dtype == torch.float64 for g in got)
    host = [g.cpu().numpy() for g in got]
    want, mag = orc.moments64(x, lag, w), orc.abs_moments64(x, lag, w)
    ratio = max(worst(np.abs(h - r), kt.WMOM_CHAIN * U * a) for h, r, a in zip(host, want, mag))
    # whole rows against extended precision: the tile edges and two seeded rows
    rows = sorted({0, 63, 64, F - 1, *np.random.default_rng(case).integers(0, F, 2).tolist()})
    exact = orc.moment_rows_exact(x, lag, w, rows)
    sub = [host[0], host[1][rows], host[2][rows], host[3][rows], host[4][rows], host[5][rows]]
    suba = [mag[0], mag[1][rows], mag[2][rows], mag[3][rows], mag[4][rows], mag[5][rows]]
    ratio_x = max(worst(np.abs((h.astype(np.longdouble) - e).astype(np.float64)), kt.WMOM_CHAIN * U * a) for h, e, a in zip(sub, exact, suba))
    print(f"PARITY wmoments.n{n}.F{F}.lag{lag}.{'signed' if weighted else 'unit'} worst error / bar: all entries against float64 {ratio:.3e}, "
          f"{len(rows)} rows against extended precision {ratio_x:.3e}")
    assert ratio <= 1.0 and ratio_x <= 1.0


def test_a_nan_reaches_only_the_entries_of_its_column(dev, moment_inputs):
    from lam_slide_amd import koopman_tica as kt
    n, F, lag = MOMENT_SHAPES[1]
    x, w = moment_inputs[1]
    t0, c = 9, 77  # lag <= t0 < n - lag: the row enters both windows
    bad = x.copy()
    bad[t0, c] = np.nan
    wd = torch.from_numpy(w).to(dev)
    clean = kt.weighted_moments(torch.from_numpy(x).to(dev), lag, wd)
    got = kt.weighted_moments(torch.from_numpy(bad).to(dev), lag, wd)
    keep = torch.ones(F, dtype=torch.bool, device=dev)
    keep[c] = False
    assert same_bits(got[0], clean[0])
    for g, r in zip(got[1:3], clean[1:3]):
        assert bool(torch.isnan(g[c])) and same_bits(g[keep], r[keep])
    for g, r in zip(got[3:], clean[3:]):
        assert bool(torch.isnan(g[c]).all()) and bool(torch.isnan(g[:, c]).all()) and same_bits(g[keep][:, keep], r[keep][:, keep])


def test_a_zero_column_past_128_agrees_with_lagged_moments(dev):
    from lam_slide_amd import _lib, koopman_tica as kt, tica
    n, F, lag = 1500, 129, 40
    x = orc.gaussian(n, F, seed=9)
    x[:, 128] = 0.0
    xd = torch.from_numpy(x).to(dev)
    sw, sx, sy, xx, yy, xy = kt.weighted_moments(xd, lag)
    assert kt.last_path["weighted_moments"] == "fused" and float(sw) == n - lag
    narrow = tica.lagged_moments(xd[:, :128].contiguous(), lag)
    assert tica.last_path["lagged_moments"] == "fused"
    mag = orc.abs_moments64(x[:, :128], lag)[1:]
    bars = kt.WMOM_CHAIN + _lib.MOM_CHAIN + _lib.mom_segments(n, lag) + 2  # the sum of the two bounds
    ratio = 0.0
    for g, r, a in zip((sx[:128], sy[:128], xx[:128, :128], yy[:128, :128], xy[:128, :128]), narrow, mag):
        ratio = max(ratio, worst((g - r).abs().cpu().numpy(), bars * U * a))
    print(f"PARITY wmoments.F129 leading 128 x 128 blocks against lsl_lagged_moments: worst difference / (sum of the two bars) {ratio:.3e}")
    assert ratio <= 1.0
    for g in (sx[128], sy[128], xx[128], yy[128], xy[128], xy[:, 128]):
        assert float(g.abs().max()) == 0.0


# ---- weights and projection ----
@pytest.mark.parametrize("d", orc.PROJ_D)
@pytest.mark.parametrize("F", orc.PROJ_F)
def test_affine_weights_and_wide_projection(dev, F, d):
    from lam_slide_amd import koopman_tica as kt
    x, mean, W, u, c = orc.projection_case(F, d)
    acc, mag = orc.project_sequential(x, mean, W)
    decided = orc.fp32_rounding_is_decided(acc, (F + 2) * U * mag)
    w64 = orc.project_sequential(x, np.zeros(F), u[:, None])
    model = kt.WideTicaModel(mean, W, np.ones(d), d, kinetic_map=False)
    kw = kt.KoopmanWeights(u, c)
    excepted, entries, ratio_w = 0, 0, 0.0
    for rows in orc.PROJ_ROWS:
        xd = torch.from_numpy(x[:rows]).to(dev)
        lim = torch.tensor([[float("inf")] * d, [float("-inf")] * d], dtype=torch.float32, device=dev)
        y = model.transform(xd, lim)
        assert kt.last_path["transform"] == "fused" and y.shape == (rows, d) and y.dtype == torch.float32
        yh = y.cpu().numpy()
        ok = decided[:rows]
        assert np.array_equal(yh[ok], acc[:rows].astype(np.float32)[ok])
        near = ~ok  # an undecided entry still lies within the slack of the oracle's value, rounded
        assert np.all(np.abs(yh[near].astype(np.float64) - acc[:rows][near]) <= 2.0 ** -23 * np.abs(acc[:rows][near]))
        excepted, entries = excepted + int(near.sum()), entries + ok.size
        assert np.array_equal(lim.cpu().numpy(), np.stack([yh.min(axis=0), yh.max(axis=0)]))
        assert same_bits(y.view(torch.int32).long(), model.transform(xd).view(torch.int32).long())
        wgt = kw.weights(xd)
        assert kt.last_path["weights"] == "fused" and wgt.dtype == torch.float64 and wgt.shape == (rows,)
        ratio_w = max(ratio_w, worst(np.abs(wgt.cpu().numpy() - (w64[0][:rows, 0] + c)), (F + 2) * U * (w64[1][:rows, 0] + abs(c))))
        if rows >= 65:  # NaN rows are written as NaN and leave the limits alone; the limits take part in the minimum / maximum themselves
            bad = x[:rows].copy()
            bad[3, F // 2] = np.nan
            lim2 = torch.tensor([[0.0] * d, [0.5] * d], dtype=torch.float32, device=dev)
            y2 = model.transform(torch.from_numpy(bad).to(dev), lim2).cpu().numpy()
            good = np.ones(rows, dtype=bool)
            good[3] = False
            assert np.isnan(y2[3]).all() and np.array_equal(y2[good], yh[good])
            assert np.array_equal(lim2.cpu().numpy(), np.stack([np.minimum(0.0, yh[good].min(axis=0)), np.maximum(0.5, yh[good].max(axis=0))]).astype(np.float32))
    print(f"PARITY wproject.F{F}.d{d} rows {orc.PROJ_ROWS}: entries excepted near a float32 rounding boundary {excepted} of {entries}; "
          f"affine weights worst error / bar {ratio_w:.3e}")
    assert excepted * 10 ** 4 <= entries and ratio_w <= 1.0


# ---- end to end, stage by stage ----
def test_run_tica_project_histogram_and_distances_end_to_end(dev):
    from lam_slide_amd import koopman_tica as kt, tica, tica_histograms, tica_jsd, torsion_stats
    lag, F = 50, 300
    ref, s = orc.planted(6000, F, seed=11, dwell=400, dwell2=120)
    traj = orc.planted(2000, F, seed=12, dwell=400, dwell2=120)[0]
    rd, td = torch.from_numpy(ref).to(dev), torch.from_numpy(traj).to(dev)
    m = ref.shape[0] - lag
    # stage 1: the Koopman weights from device moments against the oracle's vector
    kw = kt.koopman_weights(rd, lag)
    assert kt.last_path["koopman_weights"] == "fused"
    u_b, c_b, _ = orc.koopman_brute(ref, lag)
    e_u = float(np.abs(kw.u - u_b).max() / np.abs(u_b).max())
    w = kw.weights(rd[:m])
    wh = w.cpu().numpy()
    # stage 2: the model from device moments against the model from oracle moments under the device's own weights
    moments = kt.weighted_moments(rd, lag, w)
    model = kt.model_from_moments(moments, lag, 40)
    model_o = kt.model_from_moments(tuple(torch.from_numpy(np.asarray(v)) for v in orc.moments64(ref, lag, wh)), lag, 40)
    e_lam = float(np.abs(model.eigenvalues[:2] - model_o.eigenvalues[:2]).max())
    lam_o = model_o.eigenvalues
    print(f"PARITY e2e.koopman u against the brute-force eigenvector {e_u:.3e} (relative, no bar: the oracle's own moments differ); mean weight - 1 "
          f"{abs(wh.mean() - 1):.3e}; eigenvalues {lam_o[0]:.4f} {lam_o[1]:.4f} {lam_o[2]:.4f}, device-moment model against oracle-moment model "
          f"{e_lam:.3e} bar 1.0e-10")
    assert lam_o[1] - lam_o[2] > 0.05 and lam_o[0] - lam_o[1] > 0.05 and e_lam <= 1e-10 and model.dim == 40
    full = kt.run_tica(rd, lag, 40)
    assert kt.last_path["run_tica"] == "fused" and np.array_equal(full.eigenvalues, model.eigenvalues) and np.array_equal(full.W, model.W)
    # stage 3: projections, joint limits, edges and counts
    h = tica_histograms(model, rd, td)
    assert tica.last_path["tica_histograms"] == "fused" and kt.last_path["transform"] == "fused"
    r = abs(np.corrcoef(h.y_ref[:, 0].cpu().numpy().astype(np.float64), s)[0, 1])
    excepted = 0
    for x, y in ((ref, h.y_ref), (traj, h.y_traj)):
        acc, mag = orc.project_sequential(x, model.mean, model.W)
        ok = orc.fp32_rounding_is_decided(acc, (F + 2) * U * mag)
        assert np.array_equal(y.cpu().numpy()[ok], acc.astype(np.float32)[ok])
        excepted += int((~ok).sum())
    print(f"PARITY e2e.project entries excepted near a float32 rounding boundary {excepted} of {8000 * 40}; |corr(TIC-0, planted coordinate)| {r:.4f}")
    assert r >= 0.95
    yr, yt = h.y_ref.cpu().numpy().astype(np.float64), h.y_traj.cpu().numpy().astype(np.float64)
    lo, hi = np.minimum(yr.min(0), yt.min(0)), np.maximum(yr.max(0), yt.max(0))
    assert np.array_equal(h.lim.cpu().numpy().astype(np.float64), np.stack([lo, hi]))
    e1, ea, eb = h.edges.cpu().numpy(), h.edges2a.cpu().numpy(), h.edges2b.cpu().numpy()
    for e, want in ((e1, np.linspace(lo[0], hi[0], 101)), (ea, np.linspace(lo[0], hi[0], 51)), (eb, np.linspace(lo[1], hi[1], 51))):
        assert np.array_equal(e.view(np.int64), want.view(np.int64))
    counts = {}
    for name, y, c, c2 in (("ref", yr, h.ref_counts, h.ref_counts2), ("traj", yt, h.traj_counts, h.traj_counts2)):
        counts[name] = (np.histogram(y[:, 0], bins=e1)[0], np.histogram2d(y[:, 0], y[:, 1], bins=(ea, eb))[0])
        assert np.array_equal(c.cpu().numpy(), counts[name][0]) and np.array_equal(c2.cpu().numpy(), counts[name][1])
        assert int(c.sum()) == len(y) == int(c2.sum())
    # stage 4: the distances
    d = tica_jsd(model, rd, td)
    assert tica.last_path["tica_jsd"] == "fused" and torsion_stats.last_path["js_distance"] == "fused" and list(d) == ["TICA-0", "TICA-0,1"]
    e0 = abs(d["TICA-0"] ** 2 - jensenshannon(counts["ref"][0], counts["traj"][0]) ** 2)
    e01 = abs(d["TICA-0,1"] ** 2 - jensenshannon(counts["ref"][1].reshape(-1), counts["traj"][1].reshape(-1)) ** 2)
    print(f"PARITY e2e.jsd TICA-0 |d^2 - scipy| {e0:.3e} bar {100 * 2.0 ** -50:.1e}; TICA-0,1 {e01:.3e} bar {2500 * 2.0 ** -50:.1e}")
    assert e0 <= 100 * 2.0 ** -50 and e01 <= 2500 * 2.0 ** -50


# ---- no synchronisation ----
def test_traj_analysis_from_positions_without_synchronising(dev, golden):
    """The only synchronising steps of ``traj_analysis(..., tica_lagtime=)`` are the two host eigenproblems of ``run_tica``: the copy of
    (C00, C0t, mu0, mut) down and of ``u`` up (the Koopman step), the copy of (C0, Ct, mean) down and of the mean and ``W`` up
    (``solve_tica``) - ``koopman_tica._to_host`` / ``_to_device`` switch the sync debug mode to "default" around those copies alone."""
    from lam_slide_amd import StructureTables, koopman_tica as kt, structure_stats, tica_features, traj_analysis
    from lam_slide_amd.peptide_loss import residue_tables
    tables = residue_tables(golden("f18_peptide_loss.npz").group("tables"))
    n, R, seed = sorc.CASES[3]
    st = StructureTables(sorc.aatype(R), tables)
    st.on(dev)
    ref = torch.from_numpy(sorc.chain(n, R, seed).reshape(n, R * 14, 3)).to(dev)
    model = torch.from_numpy(sorc.chain(n, R, seed + 100).reshape(n, R * 14, 3)).to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = traj_analysis(model, ref, st, tica_lagtime=20)
        assert torch.cuda.get_sync_debug_mode() == 2  # (the helpers put the mode back)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert structure_stats.last_path["traj_analysis"] == "fused" and kt.last_path["run_tica"] == "fused" and kt.last_path["transform"] == "fused"
    assert list(got) == ["ramachandran_js", "pwd_js", "rg_js", "tic_js", "tic2d_js", "val_ca", "rmse_contact"]
    assert all(v.is_cuda and v.dtype == torch.float64 and v.shape == () for v in got.values())
    fr, fm = tica_features(ref, st), tica_features(model, st)
    assert kt.MIN_F <= fr.shape[1] <= kt.MAX_F
    tm = kt.run_tica(fr, 20, 40)
    want = traj_analysis(model, ref, st, tm.transform(fr), tm.transform(fm))
    vals = {k: float(v) for k, v in got.items()}
    print(f"PARITY traj_analysis.n{n}.R{R} F {fr.shape[1]} lag 20: tic_js {vals['tic_js']:.6f} tic2d_js {vals['tic2d_js']:.6f}")
    for k, v in want.items():
        assert vals[k] == float(v) and np.isfinite(vals[k]), k
