"""GPU tests of the TICA and state statistics on the device (``lsl_lagged_moments`` / ``lsl_project`` / ``lsl_assign_centers`` /
``lsl_transition_counts`` behind ``lam_slide_amd.tica``) against the numpy / scipy oracle of tests/tica_oracle.py.

Bars.
  moments      every entry: |device - oracle| <= (MOM_CHAIN + segments + 2) * 2^-53 * sum_t |x_a x_b| over the entry's own window (for sx /
               sy: sum_t |x_a|).  The products of float32 values are exact in float64, every addition rounds once, a segment is a chain
               of at most MOM_CHAIN additions and the segments add in order; the test computes the sum.  xx and yy bit-symmetric, a
               series alone has the bits it has in the batch, a repeated call gives the same bits.
  projection   |y - y64| <= 2^-24 |y64| + 2^-149 + (F + 2) * 2^-53 * sum_f |(x_f - mean_f) W_fj| (one subtraction and one fused
               addition per f in float64, one rounding to float32); the limits equal the elementwise minimum / maximum of what they
               held and of both outputs exactly; NaN rows leave them untouched.
  assignment   labels equal the float64 oracle's except rows whose two smallest oracle distances differ by at most (d + 2) * 2^-52 x
               the smaller one; at most 0.1 % of the rows may be excepted, and with the seeded inputs none is apart from the rows of the
               planted duplicate centre, where the lowest index must win.  Counts are integers.
  transitions  equal to ``np.add.at`` as integers; two calls give exactly twice the counts; lag >= n leaves the table unchanged.
  end to end   projections to the projection bar, histogram counts equal to ``np.histogram`` / ``np.histogram2d`` on the device's own
               float32 projections and device-built edges as integers, both JSD values within bins * 2^-50 in d^2 of scipy on those
               counts, eigenvalues of the model fitted from device moments within 1e-10 of the oracle's.
Measured values: profiles/tica_parity.txt."""
import numpy as np
import pytest
import torch
from scipy.spatial.distance import jensenshannon

import tica_oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


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
def moment_shapes():
    from lam_slide_amd import _lib
    seg = _lib.MOM_SEG
    return [(1, 2, 1, 1), (1, 65, 5, 1), (2, 1000, 12, 50), (1, 5000, 33, 1000), (1, 3 * seg + 17, 128, seg + 3), (3, 300, 7, 299)]


@pytest.mark.parametrize("case", range(6))
def test_lagged_moments_against_the_direct_sums(dev, case):
    from lam_slide_amd import _lib, lagged_moments, tica
    S, n, F, lag = moment_shapes()[case]
    x = np.stack([orc.series(n, F, seed=1000 * case + s) for s in range(S)])
    xd = torch.from_numpy(x).to(dev)
    got = lagged_moments(xd, lag)
    assert tica.last_path["lagged_moments"] == "fused" and all(g.dtype == torch.float64 for g in got)
    nseg = _lib.mom_segments(n, lag)
    assert nseg == -(-(n - lag) // _lib.MOM_SEG) and (case != 4 or (nseg == 3 and lag > _lib.MOM_SEG))
    ratio = 0.0
    for s in range(S):
        want, absum = orc.moments64(x[s], lag)
        for g, w, a, name in zip(got, want, absum, ("sx", "sy", "xx", "yy", "xy")):
            assert g[s].shape == w.shape, name
            ratio = max(ratio, worst(np.abs(g[s].cpu().numpy() - w), (_lib.MOM_CHAIN + nseg + 2) * U * a))
    print(f"PARITY moments.S{S}.n{n}.F{F}.lag{lag} segments {nseg} worst error / bar {ratio:.3e}")
    assert ratio <= 1.0
    assert same_bits(got[2], got[2].transpose(-1, -2)) and same_bits(got[3], got[3].transpose(-1, -2))  # xx, yy bit-symmetric
    alone = lagged_moments(xd[S - 1], lag)
    again = lagged_moments(xd, lag)
    for g, a, r in zip(got, alone, again):
        assert same_bits(a, g[S - 1]) and same_bits(r, g)


def test_lagged_moments_dispatch_and_covariances(dev):
    from lam_slide_amd import lagged_moments, tica, tica_covariances
    x = orc.series(4000, 5, seed=100)
    xd = torch.from_numpy(x).to(dev)
    mean, C0, Ct = tica_covariances(xd, 10)
    m64, c0, ct = orc.covariances64(x, 10)
    assert tica.last_path["tica_covariances"] == "fused" and C0.is_cuda and same_bits(C0, C0.T) and same_bits(Ct, Ct.T)
    assert float(np.abs(mean.cpu().numpy() - m64).max()) <= 1e-15 and float(np.abs(C0.cpu().numpy() - c0).max()) <= 1e-15
    assert float(np.abs(Ct.cpu().numpy() - ct).max()) <= 1e-15
    lagged_moments(xd.double(), 10)  # float64 input: the restatement
    assert tica.last_path["lagged_moments"] == "torch"
    lagged_moments(torch.zeros(4, 129, device=dev), 1)  # one feature more than the native form
    assert tica.last_path["lagged_moments"] == "torch"


# ---- projection ----
@pytest.mark.parametrize("n,F,d", [(1, 1, 1), (257, 5, 2), (1000, 33, 10), (4097, 128, 16)])
def test_projection_and_running_limits(dev, n, F, d):
    from lam_slide_amd import TicaModel, tica
    rng = np.random.default_rng(7 * n + F)
    mean, W = 0.1 * rng.standard_normal(F), rng.standard_normal((F, d))
    model = TicaModel.from_arrays(mean, W, np.ones(d), kinetic_map=False)
    xa, xb = orc.series(n, F, seed=n), orc.series(n, F, seed=n + 1)
    if n > 10:
        xb[3, F // 2] = np.nan  # a NaN row in the second call: ignored by the limits
    lim_in = np.stack([rng.standard_normal(d), rng.standard_normal(d)]).astype(np.float32)
    lim_in[0, 0], lim_in[1, d - 1] = -1e30, 1e30  # two entries that must survive
    lim = torch.from_numpy(lim_in.copy()).to(dev)
    ya = model.transform(torch.from_numpy(xa).to(dev), lim)
    yb = model.transform(torch.from_numpy(xb).to(dev), lim)
    assert tica.last_path["transform"] == "fused" and ya.dtype == torch.float32 and ya.shape == (n, d)
    ratio, both = 0.0, []
    for x, y in ((xa, ya), (xb, yb)):
        y64, absum = orc.project64(x, model.mean, model.W)
        yh = y.cpu().numpy()
        ok = ~np.isnan(y64)
        assert np.array_equal(np.isnan(yh), ~ok)
        bar = 2.0 ** -24 * np.abs(y64) + 2.0 ** -149 + (F + 2) * U * absum
        ratio = max(ratio, worst(np.abs(yh.astype(np.float64) - y64)[ok], bar[ok]))
        both.append(yh)
    print(f"PARITY project.n{n}.F{F}.d{d} worst error / bar {ratio:.3e}")
    assert ratio <= 1.0
    cat = np.concatenate(both)
    want = np.stack([np.minimum(lim_in[0], np.nanmin(cat, axis=0)), np.maximum(lim_in[1], np.nanmax(cat, axis=0))])
    got = lim.cpu().numpy()
    assert np.array_equal(got, want) and got[0, 0] == np.float32(-1e30) and got[1, d - 1] == np.float32(1e30)
    nan_rows = torch.full((3, F), float("nan"), device=dev)
    model.transform(nan_rows, lim)  # only NaN rows: the limits stay
    assert np.array_equal(lim.cpu().numpy(), want)
    assert torch.equal(model.transform(torch.from_numpy(xa).to(dev)), ya)  # without limits: the same values


# ---- nearest centre ----
@pytest.mark.parametrize("n,d,k", [(1, 1, 1), (300, 2, 100), (1025, 10, 100), (513, 64, 128)])
def test_assignment_against_the_float64_argmin(dev, n, d, k):
    from lam_slide_amd import assign_centers, tica
    rng = np.random.default_rng(n + d + k)
    y = rng.standard_normal((n, d)).astype(np.float32)
    centers = rng.standard_normal((k, d)).astype(np.float32)
    dup = None
    if k > 1:
        dup = (k // 3, k - 2)
        centers[dup[0]] = 20.0 + centers[dup[0]]  # away from the cloud: only the planted rows are nearest to it
        centers[dup[1]] = centers[dup[0]]        # an exact duplicate: the lowest index wins
        y[5] = centers[dup[0]] + np.float32(0.01)
        y[n // 2] = centers[dup[0]]
        y[7, d - 1] = np.nan
    want, smallest, gap = orc.assign64(y, centers)
    labels, counts = assign_centers(torch.from_numpy(y).to(dev), torch.from_numpy(centers).to(dev))
    assert tica.last_path["assign_centers"] == "fused" and labels.dtype == torch.int32 and counts.dtype == torch.int64 and counts.shape == (k,)
    got = labels.cpu().numpy()
    tied = (gap == 0) & (want >= 0)  # the rows of the planted duplicate
    close = (gap <= (d + 2) * 2.0 ** -52 * smallest) & (want >= 0) & ~tied
    print(f"PARITY assign.n{n}.d{d}.k{k} rows excepted {int(close.sum())} of {n} (the duplicate's rows: {int(tied.sum())})")
    assert int(close.sum()) == 0 and close.sum() <= 0.001 * n
    assert np.array_equal(got[~close], want[~close])
    if dup:
        assert int(tied.sum()) == 2 and np.all(got[tied] == dup[0]) and got[7] == -1 and not (got == dup[1]).any()
    assert np.array_equal(counts.cpu().numpy(), np.bincount(got[got >= 0], minlength=k)) and int(counts.sum()) == n - int((got < 0).sum())
    # through a state map with one value outside the states, counted per state
    ns = min(10, k)
    smap = rng.integers(0, ns, size=k).astype(np.int32)
    smap[int(got[0]) if got[0] >= 0 else 0] = ns + 3
    lab2, cnt2 = assign_centers(torch.from_numpy(y).to(dev), centers, state_map=smap, nstates=ns)
    want2 = np.where(got >= 0, smap[np.maximum(got, 0)], -1)
    want2[want2 >= ns] = -1
    assert tica.last_path["assign_centers"] == "fused" and np.array_equal(lab2.cpu().numpy(), want2) and want2[0] == -1
    assert np.array_equal(cnt2.cpu().numpy(), np.bincount(want2[want2 >= 0], minlength=ns))


def test_assignment_outside_the_native_form_takes_the_restatement(dev):
    from lam_slide_amd import assign_centers, tica
    y = torch.randn(50, 65, device=dev)
    assign_centers(y, torch.randn(4, 65, device=dev))  # d = 65
    assert tica.last_path["assign_centers"] == "torch"
    labels, _ = assign_centers(y[:, :9].contiguous(), torch.randn(1024, 9, device=dev))  # k * d = 9216 > 8192
    assert tica.last_path["assign_centers"] == "torch" and labels.dtype == torch.int32 and labels.is_cuda


# ---- transition counts ----
@pytest.mark.parametrize("S,n,lag,ns", [(1, 2, 1, 2), (1, 1000, 1, 10), (1, 1000, 999, 10), (2, 5000, 1000, 100), (1, 3000, 7, 128)])
def test_transition_counts_equal_add_at(dev, S, n, lag, ns):
    from lam_slide_amd import _lib, tica, transition_counts
    d = np.stack([orc.labels(n, ns, seed=10 * n + s, holes=0.02 if n > 2 else 0.0) for s in range(S)])
    assert n <= 2 or (d == -1).any()
    dd = torch.from_numpy(d).to(dev)
    got = transition_counts(dd, lag, ns)
    want = np.stack([orc.transitions_np(d[s], lag, ns) for s in range(S)])
    assert tica.last_path["transition_counts"] == "fused" and got.dtype == torch.int64 and got.shape == (S, ns, ns)
    assert np.array_equal(got.cpu().numpy(), want) and int(want.sum()) > 0
    assert torch.equal(transition_counts(dd[0].long(), lag, ns), got[0])  # one series, int64 labels
    # the table is added to: a second call gives exactly twice the counts; lag >= n adds nothing
    lib, st = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    table = got.clone()
    assert lib.lsl_transition_counts(dd.data_ptr(), S, n, lag, ns, table.data_ptr(), st) == 0
    assert np.array_equal(table.cpu().numpy(), 2 * want)
    for big in (n, n + 5):
        assert lib.lsl_transition_counts(dd.data_ptr(), S, n, big, ns, table.data_ptr(), st) == 0
    assert np.array_equal(table.cpu().numpy(), 2 * want) and int(transition_counts(dd, n, ns).sum()) == 0


# ---- end to end ----
def test_fit_project_histogram_and_distances_end_to_end(dev):
    from lam_slide_amd import TicaModel, solve_tica, summary_metrics, tica, tica_histograms, tica_jsd, torsion_stats
    n, F, lag = orc.CASES[1]
    ref, traj = orc.series(n, F, seed=101), orc.series(2000, F, seed=7)
    rd, td = torch.from_numpy(ref).to(dev), torch.from_numpy(traj).to(dev)
    model = TicaModel.fit(rd, lag=lag)
    assert tica.last_path["fit"] == "fused" and model.dim == 3
    lam, R = solve_tica(*orc.covariances64(ref, lag)[1:])
    e_lam = float(np.abs(model.eigenvalues - lam).max())
    print(f"PARITY e2e.eigenvalues device-moment model against oracle-moment model {e_lam:.3e} bar 1.0e-10")
    assert e_lam <= 1e-10
    h = tica_histograms(model, rd, td)
    assert tica.last_path["tica_histograms"] == "fused" and tica.last_path["transform"] == "fused"
    ratio = 0.0
    for x, y in ((ref, h.y_ref), (traj, h.y_traj)):
        y64, absum = orc.project64(x, model.mean, model.W)
        ratio = max(ratio, worst(np.abs(y.cpu().numpy().astype(np.float64) - y64), 2.0 ** -24 * np.abs(y64) + 2.0 ** -149 + (F + 2) * U * absum))
    print(f"PARITY e2e.project worst error / bar {ratio:.3e}")
    assert ratio <= 1.0
    yr, yt = h.y_ref.cpu().numpy().astype(np.float64), h.y_traj.cpu().numpy().astype(np.float64)
    lo, hi = np.minimum(yr.min(0), yt.min(0)), np.maximum(yr.max(0), yt.max(0))
    assert np.array_equal(h.lim.cpu().numpy().astype(np.float64), np.stack([lo, hi]))
    e1, ea, eb = h.edges.cpu().numpy(), h.edges2a.cpu().numpy(), h.edges2b.cpu().numpy()
    for e, want in ((e1, np.linspace(lo[0], hi[0], 101)), (ea, np.linspace(lo[0], hi[0], 51)), (eb, np.linspace(lo[1], hi[1], 51))):
        assert np.array_equal(e.view(np.int64), want.view(np.int64))  # np.linspace's bits, built on the device
    counts = {}
    for name, y, c, c2 in (("ref", yr, h.ref_counts, h.ref_counts2), ("traj", yt, h.traj_counts, h.traj_counts2)):
        counts[name] = (np.histogram(y[:, 0], bins=e1)[0], np.histogram2d(y[:, 0], y[:, 1], bins=(ea, eb))[0])
        assert np.array_equal(c.cpu().numpy(), counts[name][0]) and np.array_equal(c2.cpu().numpy(), counts[name][1])
        assert int(c.sum()) == len(y) == int(c2.sum())
    d = tica_jsd(model, rd, td)
    assert tica.last_path["tica_jsd"] == "fused" and torsion_stats.last_path["js_distance"] == "fused" and list(d) == ["TICA-0", "TICA-0,1"]
    e0 = abs(d["TICA-0"] ** 2 - jensenshannon(counts["ref"][0], counts["traj"][0]) ** 2)
    e01 = abs(d["TICA-0,1"] ** 2 - jensenshannon(counts["ref"][1].reshape(-1), counts["traj"][1].reshape(-1)) ** 2)
    print(f"PARITY e2e.jsd TICA-0 |d^2 - scipy| {e0:.3e} bar {100 * 2.0 ** -50:.1e}; TICA-0,1 {e01:.3e} bar {2500 * 2.0 ** -50:.1e}")
    assert e0 <= 100 * 2.0 ** -50 and e01 <= 2500 * 2.0 ** -50
    out = summary_metrics([{"PHI 1": 0.25, **d}])
    assert out["TICA-0"] == d["TICA-0"] and out["TICA-0,1"] == d["TICA-0,1"] and out["BB"] == 0.25
    # a record, no bar: the same pipeline in float64 throughout (values that cross a bin edge make the difference input-dependent)
    lam64, R64 = solve_tica(*orc.covariances64(ref, lag)[1:])
    W64 = R64[:, :3] * lam64[:3]
    p_ref, p_traj = orc.project64(ref, orc.covariances64(ref, lag)[0], W64)[0], orc.project64(traj, orc.covariances64(ref, lag)[0], W64)[0]
    lo64, hi64 = np.minimum(p_ref.min(0), p_traj.min(0)), np.maximum(p_ref.max(0), p_traj.max(0))
    j0 = jensenshannon(np.histogram(p_ref[:, 0], range=(lo64[0], hi64[0]), bins=100)[0], np.histogram(p_traj[:, 0], range=(lo64[0], hi64[0]), bins=100)[0])
    rng2 = ((lo64[0], hi64[0]), (lo64[1], hi64[1]))
    j01 = jensenshannon(np.histogram2d(p_ref[:, 0], p_ref[:, 1], range=rng2, bins=50)[0].reshape(-1),
                        np.histogram2d(p_traj[:, 0], p_traj[:, 1], range=rng2, bins=50)[0].reshape(-1))
    print(f"PARITY e2e.float64-pipeline TICA-0 device {d['TICA-0']:.6f} float64 {j0:.6f} difference {abs(d['TICA-0'] - j0):.3e}; "
          f"TICA-0,1 device {d['TICA-0,1']:.6f} float64 {j01:.6f} difference {abs(d['TICA-0,1'] - j01):.3e} (no bar)")


def test_states_and_autocovariance_after_the_projection(dev):
    """The Markov half behind the projection: centres from the caller, labels, occupancies, the count matrix, the MSMS distance."""
    from lam_slide_amd import TicaModel, assign_centers, metastable_jsd, tica, tica_autocovariance, torsion_stats, transition_counts
    n, F, lag = orc.CASES[0]
    ref, traj = orc.series(n, F, seed=100), orc.series(1000, F, seed=8)
    rd, td = torch.from_numpy(ref).to(dev), torch.from_numpy(traj).to(dev)
    model = TicaModel.fit(rd, lag=lag)
    yr, yt = model.transform(rd), model.transform(td)
    centers = yr[:: n // 100][:100].contiguous()  # 100 frames of the reference as centres (k-means fitting is the caller's)
    smap = np.arange(100, dtype=np.int32) % 10
    lr, cr = assign_centers(yr, centers, state_map=smap, nstates=10)
    lt, ct = assign_centers(yt, centers, state_map=smap, nstates=10)
    want, _, gap = orc.assign64(yr.cpu().numpy(), centers.cpu().numpy())
    assert np.array_equal(lr.cpu().numpy()[gap > 0], smap[want[gap > 0]]) and int(cr.sum()) == n and int(ct.sum()) == 1000
    msms = metastable_jsd(cr, ct)
    assert tica.last_path["metastable_jsd"] == "fused" and abs(float(msms) ** 2 - jensenshannon(cr.cpu().numpy(), ct.cpu().numpy()) ** 2) <= 10 * 2.0 ** -50
    C = transition_counts(lt, 5, 10)
    assert np.array_equal(C.cpu().numpy(), orc.transitions_np(lt.cpu().numpy(), 5, 10)) and int(C.sum()) == 995
    ac = tica_autocovariance(yt, 50)
    y0 = yt[:, 0].double().cpu().numpy()
    direct = np.array([np.dot(y0[:1000 - k], y0[k:]) / (1000 - k) for k in range(51)])
    assert torsion_stats.last_path["lagged_products"] == "fused" and ac.shape == (51,)
    assert float(np.abs(ac.double().cpu().numpy() - direct).max()) <= 456 * 2.0 ** -24 * float(np.abs(y0).max()) ** 2  # the lagged-products bar, scaled
