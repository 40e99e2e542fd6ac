"""GPU tests of the torsion statistics on the device (``lsl_dihedral_angles`` / ``lsl_histogram`` / ``lsl_lag_products`` /
``lsl_js_distance`` behind ``lam_slide_amd.torsion_stats``) against the numpy / scipy oracle of tests/torsstat_oracle.py.

Bars.
  dihedrals   wrapped |device - float64 oracle|, maximum over all angles <= 4 x the same figure of the oracle formula evaluated in float32
              numpy on the same inputs (measured per case: the factor covers another equally valid float32 operation order and atan2f).
  histograms  equal to ``np.histogram`` / ``np.histogram2d`` on the same float32 values as integers; from positions: equal once every
              angle whose float64 value lies within the dihedral bar of an edge is left out, and at most 1 % may be left out.
  JSD         |d^2 - d^2_scipy| <= bins * 2^-50 (the fp64 terms are at most 2 ln 2 in absolute sum; summation and log error
              <= (bins + 8) 2^-53 2 ln 2; the bar is about five times that).
  lagged      |device - direct float64 sum| <= (m + 8) 2^-24 per lag for |x| <= 1, m = 448 the kernel's longest float32 addition chain;
              ``decorrelation`` to the same bar over (1 - baseline).
Measured values: profiles/torsion_stats_parity.txt."""
import math

import numpy as np
import pytest
import torch
from scipy.spatial.distance import jensenshannon

import torsstat_oracle as orc

pytestmark = pytest.mark.gpu

PI = math.pi
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables(golden):
    from lam_slide_amd.peptide_loss import residue_tables
    return residue_tables(golden("f18_peptide_loss.npz").group("tables"))


@pytest.fixture(scope="module")
def peptides(golden, tables):
    """{R: (base positions [R * 14, 3], quads [Q <= 40, 4], labels)} of F18's R = 4 and R = 23 cases."""
    from lam_slide_amd import eval_torsion_quads
    f = golden("f18_peptide_loss.npz")
    out = {}
    for R, name in ((4, "f5_r4"), (23, "f9_r23")):
        c = f.group(name)
        quads, labels = eval_torsion_quads(c["aatype"][0], tables)
        out[R] = (c["target"][0].numpy().reshape(-1, 3), quads[:40], labels[:40])
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def dihedral_case(peptides, R, S, n):
    """(frames float32 [S, n, A, 3], quads, float64 oracle angles, the bar = 4 x the float32 oracle's error)."""
    base, quads, _ = peptides[R]
    frames = np.stack([orc.ar1_frames(base, n, seed=100 * R + s) for s in range(S)])
    want = orc.dihedral_np(frames, quads, np.float64)
    ref32 = float(orc.wrapped_diff(orc.dihedral_np(frames, quads, np.float32), want).max())
    return frames, quads, want, ref32


# ---- dihedrals ----
@pytest.mark.parametrize("R", [4, 23])
@pytest.mark.parametrize("S,n", [(1, 1), (1, 63), (2, 65), (1, 257)])
def test_dihedral_angles_against_the_float64_formula(dev, peptides, R, S, n):
    from lam_slide_amd import dihedral_angles, torsion_stats
    frames, quads, want, ref32 = dihedral_case(peptides, R, S, n)
    pos = torch.from_numpy(frames).to(dev)
    got = dihedral_angles(pos, quads)
    assert torsion_stats.last_path["dihedral_angles"] == "fused" and got.dtype == torch.float32 and got.shape == (S, n, len(quads))
    err = float(orc.wrapped_diff(got.cpu().numpy(), want).max())
    print(f"PARITY dihedral.R{R}.S{S}.n{n} device {err:.3e} float32-oracle {ref32:.3e} bar {4 * ref32:.3e}")
    assert ref32 > 0 and err <= 4 * ref32
    assert float(got.abs().max()) <= np.float32(PI)
    # a frame alone and inside the batch: the same bits; Q = 1; a table that repeats atoms (and a quadruple) across quadruples
    s, t = S - 1, n // 2
    assert same_bits(dihedral_angles(pos[s, t], quads), got[s, t])
    assert same_bits(dihedral_angles(pos, quads[3:4]), got[..., 3:4])
    rep = np.stack([quads[0], quads[1], quads[0], quads[1][::-1], [quads[0][0], quads[0][1], quads[1][2], quads[1][3]]]).astype(np.int32)
    got_rep = dihedral_angles(pos, rep)
    want_rep = orc.dihedral_np(frames, rep, np.float64)
    assert same_bits(got_rep[..., 2], got[..., 0]) and same_bits(got_rep[..., 1], got[..., 1])
    ref_rep = float(orc.wrapped_diff(orc.dihedral_np(frames, rep, np.float32), want_rep).max())
    assert float(orc.wrapped_diff(got_rep.cpu().numpy(), want_rep).max()) <= 4 * ref_rep


def test_dihedral_of_the_largest_native_frame_and_refusals(dev):
    from lam_slide_amd import _lib, dihedral_angles, torsion_stats
    rng = np.random.default_rng(2)
    A = _lib.TORS_MAX_A
    frames = rng.standard_normal((3, A, 3)).astype(np.float32)
    quads = np.stack([[0, 1, 2, 3], [A - 4, A - 3, A - 2, A - 1], [A - 1, 0, A // 2, 7]]).astype(np.int32)
    want = orc.dihedral_np(frames, quads, np.float64)
    ref32 = float(orc.wrapped_diff(orc.dihedral_np(frames, quads, np.float32), want).max())
    got = dihedral_angles(torch.from_numpy(frames).to(dev), quads)
    assert torsion_stats.last_path["dihedral_angles"] == "fused"
    assert float(orc.wrapped_diff(got.cpu().numpy(), want).max()) <= 4 * ref32
    big = torch.zeros(1, A + 1, 3, device=dev)  # one atom more than a frame in LDS: the restatement
    dihedral_angles(big, quads)
    assert torsion_stats.last_path["dihedral_angles"] == "torch"
    with pytest.raises(ValueError, match="outside the frame"):
        dihedral_angles(torch.from_numpy(frames).to(dev), [[0, 1, 2, A]])


# ---- histograms ----
@pytest.mark.parametrize("Q", [1, 7, 33])
@pytest.mark.parametrize("n", [1, 1000, 4097])
def test_histograms_equal_numpy(dev, Q, n):
    from lam_slide_amd import angle_histograms, torsion_stats
    x = orc.planted_angles(n, Q, seed=10 * Q + n)
    pairs = [(1, 2), (3, 4)] if Q >= 5 else None
    counts, counts2 = angle_histograms(torch.from_numpy(x).to(dev), pairs=pairs)
    assert torsion_stats.last_path["angle_histograms"] == "fused" and counts.dtype == torch.int64 and counts.shape == (Q, 100)
    assert np.array_equal(counts.cpu().numpy(), orc.hist_np(x, 100, -PI, PI))
    inside = (x.astype(np.float64) >= -PI) & (x.astype(np.float64) <= PI)
    assert int(counts.sum()) == int(inside.sum())
    if n >= 1000:
        assert not inside.all() and np.isnan(x).any() and (x == np.float32(PI)).any()  # (the planted values are there)
    if pairs:
        assert counts2.dtype == torch.int64 and counts2.shape == (2, 50, 50)
        assert np.array_equal(counts2.cpu().numpy(), orc.hist2_np(x, pairs, 50, -PI, PI))
        assert [int(c.sum()) for c in counts2] == [int((inside[:, a] & inside[:, b]).sum()) for a, b in pairs]
    else:
        assert counts2 is None


def test_histograms_batched_other_ranges_and_column_tiles(dev):
    """S > 1, a caller-given range (the TICA form), bins that leave one column per tile (bins = 2048: qt = 4 of Q = 7), bins2 at its limit."""
    from lam_slide_amd import angle_histograms, torsion_stats
    for bins, bins2, lo, hi in ((14, 7, -1.0, 2.5), (13, 7, -1.0, 2.5), (2048, 90, -PI, PI), (1, 1, -4.0, 4.0)):
        x = np.stack([orc.planted_angles(1500, 7, seed=s, bins=bins, lo=lo, hi=hi, bins2=bins2) for s in range(3)])
        xd = torch.from_numpy(x).to(dev)
        if hi != PI:  # float32 holds these ends (and, at 14 / 7 bins, every edge): values sit exactly on edges[0] and edges[bins]
            assert (x.astype(np.float64) == hi).sum() >= 21 and (x.astype(np.float64) == lo).sum() >= 21
        c, c2 = angle_histograms(xd, bins=bins, pairs=[(1, 2), (6, 0)], bins2=bins2, range=(lo, hi))
        assert torsion_stats.last_path["angle_histograms"] == "fused" and c.shape == (3, 7, bins) and c2.shape == (3, 2, bins2, bins2)
        for s in range(3):
            assert np.array_equal(c[s].cpu().numpy(), orc.hist_np(x[s], bins, lo, hi)), (bins, s)
            assert np.array_equal(c2[s].cpu().numpy(), orc.hist2_np(x[s], [(1, 2), (6, 0)], bins2, lo, hi)), (bins2, s)
            if hi != PI:  # the values on the right end are in the last bin
                assert all(int(c[s, q, -1]) >= int((x[s, :, q] == np.float32(hi)).sum()) > 0 for q in range(7))
                assert int(c2[s, 0, -1, -1]) >= 1 and int(c2[s, 0, 0, 0]) >= 1  # (the rows with every coordinate on an end)
    angle_histograms(xd, bins=2049)  # beyond the edge table in LDS: the restatement
    assert torsion_stats.last_path["angle_histograms"] == "torch"


def test_values_exactly_on_edges(dev):
    """Every edge of a table that float32 holds exactly (-1 .. 2.5 in steps of 0.25 / 0.5), once each: v == edges[i] belongs to bin i, and
    v == edges[bins] to the last bin, which is closed on the right - so each bin holds one value and the last one two; in the joint table
    the same for each coordinate.  Against numpy and against the counts written out."""
    from lam_slide_amd import angle_histograms, torsion_stats
    e1, e2 = np.linspace(-1.0, 2.5, 15), np.linspace(-1.0, 2.5, 8)
    assert np.array_equal(e1.astype(np.float32).astype(np.float64), e1)
    ga, gb = np.meshgrid(e2, e2, indexing="ij")
    x = np.full((64, 3), np.nan, dtype=np.float32)
    x[:15, 0], x[:64, 1], x[:64, 2] = e1, ga.reshape(-1), gb.reshape(-1)
    c, c2 = angle_histograms(torch.from_numpy(x).to(dev), bins=14, pairs=[(1, 2), (2, 1)], bins2=7, range=(-1.0, 2.5))
    assert torsion_stats.last_path["angle_histograms"] == "fused"
    ones = np.array([1] * 13 + [2])
    assert c[0].tolist() == ones.tolist()
    assert c[1].tolist() == [8, 0] * 6 + [8, 8]  # the 8 edges of the 7-bin table are every other edge of the 14-bin one, 8 times each
    joint = np.outer([1] * 6 + [2], [1] * 6 + [2])
    assert np.array_equal(c2[0].cpu().numpy(), joint) and np.array_equal(c2[1].cpu().numpy(), joint) and int(c2[0][-1, -1]) == 4
    assert np.array_equal(c.cpu().numpy(), orc.hist_np(x, 14, -1.0, 2.5)) and np.array_equal(c2.cpu().numpy(), orc.hist2_np(x, [(1, 2), (2, 1)], 7, -1.0, 2.5))
    # the float32 neighbours of the two ends: just inside is counted, just outside is dropped
    f32 = np.float32
    y = np.array([[np.nextafter(f32(2.5), f32(9)), np.nextafter(f32(2.5), f32(0)), np.nextafter(f32(-1), f32(-9)), np.nextafter(f32(-1), f32(0))]], dtype=np.float32).T
    cy, _ = angle_histograms(torch.from_numpy(y).to(dev), bins=14, range=(-1.0, 2.5))
    assert cy[0].tolist() == [1] + [0] * 12 + [1]


def test_accumulator_in_three_chunks_equals_one_call(dev, peptides):
    from lam_slide_amd import TorsionStats, angle_histograms, dihedral_angles
    base, quads, labels = peptides[4]
    frames = torch.from_numpy(orc.ar1_frames(base, 1000, seed=21)).to(dev)
    whole, parts = TorsionStats(quads, labels), TorsionStats(quads, labels)
    ang = whole.update(frames.reshape(-1, 4, 14, 3))
    for lo, hi in ((0, 1), (1, 400), (400, 1000)):
        parts.update(frames[lo:hi])
    assert whole.path == parts.path == "fused" and parts.n_frames == 1000 and whole.counts.is_cuda
    assert torch.equal(whole.counts, parts.counts) and torch.equal(whole.counts2, parts.counts2)
    c, c2 = angle_histograms(dihedral_angles(frames, quads), pairs=[(1, 2), (3, 4)])
    assert same_bits(ang, dihedral_angles(frames, quads)) and torch.equal(whole.counts, c) and torch.equal(whole.counts2, c2)
    assert np.array_equal(c.cpu().numpy(), orc.hist_np(ang.cpu().numpy(), 100, -PI, PI)) and int(c.sum()) == 1000 * len(quads)
    # the distances to a second trajectory: the reference's out["JSD"] dict, against scipy on the same counts
    ref = TorsionStats(quads, labels)
    ref.update(torch.from_numpy(orc.ar1_frames(base, 800, seed=22, sigma=0.1)).to(dev))
    d = whole.jsd(ref)
    pair_keys = [f"{labels[1]}|{labels[2]}", f"{labels[3]}|{labels[4]}"]
    assert list(d) == labels + pair_keys
    rc, wc, rc2, wc2 = (t.cpu().numpy() for t in (ref.counts, whole.counts, ref.counts2, whole.counts2))
    for q, s in enumerate(labels):
        assert abs(d[s] ** 2 - jensenshannon(rc[q], wc[q]) ** 2) <= 100 * 2.0 ** -50, s
    for p, s in enumerate(pair_keys):
        assert abs(d[s] ** 2 - jensenshannon(rc2[p].reshape(-1), wc2[p].reshape(-1)) ** 2) <= 2500 * 2.0 ** -50, s
    assert whole.jsd((rc, rc2)) == d and all(v == 0.0 for v in whole.jsd(parts).values())


@pytest.mark.parametrize("R,n", [(4, 4097), (23, 257)])
def test_positions_to_counts_end_to_end(dev, peptides, R, n):
    """Device angles may land on the other side of an edge from the float64 angles: every angle whose float64 value is within delta (the
    dihedral bar of these inputs) of an edge is left out on both sides, the counts of the others must be equal - and the left-out
    share stays below 1 % (expected 100 * 2 delta / 2 pi), so that the exclusion cannot hide a failure."""
    from lam_slide_amd import angle_histograms, dihedral_angles
    frames, quads, want, ref32 = dihedral_case(peptides, R, 1, n)
    delta = 4 * ref32
    edges = np.linspace(-PI, PI, 101)
    near = np.abs(want[0][..., None] - edges).min(axis=-1) <= delta  # [n, Q]
    share = float(near.mean())
    print(f"PARITY end_to_end.R{R}.n{n} delta {delta:.3e} left-out share {share:.3e} cap 1.0e-02")
    assert share <= 0.01
    ang = dihedral_angles(torch.from_numpy(frames[0]).to(dev), quads)
    ang = torch.where(torch.from_numpy(near).to(dev), torch.full((), float("nan"), device=dev), ang)  # (NaN is dropped)
    counts, _ = angle_histograms(ang)
    kept = np.where(near, np.nan, want[0])
    assert np.array_equal(counts.cpu().numpy(), orc.hist_np(kept, 100, -PI, PI)) and int(counts.sum()) == int((~near).sum())


# ---- Jensen-Shannon distance ----
@pytest.mark.parametrize("bins", [100, 2500, 1, 257])
def test_js_distance_against_scipy(dev, bins):
    from lam_slide_amd import js_distance, torsion_stats
    rng = np.random.default_rng(bins)
    a, b = rng.integers(0, 400, size=(7, bins)), rng.integers(0, 400, size=(7, bins))
    a[1, ::3] = 0
    b[1, 1::3] = 0       # empty bins on either side (and on both where bins = 1)
    b[2] = a[2]          # equal rows
    a[3, bins // 2:] = 0
    b[3, :bins // 2] = 0  # disjoint rows
    a[4] = 0             # an all-zero row
    a[5] = rng.integers(0, 2, size=bins) * rng.integers(1, 10 ** 9, size=bins)  # large counts, many empty bins
    a[5, 0] = b[5, 0] = 1
    got = js_distance(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    assert torsion_stats.last_path["js_distance"] == "fused" and got.dtype == torch.float64 and got.shape == (7,)
    got = got.cpu().numpy()
    bar, worst = bins * 2.0 ** -50, 0.0
    for r in (0, 1, 5, 6) + ((3,) if bins > 1 else ()):
        with np.errstate(invalid="ignore"):  # (scipy's own 0 / 0 of an all-zero row)
            want = jensenshannon(a[r], b[r])
        if np.isnan(want):  # (bins = 1 with an empty side)
            assert np.isnan(got[r])
            continue
        worst = max(worst, abs(got[r] ** 2 - want ** 2))
    print(f"PARITY jsd.bins{bins} measured {worst:.3e} bar {bar:.1e}")
    assert worst <= bar
    assert got[2] == 0.0 and np.isnan(got[4])
    if bins > 1:
        assert abs(got[3] ** 2 - math.log(2)) <= bar and int(np.isnan(got).sum()) == 1
    # int32 tables, and a table alone: the same values
    g32 = js_distance(torch.from_numpy(a[:4].astype(np.int32)).to(dev), torch.from_numpy(b[:4].astype(np.int32)).to(dev))
    assert np.array_equal(g32.cpu().numpy()[:4], got[:4], equal_nan=True) and float(js_distance(torch.from_numpy(a[0]).to(dev), torch.from_numpy(b[0]).to(dev))) == got[0]


# ---- lagged products ----
@pytest.fixture(scope="module")
def series(peptides):
    """x float32 [3, 4097, 40] in [-1, 1]: sin of the first 40 torsions of three R = 23 trajectories, and the float64 oracle of every
    tested (n, nlag) on x[:, :n] - computed once."""
    base, quads, _ = peptides[23]
    x = np.stack([np.sin(orc.dihedral_np(orc.ar1_frames(base, 4097, seed=300 + s, sigma=0.3), quads, np.float64)) for s in range(3)]).astype(np.float32)
    assert x.shape == (3, 4097, 40) and np.abs(x).max() <= 1
    return x, {(n, nlag): orc.lag64(x[:, :n], nlag) for n, nlag in ((2, 1), (1000, 999), (1000, 1), (4097, 1000))}


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("C", [1, 40])
@pytest.mark.parametrize("n,nlag", [(2, 1), (1000, 999), (1000, 1), (4097, 1000)])
def test_lagged_products_against_the_direct_float64_sum(dev, series, n, nlag, C, S):
    from lam_slide_amd import _lib, lagged_products, torsion_stats
    x, oracle = series
    want = oracle[(n, nlag)][:S, :C]
    xd = torch.from_numpy(np.ascontiguousarray(x[:S, :n, :C])).to(dev)
    got = lagged_products(xd, nlag)
    assert torsion_stats.last_path["lagged_products"] == "fused" and got.dtype == torch.float32 and got.shape == (S, C, nlag + 1)
    bar = (_lib.LAG_CHUNK + 8) * EPS
    err = float(np.abs(got.cpu().double().numpy() - want).max())
    print(f"PARITY lag.n{n}.nlag{nlag}.C{C}.S{S} measured {err:.3e} bar {bar:.1e}")
    assert _lib.LAG_CHUNK <= 504 and err <= bar
    # a series alone and inside the batch, a channel alone and beside the others: the same bits; [n, C] is S = 1
    s, c = S - 1, C // 2
    assert same_bits(lagged_products(xd[s:s + 1].contiguous(), nlag)[0], got[s])
    assert same_bits(lagged_products(xd[:, :, c:c + 1].contiguous(), nlag)[:, 0], got[:, c])
    assert same_bits(lagged_products(xd[0], nlag), got[0])


def test_lagged_products_split_over_channels_and_refusals(dev, series, monkeypatch):
    from lam_slide_amd import lagged_products, torsion_stats
    x, _ = series
    xd = torch.from_numpy(np.ascontiguousarray(x[:2, :1000, :7])).to(dev)
    whole = lagged_products(xd, 500)
    monkeypatch.setattr(torsion_stats, "LAG_WORKSPACE_BYTES", 3 * 2 * 3 * 501 * 8)  # room for three channels of the two series at a time
    assert same_bits(lagged_products(xd, 500), whole) and torsion_stats.last_path["lagged_products"] == "fused"
    with pytest.raises(ValueError, match="nlag"):
        lagged_products(xd, 1000)
    nan = xd.clone()
    nan[0, 500, 3] = float("nan")  # a NaN reaches every lag of its own series and channel, nothing else
    got = lagged_products(nan, 500)
    assert bool(torch.isnan(got[0, 3]).all()) and int(torch.isnan(got).sum()) == 501


def test_decorrelation_against_the_oracle(dev, peptides):
    from lam_slide_amd import _lib, decorrelation, torsion_stats
    base, quads, _ = peptides[4]
    ang = orc.dihedral_np(orc.ar1_frames(base, 4097, seed=8, sigma=0.6), quads, np.float32)  # wide: every baseline below 0.9
    want, baseline = orc.decorrelation64(ang, 1000)
    assert float(baseline.max()) < 0.9
    got = decorrelation(torch.from_numpy(ang).to(dev), 1000)
    assert torsion_stats.last_path["decorrelation"] == "fused" and got.dtype == torch.float32 and got.shape == (len(quads), 1001)
    # sin / cos are the device's float32 ones: their rounding (2^-24 each, |x| <= 1) moves a mean of products by at most 2 * 2^-24
    bar = (_lib.LAG_CHUNK + 8) * EPS
    err = float((np.abs(got.cpu().double().numpy() - want) * (1 - baseline[:, None])).max())
    print(f"PARITY decorrelation measured {err:.3e} bar {bar:.1e}")
    assert err <= bar


# ---- dispatch and the flow behind the sampler ----
def test_dispatch_rules(dev, peptides):
    from lam_slide_amd import TorsionStats, angle_histograms, dihedral_angles, js_distance, lagged_products, torsion_stats
    frames, quads, want, ref32 = dihedral_case(peptides, 4, 1, 65)
    pos = torch.from_numpy(frames[0])
    lp = torsion_stats.last_path
    for p in (pos, pos.to(dev).double(), pos.to(dev).requires_grad_(True)):  # CPU, float64, requires_grad: the restatement
        ang = dihedral_angles(p, quads)
        assert lp["dihedral_angles"] == "torch" and ang.device == p.device
        assert float(orc.wrapped_diff(ang.detach().cpu().numpy(), want[0]).max()) <= 4 * ref32
    ang = dihedral_angles(pos.to(dev), quads)
    assert lp["dihedral_angles"] == "fused"
    for a in (ang.cpu(), ang.double()):
        c, _ = angle_histograms(a)
        assert lp["angle_histograms"] == "torch" and c.device == a.device and np.array_equal(c.cpu().numpy(), orc.hist_np(ang.cpu().numpy(), 100, -PI, PI))
    x = torch.sin(ang)
    fused = lagged_products(x, 64)
    assert lp["lagged_products"] == "fused"
    for v in (x.cpu(), x.double()):
        r = lagged_products(v, 64)
        assert lp["lagged_products"] == "torch" and r.device == v.device and float((r.cpu().double() - fused.cpu().double()).abs().max()) <= 456 * EPS
    c = angle_histograms(ang)[0]
    assert float(js_distance(c.cpu(), c.cpu().flip(0)).sub(js_distance(c, c.flip(0)).cpu()).abs().max()) < 1e-12 and lp["js_distance"] == "fused"
    js_distance(c.double(), c.double())
    assert lp["js_distance"] == "torch"
    st = TorsionStats(quads, [f"PHI {i}" for i in range(len(quads))])
    st.update(pos.to(dev).double())
    assert st.path == "torch" and st.counts.is_cuda


def test_rollout_to_statistics_stays_on_the_device(dev, peptides):
    """RolloutSampler.sample_rollout -> TorsionStats.update -> .jsd: positions, angles and counts never leave the device before the
    final read (a stub model in place of the network: seeded displacements of the conditioning frame)."""
    from lam_slide_amd import RolloutSampler, TorsionStats
    base, quads, labels = peptides[4]
    T, R = 16, 4

    class Stub:
        shift, scale, n_timesteps = 0.0, 1.0, T

        def __init__(self):
            self.g = torch.Generator(device=dev).manual_seed(3)

        def sample(self, batch):
            pos = batch["atom14_pos"]  # [1, T, R, 14, 3]
            return {"atom14_pos": pos + 0.05 * torch.randn(pos.shape, generator=self.g, device=dev).cumsum(dim=1)}

    cond = torch.from_numpy(base).to(dev).reshape(R, 14, 3)
    stats = TorsionStats(quads, labels)
    rollout = RolloutSampler(Stub()).sample_rollout(cond, torch.zeros(R, dtype=torch.long, device=dev), torch.ones(R, 14, device=dev), num_rollouts=3)
    assert rollout.is_cuda and rollout.shape[-3:] == (R, 14, 3)
    for chunk in rollout.reshape(3, -1, R, 14, 3):
        stats.update(chunk)
    assert stats.path == "fused" and stats.counts.is_cuda and stats.n_frames == rollout.reshape(-1, R, 14, 3).shape[0]
    d = stats.jsd(stats)
    assert list(d)[:len(labels)] == labels and all(v == 0.0 for v in d.values())
    assert int(stats.counts.sum()) == stats.n_frames * len(quads)
