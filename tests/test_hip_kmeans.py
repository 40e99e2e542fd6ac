"""GPU tests of k-means fitting on the device (``lsl_kmeans_step`` / ``lsl_kmeans_nearest_rows`` behind ``lam_slide_amd.kmeans``) against the
numpy float64 oracle of tests/kmeans_oracle.py.

Bars.
  labels       equal the oracle's, except rows whose relative gap between the two smallest oracle distances is in (0, 1e-12) (the device
               fuses the sum over j, the oracle does not: both are correct float64 evaluations); at most 0.1 % of the rows may be
               excepted and with the seeded inputs the oracle alone excepts none.  An exact tie (gap 0: a duplicate centre) goes to the
               lowest index in both.
  centres      against the oracle's update computed from the DEVICE's labels: half a float32 ulp of the centre (the one rounding) plus
               (SEG + segments + 2) * 2^-53 * sum |y| / count (a segment is a chain of at most SEG float64 additions, the segments add in
               order, one division) - ``kmeans_oracle.center_bar``, a formula of the shape.
  counts, the changed-label count: exact integers.
  inertia      |J - sum of the oracle's distances at the device's labels| <= (SEG / 16 + 8 + segments + d + 4) * 2^-53 * J: a thread adds
               at most SEG / 16 sub-tiles, the tree has 8 levels, the segments add in order, a distance is d fused operations.
  fixed point, batch independence, repeatability: bit for bit.
Measured values: profiles/kmeans_parity.txt."""
import math

import numpy as np
import pytest
import torch

import kmeans_oracle as orc
from conftest import parity

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SEG = orc.SEG


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def worst(err, bar):
    """max err / bar over the entries (an entry whose bar is 0 must be exact)."""
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    assert np.all(err[bar == 0] == 0)
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0


class Buffers:
    """The caller's side of ``lsl_kmeans_step``: y [S, n, d], centres [S, k, d] numpy -> the device buffers, one ``step`` per call."""

    def __init__(self, dev, y, centers, prev=None):
        from lam_slide_amd import _lib
        self.dev, (self.S, self.n, self.d), self.k = dev, y.shape, centers.shape[1]
        self.y = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
        self.centers = torch.from_numpy(np.ascontiguousarray(centers)).to(dev)
        self.labels = torch.full((self.S, self.n), -2, dtype=torch.int32, device=dev) if prev is None else torch.from_numpy(prev.astype(np.int32)).to(dev)
        self.counts = torch.zeros(self.S, self.k, dtype=torch.int64, device=dev)
        self.state = torch.zeros(self.S, 4, dtype=torch.float64, device=dev)
        self.done = torch.zeros(self.S, dtype=torch.int32, device=dev)
        self.need = _lib.load().lsl_kmeans_workspace_bytes(self.S, self.n, self.d, self.k)
        assert self.need > 0
        self.ws = torch.zeros(self.need, dtype=torch.uint8, device=dev)

    def step(self, update=1, rel_tol=0.0, center_tol=0.0):
        from lam_slide_amd import _lib
        _lib.call(self.dev, "lsl_kmeans_step", self.y.data_ptr(), self.S, self.n, self.d, self.centers.data_ptr(), self.k, self.labels.data_ptr(),
                  self.counts.data_ptr(), self.state.data_ptr(), self.done.data_ptr(), update, rel_tol, center_tol, self.ws.data_ptr(), self.need)

    def changed(self):
        """The changed-label counts of the last step [S]: the last int32 table of the workspace, one entry per (series, segment)."""
        units = self.S * -(-self.n // SEG)
        off = units * (self.k * self.d + 1) * 8 + units * self.k * 4
        return self.ws[off:off + 4 * units].view(torch.int32).reshape(self.S, -1).sum(dim=1).cpu().numpy()

    def snapshot(self):
        return tuple(t.clone() for t in (self.centers, self.labels, self.counts, self.state, self.done))


def inertia_bar(n, d, J):
    return (SEG / 16 + 8 + -(-n // SEG) + d + 4) * U * J


# ---- one step against the oracle ----
STEP_SHAPES = {  # name: (S, n, k, d)
    "n1": (1, 1, 3, 2), "seg-1": (1, SEG - 1, 7, 3), "seg": (1, SEG, 7, 3), "seg+1": (1, SEG + 1, 7, 3), "2seg+17": (2, 2 * SEG + 17, 7, 3),
    "k1": (1, 300, 1, 3), "k=n": (1, 50, 50, 2), "k=n.big": (1, 300, 300, 2), "cells.d64": (1, 300, 128, 64), "cells.k1024": (1, 3000, 1024, 8),
    "d1": (1, 500, 9, 1), "packed": (5, 60, 20, 2), "packed.n64": (3, 64, 32, 16), "duplicate": (1, 700, 8, 3), "nan": (2, 700, 8, 3), "d48": (1, 200, 5, 48),
}


@pytest.mark.parametrize("name", sorted(STEP_SHAPES))
def test_one_step_against_the_oracle(dev, name):
    S, n, k, d = STEP_SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    y = np.stack([orc.blobs(n, min(k, 12), d, seed=1000 + 7 * s + sum(map(ord, name)), spread=1.0, sep=2.5) for s in range(S)])
    c = np.stack([y[s][(np.arange(k) * n) // k] + (0.25 * rng.standard_normal((k, d))).astype(np.float32) for s in range(S)])
    if name.startswith("k=n"):
        c = y.copy()  # every row its own centre
    if name == "duplicate":
        c[0, 5] = c[0, 2]  # a planted duplicate centre: the lowest index wins, the other stays empty
    if name == "nan":
        y[0, 13] = np.nan
        y[1, 400, 2] = np.nan
        y[1, n - 1, 0] = np.nan
    prev = rng.integers(-1, k, size=(S, n))
    b = Buffers(dev, y, c, prev)
    b.step()
    torch.cuda.synchronize()
    lab, counts, newc, state = b.labels.cpu().numpy(), b.counts.cpu().numpy(), b.centers.cpu().numpy(), b.state.cpu().numpy()
    changed = b.changed()
    excepted = 0
    for s in range(S):
        want = orc.step(y[s], c[s], prev[s])
        near = (want["gap"] > 0) & (want["gap"] < 1e-12)
        assert near.sum() == 0  # the seeds: the oracle alone excepts none
        excepted += int(near.sum())
        assert np.array_equal(lab[s][~near], want["labels"][~near]), (name, s)
        assert lab[s].min() >= -1 and lab[s].max() < k
        assert np.array_equal(counts[s], np.bincount(lab[s][lab[s] >= 0], minlength=k)) and changed[s] == int((lab[s] != prev[s]).sum())
        mine, cnt = orc.update(y[s], lab[s].astype(np.int64), c[s])  # the oracle's update from the device's labels
        bar = orc.center_bar(y[s], lab[s].astype(np.int64), mine, cnt)
        parity(f"step.{name}.s{s}.centres", worst(np.abs(newc[s].astype(np.float64) - mine.astype(np.float64)), bar), 1.0 + 1e-9)
        assert np.array_equal(newc[s][cnt == 0].view(np.int32), c[s][cnt == 0].view(np.int32))  # an empty cluster keeps its bits
        dist = orc.distances(y[s], c[s])
        J = math.fsum(np.where(lab[s] >= 0, dist[np.arange(n), np.maximum(lab[s], 0)], 0.0))  # (exactly rounded)
        assert state[s, 0] == 1.0 and state[s, 2] == 0.0
        if J > 0:
            parity(f"step.{name}.s{s}.inertia", abs(state[s, 1] - J) / inertia_bar(n, d, J), 1.0)
        else:
            assert state[s, 1] == 0.0
        shift = float(((newc[s].astype(np.float64) - c[s].astype(np.float64)) ** 2).sum())
        assert abs(state[s, 3] - shift) <= (k * d + 10) * U * shift
    assert excepted <= 0.001 * S * n
    if name == "duplicate":
        assert counts[0, 5] == 0 and (lab[0] != 5).all() and counts[0, 2] > 0
    if name == "nan":
        assert lab[0, 13] == -1 and lab[1, 400] == -1 and lab[1, n - 1] == -1 and counts.sum() == S * n - 3
    if name.startswith("k=n"):
        assert np.array_equal(lab[0], np.arange(n)) and (counts == 1).all() and np.array_equal(newc.view(np.int32), c.view(np.int32))


# ---- the full fit ----
@pytest.mark.parametrize("init", ("stride", "explicit"))
def test_full_fit_of_separated_blobs_and_the_fixed_point(dev, init):
    from lam_slide_amd import kmeans
    n, k, d = 2 * SEG + 300, 6, 3
    y = orc.blobs(n, k, d, seed=77, spread=0.3, sep=10.0)  # separation >> spread
    c0 = y[(np.arange(k) * n) // k] if init == "stride" else (y[:k] + np.float32(0.5))
    want = orc.fit(y, c0, max_iter=100, rel_tol=1e-5)
    assert want["converged"] and want["min_gap"] > 1e-9 and want["n_iter"] >= 2
    yt = torch.from_numpy(y).to(dev)
    res = kmeans.kmeans_fit(yt, k, init="stride" if init == "stride" else torch.from_numpy(c0), max_iter=100, rel_tol=1e-5)
    assert res.path == "fused" and kmeans.last_path["kmeans_fit"] == "fused"
    lab = res.labels.cpu().numpy()
    assert np.array_equal(lab, want["labels"]) and int(res.n_iter) == want["n_iter"] and bool(res.converged)
    assert np.array_equal(res.counts.cpu().numpy(), want["counts"])
    bar = orc.center_bar(y, want["labels"], want["centers"], want["counts"])
    parity(f"fit.{init}.centres", worst(np.abs(res.centers.cpu().numpy().astype(np.float64) - want["centers"].astype(np.float64)), bar), 1.0 + 1e-9)
    parity(f"fit.{init}.inertia", abs(float(res.inertia) - want["inertia"]) / inertia_bar(n, d, want["inertia"]), 1.0)
    # through the C ABI, iterated until no label changes (rel_tol = 0): one more step changes no bit of any buffer - done is honoured -
    # and with the flag cleared the iteration itself is a fixed point of centres, labels and counts
    want0 = orc.fit(y, c0, max_iter=100, rel_tol=0.0)
    res0 = kmeans.kmeans_fit(yt, k, init=torch.from_numpy(c0), max_iter=100, rel_tol=0.0)
    assert want0["converged"] and int(res0.n_iter) == want0["n_iter"] and np.array_equal(res0.labels.cpu().numpy(), want0["labels"])
    b = Buffers(dev, y[None], c0[None])
    for _ in range(want0["n_iter"] + 3):
        b.step()
    assert int(b.done[0]) == 1 and same_bits(b.centers[0], res0.centers) and int(b.state[0, 0]) == want0["n_iter"]
    before = b.snapshot()
    b.step()
    torch.cuda.synchronize()
    for x, z in zip(before, b.snapshot()):
        assert same_bits(x, z)
    b.done.zero_()
    b.step()
    assert same_bits(before[0], b.centers) and same_bits(before[1], b.labels) and same_bits(before[2], b.counts) and int(b.changed()[0]) == 0
    assert int(b.done[0]) == 1 and int(b.state[0, 0]) == want0["n_iter"] + 1
    b.step(0)
    assert same_bits(b.labels[0], res0.labels) and same_bits(b.state[0, 1], res0.inertia) and same_bits(before[0], b.centers) and same_bits(b.counts[0], res0.counts)


# ---- invariants on general data ----
def test_invariants_on_general_data(dev):
    n, k, d = 50_000, 100, 4
    y = orc.blobs(n, 30, d, seed=5, spread=1.0, sep=1.5)  # overlapping: a long iteration
    nan_rows = (3, 777, n - 1)
    for t in nan_rows:
        y[t, t % d] = np.nan
    b = Buffers(dev, y[None], y[None, (np.arange(k) * n) // k + 1])
    J, cmax, worst_ratio = [], [], 0.0
    for it in range(100):
        cmax.append(float(b.centers.abs().max()))
        b.step(1, 0.0)
        J.append(float(b.state[0, 1]))
        if int(b.done[0]):
            break
    for i in range(1, len(J)):
        eps = 2.0 ** -24 * cmax[i]  # rounding every coordinate of every centre to float32 moves a row's distance by at most ...
        slack = 2 * np.sqrt(n * d * J[i - 1]) * eps + n * d * eps * eps
        assert J[i] <= J[i - 1] + slack, (i, J[i - 1], J[i], slack)
        worst_ratio = max(worst_ratio, (J[i] - J[i - 1]) / slack)
    parity("invariants.inertia_rise_over_slack", max(worst_ratio, 0.0), 1.0)
    print(f"invariants: {len(J)} iterations, J {J[0]:.6e} -> {J[-1]:.6e}, done = {int(b.done[0])}")
    assert len(J) >= 10 and J[-1] < J[0]
    b.step(0)
    lab, counts = b.labels[0].cpu().numpy(), b.counts[0].cpu().numpy()
    assert counts.sum() == n - len(nan_rows) and lab.min() == -1 and lab.max() <= k - 1 and (lab[list(nan_rows)] == -1).all() and (lab == -1).sum() == len(nan_rows)
    assert np.array_equal(counts, np.bincount(lab[lab >= 0], minlength=k)) and float(b.state[0, 1]) <= J[-1] * (1 + 1e-12) + 1e-300


# ---- empty clusters ----
def test_surplus_centres_keep_their_bits(dev):
    from lam_slide_amd import kmeans
    pts = np.array([[0, 0], [4, 0], [0, 4], [4, 4], [9, 9]], dtype=np.float32)
    y = pts[np.arange(40) % 5]
    init = np.concatenate([pts + np.float32(0.25), np.array([[1e3, 1e3], [-1e3, 7.5], [3e3, -2e3]], dtype=np.float32)])
    res = kmeans.kmeans_fit(torch.from_numpy(y).to(dev), 8, init=torch.from_numpy(init), rel_tol=0.0)
    assert res.path == "fused" and bool(res.converged) and int(res.n_iter) == 2
    assert same_bits(res.centers[5:].cpu(), torch.from_numpy(init[5:])) and res.counts.tolist() == [8] * 5 + [0] * 3
    assert same_bits(res.centers[:5].cpu(), torch.from_numpy(pts)) and float(res.inertia) == 0.0


# ---- batch independence ----
def test_a_series_has_the_same_bits_alone_and_in_a_batch(dev):
    from lam_slide_amd import kmeans
    S, n, k, d = 37, SEG + 500, 6, 3
    y = np.stack([orc.blobs(n, k, d, seed=300 + s, spread=0.2 + 0.12 * (s % 9), sep=3.0) for s in range(S)])  # blobs of different difficulty
    y[30] = y[4]
    yt = torch.from_numpy(y).to(dev)
    batch = kmeans.kmeans_fit(yt, k, init="stride", rel_tol=0.0)
    alone = kmeans.kmeans_fit(yt[4], k, init="stride", rel_tol=0.0)
    again = kmeans.kmeans_fit(yt, k, init="stride", rel_tol=0.0)
    iters = batch.n_iter.tolist()
    print(f"batch: n_iter {sorted(set(iters))}, the series alone {int(alone.n_iter)}")
    assert len(set(iters)) >= 3 and min(iters) < int(alone.n_iter) < max(iters) and bool(alone.converged)
    for s in (4, 30):
        for f in ("centers", "labels", "counts", "inertia", "n_iter", "converged"):
            assert same_bits(getattr(batch, f)[s], getattr(alone, f)), (s, f)
    for f in ("centers", "labels", "counts", "inertia", "n_iter", "converged"):
        assert same_bits(getattr(batch, f), getattr(again, f)), f  # a fit run twice: identical bits
    # the state table too, through the C ABI
    c0 = y[:, (np.arange(k) * n) // k]
    b1, b37 = Buffers(dev, y[4:5], c0[4:5]), Buffers(dev, y, c0)
    for _ in range(max(iters) + 1):
        b1.step()
        b37.step()
    assert same_bits(b1.state[0], b37.state[4]) and same_bits(b1.state[0], b37.state[30]) and int(b37.done.sum()) == S


def test_tiny_series_packed_several_to_a_workgroup(dev):
    from lam_slide_amd import kmeans
    S, n, k, d = 300, 60, 20, 2
    y = np.stack([orc.blobs(n, 5, d, seed=500 + s, spread=0.3 + 0.05 * (s % 7), sep=2.0) for s in range(S)])
    y[298] = y[1]
    yt = torch.from_numpy(y).to(dev)
    batch = kmeans.kmeans_fit(yt, k, seed=9, rel_tol=0.0)
    alone = kmeans.kmeans_fit(yt[1:2], k, init=kmeans.initial_centers(yt, k, "kmeans++", seed=9)[1:2], rel_tol=0.0)
    assert batch.path == alone.path == "fused" and len(set(batch.n_iter.tolist())) >= 3
    for s in (1, 298):  # slots 1 and 2 of their workgroups; alone: slot 0
        if s == 298:
            one = kmeans.kmeans_fit(yt[298:299], k, init=kmeans.initial_centers(yt, k, "kmeans++", seed=9)[298:299], rel_tol=0.0)
        else:
            one = alone
        for f in ("centers", "labels", "counts", "inertia", "n_iter", "converged"):
            assert same_bits(getattr(batch, f)[s], getattr(one, f)[0]), (s, f)
    # and against the oracle, series by series
    c0 = kmeans.initial_centers(yt, k, "kmeans++", seed=9).cpu().numpy()
    lab, cen = batch.labels.cpu().numpy(), batch.centers.cpu().numpy()
    checked = 0
    for s in range(0, S, 23):
        want = orc.fit(y[s], c0[s], rel_tol=0.0)
        if want["min_gap"] <= 1e-12:
            continue
        assert np.array_equal(lab[s], want["labels"]) and int(batch.n_iter[s]) == want["n_iter"] and bool(batch.converged[s])
        bar = orc.center_bar(y[s], want["labels"], want["centers"], want["counts"])
        assert worst(np.abs(cen[s].astype(np.float64) - want["centers"].astype(np.float64)), bar) <= 1.0
        checked += 1
    assert checked >= 10


# ---- nearest_rows ----
@pytest.mark.parametrize("S,n,k,d", ((6, 60, 20, 2), (3, 1000, 7, 3), (2, 64, 5, 64), (2, 65, 1024, 8)))
def test_nearest_rows_against_argmin(dev, S, n, k, d):
    from lam_slide_amd import kmeans
    y = np.stack([orc.blobs(n, 6, d, seed=700 + s + n) for s in range(S)])
    c = np.stack([orc.blobs(k, 6, d, seed=800 + s + n) for s in range(S)])
    y[0, n // 2] = y[0, 5]  # a planted duplicate row: the lowest t wins
    c[0, 0] = y[0, 5]
    y[1, 2] = np.nan
    y[1, n - 1, d - 1] = np.nan
    c[1, 0] = 0.0
    y[S - 1] = np.nan  # no finite row: -1
    rows = kmeans.nearest_rows(torch.from_numpy(y).to(dev), torch.from_numpy(c).to(dev))
    assert kmeans.last_path["nearest_rows"] == "fused" and rows.dtype == torch.int32 and rows.shape == (S, k)
    rows = rows.cpu().numpy()
    excepted = 0
    for s in range(S):
        want, gap = orc.nearest(y[s], c[s])
        near = (gap > 0) & (gap < 1e-12)
        excepted += int(near.sum())
        assert np.array_equal(rows[s][~near], want[~near]), s
    assert excepted <= 0.001 * S * k
    assert rows[0, 0] == 5 and (rows[S - 1] == -1).all() and 2 not in rows[1] and n - 1 not in rows[1]


# ---- post_process end to end ----
def test_post_process_end_to_end_at_reduced_nba_shape(dev):
    from lam_slide_amd import DisplacementMeter, displacement_errors, metrics
    g = torch.Generator().manual_seed(21)
    K, R, B, T, A, D, c1 = 12, 4, 3, 9, 11, 2, 3
    target = torch.randn(B, T, A, D, generator=g)
    pred = target[None] + 0.5 * torch.randn(K, B, T, A, D, generator=g)
    mask = torch.ones(B, A, dtype=torch.bool)
    mask[1, 0] = mask[2, 7] = False
    r = displacement_errors(pred.to(dev), target.to(dev), mask.to(dev), first_frame=c1, num_runs=R, post_process=True, post_kmeans={"seed": 11})
    from lam_slide_amd import kmeans
    assert r.path == "fused" and r.post_fit.path == "fused" and kmeans.last_path["nearest_rows"] == "fused" and kmeans.last_path["kmeans_fit"] == "fused"
    # the torch restatement, fed the device's centres
    cpu = displacement_errors(pred, target, mask, first_frame=c1, num_runs=R)
    rows_cpu, _ = metrics.displacement_rows(pred, target, first_frame=c1)
    centers = r.post_fit.centers.cpu()
    post, totals, sel, _ = metrics.post_process_errors(rows_cpu, pred[:, :, T - 1], R, mask, centers=centers)
    finals = pred[:, :, T - 1].permute(1, 2, 0, 3).reshape(B * A, K, D).numpy()
    gaps = np.array([orc.nearest(finals[i], centers[i].numpy())[1].min() for i in range(B * A)])
    clear = torch.from_numpy((gaps == 0) | (gaps >= 1e-12)).reshape(B, A)
    assert int((~clear).sum()) <= 1 and torch.equal(r.post_rows.cpu()[clear], sel[clear])
    keep = mask & clear
    bar = 2 * (T - c1 + D + 4) * 2.0 ** -24  # the bar of rows: (Tf + D + 4) * 2^-24 on each side
    rel = lambda a, b: float(((a.double() - b.double()).abs() / b.double().abs())[keep].max())  # noqa: E731
    parity("post_process.ade_post", rel(r.ade_post.cpu(), post[..., 0]), bar)
    parity("post_process.fde_post", rel(r.fde_post.cpu(), post[..., 1]), bar)
    parity("post_process.ade", rel(r.ade.cpu(), cpu.ade), bar)
    assert torch.isnan(r.ade_post[1, 0]) and torch.isnan(r.fde_post[2, 7]) and int(torch.isnan(r.ade_post).sum()) == 2 == int(torch.isnan(r.fde_post).sum())
    plain = displacement_errors(pred.to(dev), target.to(dev), mask.to(dev), first_frame=c1, num_runs=R)
    assert same_bits(plain.ade, r.ade) and same_bits(plain.totals, r.totals) and plain.ade_post is None
    m = DisplacementMeter(2.0)
    m.update(r)
    out = m.compute()
    a, f = r.real_post()
    assert abs(out["ade_post"] - 2.0 * float(a.double().mean())) <= 1e-12 * out["ade_post"] and abs(out["fde_post"] - 2.0 * float(f.double().mean())) <= 1e-12 * out["fde_post"]
    assert abs(out["ade"] - 2.0 * float(r.real()[0].double().mean())) <= 1e-12 * out["ade"]


# ---- fit_microstates in the chain ----
def test_fit_microstates_in_the_chain(dev):
    from lam_slide_amd import assign_centers, fit_microstates, kmeans, tica, transition_counts
    n, k = 20_000, 100
    rng = np.random.default_rng(3)
    x = np.cumsum(0.05 * rng.standard_normal((n, 3)), axis=0)  # a slow random walk: what a TICA projection looks like
    y = torch.from_numpy((x - x.mean(axis=0)).astype(np.float32)).to(dev)
    centers = fit_microstates(y, k=k, max_iter=30)
    labels, counts = assign_centers(y, centers)
    C = transition_counts(labels, 10, k)
    assert tica.last_path["fit_microstates"] == "fused" and tica.last_path["assign_centers"] == "fused" and tica.last_path["transition_counts"] == "fused"
    fit = kmeans.kmeans_fit(y, k, max_iter=30, seed=137)  # what fit_microstates ran
    host = torch.stack([counts, fit.counts, C.sum(dim=1) + torch.bincount(labels[-10:].long(), minlength=k)]).cpu()  # (the one read)
    assert same_bits(centers, fit.centers) and torch.equal(labels, fit.labels)
    assert torch.equal(host[0], host[1]) and int(host[0].sum()) == n and torch.equal(host[2], host[0])
