"""GPU tests of the structure statistics on the device (``lsl_pair_distances`` / ``lsl_ca_frame_stats`` / ``lsl_histogram_columns`` /
``lsl_js_distance_density`` behind ``lam_slide_amd.structure_stats``) against the numpy / scipy oracle of tests/structstat_oracle.py, at its
six seeded shapes: F = 1, a partial last workgroup, zero / one / many C-alpha pairs, a tile boundary of the histogram rows at n = 1025.

Bars.
  distances    |d - d64| <= 5 * 2^-24 * d64 against float64 on the same float32 inputs: one subtraction, three products, two additions and a
               square root of at most one float32 rounding each.  A frame alone has the bits it has in the batch, a repeated call gives the
               same bits, a host index outside the frame raises and enqueues nothing.
  frame stats  |rg - rg64| <= 2^-23 * rg64 (one float32 rounding; the float64 part is far below it).  flags, tally and contacts equal the
               float64 oracle's as integers; a frame may be excepted only if one of its distances is within 2^-20 (relative) of a threshold,
               at most 0.1 % of the frames - with the seeded inputs none is, and the test asserts that.  Two calls give exactly twice the
               tallies, cells with i >= j are untouched, NULL outputs are accepted.
  histograms   counts equal ``np.histogram`` on the device's own float32 values and the device-built edges as integers; the edges have
               ``np.linspace``'s bits.
  density JS   |d^2 - d^2_scipy| <= 2 * cells * 2^-50 against ``jensenshannon`` of numpy's ``density=True`` histograms + 1e-6 of the same
               values and edges, cells = 49 for a row, 2401 for a joint table: the bar of test_hip_tica's end-to-end JSD (cells * 2^-50),
               doubled for the two extra divisions and the addition per cell.  A row with no count on one side gives NaN.
  end to end   every key of ``traj_analysis`` against the oracle fed with the device's own features: the JS keys to the JS bar, val_ca
               exact, rmse_contact within 1e-14; no synchronising call inside ``traj_analysis``.
Measured values: profiles/structure_stats_parity.txt."""
import numpy as np
import pytest
import torch

import structstat_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables(golden):
    from lam_slide_amd.peptide_loss import residue_tables
    return residue_tables(golden("f18_peptide_loss.npz").group("tables"))


@pytest.fixture(scope="module")
def chains(dev):
    """{(n, R, seed): (host float32 [n, R * 14, 3], the same on the device)}, each made once."""
    cache = {}

    def get(n, R, seed):
        if (n, R, seed) not in cache:
            pos = orc.chain(n, R, seed).reshape(n, R * 14, 3)
            cache[(n, R, seed)] = (pos, torch.from_numpy(pos).to(dev))
        return cache[(n, R, seed)]

    return get


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def js_bar(cells):
    return 2 * cells * 2.0 ** -50


def js_ratio(got, want, cells):
    """max |d^2 - d^2_scipy| / bar over the entries; NaN must meet NaN."""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] ** 2 - want[ok] ** 2) / js_bar(cells)).max()) if ok.any() else 0.0


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- distances ----
@pytest.mark.parametrize("case", range(6))
def test_pair_distances_against_float64(dev, chains, case):
    from lam_slide_amd import _lib, ca_pair_table, pair_distances, structure_stats, triu_pairs
    n, R, seed = orc.CASES[case]
    pos, pd = chains(n, R, seed)
    ca = np.arange(R) * 14 + 1
    tables_ = [t for t in (ca[ca_pair_table(R)], triu_pairs(np.arange(0, R * 14, 5))) if len(t)]  # none / one / many C-alpha pairs, and a general table
    assert len(tables_) == (1 if R == 4 else 2) and (R != 5 or len(tables_[0]) == 1)
    worst = 0.0
    for pairs in tables_:
        got = pair_distances(pd, pairs)
        assert structure_stats.last_path["pair_distances"] == "fused" and got.dtype == torch.float32 and got.shape == (n, len(pairs))
        want = orc.dist64(pos, pairs)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        assert np.all(err <= 5 * 2.0 ** -24 * want)
        worst = max(worst, float((err / (5 * 2.0 ** -24 * want)).max()))
        assert same_bits(pair_distances(pd, pairs), got)  # a repeated call
        for f in sorted({0, n // 2, n - 1}):  # a frame alone has the bits it has in the batch
            assert same_bits(pair_distances(pd[f:f + 1], pairs), got[f:f + 1])
    print(f"PARITY distances.n{n}.R{R} worst error / bar {worst:.3e}")
    # a host index outside the frame: refused before any launch, the output untouched
    pairs = np.ascontiguousarray(tables_[-1].astype(np.int32))
    bad = pairs.copy()
    bad[-1, 1] = R * 14
    with pytest.raises(ValueError, match="outside the frame"):
        pair_distances(pd, bad)
    out = torch.full((n, len(pairs)), -7.0, dtype=torch.float32, device=dev)
    on = torch.from_numpy(pairs).to(dev)
    rc = _lib.load().lsl_pair_distances(pd.data_ptr(), on.data_ptr(), bad.ctypes.data, n, R * 14, len(pairs), out.data_ptr(), stream(dev))
    torch.cuda.synchronize()
    assert rc == -3 and b"outside the frame" in _lib.load().lsl_last_error() and bool((out == -7.0).all())


def test_more_pairs_than_one_call_holds(dev):
    from lam_slide_amd import pair_distances, structure_stats, triu_pairs
    pos = np.random.default_rng(11).standard_normal((2, 364, 3)).astype(np.float32)
    pairs = triu_pairs(np.arange(364))
    assert len(pairs) == 66066 > structure_stats.MAX_P
    got = pair_distances(torch.from_numpy(pos).to(dev), pairs)
    want = orc.dist64(pos, pairs)
    assert structure_stats.last_path["pair_distances"] == "fused" and got.shape == want.shape
    assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - want) <= 5 * 2.0 ** -24 * want)


# ---- frame statistics ----
@pytest.mark.parametrize("case", range(6))
def test_ca_frame_stats_against_float64(dev, chains, case):
    from lam_slide_amd import _lib, ca_frame_stats, structure_stats
    n, R, seed = orc.CASES[case]
    pos, pd = chains(n, R, seed)
    ca = (np.arange(R) * 14 + 1).astype(np.int32)
    got = ca_frame_stats(pd, ca)
    assert structure_stats.last_path["ca_frame_stats"] == "fused"
    rg, flags, tally, contacts, near = orc.ca_stats64(pos, ca)
    assert got.rg.dtype == torch.float32 and got.flags.dtype == torch.int32 and got.tally.dtype == got.contacts.dtype == torch.int64
    err = np.abs(got.rg.cpu().numpy().astype(np.float64) - rg)
    assert np.all(err <= 2.0 ** -23 * rg)
    print(f"PARITY frame_stats.n{n}.R{R} rg worst error / bar {float((err / (2.0 ** -23 * rg)).max()):.3e}; frames near a threshold {int(near.sum())} of {n}; "
          f"tally {tally.tolist()}")
    assert int(near.sum()) == 0  # (the rule allows 0.1 % of the frames; the seeded inputs have none)
    assert np.array_equal(got.flags.cpu().numpy(), flags) and np.array_equal(got.tally.cpu().numpy(), tally)
    assert np.array_equal(got.contacts.cpu().numpy(), contacts)
    for f in sorted({0, n // 2, n - 1}):  # a frame alone has the bits it has in the batch
        one = ca_frame_stats(pd[f:f + 1], ca)
        assert same_bits(one.rg, got.rg[f:f + 1]) and int(one.flags[0]) == int(flags[f])
    # the raw entry point: tables that are added to, cells with i >= j untouched, NULL outputs
    lib, st = _lib.load(), stream(dev)
    sel = torch.from_numpy(ca).to(dev)
    tl = torch.full((4,), 3, dtype=torch.int64, device=dev)
    ct = torch.full((R, R), 5, dtype=torch.int64, device=dev)
    call = lambda rg_, fl_, tl_, ct_: lib.lsl_ca_frame_stats(pd.data_ptr(), sel.data_ptr(), ca.ctypes.data, n, R * 14, R, 0.3, 0.419, 1.0, rg_, fl_, tl_, ct_, st)  # noqa: E731
    assert call(None, None, tl.data_ptr(), ct.data_ptr()) == 0
    assert np.array_equal(tl.cpu().numpy(), 3 + tally) and np.array_equal(ct.cpu().numpy(), 5 + contacts)
    assert call(None, None, tl.data_ptr(), ct.data_ptr()) == 0  # two calls: exactly twice
    assert np.array_equal(tl.cpu().numpy(), 3 + 2 * tally) and np.array_equal(ct.cpu().numpy(), 5 + 2 * contacts)
    assert torch.equal(ct.tril(), torch.full_like(ct, 5).tril())
    rg_only, fl_only = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    assert call(rg_only.data_ptr(), None, None, None) == 0 and call(None, fl_only.data_ptr(), None, None) == 0
    assert call(None, None, None, None) == 0
    assert same_bits(rg_only, got.rg) and torch.equal(fl_only, got.flags)
    bad = ca.copy()
    bad[0] = R * 14
    assert lib.lsl_ca_frame_stats(pd.data_ptr(), sel.data_ptr(), bad.ctypes.data, n, R * 14, R, 0.3, 0.419, 1.0, rg_only.data_ptr(), None, tl.data_ptr(), None, st) == -3
    torch.cuda.synchronize()
    assert np.array_equal(tl.cpu().numpy(), 3 + 2 * tally)  # refused: nothing enqueued


def test_the_longest_selection(dev):
    """R = 146: the frame tile is 14 frames, 10585 pair cells per workgroup."""
    from lam_slide_amd import ca_frame_stats, structure_stats
    R, n = structure_stats.MAX_R, 31
    pos = orc.chain(n, R, 9).reshape(n, R * 14, 3)
    ca = np.arange(R) * 14 + 1
    got = ca_frame_stats(torch.from_numpy(pos).to(dev), ca)
    rg, flags, tally, contacts, near = orc.ca_stats64(pos, ca)
    assert structure_stats.last_path["ca_frame_stats"] == "fused" and not near.any()
    assert np.all(np.abs(got.rg.cpu().numpy().astype(np.float64) - rg) <= 2.0 ** -23 * rg)
    assert np.array_equal(got.flags.cpu().numpy(), flags) and np.array_equal(got.tally.cpu().numpy(), tally)
    assert np.array_equal(got.contacts.cpu().numpy(), contacts)


# ---- column histograms and density JS ----
@pytest.fixture(scope="module")
def columns(dev, chains):
    """{case: (ref, model)}: the device's own float32 C-alpha distances two or more residues apart (R = 4 has three columns, R = 20 has
    171: three column tiles at 49 bins) of chain(n, R, seed) and chain(n + 3, R, seed + 100)."""
    from lam_slide_amd import ca_pair_table, pair_distances
    cache = {}

    def get(case):
        if case not in cache:
            n, R, seed = orc.CASES[case]
            pairs = (np.arange(R) * 14 + 1)[ca_pair_table(R, offset=1)]
            cache[case] = (pair_distances(chains(n, R, seed)[1], pairs), pair_distances(chains(n + 3, R, seed + 100)[1], pairs))
        return cache[case]

    return get


@pytest.mark.parametrize("case", range(6))
def test_column_histograms_equal_numpy(dev, columns, case):
    from lam_slide_amd import column_edges, histogram_columns, structure_stats
    ref, model = columns(case)
    edges = column_edges(ref, 50)
    want_edges = orc.edges_np(ref.cpu().numpy(), 50)
    assert edges.is_cuda and np.array_equal(edges.cpu().numpy().view(np.int64), want_edges.view(np.int64))  # np.linspace's bits
    for x in (ref, model):
        counts = histogram_columns(x, edges)
        assert structure_stats.last_path["histogram_columns"] == "fused" and counts.shape == (x.shape[1], 49)
        v = x.cpu().numpy().astype(np.float64)
        want = np.stack([np.histogram(v[:, q], bins=want_edges[q])[0] for q in range(v.shape[1])])
        assert np.array_equal(counts.cpu().numpy(), want)
        first = counts.clone()
        assert histogram_columns(x, edges, counts) is counts and torch.equal(counts, 2 * first)  # added to
    assert int(histogram_columns(ref, edges).sum()) == ref.numel() or orc.CASES[case][0] == 1  # the reference's extremes are its own edges


@pytest.mark.parametrize("case", range(6))
def test_density_js_against_scipy(dev, columns, case):
    from lam_slide_amd import density_js, joint_density_js, structure_stats
    ref, model = columns(case)
    r, m = ref.cpu().numpy(), model.cpu().numpy()
    edges = orc.edges_np(r, 50)
    js, mean = density_js(ref, model, 50)
    assert structure_stats.last_path["density_js"] == "fused" and js.dtype == torch.float64 and js.shape == (r.shape[1],)
    want, want_mean = orc.density_js_np(r, m, edges)
    r1 = js_ratio(js.cpu().numpy(), want, 49)
    assert r1 <= 1.0 and js_ratio(float(mean), want_mean, 49) <= 1.0
    joint = joint_density_js(ref[:, 0], ref[:, -1], model[:, 0], model[:, -1], 50)
    assert structure_stats.last_path["joint_density_js"] == "fused" and joint.shape == ()
    r2 = js_ratio(float(joint), orc.joint_js_np(r[:, 0], r[:, -1], m[:, 0], m[:, -1], edges[0], edges[-1]), 49 * 49)
    n, R, _ = orc.CASES[case]
    print(f"PARITY density_js.n{n}.R{R} rows {r.shape[1]} worst |d^2 - scipy| / bar: 1-D {r1:.3e} (bar {js_bar(49):.1e}), 2-D {r2:.3e} (bar {js_bar(2401):.1e})")
    assert r2 <= 1.0 and bool(np.isnan(want).all()) == (n == 1)


def test_a_row_without_counts_gives_nan(dev):
    from lam_slide_amd import js_distance_density, structure_stats
    a = torch.tensor([[3, 0, 5], [1, 2, 3], [0, 0, 0]], device=dev)
    b = torch.tensor([[0, 0, 0], [3, 2, 1], [1, 1, 1]], device=dev)
    m = torch.tensor([[0.5, 0.5, 0.5], [0.5, 0.25, 0.5], [1.0, 1.0, 1.0]], dtype=torch.float64, device=dev)
    out = js_distance_density(a, b, m).cpu().numpy()
    assert structure_stats.last_path["js_distance_density"] == "fused"
    w = np.array([0.5, 0.25, 0.5])
    want = orc.jensenshannon(np.array([1, 2, 3]) / w / 6 + 1e-6, np.array([3, 2, 1]) / w / 6 + 1e-6)
    assert np.isnan(out[0]) and np.isnan(out[2]) and abs(out[1] ** 2 - want ** 2) <= js_bar(3)
    m[1, 1] = 0.0
    assert bool(torch.isnan(js_distance_density(a, b, m)[1]))  # a cell of size zero


# ---- end to end ----
@pytest.mark.parametrize("case", (3, 5))
def test_traj_analysis_end_to_end_without_synchronising(dev, tables, chains, case):
    from lam_slide_amd import StructureTables, ca_frame_stats, dihedral_angles, pair_distances, structure_stats, traj_analysis, triu_pairs
    n, R, seed = orc.CASES[case]
    st = StructureTables(orc.aatype(R), tables)
    st.on(dev)  # the index tables, uploaded once
    (_, ref), (_, model) = chains(n, R, seed), chains(n, R, seed + 100)
    tr, tm = orc.tics(n, seed), orc.tics(n, seed + 100)
    trd, tmd = torch.from_numpy(tr).to(dev), torch.from_numpy(tm).to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = traj_analysis(model, ref, st, trd, tmd)
        with pytest.raises(RuntimeError, match="synchroniz"):  # (the mode does see an upload: tables that are not on the device yet)
            traj_analysis(model, ref, StructureTables(orc.aatype(R), tables))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert structure_stats.last_path["traj_analysis"] == "fused"
    assert list(got) == ["ramachandran_js", "pwd_js", "rg_js", "tic_js", "tic2d_js", "val_ca", "rmse_contact"]
    assert all(v.is_cuda and v.dtype == torch.float64 and v.shape == () for v in got.values())

    def features(p, tics):
        ang = dihedral_angles(p, st.rama).cpu().numpy()
        return {"phi0": ang[:, 0], "psi0": ang[:, 1], "pwd": pair_distances(p, st.ca_pairs).cpu().numpy(), "rg": ca_frame_stats(p, st.ca).rg.cpu().numpy(),
                "ca_dist": pair_distances(p, triu_pairs(st.ca)).cpu().numpy(), "tics": tics}

    want = orc.traj_analysis_np(features(ref, tr), features(model, tm))
    ratios = {k: js_ratio(float(got[k]), want[k], 2401 if k in ("ramachandran_js", "tic2d_js") else 49) for k in got if k.endswith("_js")}
    e_rmse = abs(float(got["rmse_contact"]) - want["rmse_contact"])
    print(f"PARITY e2e.n{n}.R{R} |d^2 - scipy| / bar " + ", ".join(f"{k} {v:.3e}" for k, v in ratios.items())
          + f"; val_ca {float(got['val_ca']):.6f} (oracle {want['val_ca']:.6f}); rmse_contact error {e_rmse:.3e} bar 1.0e-14")
    assert max(ratios.values()) <= 1.0 and float(got["val_ca"]) == want["val_ca"] and e_rmse <= 1e-14
    assert all(0.0 < float(got[k]) < 1.0 for k in ratios) and 0.0 < float(got["val_ca"]) < 1.0
