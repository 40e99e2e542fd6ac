"""``lam_slide_amd.torsion_stats`` without a GPU: the numpy / torch restatements of the peptide evaluation's torsion statistics against the
oracle of tests/torsstat_oracle.py (the float64 four-point dihedral, ``np.histogram`` / ``np.histogram2d``,
``scipy.spatial.distance.jensenshannon``, the direct float64 lagged sum), the quadruple builders against the residue tables, the
``calc_summary_metrics`` grouping, the accumulator, and the C ABI (symbols, header, refusals before anything touches a GPU).

Inputs: the target atom14 positions of fixture F18's R = 4 and R = 23 cases, made a trajectory by a seeded AR(1) perturbation."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.spatial.distance import jensenshannon

import torsstat_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi
ALA, ARG, GLY, SER = 0, 1, 7, 15  # residue_constants.restypes order: A R N D C Q E G H I L K M F P S T W Y V


@pytest.fixture(scope="module")
def tables(golden):
    from lam_slide_amd.peptide_loss import residue_tables
    return residue_tables(golden("f18_peptide_loss.npz").group("tables"))


@pytest.fixture(scope="module")
def cases(golden, tables):
    """{R: (frames float32 [n, R * 14, 3], quads, labels)} for R = 4 (n = 1000) and R = 23 (n = 257, the first 40 torsions)."""
    from lam_slide_amd import eval_torsion_quads
    f = golden("f18_peptide_loss.npz")
    out = {}
    for R, name, n in ((4, "f5_r4", 1000), (23, "f9_r23", 257)):
        c = f.group(name)
        quads, labels = eval_torsion_quads(c["aatype"][0], tables)
        out[R] = (torch.from_numpy(orc.ar1_frames(c["target"][0].numpy(), n, seed=R)), quads[:40], labels[:40])
    return out


def test_dihedral_restatement_against_the_float64_formula(cases):
    from lam_slide_amd import dihedral_angles, torsion_stats
    for R, (frames, quads, _) in cases.items():
        want = orc.dihedral_np(frames.numpy(), quads, np.float64)
        got64 = dihedral_angles(frames.double(), quads)
        assert torsion_stats.last_path["dihedral_angles"] == "torch" and got64.dtype == torch.float64 and got64.shape == want.shape
        assert float(orc.wrapped_diff(got64.numpy(), want).max()) < 1e-12
        ref32 = float(orc.wrapped_diff(orc.dihedral_np(frames.numpy(), quads, np.float32), want).max())
        got32 = dihedral_angles(frames, torch.from_numpy(quads))  # (a tensor table works too)
        err = float(orc.wrapped_diff(got32.numpy(), want).max())
        print(f"R = {R}: float32 restatement {err:.2e}, float32 oracle {ref32:.2e}")
        assert got32.dtype == torch.float32 and err <= 4 * ref32
        assert float(np.abs(want).max()) <= PI and float(np.abs(want).std()) > 0.3  # (angles all over the circle)
    frames, quads, _ = cases[4]
    assert dihedral_angles(frames[0], quads).shape == (len(quads),) and dihedral_angles(frames.reshape(10, 100, -1, 3), quads[:1]).shape == (10, 100, 1)
    with pytest.raises(ValueError, match="outside the frame"):
        dihedral_angles(frames, [[0, 1, 2, 56]])
    with pytest.raises(ValueError, match="quads"):
        dihedral_angles(frames, [[0, 1, 2]])
    with pytest.raises(ValueError, match="pos"):
        dihedral_angles(frames[..., :2], quads)


def test_histogram_restatement_is_numpy(cases):
    from lam_slide_amd import angle_histograms, dihedral_angles, torsion_stats
    x = orc.planted_angles(1000, 7, seed=3)
    pairs = [(1, 2), (3, 4)]
    counts, counts2 = angle_histograms(torch.from_numpy(x), pairs=pairs)
    assert torsion_stats.last_path["angle_histograms"] == "torch" and counts.dtype == counts2.dtype == torch.int64
    assert counts.shape == (7, 100) and counts2.shape == (2, 50, 50)
    assert np.array_equal(counts.numpy(), orc.hist_np(x, 100, -PI, PI)) and np.array_equal(counts2.numpy(), orc.hist2_np(x, pairs, 50, -PI, PI))
    inside = (x.astype(np.float64) >= -PI) & (x.astype(np.float64) <= PI)
    assert int(counts.sum()) == int(inside.sum()) and int(counts2[0].sum()) == int((inside[:, 1] & inside[:, 2]).sum())
    assert 0 < int((~inside).sum()) < x.size // 20  # (NaN, +-inf, the float32 neighbours outside +-pi and the uniform margin)
    # a range whose edges float32 holds exactly, every edge once: v == edges[i] is in bin i, v == edges[bins] in the last bin (closed)
    e1 = np.linspace(-1.0, 2.5, 15)
    c, _ = angle_histograms(torch.from_numpy(e1.astype(np.float32))[:, None], bins=14, range=(-1.0, 2.5))
    assert c[0].tolist() == [1] * 13 + [2]
    xe = orc.planted_angles(1000, 7, seed=4, bins=14, lo=-1.0, hi=2.5, bins2=7)
    c, c2 = angle_histograms(torch.from_numpy(xe), bins=14, pairs=pairs, bins2=7, range=(-1.0, 2.5))
    assert (xe == 2.5).sum() >= 7 and np.array_equal(c.numpy(), orc.hist_np(xe, 14, -1.0, 2.5)) and np.array_equal(c2.numpy(), orc.hist2_np(xe, pairs, 7, -1.0, 2.5))
    # batched [S, n, Q], another range, no pairs
    xs = torch.from_numpy(np.stack([x, x[::-1].copy()]))
    c3, none = angle_histograms(xs, bins=13, range=(-1.0, 2.5))
    assert none is None and c3.shape == (2, 7, 13) and torch.equal(c3[0], c3[1]) and np.array_equal(c3[0].numpy(), orc.hist_np(x, 13, -1.0, 2.5))
    # angles of a trajectory
    frames, quads, _ = cases[4]
    ang = dihedral_angles(frames, quads)
    assert np.array_equal(angle_histograms(ang)[0].numpy(), orc.hist_np(ang.numpy(), 100, -PI, PI))
    for kw in (dict(bins=0), dict(range=(1.0, 1.0)), dict(range=(2.0, -2.0)), dict(range=(0.0, float("inf"))), dict(pairs=[(0, 7)]),
               dict(pairs=[(-1, 2)]), dict(pairs=[(0, 1)], bins2=0), dict(pairs=[(0, 1, 2)])):
        with pytest.raises(ValueError):
            angle_histograms(torch.from_numpy(x), **kw)


def test_js_restatement_against_scipy():
    from lam_slide_amd import js_distance, torsion_stats
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 50, size=(6, 100)), rng.integers(0, 50, size=(6, 100))
    a[1, ::3] = 0
    b[1, 1::3] = 0       # empty bins on either side
    b[2] = a[2]          # equal rows
    a[3, 50:] = 0
    b[3, :50] = 0        # disjoint rows
    a[4] = 0             # an all-zero row
    got = js_distance(torch.from_numpy(a), torch.from_numpy(b))
    assert torsion_stats.last_path["js_distance"] == "torch" and got.dtype == torch.float64 and got.shape == (6,)
    for r in (0, 1, 3, 5):
        assert abs(float(got[r]) ** 2 - jensenshannon(a[r], b[r]) ** 2) <= 100 * 2.0 ** -50, r
    assert float(got[2]) == 0.0 and abs(float(got[3]) ** 2 - math.log(2)) <= 100 * 2.0 ** -50
    assert math.isnan(float(got[4])) and int(torch.isnan(got).sum()) == 1
    assert js_distance(torch.from_numpy(a[0]), torch.from_numpy(b[0])).shape == ()
    with pytest.raises(ValueError):
        js_distance(torch.from_numpy(a), torch.from_numpy(b[:, :50]))


def test_lagged_products_and_decorrelation_restatements(cases):
    from lam_slide_amd import decorrelation, dihedral_angles, lagged_products, torsion_stats
    frames, quads, _ = cases[4]
    ang = dihedral_angles(frames.double(), quads)
    x = torch.sin(ang).float()
    want = orc.lag64(x.numpy(), 999)
    got = lagged_products(x, 999)
    assert torsion_stats.last_path["lagged_products"] == "torch" and got.dtype == torch.float32 and got.shape == (len(quads), 1000)
    assert float(np.abs(got.double().numpy() - want).max()) <= 2.0 ** -24  # (float64 sums, rounded once; |ac| <= 1)
    got64 = lagged_products(torch.stack([x, -x]).double(), 10)
    assert got64.dtype == torch.float64 and got64.shape == (2, len(quads), 11) and torch.equal(got64[0], got64[1])
    assert float(np.abs(got64[0].numpy() - want[:, :11]).max()) < 1e-14
    assert abs(float(lagged_products(torch.tensor([[2.0], [3.0]]), 1)[0, 1]) - 6.0) == 0.0  # n = 2: one term at lag 1
    for bad in (1000, -1, 5000):
        with pytest.raises(ValueError, match="nlag"):
            lagged_products(x, bad)
    # decorrelation: a wider perturbation (sigma = 0.6), so that every torsion's baseline |mean e^{i angle}|^2 is below 0.9
    ang = dihedral_angles(torch.from_numpy(orc.ar1_frames(frames[0].numpy(), 1000, seed=8, sigma=0.6)), quads)
    d_want, base = orc.decorrelation64(ang.numpy(), 200)
    d = decorrelation(ang, 200)
    assert torsion_stats.last_path["decorrelation"] == "torch" and d.dtype == torch.float32 and d.shape == (len(quads), 201)
    assert float(base.max()) < 0.9  # (the bar below is a statement about curves that are not flat)
    assert float((np.abs(d.double().numpy() - d_want) * (1 - base[:, None])).max()) <= 8 * 2.0 ** -24
    assert float(np.abs(d_want[:, 0] - 1).max()) < 1e-6 and float(d_want[:, 100].max()) < 0.9  # starts at 1 (sin^2 + cos^2), decays


def test_topology_atoms_is_the_atom37_mask_enumeration(golden, tables):
    from lam_slide_amd import topology_atoms
    t = golden("f18_peptide_loss.npz").group("tables")
    mask, to14 = t["restype_atom37_mask"].numpy(), t["restype_atom37_to_atom14"].numpy()
    aatype = [ARG, GLY, 20, ALA, 13]  # (the unknown type has no atoms)
    want = [r * 14 + int(to14[aa, s]) for r, aa in enumerate(aatype) for s in range(37) if mask[aa, s]]
    got = topology_atoms(torch.tensor(aatype), tables)
    assert got.dtype == np.int64 and got.tolist() == want and len(want) == int(mask[aatype].sum())
    assert len(set(want)) == len(want) and all(v // 14 != 2 for v in want)
    # the heavy atoms of ARG in atom37 order start N, CA, C, CB, O: atom14 slots 0, 1, 2, 4, 3
    assert got[:5].tolist() == [0, 1, 2, 4, 3] and topology_atoms([GLY], tables).tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        topology_atoms([21], tables)


def test_eval_torsion_quads_of_a_tetrapeptide(tables):
    from lam_slide_amd import eval_torsion_quads
    aatype = [ALA, GLY, ARG, SER]
    quads, labels = eval_torsion_quads(aatype, tables)
    assert quads.dtype == np.int32 and quads.shape == (len(labels), 4) and quads.min() >= 0 and quads.max() < 4 * 14
    assert labels[:6] == ["PHI 1", "PSI 0", "PHI 2", "PSI 1", "PHI 3", "PSI 2"]  # interleaved
    assert sum("PHI" in s for s in labels) == 3 and sum("PSI" in s for s in labels) == 3
    chi = {r: [s for s in labels if s.startswith("CHI") and s.endswith(f" {r}")] for r in range(4)}
    assert chi[0] == [] and chi[1] == [] and chi[2] == ["CHI1 2", "CHI2 2", "CHI3 2", "CHI4 2"] and chi[3] == ["CHI1 3"]
    # phi 1 = (C of 0, N, CA, C of 1), psi 0 = (N, CA, C of 0, N of 1); N, CA, C are atom14 slots 0, 1, 2
    assert quads[0].tolist() == [2, 14, 15, 16] and quads[1].tolist() == [0, 1, 2, 14]
    # chi1 of ARG: N, CA, CB, CG = atom14 slots 0, 1, 4, 5 of residue 2; every chi stays inside its residue
    assert quads[labels.index("CHI1 2")].tolist() == [28, 29, 32, 33]
    for q, s in zip(quads, labels):
        if s.startswith("CHI"):
            assert set(int(v) // 14 for v in q) == {int(s.split()[1])} and len(set(q.tolist())) == 4
    bb, bl = eval_torsion_quads(aatype, tables, sidechains=False)
    assert bl == labels[:6] and np.array_equal(bb, quads[:6])
    assert eval_torsion_quads([ALA, 20, ALA], tables)[1] == [] and eval_torsion_quads([ARG], tables, sidechains=False)[0].shape == (0, 4)


def test_summary_metrics_groups_like_calc_summary_metrics():
    from lam_slide_amd import TorsionStats, summary_metrics
    a = {"PHI 1": 0.1, "PSI 0": 0.3, "CHI1 2": 0.5, "PSI 0|PHI 2": 0.9, "TICA-0": 0.2, "TICA-0,1": 0.4}
    b = {"PHI 1": 0.2, "CHI1 0": 0.7, "CHI2 0": 0.9, "PHI 1|PSI 0": 0.8, "TICA-0": 0.4, "TICA-0,1": 0.6}
    out = summary_metrics([a, b])
    assert out.keys() == {"BB", "SC", "ALL", "TICA-0", "TICA-0,1"}
    assert out["BB"] == pytest.approx(np.mean([0.1, 0.3, 0.2])) and out["SC"] == pytest.approx(np.mean([0.5, 0.7, 0.9]))
    assert out["ALL"] == pytest.approx(np.mean([0.1, 0.3, 0.5, 0.2, 0.7, 0.9]))  # the "a|b" keys are in neither BB nor ALL
    assert out["TICA-0"] == pytest.approx(0.3) and out["TICA-0,1"] == pytest.approx(0.5)
    only = TorsionStats.summary_metrics([{"PHI 1": 0.25, "PHI 1|PSI 0": 0.75}])
    assert only["BB"] == only["ALL"] == 0.25 and math.isnan(only["SC"]) and "TICA-0" not in only


def test_accumulator_adds_chunks_and_names_the_distances(cases):
    from lam_slide_amd import TorsionStats, angle_histograms, dihedral_angles
    frames, quads, labels = cases[4]
    whole, parts = TorsionStats(quads, labels), TorsionStats(quads, labels)
    ang = whole.update(frames.reshape(-1, 4, 14, 3))
    for lo, hi in ((0, 1), (1, 400), (400, 1000)):
        parts.update(frames[lo:hi])
    assert whole.path == parts.path == "torch" and parts.n_frames == 1000
    assert torch.equal(whole.counts, parts.counts) and torch.equal(whole.counts2, parts.counts2)
    c, c2 = angle_histograms(dihedral_angles(frames, quads), pairs=[(1, 2), (3, 4)])
    assert torch.equal(ang, dihedral_angles(frames, quads)) and torch.equal(whole.counts, c) and torch.equal(whole.counts2, c2)
    ref = TorsionStats(quads, labels)
    ref.update(torch.from_numpy(orc.ar1_frames(frames[0].numpy(), 800, seed=77, sigma=0.1)))
    d = whole.jsd(ref)
    assert list(d)[:len(labels)] == labels and list(d)[len(labels):] == [f"{labels[1]}|{labels[2]}", f"{labels[3]}|{labels[4]}"]
    for q, s in enumerate(labels):
        assert abs(d[s] ** 2 - jensenshannon(ref.counts[q].numpy(), whole.counts[q].numpy()) ** 2) <= 100 * 2.0 ** -50
    assert abs(d[f"{labels[1]}|{labels[2]}"] ** 2 - jensenshannon(ref.counts2[0].reshape(-1).numpy(), whole.counts2[0].reshape(-1).numpy()) ** 2) <= 2500 * 2.0 ** -50
    assert whole.jsd((ref.counts, ref.counts2)) == d and whole.jsd({"counts": ref.counts.numpy(), "counts2": ref.counts2.numpy()}) == d
    assert all(v == 0.0 for v in whole.jsd(parts).values())
    two = TorsionStats(quads[:2], labels[:2])  # fewer than three columns: no pair fits
    two.update(frames[:5])
    assert two.counts2 is None and list(two.jsd((two.counts, None))) == labels[:2]
    with pytest.raises(ValueError):
        whole.jsd((ref.counts[:3], ref.counts2))
    with pytest.raises(RuntimeError):
        TorsionStats(quads, labels).jsd(ref)
    with pytest.raises(ValueError):
        TorsionStats(quads, labels[:-1])
    with pytest.raises(ValueError, match="outside the frame"):
        TorsionStats(quads, labels).update(frames[:, :40])


def test_library_exports_and_header_declare_the_torsion_statistics():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    for s in ("lsl_dihedral_angles", "lsl_histogram", "lsl_lag_products_workspace_bytes", "lsl_lag_products", "lsl_js_distance"):
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
        assert re.fullmatch(r"lsl_[a-z_]+", s)
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6  # no new ABI number: a stale library is found by the missing symbols
    src = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_torsstat.hip.h")).read()
    macro = lambda name: int(re.search(r"#define " + name + r" (\d+)", src).group(1))  # noqa: E731
    assert macro("LSL_TORS_MAX_A") == _lib.TORS_MAX_A and macro("LSL_HIST_MAX_BINS") == _lib.HIST_MAX_BINS
    assert macro("LSL_HIST2_MAX_BINS") == _lib.HIST2_MAX_BINS and macro("LSL_HIST2_MAX_BINS") ** 2 <= macro("LSL_HIST_CELLS")
    assert macro("LSL_LAG_CHUNK") == _lib.LAG_CHUNK <= 504  # the longest float32 addition chain m of the lagged products
    assert "atomicAdd" in src and not re.search(r"atomicAdd\([^;]*(float|double)", src)  # integer atomics only


def test_entry_points_validate_arguments_without_gpu():
    from lam_slide_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    quads = np.array([[0, 1, 2, 3], [4, 5, 6, 55]], dtype=np.int32)
    pairs = np.array([[1, 2], [3, 4]], dtype=np.int32)
    hq, hp = quads.ctypes.data, pairs.ctypes.data
    dih = lambda pos=one, q=one, qh=hq, F=10, A=56, Q=2, out=one: lib.lsl_dihedral_angles(pos, q, qh, F, A, Q, out, None)  # noqa: E731
    hist = lambda x=one, S=1, n=100, Q=5, edges=one, bins=100, counts=one, p=one, ph=hp, P=2, ea=one, eb=one, bins2=50, c2=one: \
        lib.lsl_histogram(x, S, n, Q, edges, bins, counts, p, ph, P, ea, eb, bins2, c2, None)  # noqa: E731
    lag = lambda x=one, S=1, n=1000, Cc=40, nlag=999, ac=one, ws=one, nbytes=1 << 40: lib.lsl_lag_products(x, S, n, Cc, nlag, ac, ws, nbytes, None)  # noqa: E731
    js = lambda a=one, b=one, rows=3, bins=100, out=one: lib.lsl_js_distance(a, b, rows, bins, out, None)  # noqa: E731
    assert dih(pos=None) == -1 and dih(q=None) == -1 and dih(qh=None) == -1 and dih(out=None) == -1
    assert hist(x=None) == -1 and hist(edges=None) == -1 and hist(counts=None) == -1
    assert hist(p=None) == -1 and hist(ph=None) == -1 and hist(ea=None) == -1 and hist(eb=None) == -1 and hist(c2=None) == -1
    assert lag(x=None) == -1 and lag(ac=None) == -1 and lag(ws=None) == -1
    assert js(a=None) == -1 and js(b=None) == -1 and js(out=None) == -1
    # refused shapes: -3 and a text
    assert dih(A=55) == -3 and b"quads[1][3] = 55" in lib.lsl_last_error()  # an index outside the frame
    bad = quads.copy()
    bad[0, 1] = -1
    assert dih(qh=bad.ctypes.data) == -3 and b"quads[0][1] = -1" in lib.lsl_last_error()
    for kw in (dict(A=0), dict(A=2045), dict(Q=0), dict(F=0), dict(F=-5)):
        assert dih(**kw) == -3, kw
    assert hist(bins=0) == -3 and b"bins = 0" in lib.lsl_last_error()
    assert hist(Q=4) == -3 and b"pairs[1][1] = 4" in lib.lsl_last_error()  # a pair beyond the columns
    for kw in (dict(bins=2049), dict(bins2=0), dict(bins2=91), dict(S=0), dict(S=65536), dict(n=0), dict(Q=0), dict(P=-1)):
        assert hist(**kw) == -3, kw
    assert lag(nlag=1000) == -3 and b"nlag" in lib.lsl_last_error()  # nlag >= n
    for kw in (dict(nlag=-1), dict(n=0), dict(S=0), dict(Cc=0), dict(S=256, Cc=256), dict(n=1 << 22, nlag=1 << 21)):
        assert lag(**kw) == -3, kw
    assert lag(nbytes=8) == -4 and b"workspace" in lib.lsl_last_error()
    assert js(rows=0) == -3 and js(bins=0) == -3 and b"bins = 0" in lib.lsl_last_error()
    # the workspace of the lagged products: fp64 sums per (series, channel, segment of chunks, lag); 0 for a refused shape
    need = lib.lsl_lag_products_workspace_bytes
    assert need(1, 1000, 40, 999) == 40 * 3 * 1000 * 8 and need(3, 2, 1, 1) == 3 * 1 * 2 * 8  # 1000 steps: 3 chunks of 448
    assert need(1, 4097, 40, 1000) == 40 * 10 * 1001 * 8 and need(1, 1000, 40, 1000) == 0
    assert need(1, 1 << 20, 1, (1 << 20) - 1) == 2 * (1 << 20) * 8  # the segment sums of a channel stay within 2^21 values
    assert need(1, 2 ** 31 - 1, 1, 0) == 64777 * 8  # a long series: 4 793 491 chunks in segments of 74, at most 65535 segments (a grid dimension)
    with pytest.raises(ValueError):
        _lib.check(-3)


def test_dispatch_rules_on_cpu_tensors(cases):
    from lam_slide_amd import torsion_stats
    frames, quads, _ = cases[4]
    assert not torsion_stats.fused_applies(frames) and not torsion_stats.fused_applies(frames.double())
    g = frames.clone().requires_grad_(True)
    ang = torsion_stats.dihedral_angles(g, quads)
    assert ang.requires_grad and torsion_stats.last_path["dihedral_angles"] == "torch"  # the restatement is differentiable
