"""``lam_slide_amd.structure_stats`` without a GPU: the numpy / torch restatements of the validation callback's structure statistics
against the float64 oracle of tests/structstat_oracle.py at its six seeded shapes, the index-table builders on a hand-written
tetrapeptide and a five-residue peptide, the conventions the reference's ``try`` / ``except`` blocks create, and the C ABI (symbols,
header, refusals before anything touches a GPU).

Bars (the same as on the device, tests/test_hip_structure_stats.py): distances 5 * 2^-24 relative (one subtraction, three products, two
additions and a square root of at most one float32 rounding each), rg 2^-23 relative, flags / tallies / contacts / histogram counts equal as
integers, d^2 of a Jensen-Shannon distance within 2 * cells * 2^-50 of scipy's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import structstat_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALA, ARG, GLY, SER = 0, 1, 7, 15  # residue_constants.restypes order: A R N D C Q E G H I L K M F P S T W Y V
SYMBOLS = ("lsl_pair_distances", "lsl_ca_frame_stats", "lsl_histogram_columns", "lsl_js_distance_density")


@pytest.fixture(scope="module")
def tables(golden):
    from lam_slide_amd.peptide_loss import residue_tables
    return residue_tables(golden("f18_peptide_loss.npz").group("tables"))


def js_bar(cells):
    return 2 * cells * 2.0 ** -50


def close_js(got, want, cells):
    """Both NaN, or d^2 within the bar."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all((np.isnan(got) & np.isnan(want)) | (np.abs(got ** 2 - want ** 2) <= js_bar(cells))))


def atom_name(tables, aatype, index):
    """The atom37 name of frame index ``r * 14 + slot`` (through the residue tables: the set atom37 slot that maps to the atom14 slot)."""
    from lam_slide_amd.structure_stats import ATOM37_NAMES
    r, slot = divmod(int(index), 14)
    s37 = [s for s in range(37) if tables.m37[aatype[r], s] != 0 and tables.a37to14[aatype[r], s] == slot]
    assert len(s37) == 1
    return r, ATOM37_NAMES[s37[0]]


# ---- the index tables ----
def test_tables_of_a_hand_written_tetrapeptide(tables):
    from lam_slide_amd import StructureTables, backbone_torsion_quads, ca_atoms, ca_pair_table, tica_atom_selection, triu_pairs
    aa = [ALA, ARG, GLY, SER]  # atom14: N CA C O CB | N CA C O CB CG CD NE CZ NH1 NH2 | N CA C O | N CA C O CB OG
    assert ca_atoms(aa, tables).tolist() == [1, 15, 29, 43]
    bb = backbone_torsion_quads(aa, tables)
    assert bb.phi.tolist() == [[2, 14, 15, 16], [16, 28, 29, 30], [30, 42, 43, 44]]
    assert bb.psi.tolist() == [[0, 1, 2, 14], [14, 15, 16, 28], [28, 29, 30, 42]]
    assert bb.omega.tolist() == [[1, 2, 14, 15], [15, 16, 28, 29], [29, 30, 42, 43]]
    # the topology's order is atom37's (N CA C CB O CG ... CD NE NH1 NH2 CZ): CB before the dropped O, CZ after NH2
    assert tica_atom_selection(aa, tables).tolist() == [0, 1, 2, 4, 14, 15, 16, 18, 19, 20, 21, 23, 24, 22, 28, 29, 30, 42, 43, 44, 46]
    assert ca_pair_table(4).shape == (0, 2) and ca_pair_table(4, offset=1).tolist() == [[0, 2], [0, 3], [1, 3]]
    assert ca_pair_table(7).tolist() == [[0, 4], [0, 5], [0, 6], [1, 5], [1, 6], [2, 6]]  # compute_pairwise_distances' loop order
    assert triu_pairs([5, 7, 11, 2]).tolist() == [[5, 7], [5, 11], [5, 2], [7, 11], [7, 2], [11, 2]]  # np.triu_indices(k=1)
    st = StructureTables(aa, tables)
    assert st.R == 4 and st.n_tors == 3 and st.ca_pairs.shape == (0, 2) and st.rama.tolist() == [bb.phi[0].tolist(), bb.psi[0].tolist()]
    assert st.quads.dtype == np.int32 and st.quads.tolist() == np.concatenate(bb).tolist() and st.tica_pairs.shape == (21 * 20 // 2, 2)


def test_tables_of_a_five_residue_peptide_name_the_right_atoms(tables):
    from lam_slide_amd import StructureTables, backbone_torsion_quads, ca_atoms, tica_atom_selection, topology_atoms
    from lam_slide_amd.structure_stats import ATOM37_NAMES
    assert len(ATOM37_NAMES) == 37 and ATOM37_NAMES[:5] == ("N", "CA", "C", "CB", "O") and ATOM37_NAMES[-1] == "OXT"
    aa = orc.aatype(5)
    name = lambda i: atom_name(tables, aa, i)  # noqa: E731
    assert [name(i) for i in ca_atoms(aa, tables)] == [(r, "CA") for r in range(5)]
    bb = backbone_torsion_quads(aa, tables)
    for k in range(4):
        assert [name(i) for i in bb.phi[k]] == [(k, "C"), (k + 1, "N"), (k + 1, "CA"), (k + 1, "C")]
        assert [name(i) for i in bb.psi[k]] == [(k, "N"), (k, "CA"), (k, "C"), (k + 1, "N")]
        assert [name(i) for i in bb.omega[k]] == [(k, "CA"), (k, "C"), (k + 1, "N"), (k + 1, "CA")]
    sel, top = tica_atom_selection(aa, tables), topology_atoms(aa, tables)
    names = [name(i)[1] for i in sel]
    assert not any(s.startswith("O") for s in names) and all(s[0] in "CNS" for s in names)
    assert [i for i in top if not name(i)[1].startswith("O")] == sel.tolist() and len(sel) < len(top)  # the topology's order, oxygens out
    st = StructureTables(aa, tables)
    assert st.ca_pairs.tolist() == [[1, 4 * 14 + 1]] and st.tica_pairs.shape[0] == len(sel) * (len(sel) - 1) // 2


# ---- the primitives against the oracle ----
@pytest.mark.parametrize("case", range(6))
def test_distances_and_frame_stats_restatement_against_float64(case):
    from lam_slide_amd import ca_frame_stats, ca_pair_table, pair_distances, structure_stats, triu_pairs
    n, R, seed = orc.CASES[case]
    pos = orc.chain(n, R, seed).reshape(n, R * 14, 3)
    ca = np.arange(R) * 14 + 1
    for pairs in (ca[ca_pair_table(R)], triu_pairs(np.arange(0, R * 14, 5))):
        if len(pairs) == 0:
            continue
        got, want = pair_distances(torch.from_numpy(pos), pairs), orc.dist64(pos, pairs)
        assert structure_stats.last_path["pair_distances"] == "torch" and got.dtype == torch.float32 and got.shape == want.shape
        assert np.all(np.abs(got.numpy().astype(np.float64) - want) <= 5 * 2.0 ** -24 * want)
    got = ca_frame_stats(torch.from_numpy(orc.chain(n, R, seed)), ca)  # ([n, R, 14, 3] works too)
    rg, flags, tally, contacts, near = orc.ca_stats64(pos, ca)
    assert structure_stats.last_path["ca_frame_stats"] == "torch" and not near.any()
    assert got.rg.dtype == torch.float32 and np.all(np.abs(got.rg.numpy().astype(np.float64) - rg) <= 2.0 ** -23 * rg)
    assert got.flags.dtype == torch.int32 and np.array_equal(got.flags.numpy(), flags)
    assert got.tally.dtype == torch.int64 and np.array_equal(got.tally.numpy(), tally) and int(tally[0]) == n
    assert got.contacts.dtype == torch.int64 and np.array_equal(got.contacts.numpy(), contacts) and not np.tril(contacts).any()
    if n > 1:  # clashing, broken and valid frames side by side; contact rates from a few percent to 1
        assert min(tally[1:]) > 0 and contacts[np.triu_indices(R, 1)].min() < n and contacts[np.triu_indices(R, 1)].max() == n


def test_frame_stats_argument_checks():
    from lam_slide_amd import ca_frame_stats, pair_distances
    pos = torch.from_numpy(orc.chain(3, 4, 0))
    with pytest.raises(ValueError, match="outside the frame"):
        pair_distances(pos.reshape(3, 56, 3), [[0, 56]])
    with pytest.raises(ValueError, match="pairs"):
        pair_distances(pos.reshape(3, 56, 3), [[0, 1, 2]])
    with pytest.raises(ValueError, match="sel"):
        ca_frame_stats(pos, [1, 15, 56])
    with pytest.raises(ValueError, match="sel"):
        ca_frame_stats(pos, [[1, 15]])
    one = ca_frame_stats(pos, [1])  # a single atom: no pair, rg = 0
    assert one.flags.tolist() == [0, 0, 0] and one.tally.tolist() == [3, 0, 0, 3] and one.rg.tolist() == [0.0, 0.0, 0.0] and one.contacts.tolist() == [[0]]


@pytest.mark.parametrize("case", range(6))
def test_edges_histograms_and_density_js_restatement_against_numpy_and_scipy(case):
    from lam_slide_amd import ca_pair_table, column_edges, density_js, histogram_columns, joint_density_js, structure_stats
    n, R, seed = orc.CASES[case]
    ca = np.arange(R) * 14 + 1
    pairs = ca[ca_pair_table(R, offset=1)]  # (offset 1: R = 4 has pairs too)
    ref = orc.dist64(orc.chain(n, R, seed).reshape(n, -1, 3), pairs).astype(np.float32)
    model = orc.dist64(orc.chain(n + 3, R, seed + 100).reshape(n + 3, -1, 3), pairs).astype(np.float32)
    rt, mt = torch.from_numpy(ref), torch.from_numpy(model)
    edges = column_edges(rt, 50)
    want_edges = orc.edges_np(ref, 50)
    assert edges.dtype == torch.float64 and np.array_equal(edges.numpy().view(np.int64), want_edges.view(np.int64))  # np.linspace's bits
    counts = histogram_columns(mt, edges)
    assert structure_stats.last_path["histogram_columns"] == "torch" and counts.dtype == torch.int64 and counts.shape == (len(pairs), 49)
    assert np.array_equal(counts.numpy(), np.stack([np.histogram(model[:, q].astype(np.float64), bins=want_edges[q])[0] for q in range(len(pairs))]))
    first = counts.clone()
    assert histogram_columns(mt, edges, counts) is counts and torch.equal(counts, 2 * first)  # added to, in place
    js, mean = density_js(rt, mt, 50)
    want, want_mean = orc.density_js_np(ref, model, want_edges)
    assert structure_stats.last_path["density_js"] == "torch" and js.dtype == torch.float64 and js.shape == (len(pairs),) and mean.shape == ()
    assert close_js(js.numpy(), want, 49) and close_js(float(mean), want_mean, 49)
    assert bool(np.isnan(want).all()) == (n == 1)  # one reference frame: every cell has size zero
    joint = joint_density_js(rt[:, 0], rt[:, -1], mt[:, 0], mt[:, -1], 50)
    want_joint = orc.joint_js_np(ref[:, 0], ref[:, -1], model[:, 0], model[:, -1], want_edges[0], want_edges[-1])
    assert structure_stats.last_path["joint_density_js"] == "torch" and joint.shape == () and close_js(float(joint), want_joint, 49 * 49)


def test_constant_column_and_empty_row_give_nan():
    from lam_slide_amd import column_edges, density_js, js_distance_density
    rg = torch.full((40,), 0.75)
    assert column_edges(rg, 50).tolist() == [[0.75] * 50]
    js, mean = density_js(rg, rg, 50)  # a constant rg column: every cell has size zero
    assert bool(torch.isnan(js).all()) and bool(torch.isnan(mean))
    a, b = torch.tensor([[3, 0, 5], [1, 2, 3]]), torch.tensor([[0, 0, 0], [3, 2, 1]])
    m = torch.tensor([[0.5, 0.5, 0.5], [0.5, 0.25, 0.5]], dtype=torch.float64)
    out = js_distance_density(a, b, m)
    want = orc.jensenshannon(np.array([1, 2, 3]) / np.array([0.5, 0.25, 0.5]) / 6 + 1e-6, np.array([3, 2, 1]) / np.array([0.5, 0.25, 0.5]) / 6 + 1e-6)
    assert bool(torch.isnan(out[0])) and abs(float(out[1]) ** 2 - want ** 2) <= js_bar(3)  # no count on one side: NaN
    m[1, 1] = 0.0
    assert bool(torch.isnan(js_distance_density(a, b, m)[1]))  # a cell of size zero
    with pytest.raises(ValueError, match="bins"):
        column_edges(rg, 1)


# ---- the seven numbers ----
def features(pos, st, tics=None):
    """The oracle's inputs from the library's own features (float32, as given)."""
    from lam_slide_amd import ca_frame_stats, dihedral_angles, pair_distances, triu_pairs
    p = torch.from_numpy(pos)
    ang = dihedral_angles(p, st.rama).numpy()
    pwd = pair_distances(p, st.ca_pairs).numpy() if len(st.ca_pairs) else np.zeros((len(pos), 0), dtype=np.float32)
    f = {"phi0": ang[:, 0], "psi0": ang[:, 1], "pwd": pwd, "rg": ca_frame_stats(p, st.ca).rg.numpy(),
         "ca_dist": pair_distances(p, triu_pairs(st.ca)).numpy()}
    if tics is not None:
        f["tics"] = tics
    return f


@pytest.mark.parametrize("case", range(6))
def test_traj_analysis_restatement_against_the_oracle(tables, case):
    from lam_slide_amd import StructureTables, structure_stats, traj_analysis
    n, R, seed = orc.CASES[case]
    st = StructureTables(orc.aatype(R), tables)
    ref, model = orc.chain(n, R, seed).reshape(n, -1, 3), orc.chain(n + 3, R, seed + 100).reshape(n + 3, -1, 3)
    with_tics = case % 2 == 1
    tr, tm = (orc.tics(n, seed), orc.tics(n + 3, seed + 100)) if with_tics else (None, None)
    got = traj_analysis(torch.from_numpy(model), torch.from_numpy(ref), st, None if tr is None else torch.from_numpy(tr),
                        None if tm is None else torch.from_numpy(tm))
    want = orc.traj_analysis_np(features(ref, st, tr), features(model, st, tm))
    keys = ["ramachandran_js", "pwd_js", "rg_js"] + (["tic_js", "tic2d_js"] if with_tics else []) + ["val_ca", "rmse_contact"]
    assert list(got) == keys == list(want) and structure_stats.last_path["traj_analysis"] == "torch"
    assert all(v.dtype == torch.float64 and v.shape == () for v in got.values())
    for k in keys:
        g, w = float(got[k]), want[k]
        if k.endswith("_js"):
            assert close_js(g, w, 49 * 49 if k in ("ramachandran_js", "tic2d_js") else 49), (k, g, w)
        elif k == "val_ca":
            assert g == w
        else:
            assert abs(g - w) <= 1e-14, (k, g, w)
    if n > 1 and R > 4:
        assert all(0.0 < float(got[k]) < 1.0 for k in keys if k.endswith("_js")) and 0.0 < float(got["val_ca"]) < 1.0 and float(got["rmse_contact"]) > 0.0


def test_the_tetrapeptide_quirk_and_the_single_residue(tables):
    """R = 4 has no C-alpha pair four residues apart: the reference's ``np.stack([])`` raises inside the ``try`` that also holds rg_js, and both
    become 0 - while ``density_js`` on rg itself is a proper distance.  With one residue ``rmse_contact`` is 0 (the ``except``)."""
    from lam_slide_amd import StructureTables, ca_frame_stats, density_js, traj_analysis
    from lam_slide_amd.structure_stats import contact_rmse
    st = StructureTables(orc.aatype(4), tables)
    ref, model = torch.from_numpy(orc.chain(200, 4, 7)), torch.from_numpy(orc.chain(150, 4, 8))
    got = traj_analysis(model, ref, st)
    assert float(got["pwd_js"]) == 0.0 and float(got["rg_js"]) == 0.0 and float(got["ramachandran_js"]) > 0.0 and float(got["rmse_contact"]) > 0.0
    rg_js = density_js(ca_frame_stats(ref, st.ca).rg, ca_frame_stats(model, st.ca).rg)[1]
    assert 0.0 < float(rg_js) < 1.0
    one = ca_frame_stats(torch.from_numpy(orc.chain(5, 1, 0)), [1])
    assert float(contact_rmse(one.contacts, 5, one.contacts, 5)) == 0.0
    two = ca_frame_stats(ref, st.ca)
    assert float(contact_rmse(two.contacts, 200, two.contacts, 200)) == 0.0
    with pytest.raises(ValueError, match="ramachandran"):  # (the reference's phi[:, 0] raises there too)
        traj_analysis(torch.from_numpy(orc.chain(5, 1, 0)), torch.from_numpy(orc.chain(5, 1, 1)), StructureTables([ALA], tables))
    with pytest.raises(ValueError, match="tics"):
        traj_analysis(model, ref, st, tics_ref=torch.zeros(200, 2))


def test_tica_features_layout(tables):
    from lam_slide_amd import StructureTables, dihedral_angles, pair_distances, tica_features
    aa = orc.aatype(5)
    st = StructureTables(aa, tables)
    pos = torch.from_numpy(orc.chain(17, 5, 3))
    f = tica_features(pos, aa, tables)
    P = st.tica_pairs.shape[0]
    assert f.shape == (17, P + 6 * 4) and f.dtype == torch.float32 and torch.equal(f, tica_features(pos, st))
    flat = pos.reshape(17, -1, 3)
    assert torch.equal(f[:, :P], pair_distances(flat, st.tica_pairs))
    ang = dihedral_angles(flat, st.quads)
    want = [fn(ang[:, 4 * k:4 * k + 4]) for k in range(3) for fn in (torch.sin, torch.cos)]  # sin phi | cos phi | sin psi | cos psi | sin omega | cos omega
    assert torch.equal(f[:, P:], torch.cat(want, dim=1))


# ---- the C ABI ----
def test_library_exports_and_header_declare_the_structure_statistics():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib, peptide_loss, structure_stats
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    exports = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*lsl_\*;", exports) and re.search(r"local:\s*\*;", exports)  # every lsl_ symbol, nothing else
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
        assert re.fullmatch(r"lsl_[a-z_]+", s) and getattr(lib, s).argtypes is not None
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6  # no new ABI number: a stale library is found by the missing symbols
    assert ", ".join(SYMBOLS) + " added" in header
    assert len(lib.lsl_pair_distances.argtypes) == 8 and len(lib.lsl_ca_frame_stats.argtypes) == 14
    assert len(lib.lsl_histogram_columns.argtypes) == 7 and len(lib.lsl_js_distance_density.argtypes) == 8
    src = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_structstat.hip.h")).read()
    macro = lambda name: int(re.search(r"#define " + name + r" (\d+)", src).group(1))  # noqa: E731
    assert macro("LSL_PAIR_MAX_P") == structure_stats.MAX_P and macro("LSL_CA_MAX_R") == structure_stats.MAX_R == peptide_loss.MAX_R
    assert macro("LSL_CA_MAX_R") * 14 == _lib.TORS_MAX_A and macro("LSL_CA_TILE") == 256 and macro("LSL_HCOL_CELLS") > _lib.HIST_MAX_BINS
    assert "atomicAdd" in src and not re.search(r"atomicAdd\([^;]*(float|double)", src)  # integer atomics only


def test_entry_points_validate_arguments_without_gpu():
    from lam_slide_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    pairs, sel = np.array([[1, 2], [3, 55]], dtype=np.int32), np.array([1, 15, 29, 43], dtype=np.int32)
    pd = lambda pos=one, p=one, ph=pairs.ctypes.data, F=10, A=56, P=2, out=one: lib.lsl_pair_distances(pos, p, ph, F, A, P, out, None)  # noqa: E731
    ca = lambda pos=one, s=one, sh=sel.ctypes.data, F=10, A=56, R=4: lib.lsl_ca_frame_stats(pos, s, sh, F, A, R, 0.3, 0.419, 1.0, one, one, one, one, None)  # noqa: E731
    hc = lambda x=one, n=100, Q=5, e=one, bins=49, c=one: lib.lsl_histogram_columns(x, n, Q, e, bins, c, None)  # noqa: E731
    js = lambda a=one, b=one, m=one, rows=3, bins=49, out=one: lib.lsl_js_distance_density(a, b, m, rows, bins, 1e-6, out, None)  # noqa: E731
    assert pd(pos=None) == -1 and pd(p=None) == -1 and pd(ph=None) == -1 and pd(out=None) == -1
    assert ca(pos=None) == -1 and ca(s=None) == -1 and ca(sh=None) == -1
    assert hc(x=None) == -1 and hc(e=None) == -1 and hc(c=None) == -1
    assert js(a=None) == -1 and js(b=None) == -1 and js(m=None) == -1 and js(out=None) == -1
    assert pd(A=55) == -3 and b"pairs[1][1] = 55" in lib.lsl_last_error()  # an index outside the frame
    bad = pairs.copy()
    bad[0, 0] = -1
    assert pd(ph=bad.ctypes.data) == -3 and b"pairs[0][0] = -1" in lib.lsl_last_error()
    for kw in (dict(A=0), dict(A=2045), dict(P=0), dict(P=65537), dict(F=0), dict(F=-5)):
        assert pd(**kw) == -3, kw
    assert ca(A=43) == -3 and b"sel[3] = 43" in lib.lsl_last_error()
    for kw in (dict(A=0), dict(R=0), dict(R=147), dict(F=0), dict(F=-1)):
        assert ca(**kw) == -3, kw
    assert hc(bins=0) == -3 and b"bins = 0" in lib.lsl_last_error()
    for kw in (dict(bins=2049), dict(n=0), dict(Q=0), dict(Q=65536 * 2, bins=2048)):
        assert hc(**kw) == -3, kw
    for kw in (dict(rows=0), dict(bins=0)):
        assert js(**kw) == -3, kw
    # every output of lsl_ca_frame_stats NULL: accepted, nothing to do
    assert lib.lsl_ca_frame_stats(one, one, sel.ctypes.data, 10, 56, 4, 0.3, 0.419, 1.0, None, None, None, None, None) == 0
