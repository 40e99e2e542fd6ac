"""``lam_slide_amd.superpose`` without a GPU: the torch float64 restatement of the Kabsch fit, the RMSD, the centring and the RMSF against
the numpy float64 oracle of tests/superpose_oracle.py (SVD with the determinant fix) at the shapes of the device tests and at their bars
(coordinates 2^-23 of the frame's largest, rmsd 2^-23 relative + 1e-12 m, rot / trans 1e-10), its conventions (S = 0 -> identity, NaN for
the frame that holds one, proper rotations only), the atom14 wrappers on a hand-written tetrapeptide, and the C ABI: the three symbols and
every refusal before anything touches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import superpose_oracle as orc
from superpose_oracle import peptide, subset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lsl_superpose", "lsl_atom_rmsf_workspace_bytes", "lsl_atom_rmsf")


@pytest.fixture(scope="module")
def tables(golden):
    from lam_slide_amd.peptide_loss import residue_tables
    return residue_tables(golden("f18_peptide_loss.npz").group("tables"))


@pytest.mark.parametrize("A", orc.SIZES)
def test_restatement_against_the_oracle(A):
    from lam_slide_amd import superpose as sp
    F = min(orc.frame_counts(A)[-1], 40)
    ref, pos = orc.trajectory(A, F, seed=A)
    _, other = orc.trajectory(A, F, seed=A, variant=1)  # (other frames of the same structure: a per-frame reference)
    p, worst = torch.from_numpy(pos), 0.0
    sel = subset(A)
    fixed = np.zeros(A, dtype=np.uint8)
    fixed[::3] = 1
    for r, kw in ((ref, {}), (other, {}), (ref, {"atom_indices": sel}), (ref, {"fixed": fixed})):
        out, rms, rot, trans = sp.superpose(p, torch.from_numpy(r), return_rmsd=True, return_transform=True, **kw)
        assert sp.last_path["superpose"] == "torch" and out.dtype == torch.float32 and rms.dtype == torch.float32 and rot.dtype == torch.float64
        want = orc.kabsch(pos, r, kw.get("atom_indices"), kw.get("fixed"))
        worst = max(worst, orc.check_fit(want, pos, r, out.numpy(), rms.numpy(), rot.numpy(), trans.numpy()))
        if "fixed" in kw:
            assert np.array_equal(out.numpy()[:, fixed != 0], pos[:, fixed != 0])
        assert torch.equal(sp.rmsd(p, torch.from_numpy(r), atom_indices=kw.get("atom_indices")), rms)
    # reference=None with frame = F - 1, in place
    q = p.clone()
    got = sp.superpose(q, frame=F - 1, out=q)
    assert got is q
    worst = max(worst, orc.check_fit(orc.kabsch(pos, pos[F - 1]), pos, pos[F - 1], q.numpy()))
    print(f"PARITY superpose.torch.A{A}.F{F} worst error / bar {worst:.3e}")


def test_float64_and_grad_take_the_restatement():
    from lam_slide_amd import superpose as sp
    ref, pos = orc.trajectory(9, 4, seed=1)
    want = orc.kabsch(pos, ref)
    out, rms = sp.superpose(torch.from_numpy(pos).double(), torch.from_numpy(ref).double(), return_rmsd=True)
    assert out.dtype == torch.float64 and np.abs(out.numpy() - want["out"]).max() <= 1e-12 and np.abs(rms.numpy() - want["rmsd"]).max() <= 1e-6
    x = torch.from_numpy(pos).requires_grad_()
    rms = sp.rmsd(x, torch.from_numpy(ref))
    rms.sum().backward()
    assert sp.last_path["rmsd"] == "torch" and x.grad is not None and bool(torch.isfinite(x.grad).all())


def test_proper_rotations_only():
    from lam_slide_amd import superpose as sp
    ref, pos = orc.trajectory(56, 12, seed=2)
    mirrored = ref * np.array([1, 1, -1], dtype=np.float32)
    _, rms, rot, _ = sp.superpose(torch.from_numpy(pos), torch.from_numpy(mirrored), return_rmsd=True, return_transform=True)
    want = orc.kabsch(pos, mirrored)
    assert orc.is_proper_rotation(rot.numpy())
    orc.check_fit(want, pos, mirrored, rmsd=rms.numpy(), coordinates=False)
    assert np.all(want["rmsd"] > 1.0)  # (a reflection would have fitted to ~0.3)


def test_degenerate_selections_and_nan():
    from lam_slide_amd import superpose as sp
    ref, pos = orc.trajectory(12, 6, seed=3)
    pos[:, 7], ref[7] = pos[:, 4], ref[4]  # atoms 4 and 7 coincide in every frame
    pos[:, 9] = 2 * pos[:, 8] - pos[:, 5]  # 5, 8, 9 collinear
    ref[9] = 2 * ref[8] - ref[5]
    p, r = torch.from_numpy(pos), torch.from_numpy(ref)
    for sel in ([3], [3, 10], [5, 8, 9], [4, 7]):
        _, rms, rot, _ = sp.superpose(p, r, atom_indices=sel, return_rmsd=True, return_transform=True)
        want = orc.kabsch(pos, ref, sel)
        assert orc.is_proper_rotation(rot.numpy())
        orc.check_fit(want, pos, ref, rmsd=rms.numpy(), coordinates=False)
        if sel in ([3], [4, 7]):
            assert bool((rot == torch.eye(3, dtype=torch.float64)).all()) and np.all(want["zero"])
    clean = sp.superpose(p, r, return_rmsd=True, return_transform=True)
    bad = p.clone()
    bad[2, 5, 1] = float("nan")
    got = sp.superpose(bad, r, return_rmsd=True, return_transform=True)
    keep = [0, 1, 3, 4, 5]
    for g, c in zip(got, clean):
        assert bool(torch.isnan(g[2]).all()) and torch.equal(g[keep], c[keep])
    # a frame onto itself
    out, rms = sp.superpose(p, frame=3, return_rmsd=True)
    assert float(rms[3]) <= 1e-12 * np.abs(pos[3]).max() and np.abs(out[3].numpy() - pos[3]).max() <= 2.0 ** -23 * np.abs(pos[3]).max()


@pytest.mark.parametrize("A", (1, 56, 65))
def test_center_and_rmsf_against_numpy(A):
    from lam_slide_amd import superpose as sp
    for F in (1, orc.RMSF_SEG - 1, orc.RMSF_SEG, orc.RMSF_SEG + 1, 2 * orc.RMSF_SEG + 3):
        _, pos = orc.trajectory(A, F, seed=F)
        p = torch.from_numpy(pos)
        sel = subset(A)
        x = pos.astype(np.float64)
        for idx in (None, sel):
            c = sp.center_coordinates(p, idx)
            want = x - x[:, np.arange(A) if idx is None else idx].mean(axis=1, keepdims=True)
            assert c.dtype == torch.float32 and np.all(np.abs(c.numpy() - want).reshape(F, -1).max(axis=1) <= 2.0 ** -23 * np.abs(want).reshape(F, -1).max(axis=1))
        fl, mean = sp.rmsf(p, return_mean=True)
        wf, wm = orc.rmsf(pos)
        m = np.abs(x).max(axis=(0, 2))
        assert fl.dtype == torch.float32 and mean.dtype == torch.float64 and fl.shape == (A,) and mean.shape == (A, 3)
        assert np.all(np.abs(fl.numpy() - wf) <= 2.0 ** -23 * wf + 1e-12 * m) and np.all(np.abs(mean.numpy() - wm) <= 1e-12 * m[:, None])
        assert torch.equal(sp.rmsf(p, sel), fl[torch.from_numpy(sel)])


def test_atom14_wrappers_on_a_tetrapeptide(tables):
    from lam_slide_amd import StructureTables, create_trajectory, superpose_atom14
    aa, pos14, top = peptide(tables, 9)
    assert len(top) == 5 + 11 + 4 + 6
    pad = np.ones(56, dtype=bool)
    pad[top] = False
    flat = pos14.reshape(9, 56, 3)
    for frame in (0, 4):
        got = superpose_atom14(torch.from_numpy(pos14), aa, frame=frame, tables=tables)
        assert got.shape == pos14.shape and not got.numpy().reshape(9, 56, 3)[:, pad].any()
        want = orc.kabsch(flat, flat[frame], top, pad)
        orc.check_fit(want, flat, flat[frame], got.numpy().reshape(9, 56, 3))
    st = StructureTables(aa, tables)
    assert torch.equal(superpose_atom14(torch.from_numpy(pos14), st, frame=4), got)
    made = create_trajectory(torch.from_numpy(pos14), aa, tables=tables).numpy().reshape(9, 56, 3)
    x = flat.astype(np.float64)
    centred = x - x[:, top].mean(axis=1, keepdims=True)
    centred[:, pad] = 0.0
    c32 = centred.astype(np.float32)
    err = np.abs(made - orc.kabsch(c32, c32[0], top, pad)["out"]).reshape(9, -1).max(axis=1)
    assert not made[:, pad].any() and np.all(err <= 2 * 2.0 ** -23 * np.abs(centred).reshape(9, -1).max(axis=1))  # (two roundings: the centring, the fit)


def test_argument_errors():
    from lam_slide_amd import superpose as sp
    p = torch.zeros(3, 5, 3)
    for bad in (lambda: sp.superpose(torch.zeros(5, 3)), lambda: sp.superpose(p, torch.zeros(2, 5, 3)), lambda: sp.superpose(p, frame=3),
                lambda: sp.superpose(p, atom_indices=[5]), lambda: sp.superpose(p, atom_indices=[]), lambda: sp.superpose(p, fixed=[0, 1]),
                lambda: sp.superpose(p, out=torch.zeros(3, 5, 3, dtype=torch.float64)), lambda: sp.rmsf(p, atom_indices=[-1])):
        with pytest.raises(ValueError):
            bad()


# ---- the C ABI ----
def test_symbols_in_header_binding_and_export_map():
    from lam_slide_amd import _lib
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    declared = set(re.findall(r"\b(lsl_[a-z_]+)\s*\(", header))
    pattern = re.search(r"global:\s*(\S+);", open(os.path.join(_lib.SRC_DIR, "exports.map")).read()).group(1)
    assert pattern == "lsl_*"
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTED and s.startswith(pattern[:-1]) and hasattr(lib, s)
    assert re.search(r"6, later still: lsl_superpose, lsl_atom_rmsf_workspace_bytes, lsl_atom_rmsf added the same way", header)
    assert int(re.search(r"#define LSL_SUP_CENTER_ONLY (\d+)", header).group(1)) == 1
    from lam_slide_amd import superpose as sp
    kernels = open(os.path.join(_lib.SRC_DIR, "k_superpose.hip.h")).read()
    assert int(re.search(r"#define LSL_RMSF_SEG (\d+)", kernels).group(1)) == sp.RMSF_SEG == orc.RMSF_SEG and sp.MAX_A == orc.MAX_A


def test_entry_points_refuse_before_touching_the_device():
    from lam_slide_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.float32)  # (host memory: a refused call dereferences nothing but sel_host)
    pos = buf.ctypes.data
    sel = np.array([0, 2, 1], dtype=np.int32)
    sp_ = sel.ctypes.data

    def fit(pos=pos, ref=pos + 8192, ref_frames=1, sel=sp_, sel_host=sp_, n_sel=3, fixed=None, F=2, A=5, flags=0, out=None, rmsd=None, rot=None, trans=None):
        return lib.lsl_superpose(pos, ref, ref_frames, sel, sel_host, n_sel, fixed, F, A, flags, out, rmsd, rot, trans, None), lib.lsl_last_error().decode()

    assert fit() == (0, fit()[1])  # every output NULL: nothing to do, no launch
    assert fit(flags=1, ref=None)[0] == 0
    assert fit(pos=None)[0] == -1 and fit(ref=None)[0] == -1 and fit(sel_host=None)[0] == -1
    for kw, word in ((dict(A=0), "A = 0"), (dict(A=2045), "A = 2045"), (dict(n_sel=0), "n_sel = 0"), (dict(ref_frames=2, F=3), "ref_frames = 2"),
                     (dict(sel=None, sel_host=None, n_sel=3), "n_sel = 3"), (dict(F=0), "F = 0"), (dict(flags=2), "flags = 2"),
                     (dict(flags=1, rmsd=pos), "LSL_SUP_CENTER_ONLY"),
                     (dict(out=pos + 8192 + 60 - 4), "overlaps"),  # out starts on the reference's last float
                     (dict(out=pos + 8192 - 120 + 4), "overlaps"),  # out's last float (F = 2 frames of 60 bytes) is the reference's first
                     (dict(out=pos, ref=pos + 120 - 4, ref_frames=2), "overlaps")):  # a per-frame reference
        rc, msg = fit(**kw)
        assert rc == -3 and word in msg, (kw, rc, msg)
    sel[1] = 5
    rc, msg = fit()
    assert rc == -3 and "sel[1] = 5 outside the frame's atoms 0..4" in msg
    with pytest.raises(ValueError):
        _lib.check(rc)

    nbytes = lib.lsl_atom_rmsf_workspace_bytes
    assert nbytes(1, 1) == 2 * 3 * 8 and nbytes(128, 7) == 2 * 21 * 8 and nbytes(129, 7) == 4 * 21 * 8 and nbytes(0, 7) == 0 and nbytes(5, 0) == 0
    rmsf = lambda pos=pos, F=300, A=7, mean=None, out=None, ws=pos, n=nbytes(300, 7): (  # noqa: E731
        lib.lsl_atom_rmsf(pos, F, A, mean, out, ws, n, None), lib.lsl_last_error().decode())
    assert rmsf()[0] == 0  # (both outputs NULL)
    assert rmsf(pos=None)[0] == -1 and rmsf(ws=None)[0] == -1
    assert rmsf(A=0)[0] == -3 and "A = 0" in rmsf(A=0)[1] and rmsf(F=0)[0] == -3 and rmsf(F=65535 * 128 + 1)[0] == -3
    rc, msg = rmsf(n=nbytes(300, 7) - 1, out=pos)
    assert rc == -4 and "workspace too small" in msg
