"""GPU tests of rigid superposition on the device (``lsl_superpose`` / ``lsl_atom_rmsf`` behind ``lam_slide_amd.superpose``) against the
numpy float64 oracle of tests/superpose_oracle.py (Kabsch by SVD with the determinant fix on the float32 inputs widened to float64).

Shapes: A in {1, 3, 4, 56, 65 (one atom past a wave), 364, 2044}, F in {1, fpb - 1, fpb, fpb + 1, 3 fpb + 2} with fpb = 2048 // A the frames of
one workgroup; the RMSF at F in {1, 127, 128, 129, 259} around its segment of 128 frames.

Bars (derived in the oracle module, not tuned): coordinates 2^-23 of the frame's largest oracle coordinate; rmsd 2^-23 * oracle + 1e-12 m
(m the largest input magnitude of the frame); rot 1e-10, trans 1e-10 m; rmsf and the mean as the rmsd.  Coordinates are compared on every
frame, and every such frame is asserted to have a relative gap of Horn's matrix of at least 1e-3 (the seeded inputs have >= 0.19)."""
import numpy as np
import pytest
import torch

import superpose_oracle as orc
from superpose_oracle import peptide, subset

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
def data(dev):
    """{A: (ref, pos, other, the same three on the device)} at the largest F of that size, each made once and left unchanged."""
    cache = {}

    def get(A):
        if A not in cache:
            F = orc.frame_counts(A)[-1]
            ref, pos = orc.trajectory(A, F, seed=A)
            other = orc.trajectory(A, F, seed=A, variant=1)[1]
            cache[A] = (ref, pos, other) + tuple(torch.from_numpy(a).to(dev) for a in (ref, pos, other))
        return cache[A]

    return get


def same_bits(a, b):
    a, b = a.reshape(-1).contiguous(), b.reshape(-1).contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


# ---- 1. against the oracle ----
@pytest.mark.parametrize("A", orc.SIZES)
def test_superpose_against_the_oracle(dev, data, A):
    from lam_slide_amd import superpose as sp
    ref, pos, other, rd, pd, od = data(A)
    sel = subset(A)
    fixed = np.zeros(A, dtype=np.uint8)
    fixed[::3] = 1
    wants = {"shared": orc.kabsch(pos, ref), "per_frame": orc.kabsch(pos, other), "subset": orc.kabsch(pos, ref, sel),
             "fixed": orc.kabsch(pos, ref, None, fixed)}  # (frames are independent: the first F rows are the oracle of pos[:F])
    worst = 0.0
    for F in orc.frame_counts(A):
        cut = lambda w: {k: v[:F] for k, v in w.items()}  # noqa: E731
        for name, r, kw in (("shared", rd, {}), ("per_frame", od[:F], {}), ("subset", rd, {"atom_indices": sel}), ("fixed", rd, {"fixed": fixed})):
            out, rms, rot, trans = sp.superpose(pd[:F], r, return_rmsd=True, return_transform=True, **kw)
            assert sp.last_path["superpose"] == "fused" and out.dtype == torch.float32 and rms.dtype == torch.float32
            rh = other[:F] if name == "per_frame" else ref
            worst = max(worst, orc.check_fit(cut(wants[name]), pos[:F], rh, *host(out, rms, rot, trans)))
            if name == "fixed":
                assert same_bits(out[:, torch.from_numpy(fixed != 0).to(dev)], pd[:F][:, torch.from_numpy(fixed != 0).to(dev)])
            assert same_bits(sp.rmsd(pd[:F], r, atom_indices=kw.get("atom_indices")), rms) and sp.last_path["rmsd"] == "fused"
        # in place, and reference=None with frame = F - 1 (the reference lies inside out: it is copied first)
        q = pd[:F].clone()
        assert sp.superpose(q, rd, out=q) is q and same_bits(q, sp.superpose(pd[:F], rd))
        q = pd[:F].clone()
        sp.superpose(q, frame=F - 1, out=q)
        worst = max(worst, orc.check_fit(orc.kabsch(pos[:F], pos[F - 1]), pos[:F], pos[F - 1], q.cpu().numpy()))
    print(f"PARITY superpose.A{A} worst error / bar {worst:.3e}")


# ---- 2. proper rotations only ----
@pytest.mark.parametrize("A", (4, 56, 364))
def test_a_mirrored_reference_gets_a_proper_rotation(dev, data, A):
    from lam_slide_amd import superpose as sp
    ref, pos, _, _, pd, _ = data(A)
    mirrored = ref * np.array([1, 1, -1], dtype=np.float32)
    _, rms, rot, _ = sp.superpose(pd, torch.from_numpy(mirrored).to(dev), return_rmsd=True, return_transform=True)
    assert orc.is_proper_rotation(rot.cpu().numpy(), 1e-12)
    orc.check_fit(orc.kabsch(pos, mirrored), pos, mirrored, rmsd=rms.cpu().numpy(), coordinates=False)


# ---- 3. degenerate selections ----
def test_degenerate_selections(dev):
    from lam_slide_amd import superpose as sp
    ref, pos = orc.trajectory(12, 6, seed=3)
    pos[:, 7], ref[7] = pos[:, 4], ref[4]  # atoms 4 and 7 coincide in every frame
    pos[:, 9], ref[9] = 2 * pos[:, 8] - pos[:, 5], 2 * ref[8] - ref[5]  # 5, 8, 9 collinear
    p, r = torch.from_numpy(pos).to(dev), torch.from_numpy(ref).to(dev)
    for sel in ([3], [3, 10], [5, 8, 9], [4, 7]):
        _, rms, rot, _ = sp.superpose(p, r, atom_indices=sel, return_rmsd=True, return_transform=True)
        assert sp.last_path["superpose"] == "fused" and orc.is_proper_rotation(rot.cpu().numpy())
        want = orc.kabsch(pos, ref, sel)
        orc.check_fit(want, pos, ref, rmsd=rms.cpu().numpy(), coordinates=False)
        if sel in ([3], [4, 7]):
            assert np.all(want["zero"]) and bool((rot == torch.eye(3, dtype=torch.float64, device=dev)).all())


# ---- 4. a frame onto itself ----
@pytest.mark.parametrize("A", (3, 65, 2044))
def test_a_frame_onto_itself(dev, data, A):
    from lam_slide_amd import superpose as sp
    _, pos, _, _, pd, _ = data(A)
    F = pos.shape[0]
    for f in (0, F - 1):
        out, rms = sp.superpose(pd, frame=f, return_rmsd=True)
        m = float(np.abs(pos[f]).max())
        assert float(rms[f]) <= 1e-12 * m and float((out[f] - pd[f]).abs().max()) <= 2.0 ** -23 * m


# ---- 5. batch invariance ----
@pytest.mark.parametrize("A", (4, 56, 65, 2044))
def test_a_frame_has_the_same_bits_alone_and_in_any_batch(dev, data, A):
    from lam_slide_amd import superpose as sp
    _, _, _, rd, pd, _ = data(A)
    n = orc.fpb(A)
    F = pd.shape[0]  # 3 fpb + 2
    whole = sp.superpose(pd, rd, return_rmsd=True, return_transform=True)
    for f in sorted({0, n - 1, n, F - 1}):  # both sides of the workgroup boundary
        alone = sp.superpose(pd[f:f + 1], rd, return_rmsd=True, return_transform=True)
        first = sp.superpose(pd[f:], rd, return_rmsd=True, return_transform=True)
        last = sp.superpose(pd[:f + 1], rd, return_rmsd=True, return_transform=True)
        for w, a, b, c in zip(whole[:3], alone[:3], first[:3], last[:3]):  # out, rmsd, rot
            assert same_bits(a[0], w[f]) and same_bits(b[0], w[f]) and same_bits(c[f], w[f])
    again = sp.superpose(pd, rd, return_rmsd=True, return_transform=True)
    assert all(same_bits(a, b) for a, b in zip(whole, again))


# ---- 6. NaN ----
def test_a_nan_frame_gives_nan_for_that_frame_only(dev, data):
    from lam_slide_amd import superpose as sp
    _, _, _, rd, pd, _ = data(56)
    F = pd.shape[0]
    clean = sp.superpose(pd, rd, return_rmsd=True, return_transform=True)
    for f in (0, 37, F - 1):
        bad = pd.clone()
        bad[f, 11, 2] = float("nan")
        got = sp.superpose(bad, rd, return_rmsd=True, return_transform=True)
        torch.cuda.synchronize()  # (the call returns: the sweep count is fixed)
        keep = torch.arange(F, device=dev) != f
        for g, c in zip(got, clean):
            assert bool(torch.isnan(g[f]).all()) and same_bits(g[keep], c[keep])
    bad = rd.clone()
    bad[3, 0] = float("nan")
    assert all(bool(torch.isnan(g).all()) for g in sp.superpose(pd[:5], bad, return_rmsd=True, return_transform=True))


# ---- 7. centring, RMSF, the mean structure ----
@pytest.mark.parametrize("A", (1, 56, 65))
def test_center_and_rmsf_against_numpy(dev, A):
    from lam_slide_amd import superpose as sp
    seg = orc.RMSF_SEG
    _, pos = orc.trajectory(65, 2 * seg + 3, seed=17)
    for F in (1, seg - 1, seg, seg + 1, 2 * seg + 3):
        x32 = np.ascontiguousarray(pos[:F, :A])  # (the first A atoms of one trajectory: an atom must have the same bits at any A)
        p, x = torch.from_numpy(x32).to(dev), x32.astype(np.float64)
        sel = subset(A)
        for idx in (None, sel):
            c = sp.center_coordinates(p, idx)
            assert sp.last_path["center_coordinates"] == "fused" and c.dtype == torch.float32
            want = x - x[:, np.arange(A) if idx is None else idx].mean(axis=1, keepdims=True)
            assert np.all(np.abs(c.cpu().numpy() - want).reshape(F, -1).max(axis=1) <= 2.0 ** -23 * np.abs(want).reshape(F, -1).max(axis=1))
        q = p.clone()
        assert sp.center_coordinates(q, out=q) is q and same_bits(q, sp.center_coordinates(p))
        fl, mean = sp.rmsf(p, return_mean=True)
        assert sp.last_path["rmsf"] == "fused" and fl.dtype == torch.float32 and mean.dtype == torch.float64
        wf, wm = orc.rmsf(x32)
        m = np.abs(x).max(axis=(0, 2))
        assert np.all(np.abs(fl.cpu().numpy() - wf) <= 2.0 ** -23 * wf + 1e-12 * m)
        assert np.all(np.abs(mean.cpu().numpy() - wm) <= 2.0 ** -52 * np.abs(wm) + 1e-12 * m[:, None])
        assert same_bits(sp.rmsf(p, sel), fl[torch.from_numpy(sel).to(dev)])
        full, full_mean = sp.rmsf(torch.from_numpy(pos[:F]).to(dev), return_mean=True)
        assert same_bits(fl, full[:A]) and same_bits(mean, full_mean[:A])


# ---- 8. atom14 positions and the rollout ----
class _Model:
    """A stand-in for the peptide module: ``sample`` turns and shifts the conditioning frame a little more at every time step."""
    shift, scale, n_timesteps = 0.0, 2.0, 5

    def sample(self, batch):
        x = batch["atom14_pos"]  # [1, T, R, 14, 3]
        T = x.shape[1]
        ang = torch.arange(1, T + 1, device=x.device, dtype=x.dtype) * 0.3
        c, s, o, z = torch.cos(ang), torch.sin(ang), torch.ones_like(ang), torch.zeros_like(ang)
        rot = torch.stack([torch.stack([c, -s, z], -1), torch.stack([s, c, z], -1), torch.stack([z, z, o], -1)], -2)  # [T, 3, 3]
        mask = (x != 0).any(dim=-1, keepdim=True)
        y = torch.einsum("tab,otrkb->otrka", rot, x) + 0.01 * torch.sin(7.0 * x) + ang[None, :, None, None, None]
        return {"atom14_pos": y * mask}


def test_atom14_wrappers_and_the_rollout(dev, tables):
    from lam_slide_amd import RolloutSampler, StructureTables, create_trajectory, sample_rollout, superpose, superpose_atom14
    aa, pos14, top = peptide(tables, 9)
    pad = np.ones(56, dtype=bool)
    pad[top] = False
    flat = pos14.reshape(9, 56, 3)
    st = StructureTables(aa, tables)
    pd = torch.from_numpy(pos14).to(dev)
    for frame in (0, 4):
        got, rms = superpose_atom14(pd, st, frame=frame, return_rmsd=True)
        assert superpose.last_path["superpose_atom14"] == "fused" and got.shape == pos14.shape
        g = got.cpu().numpy().reshape(9, 56, 3)
        assert not g[:, pad].any()
        orc.check_fit(orc.kabsch(flat, flat[frame], top, pad), flat, flat[frame], g, rms.cpu().numpy())
        assert same_bits(superpose_atom14(pd, aa, frame=frame, tables=tables), got)
    made = create_trajectory(pd, st)
    assert superpose.last_path["create_trajectory"] == "fused"
    made = made.cpu().numpy().reshape(9, 56, 3)
    x = flat.astype(np.float64)
    centred = x - x[:, top].mean(axis=1, keepdims=True)
    centred[:, pad] = 0.0
    c32 = centred.astype(np.float32)  # (the centring rounds once, the fit once more)
    err = np.abs(made - orc.kabsch(c32, c32[0], top, pad)["out"]).reshape(9, -1).max(axis=1)
    assert not made[:, pad].any() and np.all(err <= 2 * 2.0 ** -23 * np.abs(centred).reshape(9, -1).max(axis=1))

    model, res = _Model(), torch.tensor(aa, device=dev)
    rs = RolloutSampler(model)
    mask = torch.from_numpy(~pad.reshape(4, 14)).to(dev)
    cond = pd[0] * mask[..., None]

    def one(p):  # the parent's sample_rollout, spelled out
        return model.sample(rs.create_batch(pos=p, res=res, res_mask=mask))["atom14_pos"].squeeze(0)

    plain = rs.sample_rollout(cond, res, mask, num_rollouts=2)
    assert same_bits(plain, sample_rollout(one, cond, 2, shift=model.shift, scale=model.scale)) and plain.shape == (10, 4, 14, 3)
    fitted = rs.sample_rollout(cond, res, mask, num_rollouts=2, superpose=True, tables=tables)
    assert same_bits(fitted, superpose_atom14(plain, st, frame=0))
    ph = plain.cpu().numpy().reshape(10, 56, 3)
    orc.check_fit(orc.kabsch(ph, ph[0], top, pad), ph, ph[0], fitted.cpu().numpy().reshape(10, 56, 3))
    assert not fitted.cpu().numpy().reshape(10, 56, 3)[:, pad].any()


# ---- the C ABI on the device ----
def test_null_outputs_and_adjacent_ranges(dev, data):
    from lam_slide_amd import _lib
    _, _, _, rd, pd, _ = data(56)
    lib, st = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    F = 5
    buf = torch.cat([rd.reshape(-1), torch.full((F * 56 * 3,), -7.0, device=dev)])  # the reference, then out right behind it
    out = buf[56 * 3:]
    rc = lib.lsl_superpose(pd.data_ptr(), buf.data_ptr(), 1, None, None, 56, None, F, 56, 0, out.data_ptr(), None, None, None, st)
    assert rc == 0, lib.lsl_last_error()
    from lam_slide_amd import superpose as sp
    assert same_bits(out.reshape(F, 56, 3), sp.superpose(pd[:F], rd))
    rms = torch.empty(F, dtype=torch.float32, device=dev)
    assert lib.lsl_superpose(pd.data_ptr(), rd.data_ptr(), 1, None, None, 56, None, F, 56, 0, None, rms.data_ptr(), None, None, st) == 0
    assert same_bits(rms, sp.rmsd(pd[:F], rd))
    before = buf.clone()
    assert lib.lsl_superpose(pd.data_ptr(), buf.data_ptr(), 1, None, None, 56, None, F, 56, 0, out.data_ptr() - 4, None, None, None, st) == -3
    assert b"overlaps" in lib.lsl_last_error() and same_bits(buf, before)  # (one float into the reference: refused, nothing enqueued)
