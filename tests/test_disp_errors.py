"""``lam_slide_amd.metrics`` without a GPU: the torch restatement of the reference's ADE / FDE lines (``validation_step``, the best-of-K
``test_step`` tail, ``on_test_epoch_end``) against what the reference itself returned (fixtures F11 and F14), the result object, the meter,
the dispatch rules, and the C ABI of ``lsl_disp_error_rows`` / ``lsl_disp_error_final`` (symbols, header, refusals before anything touches
a GPU).

Bars are derived, not measured.  Every term is non-negative and fp32 subtraction, sqrt and division are correctly rounded, so to first
order a per-agent value (Tf additions behind a D-term norm) is within ``(Tf + D + 4) * 2^-24`` relative of the float64 evaluation of the
same float32 inputs, and a trajectory mean over A agents within ``(Tf + D + ceil(A / TEAM) + 14) * 2^-24`` in the kernel's order (TEAM =
64 up to 64 agents, 256 above).  Against fixture values the allowance is twice the bound: they are float32 torch results themselves.  The
torch restatement adds a trajectory's Tf * A terms in torch's own order: its bar is the sequential worst case ``(Tf * A + D + 4) * 2^-24``."""
import ctypes as C
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def rows_bound(Tf, D):
    return (Tf + D + 4) * EPS


def traj_bound(Tf, D, A):
    return (Tf + D + math.ceil(A / (64 if A <= 64 else 256)) + 14) * EPS


def max_rel(got, want):
    return float(((got.double() - want.double()).abs() / want.double().abs()).max())


def quoted64(pred, true, c1):
    """The validation_step lines (second_stage/md17.py:82-86) in float64: pred, true [B, T, A, D] -> (ade [B], fde [B])."""
    p, t = pred.double()[:, c1:], true.double()[:, c1:]
    return torch.norm(t - p, dim=-1).mean(dim=(1, 2)), torch.norm(t[:, -1] - p[:, -1], dim=-1).mean(dim=1)


def f14_layout(f):
    """F14 ([N, K, T, D] rows of _compute_errors) as K = 5 samples of B = 1 scene with A = 7 agents, D = 2."""
    return f["traj"].permute(1, 2, 0, 3)[:, None].contiguous(), f["target"].permute(1, 0, 2)[None].contiguous()


def test_restatement_reproduces_the_reference_test_step_f11(golden):
    from lam_slide_amd import displacement_errors
    f = golden("f11_pedestrian_k.npz")
    pred, future, mask = f["positions"], f["true_future"], f["attention_mask"][:, -1]
    K, B, T, A, D = pred.shape
    c1 = T - future.shape[1]
    assert (K, B, T, A, D, c1) == (20, 3, 20, 4, 3, 8) and f["ades"].shape == (9,)
    full = torch.cat([f["pos"][:, :c1], future], dim=1)  # the batch's pos before test_step zeroes its future frames
    a = displacement_errors(pred, full, mask, first_frame=c1)
    b = displacement_errors(pred, future, mask, first_frame=c1)
    assert a.path == b.path == "torch" and a.num_runs == K
    for r in (a, b):
        ade, fde = r.real()
        e_a, e_f = max_rel(ade, f["ades"]), max_rel(fde, f["fdes"])
        print(f"F11 restatement: ade {e_a:.2e} fde {e_f:.2e} allowance {2 * rows_bound(T - c1, D):.2e}")
        assert ade.shape == (9,) and e_a <= 2 * rows_bound(T - c1, D) and e_f <= 2 * rows_bound(T - c1, D)
    assert torch.equal(a.ade.nan_to_num(-1.0), b.ade.nan_to_num(-1.0))  # the two target forms: the same frames
    assert torch.equal(a.fde.nan_to_num(-1.0), b.fde.nan_to_num(-1.0)) and torch.equal(a.totals, b.totals)
    assert a.ade.shape == (B, A) and a.traj_ade.shape == (K, B) and a.totals.dtype == torch.float64 and a.totals.shape == (5,)
    assert float(a.totals[2]) == 9.0 and abs(float(a.totals[0]) - float(f["ades"].double().sum())) <= 2 * rows_bound(T - c1, D) * float(a.totals[0])


def test_restatement_reproduces_the_reference_compute_errors_f14(golden):
    from lam_slide_amd import displacement_errors
    f = golden("f14_compute_errors.npz")
    pred, target = f14_layout(f)
    assert pred.shape == (5, 1, 12, 7, 2) and target.shape == (1, 12, 7, 2)
    r = displacement_errors(pred, target)
    ade, fde = r.real()
    e_a, e_f = max_rel(ade, f["ade"]), max_rel(fde, f["fde"])
    print(f"F14 restatement: ade {e_a:.2e} fde {e_f:.2e} allowance {2 * rows_bound(12, 2):.2e}")
    assert r.agent_mask is None and ade.shape == (7,) and e_a <= 2 * rows_bound(12, 2) and e_f <= 2 * rows_bound(12, 2)
    assert float(r.totals[2]) == 7.0


def test_trajectory_form_is_the_validation_step_lines():
    from lam_slide_amd import displacement_errors, displacement_rows
    g = torch.Generator().manual_seed(4)
    B, T, A, D, c1 = 3, 9, 7, 3, 4
    pred, true = torch.randn(B, T, A, D, generator=g), torch.randn(B, T, A, D, generator=g)
    want_a, want_f = quoted64(pred, true, c1)
    rows, traj = displacement_rows(pred, true, first_frame=c1)  # [B, T, A, D]: K = 1
    assert rows.shape == (1, B, A, 2) and traj.shape == (1, B, 2) and traj.dtype == torch.float32
    bar = ((T - c1) * A + D + 4) * EPS
    assert max_rel(traj[0, :, 0], want_a) <= bar and max_rel(traj[0, :, 1], want_f) <= (A + D + 4) * EPS
    rows64, traj64 = displacement_rows(pred.double(), true.double()[:, c1:], first_frame=c1)  # (the restatement keeps the dtype)
    assert traj64.dtype == torch.float64 and max_rel(traj64[0, :, 0], want_a) < 1e-14 and max_rel(traj64[0, :, 1], want_f) < 1e-14
    # the per-agent rows average to the trajectory values, and Tf = 1 makes ADE the FDE
    assert max_rel(rows64[0].mean(dim=1)[:, 0], want_a) < 1e-14
    r1, t1 = displacement_rows(pred, true, first_frame=T - 1)
    assert torch.equal(r1[..., 0], r1[..., 1]) and max_rel(t1[0, :, 1], want_f) <= (A + D + 4) * EPS
    # md17's test_step (md17.py:157-169): the same two lines per sample; totals[3:] add them over the first num_runs samples
    K = 5
    predk = torch.randn(K, B, T, A, D, generator=g)
    r = displacement_errors(predk, true, first_frame=c1, num_runs=3)
    per_k = torch.stack([torch.stack(quoted64(predk[k], true, c1)) for k in range(K)])  # [K, 2, B]
    assert max_rel(r.traj_ade, per_k[:, 0]) <= bar and max_rel(r.traj_fde, per_k[:, 1]) <= bar
    assert abs(float(r.totals[3]) - float(per_k[:3, 0].sum())) <= bar * float(per_k[:3, 0].sum()) and r.n_trajectories == 3 * B
    assert abs(float(r.totals[4]) - float(per_k[:3, 1].sum())) <= bar * float(per_k[:3, 1].sum())


def test_restatement_reads_a_window_of_both_tensors():
    """Tp != Tt, both offsets non-zero and frames left over behind both windows (the C ABI's general form): the restatement reads
    Tf frames of each and nothing behind them."""
    from lam_slide_amd import metrics
    g = torch.Generator().manual_seed(6)
    K, B, Tp, t0p, Tt, t0t, Tf, A, D = 3, 2, 10, 4, 7, 1, 5, 6, 3
    pred, target = torch.randn(K, B, Tp, A, D, generator=g).double(), torch.randn(B, Tt, A, D, generator=g).double()
    rows, traj = metrics._rows_torch(pred, target, t0p, t0t, Tf)
    cut_rows, cut_traj = metrics._rows_torch(pred[:, :, t0p:t0p + Tf], target[:, t0t:t0t + Tf], 0, 0, Tf)
    assert rows.shape == (K, B, A, 2) and traj.shape == (K, B, 2)
    assert torch.equal(rows, cut_rows) and torch.equal(traj, cut_traj)
    for k in range(K):
        want_a, want_f = quoted64(pred[k, :, t0p:t0p + Tf], target[:, t0t:t0t + Tf], 0)
        assert max_rel(traj[k, :, 0], want_a) < 1e-14 and max_rel(traj[k, :, 1], want_f) < 1e-14


def test_minima_are_independent_and_respect_num_runs():
    from lam_slide_amd import displacement_errors
    # one agent, one coordinate, two frames; errors per sample: (|d0|, |d1|)
    target = torch.zeros(1, 2, 1, 1)
    pred = torch.tensor([[1.0, 4.0], [3.0, 1.0], [0.5, 0.5]]).reshape(3, 1, 2, 1, 1)  # ADE 2.5, 2.0, 0.5; FDE 4, 1, 0.5
    r = displacement_errors(pred, target, num_runs=2)
    assert r.num_runs == 2 and float(r.ade) == 2.0 and float(r.fde) == 1.0  # sample 2 is not looked at
    r = displacement_errors(torch.tensor([[1.0, 1.5], [3.0, 1.0], [0.5, 0.5]]).reshape(3, 1, 2, 1, 1), target, num_runs=2)
    assert float(r.ade) == 1.25 and float(r.fde) == 1.0  # ADE from sample 0, FDE from sample 1
    assert float(displacement_errors(pred, target).ade) == 0.5 and float(displacement_errors(pred, target, num_runs=1).fde) == 4.0
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="num_runs"):
            displacement_errors(pred, target, num_runs=bad)


def test_nan_propagates_like_torch_min_and_masked_agents_are_nan():
    from lam_slide_amd import best_of_k_errors, displacement_errors
    g = torch.Generator().manual_seed(9)
    K, B, T, A, D, c1 = 4, 3, 6, 5, 2, 2
    pred, target = torch.randn(K, B, T, A, D, generator=g), torch.randn(B, T - c1, A, D, generator=g)
    mask = torch.rand(B, A, generator=g) > 0.3
    mask[1] = False  # one scene without a real agent
    mask[0, 0] = mask[2, 4] = True
    clean = displacement_errors(pred, target, mask, first_frame=c1)
    assert torch.equal(torch.isnan(clean.ade), ~mask) and torch.equal(torch.isnan(clean.fde), ~mask)
    assert float(clean.totals[2]) == float(mask.sum())
    # .real(): the rows and the order of best_of_k_errors

    class Stub:
        cond_idx = (0, c1)

        def sample_latents_k(self, latents, K, y=None, inits=None):
            return pred

    decode = lambda z: z  # noqa: E731  ("latents" that are positions already)
    want = best_of_k_errors(Stub(), torch.zeros(B, T, 1, 1), target, K, decode, agent_mask=mask)
    got = clean.real()
    assert got[0].shape == want[0].shape == (int(mask.sum()),)
    assert max_rel(got[0], want[0]) <= 2 * rows_bound(T - c1, D) and max_rel(got[1], want[1]) <= 2 * rows_bound(T - c1, D)
    same = best_of_k_errors(Stub(), torch.zeros(B, T, 1, 1), target, K, decode, agent_mask=mask, fused=True)  # CPU: the restatement behind it
    assert torch.equal(same[0], got[0]) and torch.equal(same[1], got[1])
    for runs in (1, 3):
        w = best_of_k_errors(Stub(), torch.zeros(B, T, 1, 1), target, K, decode, agent_mask=mask, num_runs=runs)
        s = best_of_k_errors(Stub(), torch.zeros(B, T, 1, 1), target, K, decode, agent_mask=mask, num_runs=runs, fused=True)
        assert max_rel(s[0], w[0]) <= 2 * rows_bound(T - c1, D) and max_rel(s[1], w[1]) <= 2 * rows_bound(T - c1, D)
    # a NaN in the last frame of sample 2 of agent (0, 0): that agent's two minima are NaN, nobody else's value moves
    bad = pred.clone()
    bad[2, 0, T - 1, 0, 1] = float("nan")
    r = displacement_errors(bad, target, mask, first_frame=c1)
    assert bool(torch.isnan(r.ade[0, 0])) and bool(torch.isnan(r.fde[0, 0])) and bool(torch.isnan(r.totals[0]))
    keep = torch.ones(B, A, dtype=torch.bool)
    keep[0, 0] = False
    assert torch.equal(r.ade[keep].nan_to_num(-1.0), clean.ade[keep].nan_to_num(-1.0))
    assert torch.equal(r.fde[keep].nan_to_num(-1.0), clean.fde[keep].nan_to_num(-1.0))
    # outside num_runs the NaN is not seen; in a middle frame it reaches the ADE only
    assert torch.equal(displacement_errors(bad, target, mask, first_frame=c1, num_runs=2).ade.nan_to_num(-1.0),
                       displacement_errors(pred, target, mask, first_frame=c1, num_runs=2).ade.nan_to_num(-1.0))
    mid = pred.clone()
    mid[1, 0, c1, 0, 0] = float("nan")
    r = displacement_errors(mid, target, mask, first_frame=c1)
    assert bool(torch.isnan(r.ade[0, 0])) and torch.equal(r.fde.nan_to_num(-1.0), clean.fde.nan_to_num(-1.0))
    # a NaN of a masked-out agent reaches nothing but that agent's own (already NaN) entry
    off = pred.clone()
    off[:, 1] = float("nan")
    r = displacement_errors(off, target, mask, first_frame=c1)
    assert torch.equal(r.ade.nan_to_num(-1.0), clean.ade.nan_to_num(-1.0)) and torch.equal(r.totals[:3], clean.totals[:3])
    # the mask's dtype does not matter (nonzero = real agent)
    for m in (mask.long(), mask.float() * 3.0, mask.to(torch.uint8)):
        assert torch.equal(displacement_errors(pred, target, m, first_frame=c1).totals, clean.totals)


def test_meter_arithmetic_and_the_empty_meter():
    from lam_slide_amd import DisplacementMeter, displacement_errors
    empty = DisplacementMeter().compute()
    assert set(empty) == {"ade", "fde", "traj_ade", "traj_fde"} and all(math.isnan(v) for v in empty.values())
    g = torch.Generator().manual_seed(12)
    meter, scale = DisplacementMeter(scale=2.5), 2.5
    ades, fdes, tas, tfs = [], [], [], []
    for B, runs in ((2, 3), (5, 4), (1, 1)):  # batches of different sizes: the means weigh agents and trajectories, not batches
        K, T, A, D, c1 = 4, 5, 6, 2, 2
        pred, true = torch.randn(K, B, T, A, D, generator=g), torch.randn(B, T, A, D, generator=g)
        mask = torch.rand(B, A, generator=g) > 0.4
        r = displacement_errors(pred, true, mask, first_frame=c1, num_runs=runs)
        meter.update(r)
        a, f = r.real()
        ades.append(a.double()), fdes.append(f.double())
        tas.append(r.traj_ade[:runs].double().reshape(-1)), tfs.append(r.traj_fde[:runs].double().reshape(-1))
    got = meter.compute()
    want = {"ade": torch.cat(ades).mean(), "fde": torch.cat(fdes).mean(), "traj_ade": torch.cat(tas).mean(), "traj_fde": torch.cat(tfs).mean()}
    for k in want:
        assert isinstance(got[k], float) and abs(got[k] - scale * float(want[k])) <= 1e-14 * abs(got[k]), k
    assert meter.n_trajectories == 2 * 3 + 5 * 4 + 1 and float(meter.sums[2]) == sum(len(a) for a in ades)
    # everything masked: the agent means are 0 / 0, the trajectory means (unmasked, as the reference) are not
    m2 = DisplacementMeter()
    r = displacement_errors(pred, true, torch.zeros(1, 6, dtype=torch.bool), first_frame=2)
    assert r.totals[:3].tolist() == [0.0, 0.0, 0.0] and r.real()[0].numel() == 0
    m2.update(r)
    out = m2.compute()
    assert math.isnan(out["ade"]) and math.isnan(out["fde"]) and out["traj_ade"] > 0
    m2.reset()
    assert math.isnan(m2.compute()["traj_ade"])


def test_dispatch_rules_and_argument_checks():
    from lam_slide_amd import displacement_errors, displacement_rows, metrics
    p4, t4 = torch.zeros(2, 3, 6, 5, 4), torch.ones(3, 6, 5, 4)
    assert not metrics.fused_applies(p4, t4)  # CPU tensors
    assert metrics.native_shape(1) and metrics.native_shape(4) and not metrics.native_shape(5) and not metrics.native_shape(0)
    r = displacement_errors(p4, t4)
    assert r.path == "torch" and float(r.ade[0, 0]) == 2.0  # ||(1, 1, 1, 1)||
    p5, t5 = torch.zeros(2, 3, 6, 5, 5), torch.ones(3, 6, 5, 5)
    r = displacement_errors(p5, t5, first_frame=2)
    assert r.path == "torch" and abs(float(r.fde[2, 4]) - 5 ** 0.5) < 1e-6 and r.traj_fde.shape == (2, 3)
    with pytest.raises(ValueError, match="first_frame"):
        displacement_rows(p4, t4, first_frame=6)
    with pytest.raises(ValueError, match="neither"):
        displacement_rows(p4, torch.ones(3, 5, 5, 4), first_frame=2)  # 5 frames: neither T = 6 nor T - first_frame = 4
    with pytest.raises(ValueError, match="neither"):
        displacement_rows(p4, torch.ones(2, 6, 5, 4))
    with pytest.raises(ValueError, match="expected pred"):
        displacement_rows(torch.zeros(6, 5, 4), t4)
    with pytest.raises(ValueError, match="agent_mask"):
        displacement_errors(p4, t4, torch.ones(3, 4))


def test_library_exports_and_header_declare_the_displacement_errors():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    for s in ("lsl_disp_error_rows", "lsl_disp_error_final"):
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
        assert re.fullmatch(r"lsl_[a-z_]+", s)  # (the export test of test_host_logic.py reads the header with this pattern)
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6  # no new ABI number: a stale library is found by the missing symbols
    src = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_disperr.hip.h")).read()
    assert re.search(r"#define LSL_DISP_MAX_D (\d+)", src).group(1) == str(_lib.DISP_MAX_D)
    assert re.search(r"#define LSL_DISP_MAX_UNITS (\d+)LL", src).group(1) == str(_lib.DISP_MAX_UNITS)


def test_entry_points_validate_arguments_without_gpu():
    from lam_slide_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    rows = lambda pred=one, target=one, K=4, B=3, Tp=20, t0p=8, Tt=12, t0t=0, Tf=12, A=5, D=3, out=one, traj=one: \
        lib.lsl_disp_error_rows(pred, target, K, B, Tp, t0p, Tt, t0t, Tf, A, D, out, traj, None)  # noqa: E731
    final = lambda r=one, traj=one, mask=one, K=4, runs=2, B=3, A=5, agents=one, totals=one: \
        lib.lsl_disp_error_final(r, traj, mask, K, runs, B, A, agents, totals, None)  # noqa: E731
    assert rows(pred=None) == -1 and rows(target=None) == -1 and rows(out=None) == -1
    assert final(r=None) == -1 and final(agents=None) == -1 and final(totals=None) == -1
    assert rows(D=5) == -3 and b"D = 5" in lib.lsl_last_error()
    for kw in (dict(D=0), dict(Tf=0), dict(A=0), dict(K=0), dict(B=0), dict(Tf=13), dict(t0p=9), dict(t0t=1), dict(t0p=-1), dict(t0t=-1),
               dict(K=65536, B=65536), dict(K=4096, B=4096)):  # (K * B = 2^24 units: a workgroup each would be 2^32 threads)
        assert rows(**kw) == -3, kw
    assert final(runs=0) == -3 and final(runs=5) == -3 and b"num_runs" in lib.lsl_last_error()
    for kw in (dict(runs=-1), dict(K=0), dict(B=0), dict(A=0)):
        assert final(**kw) == -3, kw
    with pytest.raises(ValueError):
        _lib.check(-3)
