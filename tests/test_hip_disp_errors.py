"""GPU tests of the displacement errors on the device (``lsl_disp_error_rows`` / ``lsl_disp_error_final`` behind ``displacement_rows``,
``displacement_errors``, ``best_of_k_errors(fused=True)`` and ``SecondStageSampler.validation_errors``): the reference's own ``test_step``
results (fixtures F11, F14), edge shapes against the float64 restatement, determinism bit for bit, masks, NaN, refusals.

Bars are derived, not measured.  Every term is non-negative and fp32 subtraction, sqrt and division are correctly rounded, so to first
order a ``rows`` value (Tf additions behind a D-term norm, one division) is within ``(Tf + D + 4) * 2^-24`` relative of the float64
evaluation of the same float32 inputs, and a ``traj`` value (a thread's ceil(A / TEAM) agents, six DPP steps, up to three wave additions, one
division behind that) within ``(Tf + D + ceil(A / TEAM) + 14) * 2^-24``.  Against fixture values the allowance is twice the bound: they are
float32 torch results themselves.  Minima and the float64 totals are exact functions of the kernel's own floats and are compared for
equality.  Measured values: profiles/disp_errors_parity.txt."""
import math

import pytest
import torch

from conftest import parity, shape_from

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def rows_bound(Tf, D):
    return (Tf + D + 4) * EPS


def traj_bound(Tf, D, A):
    return (Tf + D + math.ceil(A / (64 if A <= 64 else 256)) + 14) * EPS


def max_rel(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float(((got - want).abs() / want.abs()).max())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                                                                     b.contiguous().view(torch.int32 if b.dtype == torch.float32 else torch.int64))


def abi_rows(pred, target, t0p, t0t, Tf, with_traj=True):
    """lsl_disp_error_rows on device tensors pred [K, B, Tp, A, D] / target [B, Tt, A, D] -> (rows, traj or None)."""
    from lam_slide_amd import _lib
    K, B, Tp, A, D = pred.shape
    assert pred.is_contiguous() and target.is_contiguous() and target.shape[0] == B and tuple(target.shape[2:]) == (A, D)
    rows = torch.empty(K, B, A, 2, device=pred.device)
    traj = torch.empty(K, B, 2, device=pred.device) if with_traj else None
    _lib.check(_lib.load().lsl_disp_error_rows(pred.data_ptr(), target.data_ptr(), K, B, Tp, t0p, target.shape[1], t0t, Tf, A, D, rows.data_ptr(),
                                               None if traj is None else traj.data_ptr(), torch.cuda.current_stream(pred.device).cuda_stream))
    return rows, traj


def abi_final(rows, traj, mask, num_runs):
    """lsl_disp_error_final -> (agents [B, A, 2], totals f64 [5])."""
    from lam_slide_amd import _lib
    K, B, A, _ = rows.shape
    agents = torch.empty(B, A, 2, device=rows.device)
    totals = torch.empty(5, dtype=torch.float64, device=rows.device)
    m8 = None if mask is None else mask.to(torch.uint8).contiguous()
    _lib.check(_lib.load().lsl_disp_error_final(rows.data_ptr(), None if traj is None else traj.data_ptr(), None if m8 is None else m8.data_ptr(), K,
                                                num_runs, B, A, agents.data_ptr(), totals.data_ptr(), torch.cuda.current_stream(rows.device).cuda_stream))
    return agents, totals


def restate64(pred, target, t0p, t0t, Tf):
    """The cited reference lines in float64 on the same float32 inputs (CPU), written out here: frames t0p .. t0p + Tf - 1 of pred
    [K, B, Tp, A, D] against frames t0t .. t0t + Tf - 1 of target [B, Tt, A, D] -> (rows [K, B, A, 2], traj [K, B, 2])."""
    p, t = pred.double().cpu()[:, :, t0p:t0p + Tf], target.double().cpu()[None, :, t0t:t0t + Tf]
    err = torch.norm(t - p, dim=-1)  # [K, B, Tf, A]
    rows = torch.stack((err.mean(dim=2), err[:, :, -1]), dim=-1)                   # _compute_errors' rows before the minimum
    traj = torch.stack((err.mean(dim=(2, 3)), err[:, :, -1].mean(dim=2)), dim=-1)  # validation_step's ade / fde
    return rows, traj


def lane_order_sum(values):
    """Sum of a float64 sequence as k_disp_final adds it: lane l adds items l, l + 64, ... in order, then the lanes in lane order."""
    values = [float(v) for v in values]
    tot = 0.0
    for l in range(64):
        s = 0.0
        for v in values[l::64]:
            s += v
        tot += s
    return tot


def host_totals(agents, traj, mask, R):
    a = agents.cpu().double().reshape(-1, 2)
    keep = torch.ones(a.shape[0], dtype=torch.bool) if mask is None else mask.cpu().reshape(-1) != 0
    t = torch.zeros(0, 2, dtype=torch.float64) if traj is None else traj[:R].cpu().double().reshape(-1, 2)
    return [lane_order_sum(a[keep, 0]), lane_order_sum(a[keep, 1]), float(keep.sum()), lane_order_sum(t[:, 0]), lane_order_sum(t[:, 1])]


def check_against_float64(name, pred, target, t0p, t0t, Tf, mask, runs):
    """rows / traj against float64 within the derived bounds; agents and totals exactly from the kernel's own floats."""
    K, B, Tp, A, D = pred.shape
    rows, traj = abi_rows(pred, target, t0p, t0t, Tf)
    w_rows, w_traj = restate64(pred, target, t0p, t0t, Tf)
    parity(f"{name}.rows", max_rel(rows, w_rows), rows_bound(Tf, D))
    parity(f"{name}.traj", max_rel(traj, w_traj), traj_bound(Tf, D, A))
    if Tf == 1:
        assert same_bits(rows[..., 0], rows[..., 1])
    rows_only, none = abi_rows(pred, target, t0p, t0t, Tf, with_traj=False)  # traj is optional
    assert none is None and same_bits(rows_only, rows)
    for R in runs:
        agents, totals = abi_final(rows, traj, mask, R)
        want = rows[:R].min(dim=0).values
        if mask is not None:
            want = torch.where(mask[..., None] != 0, want, torch.full_like(want, float("nan")))
        assert same_bits(agents.nan_to_num(-1.0), want.nan_to_num(-1.0)), (name, R)
        assert totals.cpu().tolist() == host_totals(agents, traj, mask, R), (name, R)
        _, t0 = abi_final(rows, None, mask, R)
        assert t0[:3].cpu().tolist() == totals[:3].cpu().tolist() and t0[3:].cpu().tolist() == [0.0, 0.0]
    return rows, traj


def f14_layout(f):
    return f["traj"].permute(1, 2, 0, 3)[:, None].contiguous(), f["target"].permute(1, 0, 2)[None].contiguous()


def test_f11_and_f14_through_the_c_abi(golden, dev):
    f = golden("f11_pedestrian_k.npz")
    pred, future, mask = f["positions"].to(dev), f["true_future"].to(dev), f["attention_mask"][:, -1].to(dev)
    K, B, T, A, D = pred.shape
    c1 = T - future.shape[1]
    full = torch.cat([f["pos"][:, :c1].to(dev), future], dim=1).contiguous()
    rows, traj = check_against_float64("f11.abi", pred, full, c1, c1, T - c1, mask, (K,))
    rows2, traj2 = abi_rows(pred, future.contiguous(), c1, 0, T - c1)
    assert same_bits(rows, rows2) and same_bits(traj, traj2)  # the full pos with t0t = cond_idx[1] and the future alone: the same floats
    agents, totals = abi_final(rows, traj, mask, K)
    keep = mask.reshape(-1) != 0
    parity("f11.abi.ade_vs_fixture", max_rel(agents[..., 0].reshape(-1)[keep], f["ades"]), 2 * rows_bound(T - c1, D))
    parity("f11.abi.fde_vs_fixture", max_rel(agents[..., 1].reshape(-1)[keep], f["fdes"]), 2 * rows_bound(T - c1, D))
    assert float(totals[2]) == 9.0
    f = golden("f14_compute_errors.npz")
    pred, target = (x.to(dev) for x in f14_layout(f))
    rows, traj = check_against_float64("f14.abi", pred, target, 0, 0, 12, None, (5,))
    agents, _ = abi_final(rows, traj, None, 5)
    parity("f14.abi.ade_vs_fixture", max_rel(agents[0, :, 0], f["ade"]), 2 * rows_bound(12, 2))
    parity("f14.abi.fde_vs_fixture", max_rel(agents[0, :, 1], f["fde"]), 2 * rows_bound(12, 2))


# (K, B, Tp, t0p, Tt, t0t, Tf, A, D): the smallest shapes at which each mechanism can go wrong
SHAPES = {
    "one_agent": (3, 2, 5, 1, 5, 1, 4, 1, 2),
    "team64_full": (3, 2, 5, 1, 5, 1, 4, 64, 3),            # the last shape of the wave-per-unit form
    "team256_first": (3, 2, 5, 1, 5, 1, 4, 65, 3),          # the first of the workgroup-per-unit form: waves 2 and 3 idle, wave 1 one lane
    "second_agent_per_thread": (2, 2, 4, 0, 4, 0, 4, 257, 2),
    "partial_waves": (2, 2, 4, 1, 3, 0, 3, 300, 4),
    "d1": (4, 3, 6, 2, 6, 2, 4, 11, 1),
    "d2": (4, 3, 6, 2, 6, 2, 4, 11, 2),
    "d3": (4, 3, 6, 2, 6, 2, 4, 11, 3),
    "d4": (4, 3, 6, 2, 6, 2, 4, 11, 4),
    "one_frame": (3, 2, 6, 5, 6, 5, 1, 7, 3),
    "one_frame_team256": (2, 1, 3, 2, 1, 0, 1, 130, 2),
    "one_sample": (1, 3, 8, 3, 8, 3, 5, 9, 2),
    "partial_last_workgroup": (5, 1, 7, 2, 7, 2, 5, 13, 2),  # K * B = 5 units, four to a workgroup
    "offsets_differ": (3, 2, 10, 4, 7, 1, 5, 6, 3),          # Tp != Tt, both offsets non-zero, frames left over behind both windows
    "unrolled_tail": (2, 2, 13, 2, 13, 2, 11, 5, 2),         # Tf = 11: two whole groups of the frame loop's unroll and a tail
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_float64(dev, name):
    K, B, Tp, t0p, Tt, t0t, Tf, A, D = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    pred, target = torch.randn(K, B, Tp, A, D, generator=g).to(dev), torch.randn(B, Tt, A, D, generator=g).to(dev)
    mask = torch.rand(B, A, generator=g) > 0.25
    mask[0, 0] = True
    runs = sorted({1, max(K - 1, 1), K})
    check_against_float64(f"shape.{name}", pred, target, t0p, t0t, Tf, mask.to(dev), runs)
    check_against_float64(f"shape.{name}.nomask", pred, target, t0p, t0t, Tf, None, runs[-1:])


def test_index_past_2_31(dev):
    """K * B * Tp * A * D = 2.16e9 floats: the frames read lie behind element 2^31 of pred.  Only those frames are written; the rest of the
    buffer is never touched."""
    K, B, Tp, A, D, Tf = 2, 1, 66000, 4096, 4, 2
    assert (K * B - 1) * Tp * A * D < 2 ** 31 < ((K * B - 1) * Tp + Tp - Tf) * A * D
    g = torch.Generator().manual_seed(31)
    pred = torch.empty(K, B, Tp, A, D, device=dev)
    tail = torch.randn(K, B, Tf, A, D, generator=g)
    pred[:, :, Tp - Tf:] = tail.to(dev)
    target = torch.randn(B, Tf, A, D, generator=g)
    rows, traj = abi_rows(pred, target.to(dev), Tp - Tf, 0, Tf)
    w_rows, w_traj = restate64(tail, target, 0, 0, Tf)
    parity("past_2_31.rows", max_rel(rows, w_rows), rows_bound(Tf, D))
    parity("past_2_31.traj", max_rel(traj, w_traj), traj_bound(Tf, D, A))
    small, small_traj = abi_rows(tail.to(dev), target.to(dev), 0, 0, Tf)
    assert same_bits(rows, small) and same_bits(traj, small_traj)
    del pred
    torch.cuda.empty_cache()  # (8.6 GB: not kept in the allocator's cache for the rest of the session)


@pytest.mark.parametrize("A", [11, 70])  # both team forms
def test_units_shards_and_totals_bit_for_bit(dev, A):
    from lam_slide_amd import displacement_errors
    K, B, T, D, c1 = 3, 5, 7, 2, 3
    g = torch.Generator().manual_seed(A)
    pred, target = torch.randn(K, B, T, A, D, generator=g).to(dev), torch.randn(B, T, A, D, generator=g).to(dev)
    mask = (torch.rand(B, A, generator=g) > 0.3).to(dev)
    rows, traj = abi_rows(pred, target, c1, c1, T - c1)
    for k in range(K):  # a unit alone (K = B = 1) and inside the batch
        for b in range(B):
            r1, t1 = abi_rows(pred[k:k + 1, b:b + 1].contiguous(), target[b:b + 1].contiguous(), c1, c1, T - c1)
            assert same_bits(r1[0, 0], rows[k, b]) and same_bits(t1[0, 0], traj[k, b]), (k, b)
    whole = displacement_errors(pred, target, mask, first_frame=c1, num_runs=2)
    assert whole.path == "fused" and whole.totals.dtype == torch.float64 and whole.totals.is_cuda
    h = 2
    parts = [displacement_errors(pred[:, :h], target[:h], mask[:h], first_frame=c1, num_runs=2),
             displacement_errors(pred[:, h:], target[h:], mask[h:], first_frame=c1, num_runs=2)]
    for col in ("ade", "fde"):
        cat = torch.cat([getattr(p, col) for p in parts])
        assert same_bits(cat.nan_to_num(-1.0), getattr(whole, col).nan_to_num(-1.0)), col
    assert same_bits(torch.cat([p.traj_ade for p in parts], dim=1), whole.traj_ade)
    added = (parts[0].totals + parts[1].totals).cpu()
    for i in range(5):  # (sums of a few hundred float32 values are exact in float64 as a rule: one rounding is the allowance)
        assert abs(float(added[i]) - float(whole.totals[i])) <= 2.0 ** -52 * abs(float(whole.totals[i])), i
    assert float(added[2]) == float(mask.sum())
    a, f = whole.real()
    assert a.shape == (int(mask.sum()),) and same_bits(a, whole.ade[mask]) and same_bits(f, whole.fde[mask])


def test_masks_nan_and_the_meter(dev):
    from lam_slide_amd import DisplacementMeter, displacement_errors
    K, B, T, A, D, c1 = 4, 3, 6, 5, 2, 2
    g = torch.Generator().manual_seed(9)
    pred, target = torch.randn(K, B, T, A, D, generator=g).to(dev), torch.randn(B, T - c1, A, D, generator=g).to(dev)
    mask = torch.rand(B, A, generator=g) > 0.3
    mask[1] = False  # one trajectory fully masked
    mask[0, 0] = mask[2, 4] = True
    mask = mask.to(dev)
    clean = displacement_errors(pred, target, mask, first_frame=c1)
    assert clean.path == "fused" and torch.equal(torch.isnan(clean.ade), ~mask) and torch.equal(torch.isnan(clean.fde), ~mask)
    assert float(clean.totals[2]) == float(mask.sum())
    for m in (mask.long(), mask.float() * 3.0, mask.to(torch.uint8)):  # nonzero = real agent
        assert same_bits(displacement_errors(pred, target, m, first_frame=c1).totals, clean.totals)
    cpu = displacement_errors(pred.cpu(), target.cpu(), mask.cpu(), first_frame=c1)  # the restatement: same outputs, same conventions
    assert cpu.path == "torch" and torch.equal(torch.isnan(cpu.ade), torch.isnan(clean.ade.cpu()))
    parity("module.ade_vs_restatement", max_rel(clean.real()[0], cpu.real()[0]), 2 * rows_bound(T - c1, D))
    parity("module.traj_vs_restatement", max_rel(clean.traj_ade, cpu.traj_ade), traj_bound(T - c1, D, A) + ((T - c1) * A + D + 4) * EPS)
    # everything masked: totals (0, 0, 0), the meter's agent means are NaN
    none = displacement_errors(pred, target, torch.zeros(B, A, dtype=torch.bool, device=dev), first_frame=c1)
    assert none.totals[:3].cpu().tolist() == [0.0, 0.0, 0.0] and bool(torch.isnan(none.ade).all()) and none.real()[0].numel() == 0
    meter = DisplacementMeter(scale=2.0)
    meter.update(none)
    out = meter.compute()
    assert math.isnan(out["ade"]) and math.isnan(out["fde"]) and out["traj_ade"] == 2.0 * float(none.totals[3]) / (K * B)
    meter.update(clean)
    meter.update(clean)
    out = meter.compute()
    assert meter.sums.is_cuda and out["ade"] == 2.0 * (2 * float(clean.totals[0])) / (2 * float(clean.totals[2]))
    # a NaN in one sample of one agent: that agent's minimum is NaN, every other agent keeps its bits
    bad = pred.clone()
    bad[2, 0, T - 1, 0, 1] = float("nan")
    r = displacement_errors(bad, target, mask, first_frame=c1)
    assert bool(torch.isnan(r.ade[0, 0])) and bool(torch.isnan(r.fde[0, 0])) and bool(torch.isnan(r.totals[0]))
    keep = torch.ones(B, A, dtype=torch.bool, device=dev)
    keep[0, 0] = False
    assert same_bits(r.ade[keep].nan_to_num(-1.0), clean.ade[keep].nan_to_num(-1.0))
    assert same_bits(r.fde[keep].nan_to_num(-1.0), clean.fde[keep].nan_to_num(-1.0))
    assert same_bits(displacement_errors(bad, target, mask, first_frame=c1, num_runs=2).ade.nan_to_num(-1.0),
                     displacement_errors(pred, target, mask, first_frame=c1, num_runs=2).ade.nan_to_num(-1.0))  # sample 2 is not looked at
    first = pred.clone()
    first[0, 0, c1, 0, 0] = float("nan")  # in sample 0 and in a middle frame: the ADE only, and later samples do not undo it
    r = displacement_errors(first, target, mask, first_frame=c1)
    assert bool(torch.isnan(r.ade[0, 0])) and same_bits(r.fde.nan_to_num(-1.0), clean.fde.nan_to_num(-1.0))


def test_refusals_leave_the_buffers_alone_and_the_module_takes_the_torch_path(dev):
    from lam_slide_amd import _lib, displacement_errors
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    K, B, T, A = 3, 2, 4, 5
    g = torch.Generator().manual_seed(5)
    pred, target = torch.randn(K, B, T, A, 5, generator=g).to(dev), torch.randn(B, T, A, 5, generator=g).to(dev)
    rows, traj = torch.full((K, B, A, 2), 7.0, device=dev), torch.full((K, B, 2), 7.0, device=dev)
    agents, totals = torch.full((B, A, 2), 7.0, device=dev), torch.full((5,), 7.0, dtype=torch.float64, device=dev)
    p, t, r, tr, ag, to = (x.data_ptr() for x in (pred, target, rows, traj, agents, totals))
    assert lib.lsl_disp_error_rows(p, t, K, B, T, 0, T, 0, T, A, 5, r, tr, st) == -3 and b"D = 5" in lib.lsl_last_error()
    assert lib.lsl_disp_error_rows(p, t, K, B, T, 0, T, 0, 0, A, 4, r, tr, st) == -3
    assert lib.lsl_disp_error_rows(p, t, K, B, T, 1, T, 0, T, A, 4, r, tr, st) == -3  # frames 1 .. T of T
    assert lib.lsl_disp_error_rows(None, t, K, B, T, 0, T, 0, T, A, 4, r, tr, st) == -1
    assert lib.lsl_disp_error_final(r, tr, None, K, 0, B, A, ag, to, st) == -3
    assert lib.lsl_disp_error_final(r, tr, None, K, K + 1, B, A, ag, to, st) == -3
    assert lib.lsl_disp_error_final(r, tr, None, K, K, B, A, None, to, st) == -1
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in (rows, traj, agents, totals))
    mask = (torch.rand(B, A, generator=g) > 0.3).to(dev)
    assert bool(mask.any())
    got = displacement_errors(pred, target, mask, first_frame=1, num_runs=2)  # D = 5: outside the native form
    want = displacement_errors(pred.double().cpu(), target.double().cpu(), mask.cpu(), first_frame=1, num_runs=2)
    assert got.path == want.path == "torch" and got.ade.is_cuda and got.totals.dtype == torch.float64
    assert torch.equal(torch.isnan(got.ade).cpu(), torch.isnan(want.ade))
    bar = (3 * A + 5 + 4) * EPS  # torch's own float32 order: the sequential worst case over a trajectory's terms
    assert max_rel(got.real()[0], want.real()[0]) <= bar and max_rel(got.real()[1], want.real()[1]) <= bar
    assert max_rel(got.traj_ade, want.traj_ade) <= bar and max_rel(got.totals, want.totals) <= bar
    half = displacement_errors(pred[..., :4].half(), target[..., :4].half())  # another dtype: the torch path too
    assert half.path == "torch" and half.ade.dtype == torch.float16


def build_net(sh, params, dev):
    from lam_slide_amd import LatentSIV3
    net = LatentSIV3(depth=sh.depth, in_dim=sh.in_dim, hidden_size=sh.hidden_size, num_heads=sh.num_heads, vec_in_dim=sh.vec_in_dim,
                     mlp_ratio=sh.mlp_ratio, theta=sh.theta, normalize=sh.normalize, reset_parameters=False)
    net.load_state_dict(params)
    net = net.to(dev).requires_grad_(False)
    net.ensure_packed(dev)
    return net


def test_best_of_k_errors_fused_and_validation_errors_on_the_f11_chain(golden, dev):
    """The seeded backbone and stage 1 of F11 (pedestrian shape: T = 20, L = 2, A = 4, K = 20) with the fixture's initial noises: the
    fused tail against the torch chain on the same decoded bits, and ``validation_errors`` against the quoted lines in float64."""
    from lam_slide_amd import CreateTransport, SecondStageSampler, Stage1Decoder, Stage1Encoder, best_of_k_errors
    from oracle import latent_net
    f = golden("f11_pedestrian_k.npz")
    B, T, A, L, K, c0, c1, n = (int(v) for v in f["meta"])
    sh = shape_from(f.group("shape"))
    net = build_net(sh, latent_net.random_params(sh, seed=int(f["weight_seed"])), dev)
    s1 = f.group("stage1")
    enc = Stage1Encoder(s1, num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
    dec = Stage1Decoder(s1, num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)
    flat = lambda t: t.reshape(-1, *t.shape[2:])  # noqa: E731
    pos = f["pos"].clone()
    pos[:, c1:] = 0
    lat = enc.encode(flat(pos @ f["lift"]).to(dev), flat(f["entities"]).to(dev), flat(f["attention_mask"]).to(dev)).reshape(B, T, L, 32)
    y = f["embedding"].to(dev)[f["cond_scene"].long().to(dev)]
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(c0, c1), mask_cond_mean=True,
                             sampling_kwargs={"sampling_method": "euler", "num_steps": n})
    ent = flat(f["entities"]).to(dev)
    seen = []

    def decode(z):  # [N, T, L, C] -> [N, T, A, 3]
        p = dec.decode(z.reshape(-1, L, 32), ent.repeat(z.shape[0] // B, 1)).reshape(z.shape[0], T, A, 3)
        seen.append(p)
        return p

    future, amask, inits = f["true_future"].to(dev), f["attention_mask"][:, -1].to(dev), f["noises"].to(dev)
    for runs in (7, K):
        want = best_of_k_errors(drv, lat, future, K, decode, agent_mask=amask, y=y, inits=inits, num_runs=runs)
        got = best_of_k_errors(drv, lat, future, K, decode, agent_mask=amask, y=y, inits=inits, num_runs=runs, fused=True)
        assert same_bits(seen[-1], seen[-2])  # both tails saw the same decoded positions
        assert got[0].shape == want[0].shape == (9,) and got[0].is_cuda
        parity(f"f11.fused_vs_torch.ade.runs{runs}", max_rel(got[0], want[0]), 2 * rows_bound(T - c1, 3))
        parity(f"f11.fused_vs_torch.fde.runs{runs}", max_rel(got[1], want[1]), 2 * rows_bound(T - c1, 3))
    # (num_runs = K = 20 is what the fixture's test_step ran: the bar of test_hip_parity's F11 test, the network's error included)
    parity("f11.fused.ade_vs_fixture", float((got[0].double().cpu() - f["ades"].double()).norm() / f["ades"].double().norm()), 5e-4)
    parity("f11.fused.fde_vs_fixture", float((got[1].double().cpu() - f["fdes"].double()).norm() / f["fdes"].double().norm()), 5e-4)
    # validation_step on one sample: the batch's full pos, read from frame c1 on
    full = torch.cat([f["pos"][:, :c1], f["true_future"]], dim=1).to(dev)
    ade, fde = drv.validation_errors(lat, full, decode, y=y, init=inits[0])
    p64, t64 = seen[-1].double().cpu()[:, c1:], full.double().cpu()[:, c1:]
    want_a, want_f = torch.norm(t64 - p64, dim=-1).mean(dim=(1, 2)), torch.norm(t64[:, -1] - p64[:, -1], dim=-1).mean(dim=1)
    assert ade.shape == fde.shape == (B,) and ade.is_cuda
    parity("f11.validation_errors.ade", max_rel(ade, want_a), traj_bound(T - c1, 3, A))
    parity("f11.validation_errors.fde", max_rel(fde, want_f), traj_bound(T - c1, 3, A))
