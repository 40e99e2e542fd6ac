"""GPU tests of the geometry losses on the device (``lsl_geom_loss_sums`` / ``lsl_geom_loss_final`` behind ``geom_losses``, ``Loss`` and
``SecondStageSampler.validation_losses``): the reference's own loss classes on seeded inputs (fixture F17), determinism, edge shapes against
a float64 restatement, and the reference's real md17 ``model_step`` (fixture F16) end to end.

Bars.  A reduction alone: 1e-5 relative, the project's bar (tests/test_si_loss.py); the reference's fp32 classes deviate from their own
fp64 run by less than 1e-6 over the F17 cases.  End to end the losses get no bar of their own that the network's bf16 error could hide a
reduction bug under.  With delta the MEASURED deviation of the decoded positions from the oracle's decode of the fixture's ``pred``, m the
mask and n_f the real entities of frame f, the triangle inequality gives
    |sqrt(pos) - sqrt(pos_ref)|     <= ||m o delta|| / sqrt(D sum m)
    |dist - dist_ref|               <= sum_a m_a ||delta_a|| / sum m
    |sqrt(inter) - sqrt(inter_ref)| <= sqrt(sum_ij m_i m_j (||delta_i|| + ||delta_j||)^2 / sum_f n_f^2)
(||p_i - p_j|| moves by at most ||delta_i|| + ||delta_j||), each plus the 1e-5 reduction term.  One looser bar, 1e-4, stands in
``test_native_limits`` for A = 2049: that shape is outside the native form, so ``Loss`` runs torch's own fp32 ``cdist`` there, which takes
its matmul form above 25 entities (d^2 = |x|^2 + |y|^2 - 2 x.y: an absolute error of a few ulp of |x|^2 + |y|^2 in every d^2); the check is
that the generic path ran and computes the same quantity, not a statement about a kernel of this package.  Measured values, as
far as they exist: profiles/geom_loss_parity.txt."""
import pytest
import torch
from torch import nn

from conftest import parity, rel_l2

pytestmark = pytest.mark.gpu

KEYS = ("pos_loss", "dist", "inter_dist_loss")  # the order of F17's ref32 / ref64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def restate64(pred, target, mask):
    """The three losses in float64 from coordinate differences: [F, A, D] x 2, [F, A] -> (pos_loss, dist, inter_dist_loss)."""
    p, t, m = pred.double().cpu(), target.double().cpu(), (mask.cpu() != 0).double()
    sq = ((p - t) ** 2).sum(dim=-1)
    pos, dist = (sq / p.shape[-1] * m).sum() / m.sum(), (sq.sqrt() * m).sum() / m.sum()
    pair = m[:, :, None] * m[:, None, :]
    dp = torch.cdist(p, p, compute_mode="donot_use_mm_for_euclid_dist")
    dt = torch.cdist(t, t, compute_mode="donot_use_mm_for_euclid_dist")
    return pos, dist, (((dp - dt) ** 2) * pair).sum() / pair.sum()


def test_f17_cases_against_the_reference_classes(golden, dev):
    from lam_slide_amd import geom_losses
    f = golden("f17_geom_losses.npz")
    names = [str(n) for n in f.raw["names"]]
    assert len(names) == 9
    for name in names:
        c = f.group(name)
        got = geom_losses(c["pred"].to(dev), c["target"].to(dev), c["mask"].to(dev))
        assert set(got) == set(KEYS) and all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in got.values())
        if not bool(c["mask"].any()):
            assert all(bool(torch.isnan(got[k])) for k in KEYS), name  # 0 / 0, as the reference
            continue
        for i, k in enumerate(KEYS):
            parity(f"f17.{name}.{k}", rel(got[k], c["ref64"][i]), 1e-5)


def test_sums_are_batch_and_shard_invariant_bit_for_bit(dev):
    from lam_slide_amd import geom_loss_sums, geom_losses
    for F_, A, D in ((37, 11, 2), (10, 13, 3), (6, 300, 3)):
        g = torch.Generator().manual_seed(F_ * A)
        p, t = (torch.randn(F_, A, D, generator=g).to(dev) for _ in range(2))
        m = (torch.rand(F_, A, generator=g) > 0.25).to(dev)
        whole = geom_loss_sums(p, t, m)
        assert whole.shape == (F_, 5) and whole.dtype == torch.float32 and bool(torch.isfinite(whole).all())
        assert torch.equal(whole[:, 2], m.sum(dim=1).float()) and torch.equal(whole[:, 4], whole[:, 2] ** 2)
        h = F_ // 2
        halves = [geom_loss_sums(p[:h], t[:h], m[:h]), geom_loss_sums(p[h:], t[h:], m[h:])]
        assert torch.equal(torch.cat(halves), whole), (F_, A, D)
        assert torch.equal(geom_loss_sums(p.flip(0), t.flip(0), m.flip(0)).flip(0), whole), (F_, A, D)
        for f in (0, F_ - 1):
            assert torch.equal(geom_loss_sums(p[f:f + 1], t[f:f + 1], m[f:f + 1]), whole[f:f + 1])
        a, b = geom_losses(p, t, m), geom_losses(sums=torch.cat(halves))
        assert all(torch.equal(a[k], b[k]) for k in KEYS)
        # leading axes are flattened: [B, T, A, D] is [(B T), A, D]
        if F_ % 2 == 0:
            c = geom_losses(p.reshape(2, F_ // 2, A, D), t.reshape(2, F_ // 2, A, D), m.reshape(2, F_ // 2, A))
            assert all(torch.equal(a[k], c[k]) for k in KEYS)


@pytest.mark.parametrize("A", [1, 2, 63, 64, 65, 2048])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_edge_shapes_against_float64(dev, A, D):
    from lam_slide_amd import geom_loss_sums, geom_losses
    F_ = 2 if A == 2048 else 5  # (5 frames: the last workgroup of the wave-per-frame form holds one)
    g = torch.Generator().manual_seed(1000 * A + D)
    p, t = (torch.randn(F_, A, D, generator=g) for _ in range(2))
    m = torch.rand(F_, A, generator=g) > 0.25
    m[0] = True  # (at least one real entity, also at A = 1)
    want = restate64(p, t, m)
    got = geom_losses(p.to(dev), t.to(dev), m.to(dev))
    for i, k in enumerate(KEYS):
        if A == 1 and k == "inter_dist_loss":  # one entity: every pair term is the diagonal's exact 0
            assert float(got[k]) == 0.0 and float(want[i]) == 0.0
            continue
        parity(f"edge.A{A}.D{D}.{k}", rel(got[k], want[i]), 1e-5)
    # the mask's dtype does not matter (nonzero = real entity), nor does the layout: a view that is not contiguous is made contiguous
    sums = geom_loss_sums(p.to(dev), t.to(dev), m.to(dev))
    for mm in (m.long(), m.float() * 3.0, m.to(torch.uint8)):
        assert torch.equal(geom_loss_sums(p.to(dev), t.to(dev), mm.to(dev)), sums)
    pt = p.to(dev).permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert tuple(pt.shape) == (F_, A, D) and (D == 1 or not pt.is_contiguous())
    assert torch.equal(geom_loss_sums(pt, t.to(dev), m.to(dev)), sums)


def build_net(sh, params, dev):
    from lam_slide_amd import LatentSIV3
    net = LatentSIV3(depth=sh.depth, in_dim=sh.in_dim, hidden_size=sh.hidden_size, num_heads=sh.num_heads, vec_in_dim=sh.vec_in_dim,
                     mlp_ratio=sh.mlp_ratio, theta=sh.theta, normalize=sh.normalize, reset_parameters=False)
    net.load_state_dict(params)
    net = net.to(dev).requires_grad_(False)
    net.ensure_packed(dev)
    return net


class Module(nn.Module):
    """What the reference's second-stage LightningModule is to ``Loss.forward``: ``si``, ``forward == backbone(x=xt, t=t, **kw)``
    (lightning_base.py:173-174) and ``decode(latents, entities) -> {"pos": [B, T, A, D]}`` (second_stage/md17.py:127-130)."""

    def __init__(self, backbone, si, decoder, T):
        super().__init__()
        self.backbone, self.si, self.decoder, self.T = backbone, si, decoder, T
        self.decoded = None

    def forward(self, xt, t, **model_kwargs):
        return self.backbone(x=xt, t=t, **model_kwargs)

    def decode(self, latents, entities):
        pos = self.decoder.decode(latents, entities)
        self.decoded = pos.reshape(-1, self.T, *pos.shape[1:])
        return {"pos": self.decoded}


def test_native_limits(dev):
    from lam_slide_amd import Loss, ModelType, geom_loss_sums, geom_losses
    g = torch.Generator().manual_seed(7)
    p, t = (torch.randn(1, 2, 2049, 3, generator=g).to(dev) for _ in range(2))
    m = torch.ones(1, 2, 2049, dtype=torch.bool, device=dev)
    with pytest.raises(ValueError, match="2048"):
        geom_losses(p, t, m)
    with pytest.raises(ValueError):
        geom_loss_sums(torch.zeros(2, 5, 5, device=dev), torch.zeros(2, 5, 5, device=dev), torch.ones(2, 5, device=dev))  # D = 5

    class Si:
        model_type = ModelType.DATA

        def training_losses(self, model, x1, model_kwargs=None):
            return {"pred": x1, "loss": torch.ones(1, device=dev)}

    class Fixed:
        si = Si()

        def __init__(self, pos):
            self.pos = pos

        def decode(self, latents, entities):
            return {"pos": self.pos}

    batch = {"x1": torch.zeros(1, 2, 1, 1, device=dev), "model_kwargs": {}, "entities": torch.zeros(1, 2, 2049, dtype=torch.long, device=dev),
             "pos": t, "attention_mask": m}
    loss = Loss(calc_additional_losses=True)
    with torch.no_grad():
        got, _ = loss(Fixed(p), batch)
    assert loss.last_path == "generic"  # 2049 entities: outside the native form, the torch restatements
    want = restate64(p[0], t[0], m[0])
    for i, k in enumerate(KEYS):
        assert rel(got[k], want[i]) < 1e-4, k  # (fp32 torch.cdist in its matmul form)
    # one entity fewer: the device form, same object
    batch2 = dict(batch, pos=t[:, :, :2048], attention_mask=m[:, :, :2048])
    with torch.no_grad():
        got, _ = loss(Fixed(p[:, :, :2048].contiguous()), batch2)
    assert loss.last_path == "fused"
    want = restate64(p[0, :, :2048], t[0, :, :2048], m[0, :, :2048])
    for i, k in enumerate(KEYS):
        parity(f"limits.A2048.{k}", rel(got[k], want[i]), 1e-5)
    # a module the device form does not stand for, or a gradient to carry: generic on the GPU too
    class MaskedHuberLoss(nn.Module):
        def forward(self, input, target, mask):
            return (nn.functional.huber_loss(input, target, reduction="none").mean(dim=1) * mask).sum() / mask.sum()

    other = Loss(loss_pos=MaskedHuberLoss(), calc_additional_losses=True)
    with torch.no_grad():
        other(Fixed(p[:, :, :64].contiguous()), dict(batch, pos=t[:, :, :64], attention_mask=m[:, :, :64]))
    assert other.last_path == "generic"
    with torch.no_grad():  # a float64 target: the torch path promotes as the reference does, nothing is cast down
        got, _ = loss(Fixed(p[:, :, :64].contiguous()), dict(batch, pos=t[:, :, :64].double(), attention_mask=m[:, :, :64]))
    assert loss.last_path == "generic" and got["pos_loss"].dtype == torch.float64
    q = p[:, :, :64].clone().requires_grad_(True)
    with torch.enable_grad():
        got, _ = loss(Fixed(q), dict(batch, pos=t[:, :, :64], attention_mask=m[:, :, :64]))
    assert loss.last_path == "generic" and got["pos_loss"].requires_grad


def test_f16_model_step_end_to_end(golden, dev):
    """F16 = the reference's real md17 ``Wrapper.model_step`` (Loss.forward with calc_additional_losses, weights 1 / 0.25 / 0.25).  The same
    weights, latents and draws through ``lam_slide_amd.Loss`` around the HIP backbone, Transport and Stage1Decoder."""
    from lam_slide_amd import CreateTransport, Loss, SecondStageSampler, Stage1Decoder, setup_conditioning
    from oracle import harness, latent_net
    f, f9 = golden("f16_model_step.npz"), golden("f9_sample.npz")
    B, T, A, D = f["pos"].shape
    L, Cc = f["latents"].shape[2:]
    s1 = dict(f9.group("stage1"))
    s1.update(f.group("stage1_tables"))
    sh = latent_net.NetShape(depth=2, in_dim=32, hidden_size=64, mlp_ratio=2, num_heads=4)
    net = build_net(sh, f9.group("backbone"), dev)
    dec = Stage1Decoder(s1, num_head_latent=2, dim_head_latent=16, num_head_cross=8, dim_head_cross=16)
    tr = CreateTransport("GVP", "data")()
    t, x0 = f["t"].to(dev), f["x0"].to(dev)
    tr.sample = lambda x1: (t, x0, x1)  # the fixture's draws (Loss.forward lets training_losses draw)
    model = Module(net, tr, dec, T)
    lat = f["latents"].to(dev)
    x_cond, mask = setup_conditioning(lat, (0, 2), True)
    assert torch.equal(mask.cpu(), f["mask"]) and rel_l2(x_cond.cpu(), f["x_cond"]) < 2e-6
    pos, att, ent = f["pos"].to(dev), f["attention_mask"].to(dev), f["entities"].to(dev)
    batch = {"x1": lat, "model_kwargs": {"x_cond": x_cond, "x_cond_mask": mask}, "entities": ent, "pos": pos, "attention_mask": att}
    loss = Loss(weight_si_loss=1.0, weight_pos_loss=0.25, weight_inter_dist_loss=0.25, weight_norm_loss=0.0, calc_additional_losses=True)
    with torch.no_grad():
        got, pred_latent = loss(model, batch)
    assert loss.last_path == "fused" and tr.last_path == "fused" and net.last_path == "hip"
    want = f.group("losses")
    assert set(got) == set(want) == {"si_loss", "pos_loss", "inter_dist_loss", "dist", "loss"}
    assert all(bool(torch.isfinite(v)) for v in got.values())
    parity("f16.geom.pred", rel_l2(pred_latent.cpu().reshape(f["pred"].shape), f["pred"]), 5e-4)
    # delta: the decoded positions against the oracle's decode of the fixture's pred
    ref_pos = harness.decode(s1, harness.DecoderShape(), f["pred"].reshape(B * T, L, Cc), f["entities"].reshape(B * T, A)).reshape(B, T, A, D)
    m = f["attention_mask"].double()
    dn = (model.decoded.cpu().double() - ref_pos.double()).norm(dim=-1)  # ||delta_a||  [B, T, A]
    print(f"f16.geom decoded positions rel L2 {rel_l2(model.decoded.cpu(), ref_pos):.3e}, max ||delta_a|| {float(dn.max()):.3e}")
    b_pos = float(((m * dn) ** 2).sum().sqrt() / (D * m.sum()).sqrt())
    b_dist = float((m * dn).sum() / m.sum())
    pair = m[..., :, None] * m[..., None, :]
    b_inter = float(((pair * (dn[..., :, None] + dn[..., None, :]) ** 2).sum() / (m.sum(dim=-1) ** 2).sum()).sqrt())
    root = lambda k: (float(got[k]) ** 0.5, float(want[k]) ** 0.5)  # noqa: E731
    parity(f"f16.geom.sqrt_pos_loss (bound {b_pos:.2e})", abs(root("pos_loss")[0] - root("pos_loss")[1]), b_pos + 1e-5 * root("pos_loss")[1])
    parity(f"f16.geom.dist (bound {b_dist:.2e})", abs(float(got["dist"]) - float(want["dist"])), b_dist + 1e-5 * float(want["dist"]))
    parity(f"f16.geom.sqrt_inter_dist_loss (bound {b_inter:.2e})", abs(root("inter_dist_loss")[0] - root("inter_dist_loss")[1]),
           b_inter + 1e-5 * root("inter_dist_loss")[1])
    # the reduction alone, on the positions the device decoded
    alone = restate64(model.decoded.reshape(B * T, A, D), f["pos"].reshape(B * T, A, D), f["attention_mask"].reshape(B * T, A))
    for i, k in enumerate(KEYS):
        parity(f"f16.geom.reduce.{k}", rel(got[k], alone[i]), 1e-5)
    total = float(got["si_loss"]) + 0.25 * float(got["pos_loss"]) + 0.25 * float(got["inter_dist_loss"])
    assert abs(float(got["loss"]) - total) <= 1e-6 * total
    for k in ("si_loss", "pos_loss", "dist", "inter_dist_loss", "loss"):
        print(f"f16.geom {k}: {float(got[k]):.6f} reference {float(want[k]):.6f}")
    # SecondStageSampler.validation_losses: the same five numbers on the same draws, bit for bit
    drv = SecondStageSampler(net, tr, cond_idx=(0, 2), mask_cond_mean=True)
    before = drv.model_step(lat, t=t, x0=x0)
    val = drv.validation_losses(lat, pos, att, lambda pred: dec.decode(pred.reshape(B * T, L, Cc), ent.reshape(B * T, A)), t=t, x0=x0,
                                weight_si_loss=1.0, weight_pos_loss=0.25, weight_inter_dist_loss=0.25)
    assert set(val) == set(got)
    for k in got:
        assert torch.equal(val[k], got[k]), (k, float(val[k]), float(got[k]))
    assert set(before) == {"loss", "pred"} and torch.equal(before["loss"].mean(), got["si_loss"])  # model_step keeps its result
    plain = drv.validation_losses(lat, pos, att, lambda pred: dec.decode(pred.reshape(B * T, L, Cc), ent.reshape(B * T, A)), t=t, x0=x0)
    assert torch.equal(plain["loss"], plain["si_loss"]) and torch.equal(plain["pos_loss"], got["pos_loss"])  # Loss's default weights: 1, 0, 0
