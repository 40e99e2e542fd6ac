"""GPU tests of the peptide losses on the device (``lsl_geom_loss_sums`` + ``lsl_peptide_loss_sums`` + ``lsl_peptide_loss_final`` behind
``peptide_losses`` and ``PeptideLoss``): the reference's own ``Loss`` on seeded decoded positions (fixture F18b, fp64 values), determinism,
the limits of the native form, and the reference's real peptide ``model_step`` (F18c) end to end.

Bars, all against the reference's fp64 run.  ``pos_loss``, ``pos_frame_loss``, ``norm_loss``, ``inter_distance_loss``: 1e-5 relative, the
project's bar for a reduction alone (the reference's fp32 classes stay within 1e-6 of their fp64 run on these inputs).  ``torsion_loss``:
``1e-5 |ref| + 1e-6`` - the absolute term because ``1 - cos`` cancels where prediction and target are close.  Shapes: R = 1 and 4 (a wave
per frame, four frames per workgroup; F = 1, 5, 6, 40: part-filled and several workgroups), R = 5, 23, 70, 146 (a workgroup per frame;
R = 5 is the first size of that form, 146 the last the native form takes), R = 147 (refused)."""
import pytest
import torch
from torch import nn

from conftest import parity, rel_l2, shape_from

pytestmark = pytest.mark.gpu

KEYS = ("pos_loss", "pos_frame_loss", "inter_distance_loss", "norm_loss", "torsion_loss")  # the order of F18's ref32 / ref64 (+ cosine at 5)
WEIGHTS = dict(loss_si_weight=1, loss_pos_weight=0.25, loss_pos_frame_weight=0.25, loss_inter_distance_weight=0.25, loss_torsion_weight=0.0,
               loss_norm_weight=0.0)  # configs/model/peptide/second-stage.yaml


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables(golden):
    from lam_slide_amd.peptide_loss import residue_tables
    return residue_tables(golden("f18_peptide_loss.npz").group("tables"))


def check(tag, got, ref):
    """Every loss of ``got`` against the fp64 reference values ``ref`` (in the order of KEYS) at the bars of the module docstring."""
    for i, k in enumerate(KEYS):
        r = float(ref[i])
        if r != r:
            assert bool(torch.isnan(got[k])), (tag, k)  # NaN exactly where the reference has it
            continue
        assert bool(torch.isfinite(got[k])), (tag, k)
        parity(f"{tag}.{k}", abs(float(got[k]) - r), 1e-5 * abs(r) + (1e-6 if k == "torsion_loss" else 0.0))


def args_of(c, dev):
    """(pred, target, target_frame, atom14_mask, tors_target, tors_mask, aatype) of an F18b case on the device."""
    return tuple(c[k].to(dev) for k in ("pred", "target", "target_frame", "atom14_mask", "tors_target", "tors_mask")) + (c["aatype"].long().to(dev),)


def random_args(F_, R, seed, dev, tables):
    """Seeded (pred, target, target_frame, atom14_mask, tors_target, tors_mask, aatype).  Torsions are counted only where the reference's
    own mask counts them: elsewhere (no previous residue, an unknown one in front, a chi the type lacks) the four atoms are degenerate and
    the angle is normalised rounding noise in any precision."""
    from lam_slide_amd.peptide_loss import torsion_mask
    g = torch.Generator().manual_seed(seed)
    pred, target, target_frame = (torch.randn(F_, R, 14, 3, generator=g).to(dev) for _ in range(3))
    ang = torch.rand(F_, R, 7, generator=g) * 6.2831853
    am, drop = torch.rand(F_, R, 14, generator=g) > 0.25, torch.rand(F_, R, 7, generator=g) > 0.3
    aa = torch.randint(0, 21, (F_, R), generator=g)
    tm = drop & (torsion_mask(aa, tables) != 0)
    return (pred, target, target_frame, am.to(dev), torch.stack([ang.sin(), ang.cos()], dim=-1).to(dev), tm.to(dev), aa.to(dev))


def both_sums(a, tables, kind=1):
    from lam_slide_amd import geom_loss_sums, peptide_loss_sums
    pred, target, target_frame, am, tt, tm, aa = a
    A = pred.shape[-3] * 14
    return (geom_loss_sums(pred.reshape(-1, A, 3), target.reshape(-1, A, 3), am.reshape(-1, A)),
            peptide_loss_sums(pred, target_frame, am, tt, tm, aa, kind=kind, residue_tables=tables))


class Named:
    """Parameter-free modules with the names of the reference's (modules/losses.py), restated; the distances from coordinate differences."""

    class MaskedMSELoss(nn.Module):
        def forward(self, input, target, mask):
            return (((input - target) ** 2).mean(dim=1) * mask).sum() / mask.sum()

    class MaskedNormLoss(nn.Module):
        def forward(self, input, target, mask):
            return (torch.norm(input - target, dim=-1) * mask).sum() / mask.sum()

    class InterDistanceLoss(nn.Module):
        def forward(self, preds, targets, mask):
            diag_att = mask.unsqueeze(-1) * mask.unsqueeze(-2)
            cd = lambda x: torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist")  # noqa: E731
            return (((cd(preds) - cd(targets)) * diag_att) ** 2).sum() / diag_att.sum()

    class MaskedCosineLoss(nn.Module):
        def forward(self, preds, targets, mask):
            return ((1 - nn.functional.cosine_similarity(preds, targets, dim=-1)) * mask).sum() / mask.sum()

    class MaskedCosineLossV2(nn.Module):
        def forward(self, preds, targets, mask):
            return ((1 - (preds * targets).sum(dim=-1)) * mask).sum() / mask.sum()

    class MaskedHuberLoss(nn.Module):
        def forward(self, input, target, mask):
            return (nn.functional.huber_loss(input, target, reduction="none").mean(dim=1) * mask).sum() / mask.sum()


def shipped_modules(torsion="MaskedCosineLossV2"):
    return dict(loss_pos=Named.MaskedMSELoss(), loss_pos_frame=Named.MaskedMSELoss(), loss_inter_distance=Named.InterDistanceLoss(),
                loss_torsion=getattr(Named, torsion)(), loss_norm=Named.MaskedNormLoss())


class Fixed:
    """What ``Loss.forward`` touches of the LightningModule, with the SI term and the decoded positions given."""

    def __init__(self, pos):
        from lam_slide_amd import ModelType
        self.pos = pos
        self.si = self
        self.model_type = ModelType.DATA

    def training_losses(self, model, x1, model_kwargs=None):
        return {"pred": x1, "loss": torch.full((1,), 0.5, device=x1.device)}

    def decode(self, latents, entities):
        return {"atom14_pos": self.pos}


def frames_batch(a):
    """One trajectory of F frames: the batch ``PeptideLoss.forward`` reads, from (pred, target, target_frame, atom14_mask, tors_target,
    tors_mask, aatype); -> (model, batch)."""
    pred, target, target_frame, am, tt, tm, aa = a
    F_, R = pred.shape[:2]
    dev = pred.device
    batch = {"x1": torch.zeros(1, F_, 1, 1, device=dev), "model_kwargs": {}, "entities": torch.zeros(1, F_, R, dtype=torch.long, device=dev),
             "attention_mask": torch.ones(1, F_, R, dtype=torch.bool, device=dev), "atom14_pos": target[None], "atom14_pos_frame": target_frame[None],
             "torsions": tt[None], "torsions_mask": tm[None].float(), "aatype": aa[None], "atom14_mask": am[None]}
    return Fixed(pred[None]), batch


def test_f18_cases_against_the_reference_loss(golden, dev, tables):
    from lam_slide_amd import peptide_losses
    f = golden("f18_peptide_loss.npz")
    names = [str(n) for n in f.raw["names"]]
    assert len(names) == 9
    for name in names:
        c = f.group(name)
        a = args_of(c, dev)
        for kind, cols in ((1, (0, 1, 2, 3, 4)), (0, (0, 1, 2, 3, 5))):
            got = peptide_losses(*a, kind=kind, residue_tables=tables)
            assert tuple(got) == KEYS and all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in got.values())
            check(f"f18.{name}.kind{kind}", got, c["ref64"][list(cols)])
        assert bool(torch.isnan(got["torsion_loss"])) == (name == "tors_masked_f4_r4")


@pytest.mark.parametrize("R", [1, 4, 5, 23])
def test_sums_are_batch_and_shard_invariant_bit_for_bit(dev, tables, R):
    from lam_slide_amd import peptide_losses
    a = random_args(9, R, 40 + R, dev, tables)
    geom, pept = both_sums(a, tables)
    assert geom.shape == (9, 5) and pept.shape == (9, 4) and pept.dtype == torch.float32 and bool(torch.isfinite(pept).all())
    assert torch.equal(pept[:, 1], a[3].sum(dim=(1, 2)).float()) and torch.equal(pept[:, 1], geom[:, 2])
    aa = a[6]
    counted = a[5].clone()
    assert torch.equal(pept[:, 3], counted.sum(dim=(1, 2)).float())
    # frame 3 alone, and inside batches of 2, 5 and 9 frames at other positions
    sel = lambda idx: tuple(x[idx] for x in a)  # noqa: E731
    for idx, at in (([3], 0), ([3, 0], 0), ([7, 3], 1), ([8, 1, 3, 0, 2], 2), ([0, 1, 2, 4, 3], 4), ([8, 7, 6, 5, 4, 3, 2, 1, 0], 5)):
        g2, p2 = both_sums(sel(idx), tables)
        assert torch.equal(p2[at], pept[3]) and torch.equal(g2[at], geom[3]), (R, idx)
    # shards concatenated before the final against one call
    halves = [both_sums(sel(slice(0, 4)), tables), both_sums(sel(slice(4, 9)), tables)]
    cat = (torch.cat([h[0] for h in halves]), torch.cat([h[1] for h in halves]))
    assert torch.equal(cat[0], geom) and torch.equal(cat[1], pept)
    one, sharded = peptide_losses(*a, residue_tables=tables), peptide_losses(sums=cat)
    assert all(torch.equal(one[k], sharded[k]) for k in KEYS) and all(bool(torch.isfinite(v)) for v in one.values())
    # leading axes are flattened, the masks' dtypes do not matter, aatype may be any integer type
    v = tuple(x.reshape(3, 3, *x.shape[1:]) for x in a[:3]) + (a[3].reshape(3, 3, R, 14).long(), a[4].reshape(3, 3, R, 7, 2),
                                                                a[5].reshape(3, 3, R, 7).float() * 2.0, aa.reshape(3, 3, R).to(torch.int32))
    again = peptide_losses(*v, residue_tables=tables)
    assert all(torch.equal(one[k], again[k]) for k in KEYS)


@pytest.mark.parametrize("R", [4, 23])
def test_fused_and_generic_path_agree_on_the_device(golden, dev, tables, R):
    from lam_slide_amd import PeptideLoss
    c = golden("f18_peptide_loss.npz").group({4: "f5_r4", 23: "f9_r23"}[R])
    a = args_of(c, dev)
    for torsion, cols in (("MaskedCosineLossV2", (0, 1, 2, 3, 4)), ("MaskedCosineLoss", (0, 1, 2, 3, 5))):
        loss = PeptideLoss(calc_additional_losses=True, residue_tables=tables, **WEIGHTS, **shipped_modules(torsion))
        model, batch = frames_batch(a)
        with torch.no_grad():
            fused, _ = loss(model, batch)
        assert loss.last_path == "fused"
        check(f"paths.R{R}.{torsion}.fused", fused, c["ref64"][list(cols)])
        total = 0.5 + 0.25 * (float(fused["pos_loss"]) + float(fused["pos_frame_loss"]) + float(fused["inter_distance_loss"]))
        assert abs(float(fused["loss"]) - total) <= 1e-6 * total
        pred = a[0].clone().requires_grad_(True)  # a gradient to carry: the torch geometry
        model, batch = frames_batch((pred,) + a[1:])
        with torch.enable_grad():
            generic, _ = loss(model, batch)
        assert loss.last_path == "generic" and generic["pos_frame_loss"].requires_grad and generic["torsion_loss"].requires_grad
        generic = {k: v.detach() for k, v in generic.items()}
        check(f"paths.R{R}.{torsion}.generic", generic, c["ref64"][list(cols)])
        for k in KEYS:
            parity(f"paths.R{R}.{torsion}.fused_vs_generic.{k}", abs(float(fused[k]) - float(generic[k])),
                   2e-5 * abs(float(generic[k])) + (2e-6 if k == "torsion_loss" else 0.0))  # (each within its bar of the same fp64 value)
    # a module the device form does not stand for, or a float64 target: generic on the GPU too
    other = PeptideLoss(calc_additional_losses=True, residue_tables=tables, **dict(shipped_modules(), loss_pos_frame=Named.MaskedHuberLoss()))
    model, batch = frames_batch(a)
    with torch.no_grad():
        other(model, batch)
        assert other.last_path == "generic"
        got, _ = loss(model, dict(batch, atom14_pos_frame=batch["atom14_pos_frame"].double()))
    assert loss.last_path == "generic" and got["pos_frame_loss"].dtype == torch.float64


def test_native_limits(dev, tables):
    from lam_slide_amd import PeptideLoss, peptide_loss_sums, peptide_losses
    from lam_slide_amd import peptide_loss as pl
    a = random_args(1, 147, 7, dev, tables)
    pred, target, target_frame, am, tt, tm, aa = a
    with pytest.raises(ValueError, match="146"):
        peptide_loss_sums(pred, target_frame, am, tt, tm, aa, residue_tables=tables)
    with pytest.raises(ValueError, match="146"):
        peptide_losses(*a, residue_tables=tables)
    with pytest.raises(ValueError, match="kind"):
        peptide_loss_sums(pred[:, :4], target_frame[:, :4], am[:, :4], tt[:, :4], tm[:, :4], aa[:, :4], kind=2, residue_tables=tables)
    loss = PeptideLoss(calc_additional_losses=True, residue_tables=tables, **WEIGHTS, **shipped_modules())
    assert not pl.native_shape(pred.shape) and pl.native_shape(pred[:, :146].shape)
    model, batch = frames_batch(a)
    with torch.no_grad():
        generic, _ = loss(model, batch)
    assert loss.last_path == "generic"  # 147 residues: outside the native form, the torch geometry
    # one residue fewer: the device form, against the torch geometry in float64 on the same inputs
    b = tuple(x[:, :146].contiguous() for x in a)
    model, batch = frames_batch(b)
    with torch.no_grad():
        fused, _ = loss(model, batch)
    assert loss.last_path == "fused"
    m64, b64 = frames_batch(tuple(x.double().cpu() if x.is_floating_point() else x.cpu() for x in b))
    want, _ = PeptideLoss(calc_additional_losses=True, residue_tables=tables, **WEIGHTS, **shipped_modules())(m64, b64)
    check("limits.R146", fused, [want[k] for k in KEYS])
    assert all(bool(torch.isfinite(generic[k])) for k in KEYS)


@pytest.mark.parametrize("R", [4, 23])
def test_an_aatype_out_of_range_poisons_its_frame_only(dev, tables, R):
    from lam_slide_amd import peptide_losses
    a = random_args(6, R, 90 + R, dev, tables)
    _, clean = both_sums(a, tables)
    for bad_value, frame, residue in ((21, 2, R - 1), (-1, 5, 0), (2 ** 40, 0, R // 2)):
        aa = a[6].clone()
        aa[frame, residue] = bad_value
        geom, pept = both_sums(a[:6] + (aa,), tables)
        assert bool(torch.isnan(pept[frame]).all()), (bad_value, frame)
        keep = [f for f in range(6) if f != frame]
        assert torch.equal(pept[keep], clean[keep]), (bad_value, frame)  # the neighbours' bits are untouched
        got = peptide_losses(sums=(geom, pept))
        assert bool(torch.isnan(got["pos_frame_loss"])) and bool(torch.isnan(got["torsion_loss"])) and bool(torch.isfinite(got["pos_loss"]))


def build_net(sh, params, dev):
    from lam_slide_amd import LatentSIV3
    net = LatentSIV3(depth=sh.depth, in_dim=sh.in_dim, hidden_size=sh.hidden_size, num_heads=sh.num_heads, vec_in_dim=sh.vec_in_dim,
                     mlp_ratio=sh.mlp_ratio, theta=sh.theta, normalize=sh.normalize, reset_parameters=False)
    net.load_state_dict(params)
    net = net.to(dev).requires_grad_(False)
    net.ensure_packed(dev)
    return net


class Module(nn.Module):
    """What the reference's peptide LightningModule is to ``Loss.forward``: ``si``, ``forward == backbone(x=xt, t=t, **kw)``
    (lightning_base.py:173-174) and ``decode(latents, entities) -> {"atom14_pos": [B, T, R, 14, 3]}`` (second_stage/peptide.py:97-102)."""

    def __init__(self, backbone, si, decoder, T):
        super().__init__()
        self.backbone, self.si, self.decoder, self.T = backbone, si, decoder, T
        self.decoded = None

    def forward(self, xt, t, **model_kwargs):
        return self.backbone(x=xt, t=t, **model_kwargs)

    def decode(self, latents, entities):
        pos = self.decoder.decode(latents, entities)
        self.decoded = pos.reshape(-1, self.T, pos.shape[1], 14, 3)
        return {"atom14_pos": self.decoded}


def test_f18c_model_step_end_to_end(golden, dev, tables):
    """F18c = the reference's real peptide ``Wrapper.model_step`` at T = 8 (Loss.forward with the `loss:` block of its YAML).  The same
    weights (F13's first stage and seeded backbone), latents and draws through ``PeptideLoss`` around the HIP backbone, Transport and
    Stage1Decoder."""
    from lam_slide_amd import CreateTransport, PeptideLoss, Stage1Decoder, peptide_losses, setup_conditioning
    from oracle import latent_net
    f, f13 = golden("f18_peptide_loss.npz"), golden("f13_peptide.npz")
    st = f.group("step")
    B, T, R, L, c0, c1 = (int(v) for v in st["meta"][:6])
    sh = shape_from(f13.group("shape"))
    net = build_net(sh, latent_net.random_params(sh, seed=int(f13["weight_seed"])), dev)
    dec = Stage1Decoder(f13.group("stage1"), num_head_latent=2, dim_head_latent=16, num_head_cross=2, dim_head_cross=16, output="atom14_pos")
    tr = CreateTransport("GVP", "data")()
    t, x0 = st["t"].to(dev), st["x0"].to(dev)
    tr.sample = lambda x1: (t, x0, x1)  # the fixture's draws (Loss.forward lets training_losses draw)
    model = Module(net, tr, dec, T)
    lat = st["latents"].to(dev)
    x_cond, mask = setup_conditioning(lat, (c0, c1), True)
    assert torch.equal(mask.cpu(), st["mask"]) and rel_l2(x_cond.cpu(), st["x_cond"]) < 2e-6
    batch = {k: st[k].to(dev) for k in ("entities", "attention_mask", "atom14_pos", "atom14_pos_frame", "torsions", "torsions_mask", "aatype", "atom14_mask")}
    batch.update(x1=lat, model_kwargs={"x_cond": x_cond, "x_cond_mask": mask})
    loss = PeptideLoss(calc_additional_losses=True, residue_tables=tables, **WEIGHTS, **shipped_modules())
    with torch.no_grad():
        got, pred_latent = loss(model, batch)
    assert loss.last_path == "fused" and tr.last_path == "fused" and net.last_path == "hip"
    want = f.group("losses")
    assert set(got) == set(want) == {"si_loss", "loss"} | set(KEYS) and all(bool(torch.isfinite(v)) for v in got.values())
    parity("f18c.pred", rel_l2(pred_latent.cpu().reshape(st["pred"].shape), st["pred"]), 5e-4)
    print(f"f18c decoded positions rel L2 {rel_l2(model.decoded.cpu(), st['decoded']):.3e}")
    for k in ("si_loss", "loss") + KEYS:
        print(f"f18c {k}: {float(got[k]):.6f} reference {float(want[k]):.6f}")
    total = float(got["si_loss"]) + 0.25 * (float(got["pos_loss"]) + float(got["pos_frame_loss"]) + float(got["inter_distance_loss"]))
    assert abs(float(got["loss"]) - total) <= 1e-6 * total
    # the reductions alone: on the fixture's own decoded positions against the reference's fp64 run on them, and the module's five numbers
    # are what peptide_losses gives on the positions the device decoded
    targets = tuple(batch[k].reshape(B * T, *batch[k].shape[2:]) for k in ("atom14_pos", "atom14_pos_frame", "atom14_mask", "torsions", "torsions_mask", "aatype"))
    alone = peptide_losses(st["decoded"].to(dev).reshape(B * T, R, 14, 3), *targets, kind=1, residue_tables=tables)
    check("f18c.reduce", alone, st["decoded_ref64"])
    same = peptide_losses(model.decoded.reshape(B * T, R, 14, 3), *targets, kind=1, residue_tables=tables)
    assert all(torch.equal(same[k], got[k]) for k in KEYS)
