"""``lam_slide_amd.PeptideLoss`` and the peptide geometry without a GPU: the torch restatement (backbone frames, atom37 gather, torsions)
against the reference's own fp64 values per element and against its five losses (fixture F18, tools/make_fixtures.py f18), the generic
path of the ``PeptideLoss`` drop-in against the reference's real peptide ``model_step`` (F18c), the dispatch rules, and the C ABI of
``lsl_peptide_loss_sums`` / ``lsl_peptide_loss_final`` (symbols, header, argument validation before anything touches a GPU).

Bars.  Per element in fp64: 1e-9 absolute on unmasked entries (the values are O(1); both sides round at 1e-16, a torsion whose atoms are
nearly collinear amplifies that, a masked-out one is rounding noise on both sides and is not compared).  Losses: 1e-5 relative, the
project's bar for a reduction alone; the torsion loss gets ``1e-5 |ref| + 1e-6`` because ``1 - cos`` cancels.  The reference's fp32 classes
deviate from their own fp64 run by at most 9.1e-7 over the F18 cases (printed by ``tools/make_fixtures.py f18``)."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch
from torch import nn

from oracle import harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pos_loss", "pos_frame_loss", "inter_distance_loss", "norm_loss", "torsion_loss")  # the order of F18's ref32 / ref64 (+ cosine at 5)
WEIGHTS = dict(loss_si_weight=1, loss_pos_weight=0.25, loss_pos_frame_weight=0.25, loss_inter_distance_weight=0.25, loss_torsion_weight=0.0,
               loss_norm_weight=0.0)  # configs/model/peptide/second-stage.yaml


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def within(k, got, ref):
    """The bar of the issue for loss ``k`` against its fp64 reference value."""
    err = abs(float(got) - float(ref))
    return err < (1e-5 * abs(float(ref)) + 1e-6 if k == "torsion_loss" else 1e-5 * abs(float(ref)))


class RefNamed:
    """Classes with the names of the reference's modules (modules/losses.py), restated."""

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
    return dict(loss_pos=RefNamed.MaskedMSELoss(), loss_pos_frame=RefNamed.MaskedMSELoss(), loss_inter_distance=RefNamed.InterDistanceLoss(),
                loss_torsion=getattr(RefNamed, torsion)(), loss_norm=RefNamed.MaskedNormLoss())


class FixedTransport:
    def __init__(self, pred, loss, model_type=None):
        from lam_slide_amd import ModelType
        self.pred, self.loss = pred, loss
        self.model_type = ModelType.DATA if model_type is None else model_type

    def training_losses(self, model, x1, model_kwargs=None):
        return {"pred": self.pred, "loss": self.loss}


class Model:
    """What ``Loss.forward`` touches of the LightningModule: ``si`` and ``decode(latents, entities) -> {"atom14_pos": [B, T, R, 14, 3]}``
    (second_stage/peptide.py:97-102)."""

    def __init__(self, si, decode):
        self.si, self._decode = si, decode

    def decode(self, latents, entities):
        return {"atom14_pos": self._decode(latents, entities)}


def f18_cases(golden):
    f = golden("f18_peptide_loss.npz")
    for name in (str(n) for n in f.raw["names"]):
        yield name, f.group(name)


def tables_of(golden):
    from lam_slide_amd.peptide_loss import residue_tables
    return residue_tables(golden("f18_peptide_loss.npz").group("tables"))


def frames_model(pred_pos):
    F_ = pred_pos.shape[0]
    return Model(FixedTransport(torch.zeros(1, F_, 1, 1), torch.tensor([0.5])), lambda latents, entities: pred_pos.reshape(1, *pred_pos.shape))


def frames_batch(c, dtype=torch.float32):
    F_, R = c["pred"].shape[:2]
    one = lambda x: x.reshape(1, *x.shape)  # noqa: E731
    return {"x1": torch.zeros(1, F_, 1, 1), "model_kwargs": {}, "entities": torch.zeros(1, F_, R, dtype=torch.long),
            "attention_mask": torch.ones(1, F_, R, dtype=torch.bool), "atom14_pos": one(c["target"]).to(dtype),
            "atom14_pos_frame": one(c["target_frame"]).to(dtype), "torsions": one(c["tors_target"]).to(dtype), "torsions_mask": one(c["tors_mask"]).to(dtype),
            "aatype": one(c["aatype"]).long(), "atom14_mask": one(c["atom14_mask"])}


def test_restatement_matches_the_reference_per_element_in_fp64(golden):
    from lam_slide_amd.peptide_loss import atom37_positions, backbone_local, torsion_angles, torsion_mask
    tables = tables_of(golden)
    assert tables.restab.shape == (21, 20) and tables.restab.dtype.name == "int8" and tables.restab.min() == -1 and tables.restab.max() <= 13
    assert (tables.restab[:20, :4] == [0, 1, 2, 3]).all() and (tables.restab[20] == -1).all()  # N, CA, C, O of the 20 types; unknown: no atom at all
    n = 0
    for name, c in f18_cases(golden):
        p, aa = c["pred"].double(), c["aatype"].long()
        local = backbone_local(p)
        am = c["atom14_mask"]
        e_local = float((local - c["local64"])[am].abs().max())
        tors = torsion_angles(p, aa, tables)
        own = c["own_tors_mask"]
        assert torch.equal(torsion_mask(aa, tables) != 0, own), name  # the mask the dataset stores, restated
        assert not bool((c["tors_mask"] & ~own).any())
        e_tors = float((tors - c["tors64"])[own].abs().max())
        print(f"F18 restatement {name}: frame-local positions {e_local:.2e}, torsions {e_tors:.2e} (max abs, fp64, unmasked)")
        assert e_local < 1e-9 and e_tors < 1e-9, name
        a37 = atom37_positions(p, aa, tables)
        known = aa != 20
        assert a37.shape == p.shape[:2] + (37, 3) and torch.equal(a37[..., :3, :][known], p[..., :3, :][known]) and not bool(a37[~known].any())
        n += 1
    assert n == 9


def test_generic_path_matches_the_reference_losses(golden):
    from lam_slide_amd import PeptideLoss
    tables = tables_of(golden)
    for name, c in f18_cases(golden):
        for dtype in (torch.float32, torch.float64):
            for torsion, col in (("MaskedCosineLossV2", 4), ("MaskedCosineLoss", 5)):
                loss = PeptideLoss(calc_additional_losses=True, residue_tables=tables, **WEIGHTS, **shipped_modules(torsion))
                got, _ = loss(frames_model(c["pred"].to(dtype)), frames_batch(c, dtype))
                assert loss.last_path == "generic" and got["pos_loss"].dtype == dtype
                for i, k in enumerate(KEYS):
                    ref = c["ref64"][col if i == 4 else i]
                    if bool(torch.isnan(ref)):
                        assert name == "tors_masked_f4_r4" and k == "torsion_loss" and bool(torch.isnan(got[k]))
                        continue
                    print(f"F18 generic {name} {dtype} {torsion} {k}: {float(got[k]):.7f} reference {float(ref):.7f} rel {rel(got[k], ref):.2e}")
                    assert within(k, got[k], ref), (name, k)
                if name == "tors_masked_f4_r4":  # 0.0 * NaN: the reference's total is NaN too
                    assert bool(torch.isnan(got["loss"]))
                    continue
                want = 0.5 + 0.25 * (float(got["pos_loss"]) + float(got["pos_frame_loss"]) + float(got["inter_distance_loss"]))
                assert abs(float(got["loss"]) - want) <= 1e-6 * abs(want)


def test_generic_path_reproduces_the_reference_model_step(golden):
    """F18c = the reference's real peptide ``Wrapper.model_step`` at T = 8 with the `loss:` block of its YAML.  Here the fixture's ``pred``
    through the oracle's stage-1 decoder (F13's first stage) and the generic path of ``PeptideLoss``."""
    from lam_slide_amd import PeptideLoss
    f, f13 = golden("f18_peptide_loss.npz"), golden("f13_peptide.npz")
    st = f.group("step")
    B, T, R, L = (int(v) for v in st["meta"][:4])
    s1 = f13.group("stage1")
    ds = harness.DecoderShape(dim_latent=96, num_head_cross=2, num_head_latent=2)
    decode = lambda lat, ent: harness.decode(s1, ds, lat, ent, output="atom14_pos").reshape(B, T, R, 14, 3)  # noqa: E731
    batch = {k: st[k] for k in ("entities", "attention_mask", "atom14_pos", "atom14_pos_frame", "torsions", "torsions_mask", "aatype", "atom14_mask")}
    batch.update(x1=st["latents"], model_kwargs={"x_cond": st["x_cond"], "x_cond_mask": st["mask"]})
    want = f.group("losses")
    seen = {}

    def tap(lat, ent):
        seen["decoded"] = decode(lat, ent)
        return seen["decoded"]

    for mods in (shipped_modules(),):
        loss = PeptideLoss(calc_additional_losses=True, residue_tables=tables_of(golden), **WEIGHTS, **mods)
        with torch.no_grad():
            got, pred_latent = loss(Model(FixedTransport(st["pred"], st["loss"]), tap), batch)
        assert loss.last_path == "generic" and set(got) == set(want) == {"si_loss", "loss"} | set(KEYS)
        assert pred_latent.shape == (B * T, L, 96)
        assert harness.rel_l2(seen["decoded"], st["decoded"]) < 5e-6
        for k in ("si_loss", "loss") + KEYS:
            print(f"F18c generic {k}: got {float(got[k]):.7f} reference {float(want[k]):.7f} rel {rel(got[k], want[k]):.2e}")
            assert rel(got[k], want[k]) < 1e-5, k
    off = PeptideLoss(loss_si_weight=2.0)  # calc_additional_losses off: the SI term alone, nothing decoded, no tables needed
    got, pred_latent = off(Model(FixedTransport(st["pred"], st["loss"]), None), batch)
    assert set(got) == {"si_loss", "loss"} and off.last_path is None and pred_latent is st["pred"]
    assert float(got["loss"]) == 2.0 * float(st["loss"].mean())


def test_constructor_and_dispatch_rules(golden):
    from lam_slide_amd import ModelType, PeptideLoss
    from lam_slide_amd import peptide_loss as pl
    sig = inspect.signature(PeptideLoss.__init__).parameters
    assert list(sig)[1:13] == ["loss_si_weight", "loss_pos_weight", "loss_pos_frame_weight", "loss_norm_weight", "loss_torsion_weight",
                               "loss_inter_distance_weight", "loss_pos", "loss_pos_frame", "loss_norm", "loss_torsion", "loss_inter_distance",
                               "calc_additional_losses"]  # second_stage/peptide.py:107-121
    assert list(sig)[13:] == ["residue_tables"] and sig["residue_tables"].kind is inspect.Parameter.KEYWORD_ONLY
    d = PeptideLoss()
    assert (d.loss_si_weight, d.loss_pos_weight, d.loss_pos_frame_weight, d.loss_norm_weight, d.loss_torsion_weight, d.loss_inter_distance_weight,
            d.calc_additional_losses) == (1.0, 1.0, 0.0, 0.0, 0.0, 0.0, False)
    # which modules the device form stands for
    assert PeptideLoss(**shipped_modules()).torsion_kind() == 1 and PeptideLoss(**shipped_modules("MaskedCosineLoss")).torsion_kind() == 0
    assert PeptideLoss(loss_inter_distance=RefNamed.InterDistanceLoss()).torsion_kind() == 0  # None = the constructor's default of the slot
    assert PeptideLoss().torsion_kind() is None  # the reference's default for loss_inter_distance is MaskedMSELoss: not what the kernel computes
    assert PeptideLoss(**dict(shipped_modules(), loss_pos_frame=RefNamed.MaskedHuberLoss())).torsion_kind() is None
    assert PeptideLoss(**dict(shipped_modules(), loss_norm=RefNamed.MaskedMSELoss())).torsion_kind() is None  # a default's name in another slot
    assert PeptideLoss(**dict(shipped_modules(), loss_torsion=RefNamed.MaskedMSELoss())).torsion_kind() is None

    class MaskedCosineLossV2(nn.Module):  # the right name, but it carries a parameter
        def __init__(self):
            super().__init__()
            self.scale = nn.Parameter(torch.ones(()))

        def forward(self, preds, targets, mask):
            return self.scale * ((1 - (preds * targets).sum(dim=-1)) * mask).sum() / mask.sum()

    assert PeptideLoss(**dict(shipped_modules(), loss_torsion=MaskedCosineLossV2())).torsion_kind() is None
    tables = tables_of(golden)
    c = golden("f18_peptide_loss.npz").group("f5_r4")
    # CPU tensors: generic, and a given module is what gets called
    huber = PeptideLoss(calc_additional_losses=True, residue_tables=tables, **dict(shipped_modules(), loss_pos_frame=RefNamed.MaskedHuberLoss()))
    got, _ = huber(frames_model(c["pred"]), frames_batch(c))
    want = RefNamed.MaskedHuberLoss()(pl.backbone_local(c["pred"]).reshape(-1, 3), c["target_frame"].reshape(-1, 3), c["atom14_mask"].reshape(-1))
    assert huber.last_path == "generic" and torch.equal(got["pos_frame_loss"], want) and within("pos_loss", got["pos_loss"], c["ref64"][0])
    assert not huber.fused_applies(c["pred"], c["target"], c["target_frame"], c["tors_target"])
    # grad mode: generic, and the gradient reaches the decoded positions through the frames and the torsions
    pred = c["pred"].clone().requires_grad_(True)
    loss = PeptideLoss(loss_pos_weight=0.0, loss_pos_frame_weight=1.0, loss_torsion_weight=1.0, calc_additional_losses=True, residue_tables=tables,
                       **shipped_modules())
    with torch.enable_grad():
        got, _ = loss(frames_model(pred), frames_batch(c))
        got["loss"].backward()
    assert loss.last_path == "generic" and pred.grad is not None and bool(torch.isfinite(pred.grad).all()) and float(pred.grad.abs().sum()) > 0
    # the assertion on the model type (second_stage/peptide.py:305-307)
    model = frames_model(c["pred"])
    model.si.model_type = ModelType.VELOCITY
    with pytest.raises(AssertionError, match="DATA"):
        PeptideLoss(calc_additional_losses=True, residue_tables=tables)(model, frames_batch(c))
    got, _ = PeptideLoss()(model, frames_batch(c))  # (not asked for: no assertion)
    assert set(got) == {"si_loss", "loss"}
    # the tables: a dict of four arrays, a missing key is named, without them the host application's modules are imported
    with pytest.raises(KeyError, match="chi_angles_mask"):
        pl.residue_tables({k: v for k, v in golden("f18_peptide_loss.npz").group("tables").items() if k != "chi_angles_mask"})
    if pl._host_tables is None:
        with pytest.raises(ImportError, match="residue_tables="):
            PeptideLoss(calc_additional_losses=True, **shipped_modules())(frames_model(c["pred"]), frames_batch(c))
    dev_tables = tables.on(torch.device("cpu"))
    assert tables.on(torch.device("cpu")) is dev_tables and dev_tables["restab"].dtype == torch.int8  # cached per device


def test_python_wrappers_refuse_cpu_tensors(golden):
    from lam_slide_amd import peptide_loss_sums, peptide_losses
    c = golden("f18_peptide_loss.npz").group("f5_r4")
    args = (c["pred"], c["target_frame"], c["atom14_mask"], c["tors_target"], c["tors_mask"], c["aatype"].long())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        peptide_loss_sums(*args, residue_tables=tables_of(golden))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        peptide_losses(c["pred"], c["target"], *args[1:], residue_tables=tables_of(golden))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        peptide_losses(sums=(torch.zeros(4, 5), torch.zeros(4, 4)))
    with pytest.raises(TypeError):
        peptide_losses()
    with pytest.raises(TypeError):
        peptide_losses(c["pred"], c["target"], *args[1:], sums=(torch.zeros(4, 5), torch.zeros(4, 4)))


def test_library_exports_and_header_declare_the_peptide_losses():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    from lam_slide_amd import peptide_loss as pl
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    for s in ("lsl_peptide_loss_sums", "lsl_peptide_loss_final"):
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
        assert re.fullmatch(r"lsl_[a-z_]+", s) and getattr(lib, s).argtypes is not None
    assert len(lib.lsl_peptide_loss_sums.argtypes) == 12 and len(lib.lsl_peptide_loss_final.argtypes) == 5
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6  # no new ABI number: a stale library is found by the missing symbols
    assert "lsl_peptide_loss_sums, lsl_peptide_loss_final added" in header
    src = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_peptloss.hip.h")).read()
    assert "#define LSL_PEPT_MAX_R (LSL_GEOM_MAX_A / 14)" in src and pl.MAX_R == _lib.GEOM_MAX_A // 14 == 146
    # (compiled into the library: some translation unit includes it)
    assert any('#include "k_peptloss.hip.h"' in open(os.path.join(_lib.SRC_DIR, unit)).read() for unit, _ in _lib.UNITS)


def test_entry_points_validate_arguments_without_gpu():
    from lam_slide_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    ptrs = [one] * 7
    for i in range(7):
        assert lib.lsl_peptide_loss_sums(*(ptrs[:i] + [None] + ptrs[i + 1:]), 4, 4, 1, one, None) == -1, i
    assert lib.lsl_peptide_loss_sums(*ptrs, 4, 4, 1, None, None) == -1
    for F_, R, kind in ((0, 4, 1), (-1, 4, 1), (4, 0, 1), (4, -3, 0), (4, 147, 1), (4, 4, 2), (4, 4, -1)):
        assert lib.lsl_peptide_loss_sums(*ptrs, F_, R, kind, one, None) == -3, (F_, R, kind)
    assert lib.lsl_peptide_loss_sums(*ptrs, 4, 147, 1, one, None) == -3 and b"146" in lib.lsl_last_error()
    assert lib.lsl_peptide_loss_sums(*ptrs, 4, 4, 2, one, None) == -3 and b"kind" in lib.lsl_last_error()
    assert lib.lsl_peptide_loss_final(None, one, 4, one, None) == -1 and lib.lsl_peptide_loss_final(one, None, 4, one, None) == -1
    assert lib.lsl_peptide_loss_final(one, one, 4, None, None) == -1
    assert lib.lsl_peptide_loss_final(one, one, 0, one, None) == -3
    with pytest.raises(ValueError):
        _lib.check(-3)
