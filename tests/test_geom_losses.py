"""``lam_slide_amd.Loss`` and the geometry losses without a GPU: the generic path of the ``Loss`` drop-in against the reference's real md17
``model_step`` (fixture F16) and against the reference's own loss classes on seeded inputs (fixture F17, tools/make_fixtures.py f17), the
dispatch rules, and the C ABI of ``lsl_geom_loss_sums`` / ``lsl_geom_loss_final`` (symbols, header, argument validation before anything
touches a GPU).

Bars.  1e-5 relative is the project's bar for a reduction alone (tests/test_si_loss.py).  The reference's fp32 classes deviate from their
own fp64 run by at most 3.71e-7 over the F17 cases - the figure ``tools/make_fixtures.py f17`` printed when it wrote the committed fixture
(the issue that asked for F17 quotes 9.2e-7 from a run whose seeds it does not give; either way the reference stays inside the bar).
Above 25 entities ``torch.cdist`` may take its matmul form in fp32: those cases are compared with the fp64 values only."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch
from torch import nn

from oracle import harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pos_loss", "dist", "inter_dist_loss")  # the order of F17's ref32 / ref64


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


class FixedTransport:
    """``model.si`` with the outcome of ``training_losses`` fixed (the SI term has tests of its own)."""

    def __init__(self, pred, loss, model_type=None):
        from lam_slide_amd import ModelType
        self.pred, self.loss = pred, loss
        self.model_type = ModelType.DATA if model_type is None else model_type

    def training_losses(self, model, x1, model_kwargs=None):
        return {"pred": self.pred, "loss": self.loss}


class Model:
    """What ``Loss.forward`` touches of the LightningModule: ``si`` and ``decode(latents [(B T), L, C], entities [(B T), A]) -> {"pos":
    [B, T, A, D]}`` (second_stage/md17.py:127-130)."""

    def __init__(self, si, decode):
        self.si, self._decode = si, decode

    def decode(self, latents, entities):
        return {"pos": self._decode(latents, entities)}


def f17_cases(golden):
    f = golden("f17_geom_losses.npz")
    for name in (str(n) for n in f.raw["names"]):
        yield name, f.group(name)


def frames_model(pred_pos):
    """A model whose decode returns the given positions [F, A, D] as one trajectory of F frames."""
    F_ = pred_pos.shape[0]
    si = FixedTransport(torch.zeros(1, F_, 1, 1), torch.tensor([0.5]))
    return Model(si, lambda latents, entities: pred_pos.reshape(1, *pred_pos.shape))


def frames_batch(c):
    F_, A, _ = c["pred"].shape
    return {"x1": torch.zeros(1, F_, 1, 1), "model_kwargs": {}, "entities": torch.zeros(1, F_, A, dtype=torch.long),
            "pos": c["target"].reshape(1, *c["target"].shape), "attention_mask": c["mask"].reshape(1, F_, A)}


def test_loss_generic_path_reproduces_the_reference_model_step(golden):
    """F16 = the reference's real md17 ``Wrapper.model_step`` with calc_additional_losses and the weights of its YAML (1, 0.25, 0.25).  Here
    the fixture's ``pred`` through the oracle's stage-1 decoder and the generic path of ``lam_slide_amd.Loss``."""
    from lam_slide_amd import Loss
    f, f9 = golden("f16_model_step.npz"), golden("f9_sample.npz")
    s1 = dict(f9.group("stage1"))
    s1.update(f.group("stage1_tables"))  # (tables the reference renormalised in place since F9 was written; none at present)
    B, T, A, D = f["pos"].shape
    decode = lambda lat, ent: harness.decode(s1, harness.DecoderShape(), lat, ent).reshape(B, T, A, D)  # noqa: E731
    model = Model(FixedTransport(f["pred"], f["loss"]), decode)
    batch = {"x1": f["latents"], "model_kwargs": {"x_cond": f["x_cond"], "x_cond_mask": f["mask"]}, "entities": f["entities"], "pos": f["pos"],
             "attention_mask": f["attention_mask"]}
    want = f.group("losses")
    for mods in ({}, {"loss_pos": RefNamed.MaskedMSELoss(), "loss_inter_dist": RefNamed.InterDistanceLoss(), "loss_norm": RefNamed.MaskedNormLoss()}):
        loss = Loss(weight_si_loss=1.0, weight_pos_loss=0.25, weight_inter_dist_loss=0.25, weight_norm_loss=0.0, calc_additional_losses=True, **mods)
        with torch.no_grad():
            got, pred_latent = loss(model, batch)
        assert loss.last_path == "generic" and set(got) == set(want) == {"si_loss", "pos_loss", "inter_dist_loss", "dist", "loss"}
        assert pred_latent.shape == (B * T,) + tuple(f["pred"].shape[2:])  # (the reference returns the flattened latents in this branch)
        for k in ("si_loss", "pos_loss", "dist", "inter_dist_loss", "loss"):
            print(f"F16 generic {k}: got {float(got[k]):.7f} reference {float(want[k]):.7f} rel {rel(got[k], want[k]):.2e}")
            assert rel(got[k], want[k]) < 1e-5, k
    off = Loss(weight_si_loss=2.0)  # calc_additional_losses off: the SI term alone, nothing decoded
    pred = f["pred"]
    got, pred_latent = off(Model(FixedTransport(pred, f["loss"]), None), batch)
    assert set(got) == {"si_loss", "loss"} and off.last_path is None and pred_latent is pred
    assert float(got["loss"]) == 2.0 * float(f["loss"].mean())


def test_loss_generic_path_matches_the_reference_classes(golden):
    from lam_slide_amd import Loss
    n = 0
    for name, c in f17_cases(golden):
        for dtype in (torch.float32, torch.float64):
            loss = Loss(weight_pos_loss=0.5, weight_inter_dist_loss=2.0, calc_additional_losses=True)
            batch = frames_batch(c)
            batch["pos"] = batch["pos"].to(dtype)
            got, _ = loss(frames_model(c["pred"].to(dtype)), batch)
            assert loss.last_path == "generic"
            if not bool(c["mask"].any()):
                assert all(torch.isnan(got[k]) for k in KEYS + ("loss",)), name
                continue
            A = c["pred"].shape[1]
            for i, k in enumerate(KEYS):
                e64 = rel(got[k], c["ref64"][i])
                e32 = rel(got[k], c["ref32"][i]) if A <= 25 else float("nan")
                print(f"F17 generic {name} {dtype} {k}: vs fp64 {e64:.2e} vs fp32 {e32:.2e}")
                assert e64 < 1e-5 and not e32 >= 1e-5, (name, k)
            want = 0.5 + 0.5 * float(got["pos_loss"]) + 2.0 * float(got["inter_dist_loss"])
            assert abs(float(got["loss"]) - want) <= 1e-6 * abs(want)
        n += 1
    assert n == 9


class RefNamed:
    """Classes with the names of the reference's modules (modules/losses.py), restated."""

    class MaskedMSELoss(nn.Module):
        def __init__(self):
            super().__init__()
            self.mse_loss = nn.MSELoss(reduction="none")

        def forward(self, input, target, mask):
            return (self.mse_loss(input, target).mean(dim=1) * mask).sum() / mask.sum()

    class MaskedNormLoss(nn.Module):
        def forward(self, input, target, mask):
            return (torch.norm(input - target, dim=-1) * mask).sum() / mask.sum()

    class InterDistanceLoss(nn.Module):
        def forward(self, preds, targets, mask):
            diag_att = mask.unsqueeze(-1) * mask.unsqueeze(-2)
            return (((torch.cdist(preds, preds) - torch.cdist(targets, targets)) * diag_att) ** 2).sum() / diag_att.sum()

    class MaskedHuberLoss(nn.Module):
        def __init__(self, delta=1.0):
            super().__init__()
            self.huber_loss = nn.HuberLoss(reduction="none", delta=delta)

        def forward(self, input, target, mask):
            return (self.huber_loss(input, target).mean(dim=1) * mask).sum() / mask.sum()


def test_constructor_and_dispatch_rules(golden):
    from lam_slide_amd import Loss, ModelType
    params = list(inspect.signature(Loss.__init__).parameters)[1:]
    assert params == ["weight_si_loss", "weight_pos_loss", "weight_inter_dist_loss", "weight_norm_loss", "loss_pos", "loss_inter_dist", "loss_norm",
                      "calc_additional_losses"]  # second_stage/md17.py:196-206
    d = Loss()
    assert (d.weight_si_loss, d.weight_pos_loss, d.weight_inter_dist_loss, d.weight_norm_loss, d.calc_additional_losses) == (1.0, 0.0, 0.0, 0.0, False)
    # which modules the device form stands for: None or parameter-free instances named like the defaults
    assert Loss().default_modules()
    assert Loss(loss_pos=RefNamed.MaskedMSELoss(), loss_inter_dist=RefNamed.InterDistanceLoss(), loss_norm=RefNamed.MaskedNormLoss()).default_modules()
    assert not Loss(loss_pos=RefNamed.MaskedHuberLoss()).default_modules()
    assert not Loss(loss_norm=RefNamed.MaskedMSELoss()).default_modules()  # (a default's name in another slot)

    class MaskedNormLoss(nn.Module):  # the right name, but it carries a parameter
        def __init__(self):
            super().__init__()
            self.scale = nn.Parameter(torch.ones(()))

        def forward(self, input, target, mask):
            return self.scale * (torch.norm(input - target, dim=-1) * mask).sum() / mask.sum()

    assert not Loss(loss_norm=MaskedNormLoss()).default_modules()
    c = golden("f17_geom_losses.npz").group("f40_a25_d2_m40")
    # a CPU tensor: generic, and a given module is what gets called
    huber = Loss(loss_pos=RefNamed.MaskedHuberLoss(delta=0.5), calc_additional_losses=True)
    got, _ = huber(frames_model(c["pred"]), frames_batch(c))
    D = c["pred"].shape[-1]
    want = RefNamed.MaskedHuberLoss(delta=0.5)(c["pred"].reshape(-1, D), c["target"].reshape(-1, D), c["mask"].reshape(-1))
    assert huber.last_path == "generic" and torch.equal(got["pos_loss"], want) and rel(got["dist"], c["ref64"][1]) < 1e-5
    # grad mode: generic, and the gradient reaches the decoded positions
    pred = c["pred"].clone().requires_grad_(True)
    loss = Loss(weight_pos_loss=1.0, weight_inter_dist_loss=1.0, calc_additional_losses=True)
    assert not loss.fused_applies(pred, c["target"])
    with torch.enable_grad():
        got, _ = loss(frames_model(pred), frames_batch(c))
        got["loss"].backward()
    assert loss.last_path == "generic" and pred.grad is not None and bool(torch.isfinite(pred.grad).all()) and float(pred.grad.abs().sum()) > 0
    assert not bool(pred.grad[0].any())  # (frame 0 is fully masked)
    # the assertion on the model type (second_stage/md17.py:232-234)
    model = frames_model(c["pred"])
    model.si.model_type = ModelType.VELOCITY
    with pytest.raises(AssertionError, match="DATA"):
        Loss(calc_additional_losses=True)(model, frames_batch(c))
    got, _ = Loss()(model, frames_batch(c))  # (not asked for: no assertion)
    assert set(got) == {"si_loss", "loss"}


def test_python_wrappers_refuse_cpu_tensors():
    from lam_slide_amd import geom_loss_sums, geom_losses
    p, m = torch.zeros(2, 3, 5, 3), torch.ones(2, 3, 5, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geom_loss_sums(p, p, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geom_losses(p, p, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geom_losses(sums=torch.zeros(4, 5))
    with pytest.raises(TypeError):
        geom_losses()
    with pytest.raises(TypeError):
        geom_losses(p, p, m, sums=torch.zeros(4, 5))


def test_library_exports_and_header_declare_the_geometry_losses():
    import __graft_entry__ as ge
    ge.build()
    from lam_slide_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    for s in ("lsl_geom_loss_sums", "lsl_geom_loss_final"):
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b" + s + r"\s*\(", header), s
        assert re.fullmatch(r"lsl_[a-z_]+", s)  # (the export test of test_host_logic.py reads the header with this pattern)
    assert lib.lsl_version() == 6 and _lib.ABI_VERSION == 6  # no new ABI number: a stale library is found by the missing symbols
    src = open(os.path.join(ROOT, "lam_slide_amd", "csrc", "k_geomloss.hip.h")).read()
    assert re.search(r"#define LSL_GEOM_MAX_A (\d+)", src).group(1) == str(_lib.GEOM_MAX_A)
    assert re.search(r"#define LSL_GEOM_MAX_D (\d+)", src).group(1) == str(_lib.GEOM_MAX_D)


def test_entry_points_validate_arguments_without_gpu():
    from lam_slide_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch
    assert lib.lsl_geom_loss_sums(None, one, one, 4, 5, 3, one, None) == -1
    assert lib.lsl_geom_loss_sums(one, None, one, 4, 5, 3, one, None) == -1
    assert lib.lsl_geom_loss_sums(one, one, None, 4, 5, 3, one, None) == -1
    assert lib.lsl_geom_loss_sums(one, one, one, 4, 5, 3, None, None) == -1
    for F_, A, D in ((0, 5, 3), (-1, 5, 3), (4, 0, 3), (4, 2049, 3), (4, 5, 0), (4, 5, 5)):
        assert lib.lsl_geom_loss_sums(one, one, one, F_, A, D, one, None) == -3, (F_, A, D)
    assert lib.lsl_geom_loss_sums(one, one, one, 4, 2049, 3, one, None) == -3 and b"2048" in lib.lsl_last_error()
    assert lib.lsl_geom_loss_final(None, 4, one, None) == -1 and lib.lsl_geom_loss_final(one, 4, None, None) == -1
    assert lib.lsl_geom_loss_final(one, 0, one, None) == -3
    with pytest.raises(ValueError):
        _lib.check(-3)
