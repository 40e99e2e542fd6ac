"""CPU tests of the first-stage validation path (lam_slide_amd/first_stage.py, Stage1Decoder.decode_heads, lsl_decode_heads /
lsl_class_loss_sums / lsl_class_loss_final) on fixture F19 - the reference's real first-stage Wrappers of md17, nba and peptide, run
through FirstStageLightningBase.model_step in fp32 and in fp64 (tools/make_fixtures.py f19):

  * the oracle's encode + decode reproduce the latents and every head of every model (2e-6 relative L2, the F6-F8 bar);
  * the torch path of the drop-in Loss classes, on the fixture's own predictions, reproduces the reference's fp32 loss dict (1e-6), keys and
    weighted total included, and the fp64 run on the fp64 predictions to 1e-12;
  * the class-loss definition restated in fp64 equals F.cross_entropy to 1e-12, with smoothing, masks and ignored targets;
  * what is refused is refused without a GPU: K = 129, bad shapes, n_heads 0 and 9, a CPU tensor; MAX_K and MAX_HEADS equal their macros."""
import ctypes as C
import os
import re

import pytest
import torch

import first_stage_cases as fc
from conftest import ROOT, rel_l2

BAR = 2e-6


@pytest.mark.parametrize("name", fc.MODELS)
def test_oracle_reproduces_the_f19_latents_and_every_head(golden, name):
    m = fc.model(golden, name)
    z = fc.harness.encode(m.p, m.es, m.x, m.batch["entities"], m.mask)
    assert rel_l2(z, m.z) < BAR
    assert set(m.heads) == set(m.preds) and len(m.heads) >= 2
    for h in m.heads:
        assert rel_l2(fc.harness.decode(m.p, m.ds, m.z, m.batch["entities"], output=h), fc.flat(m.preds[h])) < BAR, h
    # and the fp64 oracle the fp64 run of the reference's own modules
    p64 = {k: v.double() for k, v in m.p.items()}
    assert rel_l2(fc.harness.encode(p64, m.es, m.x64, m.batch["entities"], m.mask), m.z64) < 1e-12
    for h in m.heads:
        assert rel_l2(fc.harness.decode(p64, m.ds, m.z64, m.batch["entities"], output=h), fc.flat(m.preds64[h])) < 1e-12, h


def test_f19_sizes_are_the_ones_the_tests_rely_on(golden):
    md, nba, pep = (fc.model(golden, n) for n in fc.MODELS)
    assert md.heads == ["pos", "atom"] and md.preds["atom"].shape == (6, 9, 10) and md.z.shape == (6, 8, 32) and not bool(md.mask.all())
    assert nba.heads == ["pos", "team", "group"] and [nba.preds[h].shape[-1] for h in nba.heads] == [2, 3, 2] and nba.preds["pos"].shape[:2] == (5, 11)
    assert pep.heads == ["atom14_pos", "aatype"] and pep.preds["atom14_pos"].shape == (3, 4, 14, 3) and "decoder.extender.1.weight" in pep.p


@pytest.mark.parametrize("name", fc.MODELS)
def test_torch_path_of_the_drop_ins_reproduces_the_reference_loss_dict(golden, name):
    m = fc.model(golden, name)
    loss = fc.make_loss(golden, m)
    got, preds = loss(fc.Fixed(fc.shaped(m, m.preds), m.scale), m.batch)
    assert list(got) == list(m.loss32) and set(loss.last_paths.values()) == {"generic"} and preds["pos" if name != "peptide" else "atom14_pos"] is not None
    for k, v in got.items():
        assert v.dim() == 0 and v.dtype == torch.float32
        assert abs(float(v) - float(m.loss32[k])) <= 1e-6 * abs(float(m.loss32[k])), (k, float(v), float(m.loss32[k]))
    # the weighted total and dist restated from the other keys
    w = m.weights
    parts = {"md17": [("loss_pos_weight", "pos_loss"), ("loss_inter_distance_weight", "inter_distance_loss"), ("loss_atom_type_weight", "atom_type_loss"),
                      ("loss_norm_weight", "norm_loss")],
             "nba": [("loss_pos_weight", "pos_loss"), ("loss_inter_distance_weight", "inter_distance_loss"), ("loss_norm_weight", "norm_loss"),
                     ("loss_team_weight", "team_loss"), ("loss_group_weight", "group_loss")],
             "peptide": [("loss_pos_weight", "pos_loss"), ("loss_pos_frame_weight", "pos_frame_loss"), ("loss_inter_distance_weight", "inter_distance_loss"),
                         ("loss_res_type_weight", "res_type_loss"), ("loss_norm_weight", "norm_loss"), ("loss_torsion_weight", "torsion_loss")]}[name]
    assert {k for k, _ in parts} == set(w) and {k for _, k in parts} | {"loss", "dist"} == set(got)
    total = sum(w[a] * float(m.loss64[b]) for a, b in parts)
    assert abs(total - float(m.loss64["loss"])) < 1e-12 * abs(total)
    assert abs(float(m.loss64["norm_loss"]) * m.scale - float(m.loss64["dist"])) < 1e-12
    # fp64 in, fp64 out: the same formulas as the reference's .double() run
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in m.batch.items()}
    got64, _ = loss.double()(fc.Fixed(fc.shaped(m, m.preds64), m.scale), b64)
    for k, v in got64.items():
        assert v.dtype == torch.float64 and abs(float(v) - float(m.loss64[k])) <= 1e-9 * abs(float(m.loss64[k])), (k, float(v), float(m.loss64[k]))


def test_pedestrian_drop_in_keys_and_total():
    from lam_slide_amd.first_stage import PedestrianLoss
    g = torch.Generator().manual_seed(0)
    pred, pos = torch.randn(4, 6, 2, generator=g), torch.randn(4, 6, 2, generator=g)
    mask = torch.rand(4, 6, generator=g) > 0.3
    got, preds = PedestrianLoss(loss_pos_weight=0.5, loss_inter_distance_weight=2.0, loss_norm_weight=0.25)(fc.Fixed({"pos": pred}, 3.0), {"pos": pos, "attention_mask": mask})
    assert list(got) == ["loss", "pos_loss", "inter_distance_loss", "norm_loss", "dist"] and preds["pos"] is pred
    m = mask.float()
    pl = (((pred - pos) ** 2).mean(-1) * m).sum() / m.sum()
    nl = ((pred - pos).norm(dim=-1) * m).sum() / m.sum()
    il = fc.InterDistanceLoss()(pred, pos, m)
    assert torch.allclose(got["pos_loss"], pl) and torch.allclose(got["norm_loss"], nl) and torch.allclose(got["inter_distance_loss"], il)
    assert torch.allclose(got["loss"], 0.5 * pl + 2.0 * il + 0.25 * nl) and torch.allclose(got["dist"], nl * 3.0)


def test_class_loss_definition_equals_torch_cross_entropy(golden):
    """The four lines of the header (lse, nll, smooth, loss) and the two denominators, in fp64, against F.cross_entropy / the F19 cases."""
    f = golden(fc.FIXTURE)
    names = [str(n) for n in f.raw["ce_names"]]
    assert len(names) == 7
    for name in names:
        c = f.group("ce." + name)
        mask, eps = c.get("mask"), float(c["eps"])
        _, loss = fc.ce64(c["logits"], c["target"], mask, eps)
        assert abs(float(loss) - float(c["ref64"])) <= 1e-12 * abs(float(c["ref64"])), name
        per = torch.nn.functional.cross_entropy(c["logits"].double().flatten(0, 1), c["target"].flatten(), reduction="none", label_smoothing=eps)
        want = (per * mask.flatten()).sum() / mask.sum() if mask is not None else per.sum() / (c["target"] != -100).sum()
        assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want)), name
        assert abs(float(c["ref32"]) - float(c["ref64"])) <= 1.8e-7 * abs(float(c["ref64"])), name


def test_limits_equal_their_macros():
    from lam_slide_amd import _lib, decoder, first_stage
    src = open(os.path.join(_lib.SRC_DIR, "k_classloss.hip.h")).read()
    assert first_stage.MAX_K == _lib.CLS_MAX_K == int(re.search(r"#define LSL_CLS_MAX_K (\d+)", src).group(1)) == 128
    assert first_stage.IGNORE_INDEX == _lib.CLS_IGNORE == int(re.search(r"#define LSL_CLS_IGNORE \((-\d+)\)", src).group(1)) == -100
    header = open(os.path.join(ROOT, "include", "lsl_api.h")).read()
    assert decoder.MAX_HEADS == int(re.search(r"#define LSL_DECODE_MAX_HEADS (\d+)", header).group(1)) == 8


def test_refusals_without_a_gpu(golden):
    from lam_slide_amd import ClassMeter, Stage1Decoder, _lib, class_loss_sums, class_losses
    lib = _lib.load()
    one = C.c_void_p(16)  # (never dereferenced: every call below is refused on its arguments)
    assert lib.lsl_class_loss_sums(one, one, None, 2, 3, 129, 0.0, one, None, None) == -3 and b"129" in lib.lsl_last_error()
    assert lib.lsl_class_loss_sums(one, one, None, 2, 3, 0, 0.0, one, None, None) == -3
    assert lib.lsl_class_loss_sums(one, one, None, 2, 0, 4, 0.0, one, None, None) == -3
    assert lib.lsl_class_loss_sums(one, one, None, 0, 3, 4, 0.0, one, None, None) == -3
    assert lib.lsl_class_loss_sums(one, one, None, 2, 3, 4, 1.0, one, None, None) == -3
    assert lib.lsl_class_loss_sums(one, one, None, 2, 3, 4, -0.1, one, None, None) == -3
    assert lib.lsl_class_loss_sums(None, one, None, 2, 3, 4, 0.0, one, None, None) == -1
    assert lib.lsl_class_loss_final(one, 0, one, None) == -3 and lib.lsl_class_loss_final(None, 1, one, None) == -1
    heads = (_lib.DecoderHead * 9)(*[_lib.DecoderHead(16, 16, 16, 16, 3)] * 9)
    outs = (C.c_void_p * 9)(*[16] * 9)
    for n in (0, 9):
        assert lib.lsl_decode_heads(one, heads, n, one, one, 1, 1, 1, outs, one, 1 << 30, None) == -3 and b"n_heads" in lib.lsl_last_error()
    assert lib.lsl_decode_heads(None, heads, 1, one, one, 1, 1, 1, outs, one, 1 << 30, None) == -1
    t = torch.zeros(2, 3, dtype=torch.long)
    for bad in (lambda: class_loss_sums(torch.zeros(2, 3, 129), t), lambda: class_loss_sums(torch.zeros(2, 3, 4), t[:, :2]),
                lambda: class_loss_sums(torch.zeros(2, 3, 4), t, torch.ones(2, 2)), lambda: class_loss_sums(torch.zeros(2, 3, 4), t.float()),
                lambda: class_loss_sums(torch.zeros(2, 3, 4), t, label_smoothing=1.0), lambda: class_losses(sums=torch.zeros(3, 5)),
                lambda: ClassMeter(129), lambda: ClassMeter(3).update(torch.zeros(2, 3, 4), t)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):  # no CPU path
        class_loss_sums(torch.zeros(2, 3, 4), t)
    with pytest.raises(TypeError):
        class_losses()
    m = fc.model(golden, "nba")
    dec = Stage1Decoder(m.p, **m.dec_kw)
    assert list(dec.heads.items()) == [("pos", 2), ("team", 3), ("group", 2)] and dec.output == "pos"
    with pytest.raises(RuntimeError):
        dec.decode_heads(m.z, m.batch["entities"])


def test_class_meter_formulas():
    from lam_slide_amd import ClassMeter
    c = torch.tensor([[5, 1, 0], [2, 3, 0], [0, 0, 0]])
    got = ClassMeter.formulas(c)
    assert float(got["accuracy"]) == pytest.approx(8 / 11)
    assert got["precision_per_class"].tolist() == pytest.approx([5 / 7, 3 / 4, 0.0]) and got["recall_per_class"].tolist() == pytest.approx([5 / 6, 3 / 5, 0.0])
    assert float(got["precision"]) == pytest.approx((5 / 7 + 3 / 4) / 3) and float(got["recall"]) == pytest.approx((5 / 6 + 3 / 5) / 3)
    assert float(ClassMeter.formulas(torch.zeros(2, 2, dtype=torch.long))["accuracy"]) == 0.0
