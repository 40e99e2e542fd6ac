"""GPU tests of the first-stage validation path: ``lsl_decode_heads`` behind ``Stage1Decoder.decode_heads``, ``lsl_class_loss_sums`` /
``lsl_class_loss_final`` behind ``class_loss_sums`` / ``class_losses`` / ``ClassMeter``, and ``Stage1Autoencoder`` with the four drop-in
``Loss`` classes on fixture F19 (the reference's real first-stage Wrappers of md17, nba and peptide: model_step in fp32 and in fp64).

Bars.
  * Heads: bit for bit against ``Stage1Decoder(output=h).decode``; 2e-6 relative L2 against the fp64 oracle (the F6 / F8 bar).
  * Cross-entropy alone: 1e-5 relative against an fp64 restatement / the reference's fp64 run, the project's bar for a reduction
    (tests/test_si_loss.py, tests/test_hip_geom_losses.py); the reference's own fp32 classes stay within 1.8e-7 of their fp64 run on
    inputs of this kind (K 2..128, logits of scale 1, 30, 80, smoothing 0 and 0.1, a quarter of the rows masked).
  * End to end the bars come from the MEASURED deviation delta of what the device decoded from the reference's fp64 predictions:
    the triangle-inequality bounds of tests/test_hip_geom_losses.py:5-12 for pos_loss, norm_loss and inter_distance_loss, and
    |dCE| <= 2 max|dlogit| for a class loss (cross-entropy with or without smoothing is 2-Lipschitz in the sup norm of the logits: lse
    moves by at most max|d|, so do l_y and the mean), each plus the 1e-5 reduction term.  The peptide's pos_frame_loss and torsion_loss
    (Gram-Schmidt frames: no such bound) are the bits of ``peptide_losses`` on the decoded positions, and that reduction alone is checked on
    the reference's own predictions at the bars of tests/test_hip_peptide_losses.py.
Measured values: profiles/first_stage_parity.txt."""
import numpy as np
import pytest
import torch
from torch import nn

import first_stage_cases as fc
import stage1_cases as sc
from conftest import parity, rel_l2

pytestmark = pytest.mark.gpu

HEAD_WIDTHS = (2, 3, 10, 21, 42)
REDUCTION = 1e-5
TINY = 1.1754944e-38  # the smallest normal float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# ---------------------------------------------------------------------------------------------------------- heads
def heads_model(split):
    """stage1_cases' w32 decoder (8 -> 96 latents, queries of 36, a cross block, tanh GELU) with five more heads h2 .. h42, and with
    ``split`` the 1x1-conv extender of DecoderQuerySplitter."""
    m = sc.decoder_model("w32")
    sd = dict(m.sd)
    g = torch.Generator().manual_seed(19 + split)
    dq, dl = 36, 96
    for w in HEAD_WIDTHS:
        sd[f"decoder.output_layers.h{w}.0.weight"] = (torch.rand(dq, dq, generator=g) * 2 - 1) / dq ** 0.5
        sd[f"decoder.output_layers.h{w}.0.bias"] = (torch.rand(dq, generator=g) * 2 - 1) / dq ** 0.5
        sd[f"decoder.output_layers.h{w}.2.weight"] = (torch.rand(w, dq, generator=g) * 2 - 1) / dq ** 0.5
        sd[f"decoder.output_layers.h{w}.2.bias"] = (torch.rand(w, generator=g) * 2 - 1) / dq ** 0.5
    if split:
        sd["decoder.extender.1.weight"] = (torch.rand(dl * split, dl, 1, generator=g) * 2 - 1) / dl ** 0.5
        sd["decoder.extender.1.bias"] = (torch.rand(dl * split, generator=g) * 2 - 1) / dl ** 0.5
    return sd, m.shape, m.ctor


@pytest.mark.parametrize("split", [0, 3], ids=["plain", "split3"])
def test_decode_heads_has_the_bits_of_single_head_handles_and_the_oracle_parity(split, dev):
    from lam_slide_amd import Stage1Decoder
    sd, shape, ctor = heads_model(split)
    names = ["pos"] + [f"h{w}" for w in HEAD_WIDTHS]
    dec = Stage1Decoder(sd, device=dev, **ctor)
    assert list(dec.heads) == names and dec.num_split == split
    single = {h: Stage1Decoder(sd, device=dev, output=h, **ctor) for h in names}
    sd64 = sc.to64(sd)
    for A in (1, 5, 65):
        g = torch.Generator().manual_seed(100 * split + A)
        z, ent = torch.randn(3, 8, 8, generator=g), torch.randint(0, sc.N_ENTITIES, (3, A), generator=g)
        got = dec.decode_heads(z.to(dev), ent.to(dev))
        assert list(got) == names
        for h in names:
            assert got[h].shape == (3, A, dec.heads[h]) and torch.equal(got[h], single[h].decode(z.to(dev), ent.to(dev))), (A, h)
            parity(f"fs.heads.{'split3' if split else 'plain'}.A{A}.{h}", rel_l2(got[h].cpu(), fc.harness.decode(sd64, shape, z.double(), ent, output=h)), 2e-6)
        sub = dec.decode_heads(z.to(dev), ent.to(dev), outputs=["h21", "pos"])  # a named subset, in the order given
        assert list(sub) == ["h21", "pos"] and torch.equal(sub["h21"], got["h21"]) and torch.equal(sub["pos"], got["pos"])
        assert torch.equal(dec.decode(z.to(dev), ent.to(dev)), got["pos"])  # decode() itself is unchanged
    with pytest.raises(KeyError):
        dec.decode_heads(z.to(dev), ent.to(dev), outputs=["nope"])
    with pytest.raises(ValueError):
        dec.decode_heads(z.to(dev), ent.to(dev), outputs=["pos", "pos"])


def test_refused_decode_heads_writes_no_output(dev):
    """The key limit of lsl_decode applies unchanged (md17 tile: 496 keys): the refusal leaves every outs[h] as it was."""
    import ctypes as C
    from lam_slide_amd import Stage1Decoder, _lib
    m = sc.decoder_model("md17")
    dec = Stage1Decoder(m.sd, device=dev, **m.ctor)
    z, ent = torch.zeros(1, 497, 32, device=dev), torch.zeros(1, 2, dtype=torch.long, device=dev)
    with pytest.raises(ValueError, match="LDS tile"):
        dec.decode_heads(z, ent)
    out = torch.full((1, 2, 3), 7.0, device=dev)
    ptrs = dec._head_ptrs["pos"]
    heads = (_lib.DecoderHead * 1)(_lib.DecoderHead(*ptrs, 3))
    outs = (C.c_void_p * 1)(out.data_ptr())
    ws = torch.empty(_lib.load().lsl_decode_workspace_bytes(dec._handle, 1, 497, 2), dtype=torch.uint8, device=dev)
    rc = _lib.load().lsl_decode_heads(dec._handle, heads, 1, z.data_ptr(), ent.data_ptr(), 1, 497, 2, outs, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == -3 and bool((out == 7.0).all())


@pytest.mark.parametrize("name", fc.MODELS)
def test_f19_heads_of_the_three_models(golden, name, dev):
    from lam_slide_amd import Stage1Decoder
    m = fc.model(golden, name)
    dec = Stage1Decoder(m.p, device=dev, output=m.heads[0], **m.dec_kw)
    assert list(dec.heads) == m.heads
    z, ent = m.z.to(dev), m.batch["entities"].to(dev)
    got = dec.decode_heads(z, ent)
    p64 = sc.to64(m.p)
    for h in m.heads:
        assert torch.equal(got[h], Stage1Decoder(m.p, device=dev, output=h, **m.dec_kw).decode(z, ent)), h
        parity(f"fs.f19.{name}.{h}", rel_l2(got[h].cpu(), fc.harness.decode(p64, m.ds, m.z.double(), m.batch["entities"], output=h)), 2e-6)
        parity(f"fs.f19.{name}.{h}.ref", rel_l2(got[h].cpu(), fc.flat(m.preds[h])), 4e-6)  # (both within 2e-6 of the fp64 oracle)


# ---------------------------------------------------------------------------------------------------------- cross-entropy
def test_f19_cross_entropy_cases_against_the_reference_classes(golden, dev):
    from lam_slide_amd import class_losses
    f = golden(fc.FIXTURE)
    for name in [str(n) for n in f.raw["ce_names"]]:
        c = f.group("ce." + name)
        mask = c["mask"].to(dev) if "mask" in c else None
        got = class_losses(c["logits"].to(dev), c["target"].to(dev), mask, float(c["eps"]))
        assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
        parity(f"fs.ce.{name}", rel(got, c["ref64"]), REDUCTION)


def ce_inputs(F_, A, K, scale, masked, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(F_, A, K, generator=g) * scale
    target = torch.randint(0, K, (F_, A), generator=g)
    mask = (torch.rand(F_, A, generator=g) >= 0.25) if masked else None
    if masked:
        mask[:, 0] = True  # (no empty frame here: those have a test of their own)
    return logits, target, mask


@pytest.mark.parametrize("K", [1, 2, 3, 63, 64, 65, 128])
def test_class_loss_edge_shapes_against_float64(K, dev):
    from lam_slide_amd import class_loss_sums, class_losses
    worst = 0.0
    for A in (1, 63, 64, 65, 300):
        for scale in (1.0, 80.0):
            for masked in (False, True):
                logits, target, mask = ce_inputs(5, A, K, scale, masked, 1000 * K + A)
                for eps in (0.0, 0.1):
                    sums = class_loss_sums(logits.to(dev), target.to(dev), None if mask is None else mask.to(dev), eps)
                    want, loss = fc.ce64(logits, target, mask, eps)
                    tag = (K, A, scale, masked, eps)
                    assert sums.shape == (5, 2) and torch.equal(sums[:, 1].cpu().double(), want[:, 1]), tag
                    if K == 1:  # one class: every loss is an exact 0
                        assert float(sums[:, 0].abs().max()) == 0.0 and float(class_losses(sums=sums)) == 0.0, tag
                        continue
                    # a frame's sum and the loss against their fp64 values at the 1e-5 bar.  Two absolute terms beside it, per row, for frames
                    # whose every target leads by a wide margin (true loss ~ 1e-20 and below): what fp32 cannot hold (K terms below its
                    # smallest normal number) and the restatement's own rounding (lse - l_y cancels in fp64 to a few ulp of the logits)
                    floor = A * (K * TINY + 4 * 2.22e-16 * float(logits.abs().max()))
                    err = float(((sums[:, 0].cpu().double() - want[:, 0]).abs() / (want[:, 0].abs() + floor / REDUCTION)).max())
                    err_loss = abs(float(class_losses(sums=sums)) - float(loss)) / (abs(float(loss)) + floor / REDUCTION)
                    worst = max(worst, err, err_loss)
                    assert err < REDUCTION and err_loss < REDUCTION, (tag, err, err_loss)
    parity(f"fs.ce.edge.K{K}", worst, REDUCTION)


def test_masked_frames_ignored_targets_and_bad_targets(dev):
    from lam_slide_amd import class_loss_sums, class_losses
    logits, target, mask = ce_inputs(5, 65, 10, 1.0, True, 7)
    whole = class_loss_sums(logits.to(dev), target.to(dev), mask.to(dev), 0.1)
    # an all-masked frame inside a batch leaves the others untouched; an all-masked batch gives NaN
    m2 = mask.clone()
    m2[2] = False
    part = class_loss_sums(logits.to(dev), target.to(dev), m2.to(dev), 0.1)
    keep = [0, 1, 3, 4]
    assert torch.equal(part[keep], whole[keep]) and part[2].tolist() == [0.0, 0.0]
    assert rel(class_losses(sums=part), fc.ce64(logits, target, m2, 0.1)[1]) < REDUCTION
    assert bool(torch.isnan(class_losses(logits.to(dev), target.to(dev), torch.zeros_like(mask).to(dev))))
    # masked-out rows are skipped, not multiplied: a NaN there changes nothing
    poisoned = logits.clone()
    poisoned[~mask] = float("nan")
    assert torch.equal(class_loss_sums(poisoned.to(dev), target.to(dev), mask.to(dev), 0.1), whole)
    # -100: with a mask the row still counts in n (MaskedCrossEntropyLoss divides by mask.sum()), without one it does not
    t2 = target.clone()
    t2[:, ::3] = -100
    for mk in (mask, None):
        sums = class_loss_sums(logits.to(dev), t2.to(dev), None if mk is None else mk.to(dev))
        want, loss = fc.ce64(logits, t2, mk)
        assert torch.equal(sums[:, 1].cpu().double(), want[:, 1]) and rel(class_losses(sums=sums), loss) < REDUCTION
        per = nn.functional.cross_entropy(logits.double().flatten(0, 1), t2.flatten(), reduction="none")
        ref = (per * mk.flatten()).sum() / mk.sum() if mk is not None else nn.functional.cross_entropy(logits.double().flatten(0, 1), t2.flatten())
        assert rel(class_losses(sums=sums), ref) < REDUCTION
    n_masked, n_plain = (fc.ce64(logits, t2, mk)[0][:, 1].sum() for mk in (mask, None))
    assert float(n_masked) == float(mask.sum()) and float(n_plain) == float((t2 != -100).sum()) and n_masked != n_plain
    # one out-of-range target: NaN for that frame only (a masked-out one changes nothing)
    for bad_value in (10, -1, 1 << 40):
        t3 = target.clone()
        t3[3, 0] = bad_value        # (column 0 is counted in every frame)
        t3[1][~mask[1]] = bad_value  # masked out: never read
        sums = class_loss_sums(logits.to(dev), t3.to(dev), mask.to(dev), 0.1)
        assert bool(torch.isnan(sums[3]).all()) and torch.equal(sums[[0, 1, 2, 4]], whole[[0, 1, 2, 4]])
        assert bool(torch.isnan(class_losses(sums=sums)))


def test_mask_dtypes_and_views_keep_the_bits(dev):
    from lam_slide_amd import class_loss_sums
    logits, target, mask = ce_inputs(5, 65, 21, 30.0, True, 8)
    l, t, m = logits.to(dev), target.to(dev), mask.to(dev)
    want = class_loss_sums(l, t, m, 0.1)
    for mm in (m.float(), m.to(torch.uint8) * 7, m.long(), m.double() * 0.5):
        assert torch.equal(class_loss_sums(l, t, mm, 0.1), want)
    wide = torch.zeros(5, 65, 40, device=dev)
    wide[..., 3:24] = l
    assert torch.equal(class_loss_sums(wide[..., 3:24], t.to(torch.int32), m, 0.1), want)
    assert torch.equal(class_loss_sums(l.transpose(0, 1).contiguous().transpose(0, 1), t.t().contiguous().t(), m.t().contiguous().t(), 0.1), want)
    # leading axes are flattened to frames
    assert torch.equal(class_loss_sums(l.reshape(5, 5, 13, 21), t.reshape(5, 5, 13), m.reshape(5, 5, 13), 0.1),
                       class_loss_sums(l.reshape(25, 13, 21), t.reshape(25, 13), m.reshape(25, 13), 0.1))
    assert torch.equal(class_loss_sums(l, t, torch.ones_like(m), 0.0), class_loss_sums(l, t, None, 0.0))  # (no ignored target: same rows, same n)


def test_a_frames_sums_have_the_same_bits_in_any_batch(dev):
    from lam_slide_amd import class_loss_sums, class_losses
    for A, K in ((9, 10), (130, 65)):
        logits, target, mask = ce_inputs(6, A, K, 30.0, True, 9)
        l, t, m = logits.to(dev), target.to(dev), mask.to(dev)
        whole = class_loss_sums(l, t, m, 0.1)
        halves = torch.cat([class_loss_sums(l[:3], t[:3], m[:3], 0.1), class_loss_sums(l[3:], t[3:], m[3:], 0.1)])
        assert torch.equal(halves, whole)
        assert torch.equal(class_loss_sums(l.flip(0), t.flip(0), m.flip(0), 0.1).flip(0), whole)
        assert torch.equal(torch.cat([class_loss_sums(l[i:i + 1], t[i:i + 1], m[i:i + 1], 0.1) for i in range(6)]), whole)
        assert torch.equal(class_losses(sums=halves), class_losses(l, t, m, 0.1))
        assert torch.equal(class_loss_sums(l, t, m, 0.1), whole)  # and run to run


# ---------------------------------------------------------------------------------------------------------- confusion
def test_confusion_counts_ties_and_the_meter(dev):
    from lam_slide_amd import ClassMeter, class_loss_sums
    logits, target, mask = ce_inputs(7, 65, 5, 1.0, True, 10)
    logits[0, 1] = float("nan")             # a NaN row is not counted
    logits[1, :, :] = logits[1, :, :1]      # every class equal: the lowest index wins
    logits[2, :, 3] = logits[2].max(-1).values
    logits[2, :, 1] = logits[2, :, 3]       # classes 1 and 3 tie for the maximum (unless 0 holds it too): 1 wins
    target[3, ::2] = -100
    for mk in (mask, None):
        c = torch.zeros(5, 5, dtype=torch.int64, device=dev)
        without = class_loss_sums(logits.to(dev), target.to(dev), None if mk is None else mk.to(dev))
        sums = class_loss_sums(logits.to(dev), target.to(dev), None if mk is None else mk.to(dev), confusion=c)
        want = fc.confusion_np(logits, target, mk)
        assert np.array_equal(c.cpu().numpy(), want)
        assert torch.equal(torch.nan_to_num(sums), torch.nan_to_num(without))  # the counts change no sum
        class_loss_sums(logits.to(dev), target.to(dev), None if mk is None else mk.to(dev), confusion=c)
        assert np.array_equal(c.cpu().numpy(), 2 * want)  # a second call accumulates
    rows1 = fc.confusion_np(logits[1:2], target[1:2])
    assert rows1[:, 1:].sum() == 0 and rows1[:, 0].sum() == 65
    assert fc.confusion_np(logits[2:3], target[2:3])[:, 3].sum() == 0
    meter = ClassMeter(5)
    meter.update(logits[:4].to(dev), target[:4].to(dev), mask[:4].to(dev))
    meter.update(logits[4:].to(dev), target[4:].to(dev), mask[4:].to(dev))
    want = fc.confusion_np(logits, target, mask)
    assert np.array_equal(meter.confusion.cpu().numpy(), want)
    got = meter.compute()
    diag = np.diag(want).astype(np.float64)
    safe = lambda a, b: np.where(b > 0, a / np.maximum(b, 1), 0.0)  # noqa: E731
    assert all(v.is_cuda for v in got.values())
    assert float(got["accuracy"]) == pytest.approx(diag.sum() / want.sum(), rel=1e-12)
    assert got["precision_per_class"].cpu().numpy() == pytest.approx(safe(diag, want.sum(0)), rel=1e-12)
    assert got["recall_per_class"].cpu().numpy() == pytest.approx(safe(diag, want.sum(1)), rel=1e-12)
    assert float(got["precision"]) == pytest.approx(safe(diag, want.sum(0)).mean(), rel=1e-12)
    assert float(got["recall"]) == pytest.approx(safe(diag, want.sum(1)).mean(), rel=1e-12)


# ---------------------------------------------------------------------------------------------------------- end to end
def geometry_bounds(delta, mask, D):
    """tests/test_hip_geom_losses.py:5-12: bounds on |sqrt(pos) - sqrt(ref)|, |norm - ref|, |sqrt(inter) - sqrt(ref)| from the deviation
    delta [F, A, D] of the positions under the mask [F, A]."""
    m = mask.double()
    nd = delta.double().norm(dim=-1)
    pos = float(((nd * m) ** 2).sum().sqrt() / (D * m.sum()).sqrt())
    norm = float((nd * m).sum() / m.sum())
    pair = m[:, :, None] * m[:, None, :] * (nd[:, :, None] + nd[:, None, :]) ** 2
    inter = float((pair.sum() / (m.sum(-1) ** 2).sum()).sqrt())
    return pos, norm, inter


PARITY_LINES = []


@pytest.mark.parametrize("name", fc.MODELS)
def test_autoencoder_and_drop_in_end_to_end(golden, name, dev):
    from lam_slide_amd import Stage1Autoencoder, peptide_losses
    m = fc.model(golden, name)
    x = m.x.to(dev)
    ae = Stage1Autoencoder(m.p, encoder=m.enc_kw, decoder=m.dec_kw, prepare_inputs=lambda batch: x, scale=m.scale, mask=name != "peptide",
                           output_shapes={"atom14_pos": (14, 3)} if name == "peptide" else None)
    batch = {k: v.to(dev) for k, v in m.batch.items()}
    z = ae.encode(batch)
    # against the fp64 oracle on the SAME prepare_inputs output (the fixture's fp32 one): the reference's fp64 rerun recomputes that output
    # too, and md17's PointEmbed (sines of positions times 2^k pi) moves by 1.6e-2 between fp32 and fp64, its latents by 3.2e-4
    z_ref = fc.harness.encode(sc.to64(m.p), m.es, m.x.double(), m.batch["entities"], m.mask)
    parity(f"fs.e2e.{name}.latents", rel_l2(z.cpu(), z_ref), 2e-6)
    loss = fc.make_loss(golden, m)
    got, preds = loss(ae, batch)
    assert list(got) == list(m.loss64) and list(preds) == m.heads and set(loss.last_paths.values()) == {"fused"}
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in got.values())
    PARITY_LINES.append(f"{name}: latents rel L2 vs the fp64 oracle on the same inputs {rel_l2(z.cpu(), z_ref):.3e}, vs the reference's fp64 rerun "
                        f"{rel_l2(z.cpu(), m.z64):.3e} (the reference's own fp32 run: {rel_l2(m.z, m.z64):.3e})")
    pos_key = "atom14_pos" if name == "peptide" else "pos"
    delta = preds[pos_key].cpu().double() - m.preds64[pos_key]
    if name == "peptide":
        delta, gmask, D = delta.reshape(delta.shape[0], -1, 3), m.batch["atom14_mask"].reshape(delta.shape[0], -1), 3
    else:
        gmask, D = m.batch["attention_mask"], delta.shape[-1]
    b_pos, b_norm, b_inter = geometry_bounds(delta, gmask, D)
    PARITY_LINES.append(f"{name}: decoded {pos_key} max |delta| {float(delta.abs().max()):.3e}; bounds sqrt(pos) {b_pos:.3e} norm {b_norm:.3e} sqrt(inter) {b_inter:.3e}")
    ref = {k: float(v) for k, v in m.loss64.items()}

    def record(k, diff, bound):
        PARITY_LINES.append(f"{name}: {k} device {float(got[k]):.8f} reference fp64 {ref[k]:.8f} |diff| {diff:.3e} bound {bound:.3e}")
        print(f"PARITY fs.e2e.{name}.{k} measured {diff:.3e} bar {bound:.1e}")
        assert diff <= bound, (name, k, diff, bound)

    for k, bound, root in (("pos_loss", b_pos, True), ("norm_loss", b_norm, False), ("inter_distance_loss", b_inter, True)):
        g_, r_ = (float(got[k]) ** 0.5, ref[k] ** 0.5) if root else (float(got[k]), ref[k])
        record(k, abs(g_ - r_), bound + REDUCTION * r_)
    record("dist", abs(float(got["dist"]) - ref["dist"]), m.scale * (b_norm + REDUCTION * ref["norm_loss"]) + 1e-6 * ref["dist"])  # (+ the fp32 product)
    class_keys = {"md17": [("atom_type_loss", "atom")], "nba": [("team_loss", "team"), ("group_loss", "group")], "peptide": [("res_type_loss", "aatype")]}[name]
    for k, head in class_keys:
        dl = float((preds[head].cpu().double() - m.preds64[head]).abs().max())
        PARITY_LINES.append(f"{name}: logits of {head} max |delta| {dl:.3e}")
        record(k, abs(float(got[k]) - ref[k]), 2 * dl + REDUCTION * ref[k])
    if name == "peptide":
        # frames and torsions: the bits of peptide_losses on the decoded positions; the reduction alone on the reference's own predictions
        args = (batch["atom14_pos"], batch["atom14_pos_frame"], batch["atom14_mask"], batch["torsions"], batch["torsions_mask"], batch["aatype"])
        same = peptide_losses(preds["atom14_pos"], *args, kind=0, residue_tables=loss.tables)
        alone = peptide_losses(m.preds["atom14_pos"].to(dev), *args, kind=0, residue_tables=loss.tables)
        for k in ("pos_frame_loss", "torsion_loss", "pos_loss", "norm_loss", "inter_distance_loss"):
            assert torch.equal(same[k], got[k]), k
        record("pos_frame_loss", abs(float(alone["pos_frame_loss"]) - ref["pos_frame_loss"]), REDUCTION * ref["pos_frame_loss"])
        record("torsion_loss", abs(float(alone["torsion_loss"]) - ref["torsion_loss"]), REDUCTION * ref["torsion_loss"] + 1e-6)
    # the weighted total, restated from the device's own terms
    w = m.weights
    terms = {"loss_pos_weight": "pos_loss", "loss_inter_distance_weight": "inter_distance_loss", "loss_norm_weight": "norm_loss",
             "loss_atom_type_weight": "atom_type_loss", "loss_team_weight": "team_loss", "loss_group_weight": "group_loss",
             "loss_pos_frame_weight": "pos_frame_loss", "loss_res_type_weight": "res_type_loss", "loss_torsion_weight": "torsion_loss"}
    total = sum(w[a] * float(got[terms[a]]) for a in w)
    assert abs(float(got["loss"]) - total) <= 1e-6 * abs(total)
    PARITY_LINES.append(f"{name}: loss device {float(got['loss']):.8f} reference fp64 {ref['loss']:.8f}")
    print("\n".join(line for line in PARITY_LINES if line.startswith(name)))


class MaskedHuberLoss(nn.Module):
    """modules/losses.py:16-24 restated: not a module the device form computes."""

    def __init__(self, delta: float = 1.0):
        super().__init__()
        self.huber_loss = nn.HuberLoss(reduction="none", delta=delta)

    def forward(self, input, target, mask):
        return (self.huber_loss(input, target).mean(dim=1) * mask).sum() / mask.sum()


def test_a_module_outside_the_defaults_takes_the_torch_path_for_its_term_alone(golden, dev):
    m = fc.model(golden, "md17")
    preds = {k: v.to(dev) for k, v in m.preds.items()}
    batch = {k: v.to(dev) for k, v in m.batch.items()}
    model = fc.Fixed(preds, m.scale)
    base_loss, huber_loss = fc.make_loss(golden, m), fc.make_loss(golden, m, loss_pos=MaskedHuberLoss())
    base, _ = base_loss(model, batch)
    got, _ = huber_loss(model, batch)
    assert set(base_loss.last_paths.values()) == {"fused"}
    assert huber_loss.last_paths == {"loss_pos": "generic", "loss_inter_distance": "fused", "loss_norm": "fused", "loss_atom_type": "fused"}
    for k in ("inter_distance_loss", "atom_type_loss", "norm_loss", "dist"):
        assert torch.equal(got[k], base[k]), k
    mask = m.batch["attention_mask"].double().flatten()
    want = (nn.functional.huber_loss(m.preds["pos"].double().flatten(0, 1), m.batch["pos"].double().flatten(0, 1), reduction="none").mean(1) * mask).sum() / mask.sum()
    assert got["pos_loss"].is_cuda and rel(got["pos_loss"], want) < 1e-6
    total = sum(m.weights[a] * float(got[k]) for a, k in (("loss_pos_weight", "pos_loss"), ("loss_inter_distance_weight", "inter_distance_loss"),
                                                          ("loss_atom_type_weight", "atom_type_loss"), ("loss_norm_weight", "norm_loss")))
    assert abs(float(got["loss"]) - total) <= 1e-6 * abs(total)
    # a smoothed MaskedCrossEntropyLoss-shaped module with weights is not the default either
    class Weighted(nn.Module):
        def forward(self, logits, target, mask):
            return (nn.functional.cross_entropy(logits, target, reduction="none") * mask).sum() / mask.sum() * 2.0

    other = fc.make_loss(golden, m, loss_atom_type=Weighted())
    got2, _ = other(model, batch)
    assert other.last_paths["loss_atom_type"] == "generic" and rel(got2["atom_type_loss"], 2.0 * float(base["atom_type_loss"])) < 1e-5
