"""What tests/test_first_stage.py (CPU) and tests/test_hip_first_stage.py (GPU) share of fixture F19 (tools/make_fixtures.py f19: the
reference's real first-stage Wrappers of md17 / nba / peptide, model_step in fp32 and in fp64): the oracle shapes, the constructor keywords
of Stage1Encoder / Stage1Decoder, the batches, the drop-in Loss of each model built from the fixture's weights, and fp64 restatements of
the class losses and the confusion counts."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import harness

MODELS = ("md17", "nba", "peptide")
FIXTURE = "f19_first_stage.npz"


def model(golden, name):
    """Everything F19 holds of one model, and what the oracle and the package need to rebuild it."""
    f = golden(FIXTURE)
    ec, ed, nl, dl = (int(v) for v in f[name + ".meta/enc_heads"])
    dc, dd, dnl, ddl = (int(v) for v in f[name + ".meta/dec_heads"])
    p = f.group(name + ".p")
    m = SimpleNamespace(name=name, p=p, batch=f.group(name + ".batch"), x=f[name + ".x"], z=f[name + ".z"], z64=f[name + ".z64"], x64=f[name + ".x64"],
                        preds=f.group(name + ".preds"), preds64=f.group(name + ".preds64"), loss32=f.group(name + ".loss32"),
                        loss64=f.group(name + ".loss64"), weights={k: float(v) for k, v in f.group(name + ".weights").items()},
                        scale=float(f[name + ".meta/scale"]), heads=[str(h) for h in f.raw[name + ".meta/heads"]])
    # (an npz holds no order: the heads back in the order of the reference's ModuleDict, which the fixture stores as a list of names)
    head_of = lambda k: k.split(".")[2] if k.startswith("decoder.output_layers.") else None  # noqa: E731
    m.p = p = {**{k: v for k, v in p.items() if head_of(k) is None}, **{k: v for h in m.heads for k, v in p.items() if head_of(k) == h}}
    dim_latent = p["encoder.latents"].shape[1]
    m.es = harness.EncoderShape(dim_input=m.x.shape[-1], dim_latent=dim_latent, num_latents=p["encoder.latents"].shape[0], num_head_cross=ec,
                                dim_head_cross=ed, num_head_latent=nl, dim_head_latent=dl)
    m.ds = harness.DecoderShape(dim_latent=dim_latent, num_head_cross=dc, dim_head_cross=dd, num_head_latent=dnl, dim_head_latent=ddl)
    m.enc_kw = dict(num_head_cross=ec, dim_head_cross=ed, num_head_latent=nl, dim_head_latent=dl)
    m.dec_kw = dict(num_head_cross=dc, dim_head_cross=dd, num_head_latent=dnl, dim_head_latent=ddl)
    m.mask = None if name == "peptide" else m.batch["attention_mask"]  # (first_stage/peptide.py:77-80 encodes without a mask)
    return m


def flat(t):
    """A stored head as the decoder returns it: [F, A, out_dim] (the peptide's atom14_pos is stored [F, R, 14, 3])."""
    return t.reshape(t.shape[0], t.shape[1], -1)


def shaped(m, preds):
    """The heads as the model's Loss reads them: the peptide's atom14_pos [F, R, 42] -> [F, R, 14, 3]."""
    out = dict(preds)
    if "atom14_pos" in out and out["atom14_pos"].dim() == 3:
        out["atom14_pos"] = out["atom14_pos"].reshape(*out["atom14_pos"].shape[:-1], 14, 3)
    return out


def tables(golden):
    """The reference's residue tables, as F18 stores them."""
    return {k: v.numpy() for k, v in golden("f18_peptide_loss.npz").group("tables").items()}


def make_loss(golden, m, **kw):
    """The drop-in of model m with the weights of the reference's YAML (as stored in F19)."""
    from lam_slide_amd import first_stage as fs
    cls = {"md17": fs.MD17Loss, "nba": fs.NBALoss, "peptide": fs.PeptideLoss}[m.name]
    if m.name == "peptide":
        kw.setdefault("residue_tables", tables(golden))
        kw.setdefault("loss_inter_distance", InterDistanceLoss())  # (the YAML names it; the constructor's default is MaskedMSELoss)
    return cls(**m.weights, **kw)


class InterDistanceLoss(torch.nn.Module):
    """modules/losses.py:126-134 restated (the module the first-stage YAMLs name for ``loss_inter_distance``)."""

    def forward(self, preds, targets, mask):
        diag = mask.unsqueeze(-1) * mask.unsqueeze(-2)
        return (((torch.cdist(preds, preds) - torch.cdist(targets, targets)) * diag) ** 2).sum() / diag.sum()


class Fixed:
    """What a first-stage Loss touches of the model: ``model(batch)`` and ``model.scale``; hands back the given predictions."""

    def __init__(self, preds, scale):
        self.preds, self.scale = preds, scale

    def __call__(self, batch):
        return self.preds


def ce64(logits, target, mask=None, eps=0.0):
    """fp64 restatement of lsl_class_loss_sums + final on the CPU: (sums [F, 2], loss).  logits [F, A, K]."""
    l = logits.double().cpu()
    t = target.cpu()
    K = l.shape[-1]
    lse = torch.logsumexp(l, dim=-1)
    ok = (t != -100) & ((mask.cpu() != 0) if mask is not None else torch.ones_like(t, dtype=torch.bool))
    ly = torch.gather(l, -1, t.clamp(0, K - 1)[..., None])[..., 0]
    loss = (1 - eps) * (lse - ly) + (eps * (lse - l.mean(-1)) if eps > 0 else 0.0)
    s = torch.where(ok, loss, torch.zeros_like(loss)).sum(-1)
    n = ((mask.cpu() != 0) if mask is not None else ok).double().sum(-1)
    return torch.stack([s, n], dim=-1), s.sum() / n.sum()


def confusion_np(logits, target, mask=None):
    """Integer counts [K, K] with numpy: cell [target, argmax] (np.argmax: the first of equal maxima) of every counted row."""
    l, t = logits.cpu().numpy(), target.cpu().numpy()
    K = l.shape[-1]
    ok = (t != -100) & (np.ones_like(t, dtype=bool) if mask is None else mask.cpu().numpy() != 0) & ~np.isnan(l).any(-1)
    c = np.zeros((K, K), dtype=np.int64)
    np.add.at(c, (t[ok], np.argmax(l[ok], axis=-1)), 1)
    return c
