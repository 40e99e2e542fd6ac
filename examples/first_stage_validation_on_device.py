#!/usr/bin/env python3
"""First-stage validation on the MI355X with seeded weights: what ``first_stage/md17.py`` runs as ``validation_step`` - encode -> quant ->
post_quant -> decode (both heads from one trunk) -> ``Loss`` - through ``Stage1Autoencoder`` and ``first_stage.MD17Loss``, plus the
classification counts of the atom-type head (``ClassMeter``).  With a real checkpoint, pass its state dict and the backbone's own
``prepare_inputs``; in a Hydra config the loss is ``model.loss._target_=lam_slide_amd.first_stage.MD17Loss``.
Usage (GPU box):  python examples/first_stage_validation_on_device.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lam_slide_amd import ClassMeter, Stage1Autoencoder  # noqa: E402
from lam_slide_amd.first_stage import MD17Loss  # noqa: E402
from lam_slide_amd.synthetic import seeded_decoder_state_dict, seeded_encoder_state_dict  # noqa: E402

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
B, A, n_atom_types = 32, 13, 10
sd = {**seeded_encoder_state_dict(num_latents=32, seed=1), **seeded_decoder_state_dict(seed=2)}
for k in [k for k in sd if k.startswith("decoder.output_layers.pos.0.")]:  # a second head: the atom types
    sd[k.replace(".pos.", ".atom.")] = torch.randn(sd[k].shape, generator=g) * 0.05
sd["decoder.output_layers.atom.2.weight"] = torch.randn(n_atom_types, 128, generator=g) * 0.05
sd["decoder.output_layers.atom.2.bias"] = torch.zeros(n_atom_types)
lift = torch.randn(3 + n_atom_types, 128, generator=g).to(dev) * 0.3  # stands in for the backbone's embed_atom / embed_pos / net_merge


def prepare_inputs(batch):
    return torch.cat([batch["pos"], torch.nn.functional.one_hot(batch["atom"], n_atom_types).float()], dim=-1) @ lift


heads = dict(num_head_cross=8, dim_head_cross=16, num_head_latent=2, dim_head_latent=16)
model = Stage1Autoencoder(sd, encoder=heads, decoder=heads, prepare_inputs=prepare_inputs, scale=1.0)
mask = torch.ones(B, A, dtype=torch.bool)
mask[::4, 9:] = False  # padded atoms
batch = {"pos": torch.randn(B, A, 3, generator=g), "atom": torch.randint(0, n_atom_types, (B, A), generator=g),
         "entities": torch.stack([torch.randperm(32, generator=g)[:A] for _ in range(B)]), "attention_mask": mask}
batch = {k: v.to(dev) for k, v in batch.items()}
loss = MD17Loss(loss_pos_weight=1, loss_inter_distance_weight=1, loss_atom_type_weight=0.1, loss_norm_weight=0)  # configs/model/md17/first-stage.yaml
meter = ClassMeter(n_atom_types)
losses, preds = loss(model, batch)
meter.update(preds["atom"], batch["atom"], batch["attention_mask"])
print("heads:", {k: tuple(v.shape) for k, v in preds.items()}, "paths:", loss.last_paths)
print("losses:", {k: round(float(v), 6) for k, v in losses.items()})
print("meter:", {k: (round(float(v), 4) if v.dim() == 0 else [round(float(x), 3) for x in v]) for k, v in meter.compute().items()})
