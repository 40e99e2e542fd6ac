#!/usr/bin/env python3
"""Aligned frames, RMSD and RMSF of a sampled peptide trajectory on one MI355X with synthetic (seeded) weights: chained rollouts of one
system (frozen stage-1 encode -> conditioning -> fused sampler -> frozen stage-1 decode) -> `superpose_atom14` onto the conditioning frame
-> `rmsd` to it -> `rmsf` of the heavy atoms, with one host read at the end.

Mirrors `eval_peptide.py:347` (`traj_pred.superpose(traj_pred)` before the trajectory is written) and what anyone asks of an MD-like
trajectory first, without the mdtraj trajectory: the positions never leave the device.  With a trained checkpoint, pass its state dicts
instead of the seeded ones and the peptide's own `aatype`.

    python examples/peptide_superpose_on_device.py [--rollouts 4] [--T 64]
"""
import argparse
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import CreateTransport, LatentSIV3, SecondStageSampler, Stage1Decoder, Stage1Encoder  # noqa: E402
from lam_slide_amd import RolloutSampler, StructureTables, rmsd, rmsf, superpose  # noqa: E402
from lam_slide_amd.synthetic import seeded_decoder_state_dict, seeded_encoder_state_dict, seeded_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=4)
    ap.add_argument("--T", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (the package has no CPU path)"
    dev = torch.device("cuda:0")
    T, R, L = args.T, 6, 8
    A = R * 14

    # the residue tables are the host application's (residue_constants); here: the copy the test fixtures hold
    tables = {}
    for part in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "f18_peptide_loss*.npz"))):
        tables.update({k[len("tables/"):]: v for k, v in np.load(part).items() if k.startswith("tables/")})
    aatype = [1, 13, 10, 18, 0, 7]  # ARG PHE LEU TYR ALA GLY
    st = StructureTables(aatype, tables)
    on = st.on(dev)  # the heavy atoms of the topology and the padding slots among the index tables: uploaded once
    heavy = (st.topology, on["topology"])  # (host table, device table): a selection that uploads nothing

    enc = Stage1Encoder(seeded_encoder_state_dict(num_latents=L, n_entities=128, seed=1), num_head_cross=8, dim_head_cross=16, num_head_latent=2,
                        dim_head_latent=16)
    dec = Stage1Decoder(seeded_decoder_state_dict(out_dim=3, n_entities=128, seed=2), num_head_latent=2, dim_head_latent=16, num_head_cross=8,
                        dim_head_cross=16)
    net = LatentSIV3(depth=6, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=4, reset_parameters=False)
    net.load_state_dict(seeded_state_dict(net, seed=0))
    net.to(dev)
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 1), mask_cond_mean=True,
                             sampling_kwargs={"sampling_method": "euler", "num_steps": 21})

    g = torch.Generator().manual_seed(3)
    feat = torch.randn(3, 128, generator=g).to(dev)      # stands for the dataset's prepare_inputs: positions -> encoder input
    entities = torch.arange(A, device=dev)[None].expand(T, A).contiguous()
    mask = torch.ones(T, A, dtype=torch.bool, device=dev)
    res_mask = torch.from_numpy(~st.padding.reshape(R, 14)).to(dev)
    # a conditioning frame in nanometres: C-alpha atoms 0.38 apart along a bent line, the heavy atoms 0.15 around them, the padding slots zero
    ca = torch.cumsum(0.38 * torch.nn.functional.normalize(torch.tensor([1.0, 0.0, 0.0]) + 0.6 * torch.randn(R, 3, generator=g), dim=-1), dim=0)
    cond = (ca[:, None, :] + 0.15 * torch.randn(R, 14, 3, generator=g)).to(dev) * res_mask[..., None]

    class Model:
        """What RolloutSampler needs of the peptide LightningModule: ``sample(batch)`` -> {"atom14_pos": [1, T, R, 14, 3]} from the batch
        ``create_batch`` builds (every frame repeats the conditioning frame), ``shift``, ``scale``, ``n_timesteps``."""
        shift, scale, n_timesteps = 0.0, 1.0, T

        def sample(self, batch):
            pos = batch["atom14_pos"].reshape(T, A, 3)   # all on the device
            z = enc.encode((pos @ feat).contiguous(), entities, mask)
            out = pos + 0.02 * dec.decode(drv.sample_latents(z[None])[0], entities)  # (seeded weights: keep the frames near the geometry)
            return {"atom14_pos": out.reshape(1, T, R, 14, 3) * res_mask[..., None]}

    sampler = RolloutSampler(Model())
    res = torch.tensor(aatype, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # the rollouts, then every frame fitted onto the first (the conditioning frame) on its heavy atoms, in place: eval_peptide.py:347
    pos = sampler.sample_rollout(cond, res, res_mask, num_rollouts=args.rollouts, superpose=True, tables=tables)   # [rollouts * T, R, 14, 3]
    frames = pos.reshape(-1, A, 3)
    dist = rmsd(frames, frame=0, atom_indices=heavy)                    # float32 [F]: the RMSD to the conditioning frame after the fit
    fluct, mean = rmsf(frames, atom_indices=heavy, return_mean=True)    # float32 [n heavy], float64 [n heavy, 3]: of the aligned frames
    summary = torch.stack([dist.max().double(), dist.mean().double(), fluct.max().double(), fluct.mean().double()]).cpu()  # the one host read
    dt = time.perf_counter() - t0
    print(f"{args.rollouts} rollouts x {T} frames of {R} residues, {st.topology.size} heavy atoms: {dt * 1e3:.1f} ms "
          f"({superpose.last_path['superpose_atom14']} / {superpose.last_path['rmsd']} / {superpose.last_path['rmsf']} path)  "
          f"rmsd to the conditioning frame max {summary[0]:.4f} mean {summary[1]:.4f} nm, rmsf max {summary[2]:.4f} mean {summary[3]:.4f} nm"
          "  (random weights: the numbers only show the plumbing)")


if __name__ == "__main__":
    main()
