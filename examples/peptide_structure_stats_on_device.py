#!/usr/bin/env python3
"""The structure statistics of the peptide validation on one MI355X with synthetic (seeded) weights: chained rollouts of one system (frozen
stage-1 encode -> conditioning -> fused sampler -> frozen stage-1 decode) -> `traj_analysis` against a reference trajectory - the
Ramachandran, pairwise-distance and radius-of-gyration Jensen-Shannon distances, the C-alpha validity and the contact-map error - with no
host round trip before the seven numbers are read.

Mirrors what `SIAtom14SampleCallback.sample_and_log` / `log_metrics` do around `SIAtom14SamplingWrapper.sample_traj` and
`traj_utils.traj_analysis`, without the mdtraj trajectories.  With a trained checkpoint, pass its state dicts instead of the seeded ones,
the peptide's own `aatype`, the MD frames as `pos_ref` and - for `tic_js` / `tic2d_js` - the projections of your TICA model.

    python examples/peptide_structure_stats_on_device.py [--rollouts 4] [--T 64]
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
from lam_slide_amd import RolloutSampler, StructureTables, structure_stats, tica_features, traj_analysis  # noqa: E402
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
    aatype = [1, 13, 10, 18, 0, 7]  # ARG PHE LEU TYR ALA GLY: three C-alpha pairs four or more residues apart
    st = StructureTables(aatype, tables)
    st.on(dev)  # C-alpha atoms and pairs, phi / psi / omega, the tica selection: uploaded once

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
    # a conditioning frame in nanometres: C-alpha atoms 0.38 apart along a bent line, the other slots 0.15 around them
    ca = torch.cumsum(0.38 * torch.nn.functional.normalize(torch.tensor([1.0, 0.0, 0.0]) + 0.6 * torch.randn(R, 3, generator=g), dim=-1), dim=0)
    cond = (ca[:, None, :] + 0.15 * torch.randn(R, 14, 3, generator=g)).to(dev)
    cond[:, 1] = ca.to(dev)

    class Model:
        """What RolloutSampler needs of the peptide LightningModule: ``sample(batch)`` -> {"atom14_pos": [1, T, R, 14, 3]} from the batch
        ``create_batch`` builds (every frame repeats the conditioning frame), ``shift``, ``scale``, ``n_timesteps``."""
        shift, scale, n_timesteps = 0.0, 1.0, T

        def sample(self, batch):
            pos = batch["atom14_pos"].reshape(T, A, 3)   # all on the device
            z = enc.encode((pos @ feat).contiguous(), entities, mask)
            out = pos + 0.02 * dec.decode(drv.sample_latents(z[None])[0], entities)  # (seeded weights: keep the frames near the geometry)
            return {"atom14_pos": out.reshape(1, T, R, 14, 3)}

    sampler = RolloutSampler(Model())
    res, res_mask = torch.tensor(aatype, device=dev), torch.ones(R, 14, device=dev)

    def trajectory(start):
        frames, pos = [], start
        for _ in range(args.rollouts):
            frames.append(sampler.sample_rollout(pos, res, res_mask, num_rollouts=1))   # [T, R, 14, 3], on the device
            pos = frames[-1][-1]
        return torch.cat(frames)

    pos_ref = trajectory(cond)                            # stands for the MD frames
    feats = tica_features(pos_ref, st)                    # tica_utils.tica_features' columns, for a TICA model of your own
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pos = trajectory(cond + 0.01)
    metrics = traj_analysis(pos, pos_ref, st)             # 0-d float64 tensors on the device: nothing synchronised so far
    values = {k: float(v) for k, v in metrics.items()}    # the reads (the callback's logger calls)
    dt = time.perf_counter() - t0
    print(f"{args.rollouts} rollouts x {T} frames of {R} residues ({feats.shape[1]} tica features): {dt * 1e3:.1f} ms "
          f"({structure_stats.last_path['traj_analysis']} path)  " + "  ".join(f"{k} {v:.3f}" for k, v in values.items())
          + "  (random weights: the numbers only show the plumbing)")


if __name__ == "__main__":
    main()
