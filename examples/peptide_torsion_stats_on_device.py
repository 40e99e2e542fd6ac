#!/usr/bin/env python3
"""The peptide evaluation's tail on one MI355X with synthetic (seeded) weights: chained rollouts of one system (each conditioned on the last
frame of the one before: frozen stage-1 encode -> conditioning -> fused sampler -> frozen stage-1 decode) -> torsion angles -> histograms
accumulated rollout by rollout -> Jensen-Shannon distances to a reference trajectory's counts and the decorrelation curves, with no host
round trip before the distances are read.

Mirrors what `eval_peptide.py` does around `SIAtom14SamplingWrapper.sample_rollout` and `analyze_trajectory`, without the xtc / pdb files
and the pyemma / mdtraj pass over them.  With a trained checkpoint, pass its state dicts instead of the seeded ones, the peptide's own
`aatype`, and the MD side's counts (a `TorsionStats` fed with the MD positions, or stored `(counts, counts2)`) as the reference.

    python examples/peptide_torsion_stats_on_device.py [--rollouts 4] [--T 64]
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
from lam_slide_amd import RolloutSampler, TorsionStats, decorrelation, eval_torsion_quads  # noqa: E402
from lam_slide_amd.synthetic import seeded_decoder_state_dict, seeded_encoder_state_dict, seeded_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollouts", type=int, default=4)
    ap.add_argument("--T", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (the package has no CPU path)"
    dev = torch.device("cuda:0")
    T, R, L = args.T, 4, 8
    A = R * 14

    # the residue tables are the host application's (residue_constants); here: the copy the test fixtures hold
    tables = {}
    for part in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "f18_peptide_loss*.npz"))):
        tables.update({k[len("tables/"):]: v for k, v in np.load(part).items() if k.startswith("tables/")})
    aatype = [1, 13, 10, 18]  # ARG PHE LEU TYR: phi / psi 1..3 and ten chi angles
    quads, labels = eval_torsion_quads(aatype, tables)

    # frozen first stage with the 56 atom slots as entities, and the second-stage backbone
    enc = Stage1Encoder(seeded_encoder_state_dict(num_latents=L, n_entities=64, seed=1), num_head_cross=8, dim_head_cross=16, num_head_latent=2,
                        dim_head_latent=16)
    dec = Stage1Decoder(seeded_decoder_state_dict(out_dim=3, n_entities=64, seed=2), num_head_latent=2, dim_head_latent=16, num_head_cross=8,
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
    cond = (2.0 * torch.randn(R, 14, 3, generator=g)).to(dev)

    class Model:
        """What RolloutSampler needs of the peptide LightningModule: ``sample(batch)`` -> {"atom14_pos": [1, T, R, 14, 3]} from the batch
        ``create_batch`` builds (every frame repeats the conditioning frame), ``shift``, ``scale``, ``n_timesteps``."""
        shift, scale, n_timesteps = 0.0, 1.0, T

        def sample(self, batch):
            pos = batch["atom14_pos"].reshape(T, A, 3)   # all on the device
            z = enc.encode((pos @ feat).contiguous(), entities, mask)
            out = pos + 0.3 * dec.decode(drv.sample_latents(z[None])[0], entities)  # (seeded weights: keep the frames near the geometry)
            return {"atom14_pos": out.reshape(1, T, R, 14, 3)}

    sampler = RolloutSampler(Model())
    res, res_mask = torch.tensor(aatype, device=dev), torch.ones(R, 14, device=dev)

    def trajectory(stats):
        """Rollouts arrive one at a time: each chunk of frames adds its counts on the device; the angles are kept for the curves."""
        angles, pos = [], cond
        for _ in range(args.rollouts):
            frames = sampler.sample_rollout(pos, res, res_mask, num_rollouts=1)   # [T, R, 14, 3]
            angles.append(stats.update(frames))  # angles [T, Q]; counts += on the device, no synchronisation
            pos = frames[-1]
        return torch.cat(angles)

    reference, stats = TorsionStats(quads, labels), TorsionStats(quads, labels)
    trajectory(reference)                                 # stands for the MD side's counts
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    angles = trajectory(stats)
    curves = decorrelation(angles, nlag=min(1000, angles.shape[0] - 1))    # [Q, nlag + 1] float32, on the device
    jsd = stats.jsd(reference)                            # out["JSD"]: the one synchronisation
    dt = time.perf_counter() - t0
    summary = TorsionStats.summary_metrics([jsd])         # calc_summary_metrics' BB / SC / ALL
    print(f"{args.rollouts} rollouts x {T} frames of {R} residues, {len(labels)} torsions: {dt * 1e3:.1f} ms ({stats.path} path)  "
          f"JSD BB {summary['BB']:.3f} SC {summary['SC']:.3f} ALL {summary['ALL']:.3f}  "
          f"{labels[1]}|{labels[2]} {jsd[labels[1] + '|' + labels[2]]:.3f}  decorrelation at lag 10: {float(curves[:, 10].mean()):.3f}  "
          f"(random weights: the numbers only show the plumbing)")


if __name__ == "__main__":
    main()
