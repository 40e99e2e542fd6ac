#!/usr/bin/env python3
"""Exact-flow log-likelihood of latent trajectories on one MI355X with synthetic (seeded) weights: `Sampler.sample_ode_likelihood` integrates
the probability-flow ODE from the data to the prior with the log-density change beside it; every drift evaluation is one tangent pass of the
library (`LatentSIV3.jvp`: the network output and its directional derivative along a Rademacher probe, forward mode - no activation tape) and one
`lsl_dot_rows` (Hutchinson's eps . J eps in fp64).

Mirrors `Sampler.sample_ode_likelihood` of the reference (modules/transport/transport.py:413-473); with a trained checkpoint, load its state dict
instead of the seeded one.

    python examples/likelihood_on_device.py [--B 4] [--T 30] [--L 16] [--method dopri5]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lam_slide_amd import CreateTransport, LatentSIV3, Sampler  # noqa: E402
from lam_slide_amd.synthetic import seeded_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--method", default="dopri5", choices=["dopri5", "euler", "midpoint", "heun3", "rk4"])
    ap.add_argument("--num-steps", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (the package has no CPU path)"
    dev = torch.device("cuda:0")
    B, T, L, Cc = args.B, args.T, args.L, 32

    net = LatentSIV3(depth=4, in_dim=Cc, hidden_size=256, num_heads=16, mlp_ratio=2, reset_parameters=False)
    net.load_state_dict(seeded_state_dict(net, seed=0))
    net.to(dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, L, Cc, generator=g).to(dev)                     # the latents whose likelihood is asked for
    x_cond = torch.randn(B, T, L, Cc, generator=g).to(dev)
    x_cond_mask = (torch.rand(B, T, L, generator=g) < 0.2).long().to(dev)

    torch.manual_seed(0)                                                  # the probes come from torch's generator, as in the reference
    sampler = Sampler(CreateTransport("Linear", "velocity")())
    fn = sampler.sample_ode_likelihood(sampling_method=args.method, num_steps=args.num_steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logp, z = fn(x, net, x_cond=x_cond, x_cond_mask=x_cond_mask)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert sampler.last_path == "likelihood-device"
    n_el = x[0].numel()
    bpd = -logp / (n_el * 0.6931471805599453)                             # bits per dimension
    print(f"{B} trajectories of {T} x {L} x {Cc}: {sampler.last_ode_stats['nfe']} drift evaluations in {dt * 1e3:.1f} ms; "
          f"log p = {[round(float(v), 2) for v in logp]}  bits/dim = {[round(float(v), 3) for v in bpd]}  |z| rms {float(z.pow(2).mean().sqrt()):.3f}  "
          f"(random weights: the numbers only show the plumbing)")


if __name__ == "__main__":
    main()
