#!/usr/bin/env python3
"""K draws of one conditioning with the reference's default sampler, adaptive dopri5, in ONE call on one MI355X with synthetic (seeded) weights.

dopri5's default step control chooses one step for the whole batch of a call, so folding K draws into a batch changes every draw's steps.
`step_control="trajectory"` gives every trajectory a step controller of its own, on the device: the network is evaluated once per stage for
all K draws, each at its own time, and draw k has the bits of the call that samples it alone - which the script checks for one of them.

    python examples/dopri5_k_draws_one_call.py [--K 8] [--T 30] [--L 64] [--check 3]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lam_slide_amd import CreateTransport, LatentSIV3, SecondStageSampler  # noqa: E402
from lam_slide_amd.synthetic import seeded_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--check", type=int, default=3, help="the draw that is sampled again alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (the package has no CPU path)"
    dev = torch.device("cuda:0")
    K, T, L, Cc = args.K, args.T, args.L, 32

    net = LatentSIV3(depth=4, in_dim=Cc, hidden_size=256, num_heads=16, mlp_ratio=2, reset_parameters=False)
    net.load_state_dict(seeded_state_dict(net, seed=0))
    net.to(dev)
    g = torch.Generator().manual_seed(3)
    latents = torch.randn(1, T, L, Cc, generator=g).to(dev)               # one conditioning window
    inits = torch.randn(K, 1, T, L, Cc, generator=g).to(dev)              # the K initial noises
    drv = SecondStageSampler(net, CreateTransport("GVP", "data")(), cond_idx=(0, 10),
                             sampling_kwargs={"sampling_method": "dopri5", "num_steps": 10, "controller": "device", "step_control": "trajectory"})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    draws = drv.sample_latents_k(latents, K, inits=inits)                 # [K, 1, T, L, C]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    stats = drv.last_sampler.last_ode_stats
    assert drv.last_sampler.last_path == "dopri5-device-each"
    attempts = [a + r for a, r in zip(stats["accepted"], stats["rejected"])]
    k = args.check % K
    alone = drv.sample_latents(latents, init=inits[k])                    # the same draw in a call of its own
    print(f"{K} draws of {T} x {L} x {Cc} in one call: {dt * 1e3:.1f} ms, {stats['network_passes']} network passes for {sum(stats['nfe'])} drift "
          f"evaluations; attempts per draw {attempts}; draw {k} equals its own call bit for bit: {torch.equal(draws[k], alone)}  "
          f"(random weights: the numbers only show the plumbing)")
    assert torch.equal(draws[k], alone)


if __name__ == "__main__":
    main()
