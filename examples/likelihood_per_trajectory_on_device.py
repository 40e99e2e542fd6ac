#!/usr/bin/env python3
"""Per-sample log-likelihoods that do not depend on the batch, on one MI355X with synthetic (seeded) weights:
`Sampler.sample_ode_likelihood(controller="device", step_control="trajectory")` runs the whole adaptive solve of the augmented state
`[x | logp]` inside the library (`lsl_dopri_logp_*`) with a step controller per trajectory and the Rademacher probes drawn on
the device from one seed per trajectory.  A batch of 4 is solved in one call, then every trajectory alone with its own seed: the same bits.
The default keywords (one controller for the batch) give every trajectory another `logp` than its solo call - the numbers people compare
across runs should not depend on what else was in the batch.

    python examples/likelihood_per_trajectory_on_device.py [--T 30] [--L 16] [--num-steps 10]
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
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--num-steps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (the package has no CPU path)"
    dev = torch.device("cuda:0")
    B, T, L, Cc = 4, args.T, args.L, 32

    net = LatentSIV3(depth=4, in_dim=Cc, hidden_size=256, num_heads=16, mlp_ratio=2, reset_parameters=False)
    net.load_state_dict(seeded_state_dict(net, seed=0))
    net.to(dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, L, Cc, generator=g).to(dev) * torch.tensor([1.0, 2.0, 0.5, 1.5], device=dev).reshape(B, 1, 1, 1)
    kw = {"x_cond": torch.randn(B, T, L, Cc, generator=g).to(dev), "x_cond_mask": (torch.rand(B, T, L, generator=g) < 0.2).long().to(dev)}
    seeds = [101, 102, 103, 104]                                           # one probe stream per trajectory

    def call(xs, kws, probe_seeds, **keywords):
        s = Sampler(CreateTransport("Linear", "velocity")())
        fn = s.sample_ode_likelihood(num_steps=args.num_steps, controller="device", probe_seeds=probe_seeds, **keywords)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        logp, z = fn(xs, net, **kws)
        torch.cuda.synchronize()
        return logp, s, (time.perf_counter() - t0) * 1e3

    logp, s, ms = call(x, kw, seeds, step_control="trajectory")
    assert s.last_path == "likelihood-device-solve-each"
    attempts = [a + r for a, r in zip(s.last_ode_stats["accepted"], s.last_ode_stats["rejected"])]
    print(f"one call, a controller per trajectory: {ms:.1f} ms, attempts per trajectory {attempts}, {s.last_ode_stats['network_passes']} tangent passes")
    batch, sb, _ = call(x, kw, seeds)                                       # one controller for the batch: other steps, other numbers
    for b in range(B):
        solo, _, _ = call(x[b:b + 1].contiguous(), {k: v[b:b + 1].contiguous() for k, v in kw.items()}, seeds[b:b + 1])
        same = torch.equal(solo[0], logp[b])
        print(f"  trajectory {b}: log p = {float(logp[b]):.4f}   alone {float(solo[0]):.4f} ({'same bits' if same else 'DIFFERENT'})   "
              f"under the batch's controller {float(batch[b]):.4f}")
        assert same
    print("(random weights: the numbers only show the plumbing)")


if __name__ == "__main__":
    main()
