#!/usr/bin/env python3
"""Wall time of ``Sampler.sample_ode_likelihood`` (adaptive dopri5, a fixed probe) on B trajectories, four ways, in one process on one box:

  (a) device-each   ``controller="device", step_control="trajectory"``: the augmented solve inside the library, a controller per trajectory
  (b) device-batch  ``controller="device"``: the same with one controller for the batch
  (c) host          the default keywords: the step controller in Python around ``LatentSIV3.jvp`` (the path of before the keywords)
  (d) host-solo     B sequential B = 1 calls of (c) - until (a), the only way to likelihoods that do not depend on the batch

  md17_ref  B = 4, T = 30, L = 192, depth 4, hidden 256
  peptide   B = 1 and B = 4, T = 1000, L = 2, depth 7, hidden 384
Seeded weights (lam_slide_amd/synthetic.py) and inputs, Linear / velocity, the reference's tolerances, ``--num-steps`` output times.  A seeded
network is no trained flow: a solve is cut off after ``--max-attempts`` attempts in every arm.  Host clock around whole calls, each of which
ends in a synchronise; one warm-up round of every arm, then ``--runs`` rounds that alternate the arms; median, minimum and maximum per arm.
A record, not a gate: the numbers go to profiles/likelihood_device_cost.txt.
Usage (GPU box):  python tools/likelihood_device_cost.py [--runs 3] [--max-attempts 40] [--num-steps 10]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import CreateTransport, LatentSIV3, Sampler  # noqa: E402
from lam_slide_amd.synthetic import seeded_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--max-attempts", type=int, default=40)
ap.add_argument("--num-steps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_device_cost.txt"))
args = ap.parse_args()
dev = torch.device("cuda:0")

MD17_REF = dict(depth=4, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2)
PEPTIDE = dict(depth=7, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4)
CASES = (("md17_ref", MD17_REF, 4, 30, 192), ("peptide", PEPTIDE, 1, 1000, 2), ("peptide", PEPTIDE, 4, 1000, 2))


def one_call(net, x, kw, eps, **keywords):
    """(logp or None, attempts as the sampler reports them or None) of one call; the attempt limit cuts a solve off in every arm alike"""
    s = Sampler(CreateTransport("Linear", "velocity")())
    s.ode_max_steps = args.max_attempts
    s.last_ode_stats = None
    logp = None
    try:
        logp, _ = s.sample_ode_likelihood(num_steps=args.num_steps, eps=eps, **keywords)(x, net, **kw)
    except RuntimeError as e:
        if "max_steps" not in str(e):
            raise
    torch.cuda.synchronize()
    st = s.last_ode_stats
    if st is None:
        return logp, None  # (the host loop keeps no counters of a solve the limit cut off)
    if isinstance(st["accepted"], list):
        return logp, [a + r for a, r in zip(st["accepted"], st["rejected"])]
    return logp, st["accepted"] + st["rejected"]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def show(attempts):
    return f"cut off at {args.max_attempts}" if attempts is None else str(attempts)


lines = [f"sample_ode_likelihood, adaptive dopri5 with a fixed probe (Linear / velocity, rtol 1e-3, atol 1e-6, {args.num_steps} output times, at most "
         f"{args.max_attempts} attempts a solve); measured on {torch.cuda.get_device_name(0)} (torch {torch.__version__}); host clock around whole "
         f"calls, one warm-up round, then {args.runs} rounds alternating the arms: median (min .. max) ms; a network pass is one tangent pass on the batch"]
nets = {}
for name, netkw, B, T, L in CASES:
    if name not in nets:
        net = LatentSIV3(reset_parameters=False, **netkw)
        net.load_state_dict(seeded_state_dict(net, seed=0))
        nets[name] = net.to(dev)
    net = nets[name]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, T, L, netkw["in_dim"], generator=g).to(dev)
    x = (x * torch.tensor([(1.0, 2.0, 0.5, 1.5)[b % 4] for b in range(B)], device=dev).reshape(-1, 1, 1, 1)).contiguous()  # (unequal solves)
    kw = {"x_cond": torch.randn(B, T, L, netkw["in_dim"], generator=g).to(dev), "x_cond_mask": (torch.rand(B, T, L, generator=g) < 0.2).long().to(dev)}
    eps = (torch.randint(2, x.shape, generator=g).float() * 2 - 1).to(dev)
    row = lambda b: (x[b:b + 1].contiguous(), {k: v[b:b + 1].contiguous() for k, v in kw.items()}, eps[b:b + 1].contiguous())  # noqa: E731
    arms = {
        "device-each": lambda: one_call(net, x, kw, eps, controller="device", step_control="trajectory"),
        "device-batch": lambda: one_call(net, x, kw, eps, controller="device"),
        "host": lambda: one_call(net, x, kw, eps),
        "host-solo": lambda: [one_call(net, xb, kb, eb) for xb, kb, eb in map(row, range(B))],
    }
    for fn in arms.values():
        fn()
    times, last = {k: [] for k in arms}, {}
    for _ in range(args.runs):
        for k, fn in arms.items():
            ms, last[k] = timed(fn)
            times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    each_attempts, batch_attempts, host_attempts = last["device-each"][1], last["device-batch"][1], last["host"][1]
    solo_attempts = [a for _, a in last["host-solo"]]
    if last["device-batch"][0] is not None and last["host"][0] is not None:
        assert batch_attempts == host_attempts, (batch_attempts, host_attempts)  # (the batch form takes the host controller's decisions)
    lines.append(f"{name}: B = {B}, T = {T}, L = {L}, depth {netkw['depth']}, hidden {netkw['hidden_size']} ({T * L} tokens a trajectory)")
    passes = lambda a: "-" if a is None else str(2 + 6 * (max(a) if isinstance(a, list) else a))  # noqa: E731
    for k, attempts in (("device-each", each_attempts), ("device-batch", batch_attempts), ("host", host_attempts)):
        lines.append(f"  {k:13s} {med[k]:9.1f} ms ({min(times[k]):.1f} .. {max(times[k]):.1f}); attempts {show(attempts)}; network passes {passes(attempts)}")
    lines.append(f"  {'host-solo':13s} {med['host-solo']:9.1f} ms ({min(times['host-solo']):.1f} .. {max(times['host-solo']):.1f}); attempts per call "
                 f"{[show(a) for a in solo_attempts]}; network passes at B = 1 "
                 f"{'-' if None in solo_attempts else sum(2 + 6 * a for a in solo_attempts)}")
    lines.append(f"  ratios: host / device-batch {med['host'] / med['device-batch']:5.2f}x (the same solve), host-solo / device-each "
                 f"{med['host-solo'] / med['device-each']:5.2f}x (batch-independent likelihoods), device-each / device-batch "
                 f"{med['device-each'] / med['device-batch']:5.2f}x")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
