#!/usr/bin/env python3
"""Wall time of adaptive dopri5 sampling of B trajectories with a step controller each, three ways, in one process on one box:

  (a) solo        B sequential ``controller="device"`` calls at B = 1 - the only way to these results without ``step_control="trajectory"``
  (b) trajectory  one ``controller="device", step_control="trajectory"`` call: the same results (the tool checks the bits), the network
                  evaluated once per stage for all trajectories; its attempts are the largest of the per-trajectory counts, not their sum
  (c) batch       one ``controller="device"`` call with the default step control: one controller for the batch, OTHER results; for context

  md17      the headline model at the md17 shape: T = 30, L = 256, depth 4, hidden 512, at B = 4 and B = 8
  peptide   the peptide evaluation's shape: T = 1000, L = 2, the model of configs/model/peptide/second-stage_mi355x.yaml, at B = 4
Seeded weights (lam_slide_amd/synthetic.py) and inputs, GVP / data, the reference's tolerances, ``num_steps`` output times.  A seeded network
is no trained flow: a trajectory is cut off after ``--max-attempts`` attempts in every arm (so a trajectory is the same work in (a) and (b)).
Host clock around the calls, each of which ends in a synchronising read; one warm-up round per arm (it also captures the attempt's graph),
the median of ``--runs`` rounds.  A record, not a gate: the numbers go to profiles/dopri5_each_cost.txt.
Usage (GPU box):  python tools/dopri5_each_cost.py [--runs 5] [--max-attempts 60] [--num-steps 50]"""
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
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--max-attempts", type=int, default=60)
ap.add_argument("--num-steps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dopri5_each_cost.txt"))
args = ap.parse_args()
dev = torch.device("cuda:0")

MD17 = dict(depth=4, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2)
PEPTIDE = dict(depth=7, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4)
CASES = (("md17", MD17, 4, 30, 256), ("md17", MD17, 8, 30, 256), ("peptide", PEPTIDE, 4, 1000, 2))


def one_call(net, init, kw, step_control):
    """(result, the sampler) of one device call; a solve the attempt limit cut off leaves its state and counters all the same"""
    s = Sampler(CreateTransport("GVP", "data")())
    s.ode_max_steps = args.max_attempts
    try:
        res = s.get_sample_fn("ODE", dict(num_steps=args.num_steps, controller="device", step_control=step_control))(init, net, **kw)
    except RuntimeError as e:
        if "max_steps" not in str(e):
            raise
        res = None
    return res, s


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def median_of(fn):
    fn()
    runs = [timed(fn) for _ in range(args.runs)]
    return statistics.median(r[0] for r in runs), runs[-1][1]


lines = [f"adaptive dopri5 with a step controller per trajectory (GVP / data, rtol 1e-3, atol 1e-6, {args.num_steps} output times, at most "
         f"{args.max_attempts} attempts a trajectory); measured on {torch.cuda.get_device_name(0)} (torch {torch.__version__}); host clock, "
         f"median of {args.runs} rounds after one warm-up"]
nets = {}
for name, netkw, B, T, L in CASES:
    if name not in nets:
        net = LatentSIV3(reset_parameters=False, **netkw)
        net.load_state_dict(seeded_state_dict(net, seed=0))
        nets[name] = net.to(dev)
    net = nets[name]
    g = torch.Generator().manual_seed(7)
    init = torch.randn(B, T, L, netkw["in_dim"], generator=g).to(dev)
    init = (init * torch.tensor([(1.0, 2.0, 0.5, 1.5)[b % 4] for b in range(B)], device=dev).reshape(-1, 1, 1, 1)).contiguous()  # (unequal solves)
    kw = {"x_cond": torch.randn(B, T, L, netkw["in_dim"], generator=g).to(dev), "x_cond_mask": (torch.rand(B, T, L, generator=g) < 0.2).long().to(dev)}
    one = lambda b: one_call(net, init[b:b + 1], {k: v[b:b + 1].contiguous() for k, v in kw.items()}, "batch")  # noqa: E731
    t_solo, solo = median_of(lambda: [one(b) for b in range(B)])
    t_each, (res_each, s_each) = median_of(lambda: one_call(net, init, kw, "trajectory"))
    t_batch, (_, s_batch) = median_of(lambda: one_call(net, init, kw, "batch"))
    solo_attempts = [s.last_ode_stats["accepted"] + s.last_ode_stats["rejected"] for _, s in solo]
    each_attempts = [a + r for a, r in zip(s_each.last_ode_stats["accepted"], s_each.last_ode_stats["rejected"])]
    assert each_attempts == solo_attempts, (each_attempts, solo_attempts)
    for b, (res, s) in enumerate(solo):  # (b) computes what (a) computes
        assert torch.equal(s_each.last_ode_state[b], s.last_ode_state[0]), b
        assert res is None or res_each is None or torch.equal(res_each[:, b], res[:, 0]), b
    batch_attempts = s_batch.last_ode_stats["accepted"] + s_batch.last_ode_stats["rejected"]
    cut = sum(a >= args.max_attempts for a in solo_attempts)
    lines.append(f"{name}: B = {B}, T = {T}, L = {L}, depth {netkw['depth']}, hidden {netkw['hidden_size']} ({T * L} tokens a trajectory); attempts per "
                 f"trajectory {solo_attempts}" + (f" ({cut} cut off at the limit)" if cut else ""))
    lines.append(f"  (a) solo:       {B} calls at B = 1      {t_solo * 1e3:9.2f} ms, {sum(solo_attempts)} attempts at B = 1, {t_solo * 1e6 / sum(solo_attempts):8.1f} us per attempt")
    lines.append(f"  (b) trajectory: one call at B = {B}     {t_each * 1e3:9.2f} ms, {max(each_attempts)} attempts at B = {B}, {t_each * 1e6 / max(each_attempts):8.1f} us per attempt; "
                 f"same bits as (a); (a) / (b) {t_solo / t_each:5.2f}x")
    lines.append(f"  (c) batch:      one call at B = {B}     {t_batch * 1e3:9.2f} ms, {batch_attempts} attempts at B = {B}, {t_batch * 1e6 / max(batch_attempts, 1):8.1f} us per attempt; "
                 f"other results (one controller for the batch)")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
