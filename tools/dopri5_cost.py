#!/usr/bin/env python3
"""Wall time of one adaptive dopri5 sampling call with the step controller on the host (``controller="host"``: dopri5_solve around the
library's network and Runge-Kutta calls, the path of the parent commit) against the controller on the device (``controller="device"``:
lsl_dopri_begin / lsl_dopri_advance) at ``attempts_per_poll`` = 1, 2, 4, 8, in one process on one box.

  peptide   the peptide evaluation's shape: B = 1, T = 1000, L = 2, the model of configs/model/peptide/second-stage_mi355x.yaml
  md17      the md17 reference shape at B = 4: T = 30, L = 192, depth 4, hidden 256
Seeded weights (lam_slide_amd/synthetic.py) and inputs, GVP / data, the reference's tolerances, ``num_steps`` output times.  A seeded network
is no trained flow: a solve is cut off after ``--max-attempts`` attempts (both controllers then stop at the same attempt, which the tool
checks), so a call is the same work on both sides.  Host clock around the call, which ends in a synchronising read on both paths; one
warm-up call per variant (it also captures the attempt's graph), the median of ``--runs`` calls.  A record, not a gate: the numbers go to
profiles/dopri5_cost.txt.
Usage (GPU box):  python tools/dopri5_cost.py [--runs 5] [--max-attempts 40] [--num-steps 50]"""
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
ap.add_argument("--max-attempts", type=int, default=40)
ap.add_argument("--num-steps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dopri5_cost.txt"))
args = ap.parse_args()
dev = torch.device("cuda:0")

SHAPES = {
    "peptide": (dict(depth=7, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4), 1, 1000, 2),
    "md17": (dict(depth=4, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2), 4, 30, 192),
}


def one_call(net, init, kw, controller, poll):
    """(seconds, attempts, accepted, result or None when the attempt limit cut the solve off)"""
    s = Sampler(CreateTransport("GVP", "data")())
    s.ode_max_steps, s.attempts_per_poll = args.max_attempts, poll
    fn = s.get_sample_fn("ODE", dict(num_steps=args.num_steps, controller=controller))
    res = None
    torch.cuda.synchronize()
    t = time.perf_counter()
    try:
        res = fn(init, net, **kw)
    except RuntimeError as e:
        if "max_steps" not in str(e):
            raise
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    if controller == "device" or res is not None:
        st = s.last_ode_stats
        return dt, st["accepted"] + st["rejected"], st["accepted"], res
    return dt, args.max_attempts, None, res  # (the host solver raises before it leaves its counters)


lines = [f"adaptive dopri5, one sampling call (GVP / data, rtol 1e-3, atol 1e-6, {args.num_steps} output times, at most {args.max_attempts} attempts); "
         f"measured on {torch.cuda.get_device_name(0)} (torch {torch.__version__}); host clock, median of {args.runs} calls after one warm-up"]
for name, (netkw, B, T, L) in SHAPES.items():
    net = LatentSIV3(reset_parameters=False, **netkw)
    net.load_state_dict(seeded_state_dict(net, seed=0))
    net = net.to(dev)
    g = torch.Generator().manual_seed(7)
    init = torch.randn(B, T, L, netkw["in_dim"], generator=g).to(dev)
    kw = {"x_cond": torch.randn(B, T, L, netkw["in_dim"], generator=g).to(dev), "x_cond_mask": (torch.rand(B, T, L, generator=g) < 0.2).long().to(dev)}
    rows = {}
    for controller, poll in (("host", 0), ("device", 1), ("device", 2), ("device", 4), ("device", 8)):
        one_call(net, init, kw, controller, poll)
        runs = [one_call(net, init, kw, controller, poll) for _ in range(args.runs)]
        rows[(controller, poll)] = (statistics.median(r[0] for r in runs), runs[-1][1], runs[-1][2], runs[-1][3])
    host_t, host_n, _, host_res = rows[("host", 0)]
    lines.append(f"{name}: B = {B}, T = {T}, L = {L}, depth {netkw['depth']}, hidden {netkw['hidden_size']}")
    lines.append(f"  controller=host                      {host_t * 1e3:9.2f} ms per call, {host_n} attempts, {host_t * 1e6 / max(host_n, 1):8.1f} us per attempt")
    for poll in (1, 2, 4, 8):
        t, n, acc, res = rows[("device", poll)]
        assert n == host_n, (name, poll, n, host_n)
        same = "" if res is None or host_res is None else f", max |device - host| {float((res - host_res).abs().max()):.2e}"
        lines.append(f"  controller=device attempts_per_poll={poll} {t * 1e3:9.2f} ms per call, {n} attempts ({acc} accepted), {t * 1e6 / max(n, 1):8.1f} us per attempt, "
                     f"host / device {host_t / t:5.2f}x{same}; a solve that finishes leaves up to {poll - 1} idle attempts "
                     f"({(poll - 1) * t * 1e3 / max(n, 1):.1f} ms) behind its last step")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
