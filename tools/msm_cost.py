#!/usr/bin/env python3
"""Cost of one step of the reversible maximum-likelihood iteration (``lsl_msm_reversible_step``) at ns = 10, 100, 128 states, for S = 1 and
S = 300 count matrices (an evaluation estimates three models for each of about a hundred peptides).

  device     launches of ``--steps`` steps with the stop test off (``maxerr = -1``), HIP events around one launch; the time of a launch of
             0 steps (the load of K into LDS, the state written back) is measured the same way and subtracted; one warm-up, the median of
             ``--runs`` launches, in microseconds per step
  numpy      the module's float64 restatement (``msm._estimate_numpy``) of one matrix on the host, wall clock, per step
The counts come from seeded chains, dense on their active sets.  A record, not a gate: the numbers go to profiles/msm_cost.txt.
Usage (GPU box):  python tools/msm_cost.py [--runs 5] [--steps 2000] [--host-steps 200]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import _lib, msm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--host-steps", type=int, default=200)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_cost.txt"))
args = ap.parse_args()
dev = torch.device("cuda:0")


def counts(S, ns, seed):
    """Seeded int64 [S, ns, ns]: the sliding-window counts of S chains of 400 ns steps with a sticky diagonal."""
    rng = np.random.default_rng(seed)
    out = np.zeros((S, ns, ns), dtype=np.int64)
    for s in range(S):
        P = rng.random((ns, ns)) + 3.0 * np.eye(ns)
        P /= P.sum(axis=1, keepdims=True)
        out[s] = rng.multinomial(400, P)  # (row i: 400 transitions out of state i)
    return out


def median_us(fn):
    fn()  # warm-up
    times = []
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


lines = [f"reversible MSM iteration, {args.steps} steps per launch with the stop test off; measured on {torch.cuda.get_device_name(0)} (torch {torch.__version__}), "
         f"host side on this box's CPU with numpy {np.__version__}; median of {args.runs} launches"]
for ns in (10, 100, 128):
    for S in (1, 300):
        Cm = counts(S, ns, seed=ns + S)
        cd = torch.from_numpy(Cm).to(dev)
        act = torch.empty(S, ns, dtype=torch.int32, device=dev)
        na = torch.empty(S, dtype=torch.int32, device=dev)
        x = torch.empty(S, ns, dtype=torch.float64, device=dev)
        n_iter = torch.empty(S, dtype=torch.int32, device=dev)
        err = torch.empty(S, dtype=torch.float64, device=dev)
        done = torch.empty(S, dtype=torch.int32, device=dev)
        _lib.call(dev, "lsl_msm_active_set", cd.data_ptr(), S, ns, act.data_ptr(), na.data_ptr())

        def launch(steps):
            _lib.call(dev, "lsl_msm_reversible_step", cd.data_ptr(), act.data_ptr(), S, ns, steps, 2 ** 31 - 1, -1.0, 1, x.data_ptr(), n_iter.data_ptr(),
                      err.data_ptr(), done.data_ptr())

        full, empty = median_us(lambda: launch(args.steps)), median_us(lambda: launch(0))
        assert int(n_iter.min()) == 0 and int(na.min()) == ns
        launch(args.steps)
        assert int(n_iter.min()) == args.steps
        nnz = float(((Cm + Cm.transpose(0, 2, 1)) != 0).mean())
        lines.append(f"ns = {ns:3d}, S = {S:3d} (K {100 * nnz:.0f} % non-zero): {(full - empty) / args.steps:8.3f} us per step "
                     f"(launch of {args.steps} steps {full:.1f} us, of 0 steps {empty:.1f} us)")
    t = time.perf_counter()
    n = msm._estimate_numpy(Cm[0], np.ones(ns, dtype=bool), args.host_steps, -1.0)[0]
    lines.append(f"ns = {ns:3d}, numpy restatement on the host, one matrix: {(time.perf_counter() - t) * 1e6 / n:8.3f} us per step ({n} timed)")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
