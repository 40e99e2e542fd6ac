#!/usr/bin/env python3
"""Cost of k-means fitting at its two shapes: the microstates of the peptide evaluation (S = 1, n = 10^6 projected reference frames, k = 100,
d = 4, 100 Lloyd iterations: ``analysis.get_kmeans``) and the ``post_process`` branch of the NBA test_step (S = 11 264 agents, n = K = 60
final frames, k = 20, d = 2).

  device     ``kmeans_fit`` on the GPU (``lsl_kmeans_step`` x iterations + the final pass; "stride" seeding, ``rel_tol = 0``: every
             series runs until no label changes or ``max_iter``), HIP events around the whole call
  torch      the module's own float64 restatement (``kmeans._fit_torch``) on the same device and inputs, HIP events
  numpy      a float64 Lloyd iteration on the host (``cdist(...).argmin``, ``np.add.at``, a division), wall clock; ``--host-iters``
             iterations are timed and the per-iteration time is reported beside its multiple
One warm-up, then the median of several runs.  A record, not a gate: the numbers are written to profiles/kmeans_cost.txt.
Usage (GPU box):  python tools/kmeans_cost.py [--runs 3] [--iters 100] [--host-iters 2]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.spatial.distance import cdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import kmeans  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--host-iters", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_cost.txt"))
args = ap.parse_args()
dev = torch.device("cuda:0")


def data(S, n, d, comps, seed):
    """Seeded float32 [S, n, d]: overlapping Gaussian mixtures (the iteration does not stop early on them)."""
    rng = np.random.default_rng(seed)
    means = 1.5 * rng.standard_normal((S, comps, d))
    comp = rng.integers(0, comps, size=(S, n))
    return (means[np.arange(S)[:, None], comp] + rng.standard_normal((S, n, d))).astype(np.float32)


def median_ms(fn):
    fn()  # warm-up
    times = []
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def numpy_iteration(y, c):
    """One Lloyd iteration of every series on the host -> the new centres."""
    out = c.copy()
    for s in range(y.shape[0]):
        y64 = y[s].astype(np.float64)
        lab = np.concatenate([cdist(y64[i:i + 65536], c[s].astype(np.float64), "sqeuclidean").argmin(1) for i in range(0, y64.shape[0], 65536)])
        sums = np.zeros((c.shape[1], y.shape[2]))
        np.add.at(sums, lab, y64)
        cnt = np.bincount(lab, minlength=c.shape[1])
        out[s][cnt > 0] = (sums[cnt > 0] / cnt[cnt > 0, None]).astype(np.float32)
    return out


lines = [f"k-means fitting, {args.iters} Lloyd iterations at most, \"stride\" seeding, rel_tol = 0; measured on {torch.cuda.get_device_name(0)} "
         f"(torch {torch.__version__}), host side on this box's CPU with numpy {np.__version__}; median of {args.runs} runs (min, max)"]
with torch.no_grad():
    for name, (S, n, k, d, comps) in (("peptide microstates", (1, 1_000_000, 100, 4, 30)), ("NBA post_process", (11264, 60, 20, 2, 5))):
        y = data(S, n, d, comps, seed=S)
        yd = torch.from_numpy(y).to(dev)
        c0 = kmeans.initial_centers(yd, k, "stride")
        res = kmeans.kmeans_fit(yd, k, init=c0, max_iter=args.iters, rel_tol=0.0)
        assert res.path == "fused"
        it = res.n_iter.double()
        lines.append(f"{name}: S = {S}, n = {n}, k = {k}, d = {d}; iterations run: mean {float(it.mean()):.1f}, max {int(it.max())}, "
                     f"converged {int(res.converged.sum())} of {S}")
        lines.append("  device (kmeans_fit, HIP events, binding included): %10.3f ms  (min %.3f, max %.3f)"
                     % median_ms(lambda: kmeans.kmeans_fit(yd, k, init=c0, max_iter=args.iters, rel_tol=0.0)))
        lines.append("  torch float64 restatement on the same device:      %10.3f ms  (min %.3f, max %.3f)"
                     % median_ms(lambda: kmeans._fit_torch(yd, c0, args.iters, 0.0, 0.0)))
        c = c0.cpu().numpy()
        t = time.perf_counter()
        for _ in range(args.host_iters):
            c = numpy_iteration(y, c)
        per = (time.perf_counter() - t) * 1e3 / args.host_iters
        lines.append(f"  numpy on the host: {per:10.3f} ms per iteration ({args.host_iters} timed), x {float(it.max()):.0f} iterations = {per * float(it.max()):.1f} ms")
print("\n".join(lines))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
