#!/usr/bin/env python3
"""Cost of the Koopman-reweighted TICA on wide feature tables at the peptide validation's shapes: a trajectory of n = 10^4 frames of
F = 400 (a typical tetrapeptide) and F = 1344 (four Trp: the widest) ``tica_features`` columns at lag 1000.

  lsl_weighted_moments   HIP events around the call with the Koopman weights (workspace allocated outside the timed region)
  torch float64 route    the same six sums as three dgemms on a float64 copy of the table, on the same GPU: HIP events, and the peak
                         memory the route allocates (``torch.cuda.max_memory_allocated`` above the table's own bytes)
  run_tica               wall clock of the whole fit (two passes over the table, two host eigenproblems with their copies)
  projection             HIP events around ``WideTicaModel.transform`` of the table with the joint limits (dim = 40)
One warm-up, then the median of several runs.  A record, not a gate: the numbers are written to profiles/koopman_tica_cost.txt.
Usage (GPU box):  python tools/koopman_tica_cost.py [--runs 5]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import _lib, koopman_tica as kt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "koopman_tica_cost.txt"))
args = ap.parse_args()
N, LAG, DIM = 10000, 1000, 40
dev = torch.device("cuda:0")


def features(n, F, seed):
    """Seeded float32 [n, F]: two slow two-state coordinates mixed into F noisy columns (the cost does not depend on the values)."""
    rng = np.random.default_rng(seed)
    s = np.stack([np.where(np.cumsum(rng.random(n) < 1.0 / dwell) % 2 == 0, 1.0, -1.0) for dwell in (4000, 1500)], axis=1)
    return torch.from_numpy((s @ rng.standard_normal((2, F)) + rng.standard_normal((n, F)) + rng.standard_normal(F)).astype(np.float32))


def event_ms(fn):
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


def wall_ms(fn):
    fn()
    times = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


lines = [f"Koopman-reweighted TICA on wide feature tables: n = {N}, lag = {LAG}, dim = {DIM}; measured on {torch.cuda.get_device_name(0)} "
         f"(torch {torch.__version__}); median of {args.runs} runs (min, max)"]
slower = []
with torch.no_grad():
    for F in (400, 1344):
        x = features(N, F, F).to(dev)
        m = N - LAG
        model = kt.run_tica(x, LAG, DIM)
        assert kt.last_path["run_tica"] == "fused"
        w = kt.koopman_weights(x, LAG).weights(x[:m])
        lib = _lib.load()
        need = lib.lsl_weighted_moments_workspace_bytes(N, F, LAG)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(1 + 2 * F + 3 * F * F, dtype=torch.float64, device=dev)
        k_ms = event_ms(lambda: _lib.call(dev, "lsl_weighted_moments", x.data_ptr(), N, F, LAG, w.data_ptr(), out.data_ptr(), ws.data_ptr(), need))
        t_ms = event_ms(lambda: kt._wmom_torch(x, LAG, w))
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ref = kt._wmom_torch(x, LAG, w)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        worst = max(float(((a - b).abs().max() / b.abs().max())) for a, b in zip((out[0], out[1 + 2 * F:].reshape(3, F, F)), (ref[0], torch.stack(ref[3:]))))
        fit_ms = wall_ms(lambda: kt.run_tica(x, LAG, DIM))
        lim = torch.empty(2, model.dim, dtype=torch.float32, device=dev)

        def project():
            lim[0], lim[1] = float("inf"), float("-inf")
            return model.transform(x, lim)

        p_ms = event_ms(project)
        assert kt.last_path["transform"] == "fused"
        flop = 2.0 * m * ((F + 1) * (F + 2) + F * F)  # the entries computed: two upper triangles of (F + 1)^2 and one F^2, a multiply-add per row
        lines += [f"(n, F, lag) = ({N}, {F}, {LAG}): m = {m} rows, workspace {need / 2 ** 20:.1f} MiB, output {out.numel() * 8 / 2 ** 20:.1f} MiB",
                  "  lsl_weighted_moments (HIP events):                         %9.3f ms  (min %.3f, max %.3f)" % k_ms + f"   {flop / k_ms[0] / 1e9:.1f} TFLOP/s fp64 on the entries computed",
                  "  torch float64 route, three dgemms on a converted copy:     %9.3f ms  (min %.3f, max %.3f)" % t_ms + f"   peak memory {peak / 2 ** 20:.1f} MiB above the table; "
                  f"kernel / torch = {k_ms[0] / t_ms[0]:.3f}; largest relative difference of the two {worst:.1e}",
                  "  run_tica, the whole fit (wall clock, host eigenproblems in): %7.1f ms  (min %.1f, max %.1f)" % fit_ms,
                  f"  projection with limits, {N} x {F} -> {model.dim} (HIP events):" + "         %9.3f ms  (min %.3f, max %.3f)" % p_ms]
        if k_ms[0] > t_ms[0]:
            slower.append(F)
lines.append("THE KERNEL IS SLOWER THAN THE DGEMM ROUTE AT F = " + ", ".join(str(f) for f in slower) + ": it stays for its fixed summation order, its error bound "
             "and its memory (no [n, F] float64 copies)." if slower else "The kernel is not slower than the dgemm route at either shape.")
print("\n".join(lines))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
