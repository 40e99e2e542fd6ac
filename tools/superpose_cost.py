#!/usr/bin/env python3
"""Cost of rigid superposition at the evaluation's shape: a trajectory of F = 10 000 frames (10 rollouts x T = 1000) with A = 56 atoms (a
tetrapeptide's atom14 frame) and A = 364 (26 residues); ``superpose`` onto frame 0 in place, ``rmsd`` to frame 0, ``rmsf``.

  device form   ``lsl_superpose`` / ``lsl_atom_rmsf`` behind ``lam_slide_amd.superpose`` (float32 positions on the GPU)
  restatement   the same functions on the same GPU with float64 positions, which take the torch path (``torch.linalg.eigh`` of Horn's
                matrix, einsums): what a user without the kernels would run on the device
HIP events around back-to-back calls; one warm-up, then the median of several runs.  Beside each time the bytes the function has to move
(superpose: every frame read once and written once; rmsd: read once; rmsf: read twice) over the time, and the rate of a plain device copy
of the same trajectory for comparison.  A record, not a gate: the numbers are written to profiles/superpose_cost.txt.
Usage (GPU box):  python tools/superpose_cost.py [--runs 5] [--calls 5]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import superpose as sp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "superpose_cost.txt"))
args = ap.parse_args()

F = 10000
dev = torch.device("cuda:0")


def trajectory(A, seed):
    """Seeded frames: one structure turned about z, shifted and perturbed (the cost does not depend on the values)."""
    g = torch.Generator().manual_seed(seed)
    base = 3.0 * torch.randn(A, 3, generator=g)
    ang = 6.28 * torch.rand(F, generator=g)
    c, s, o, z = torch.cos(ang), torch.sin(ang), torch.ones(F), torch.zeros(F)
    rot = torch.stack([torch.stack([c, -s, z], -1), torch.stack([s, c, z], -1), torch.stack([z, z, o], -1)], -2)
    return (torch.einsum("fab,ib->fia", rot, base) + 0.3 * torch.randn(F, A, 3, generator=g) + 10.0 * torch.randn(F, 1, 3, generator=g)).contiguous()


def median_ms(fn, calls):
    fn()  # warm-up
    times = []
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return statistics.median(times), min(times), max(times)


lines = [f"Rigid superposition at the evaluation's shape: F = {F} frames; superpose onto frame 0, rmsd to frame 0, rmsf",
         f"measured on {torch.cuda.get_device_name(0)} (torch {torch.__version__}); median of {args.runs} runs of {args.calls} back-to-back calls (min, max); "
         "binding included (allocations, the clone of the reference frame)"]
with torch.no_grad():
    for A in (56, 364):
        x32 = trajectory(A, A).to(dev)
        x64 = x32.double()
        frame_bytes = F * A * 3 * 4
        buf = torch.empty_like(x32)
        copy = median_ms(lambda: buf.copy_(x32), args.calls)
        lines.append(f"A = {A}: a trajectory is {frame_bytes / 1e6:.2f} MB; a device copy of it (read + write) takes {1e3 * copy[0]:.1f} us = {2 * frame_bytes / copy[0] / 1e6:.0f} GB/s")
        work32, work64 = x32.clone(), x64.clone()
        ref32, ref64 = x32[0].clone(), x64[0].clone()
        total = {"fused": 0.0, "torch": 0.0}
        for name, moved, f32, f64 in (
                ("superpose (in place)", 2, lambda: sp.superpose(work32, ref32, out=work32), lambda: sp.superpose(work64, ref64, out=work64)),
                ("rmsd", 1, lambda: sp.rmsd(x32, ref32), lambda: sp.rmsd(x64, ref64)),
                ("rmsf", 2, lambda: sp.rmsf(x32), lambda: sp.rmsf(x64))):
            key = name.split()[0]
            d = median_ms(f32, args.calls)
            assert sp.last_path[key] == "fused"
            t = median_ms(f64, args.calls)
            assert sp.last_path[key] == "torch"
            total["fused"] += d[0]
            total["torch"] += t[0]
            lines.append("    %-22s device form %8.1f us (min %.1f, max %.1f) = %6.0f GB/s = %.2f of the copy rate;   torch float64 %9.1f us;   ratio %.3f"
                         % (name, 1e3 * d[0], 1e3 * d[1], 1e3 * d[2], moved * frame_bytes / d[0] / 1e6, (moved * frame_bytes / d[0]) / (2 * frame_bytes / copy[0]),
                            1e3 * t[0], d[0] / t[0]))
        lines.append("    %-22s device form %8.1f us;   torch float64 %9.1f us;   ratio %.3f" % ("all three", 1e3 * total["fused"], 1e3 * total["torch"], total["fused"] / total["torch"]))
        if total["fused"] >= total["torch"]:
            lines.append("    THE DEVICE FORM DID NOT WIN AT THIS SHAPE.")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
