#!/usr/bin/env python3
"""Cost of the peptide evaluation's torsion statistics at the evaluation's shape: a trajectory of n = 10 000 frames (10 rollouts x T = 1000)
of a tetrapeptide (R = 4), the torsions of ``eval_torsion_quads``, 100-bin histograms of every torsion, 50 x 50 joint histograms of the
column pairs (1, 2) and (3, 4), the Jensen-Shannon distances to a second trajectory's counts, and the decorrelation curves to nlag = 1000.

  device path   positions on the GPU -> ``TorsionStats.update`` (dihedrals + histograms) -> ``js_distance`` -> ``decorrelation``;
                HIP events around back-to-back calls, the whole chain and each piece alone
  host path     the same positions copied to the host, then numpy / scipy: the float32 dihedral formula, ``np.histogram`` /
                ``np.histogram2d`` per column, ``jensenshannon`` per table, and the lagged sums by FFT (what statsmodels' acovf does by
                default; the direct sum is 4 * 10^8 products); wall clock, the copy included
One warm-up, then the median of several runs.  A record, not a gate: the numbers are written to profiles/torsion_stats_cost.txt.
Usage (GPU box):  python tools/torsion_stats_cost.py [--runs 5] [--calls 5]"""
import argparse
import glob
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.spatial.distance import jensenshannon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import TorsionStats, decorrelation, eval_torsion_quads, js_distance  # noqa: E402
from lam_slide_amd import dihedral_angles, angle_histograms, lagged_products  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "torsion_stats_cost.txt"))
args = ap.parse_args()

N, R, NLAG, PAIRS = 10000, 4, 1000, ((1, 2), (3, 4))
dev = torch.device("cuda:0")
tables = {}
for part in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "f18_peptide_loss*.npz"))):  # the residue tables of fixture F18
    tables.update({k[len("tables/"):]: v for k, v in np.load(part).items() if k.startswith("tables/")})
aatype = [1, 13, 10, 18]  # ARG PHE LEU TYR: 6 backbone and 10 side-chain torsions
quads, labels = eval_torsion_quads(aatype, tables)
Q = len(labels)


def trajectory(seed):
    """A seeded AR(1) random walk of R * 14 atoms around a seeded geometry (the statistics' cost does not depend on the values)."""
    g = torch.Generator().manual_seed(seed)
    base = 2.0 * torch.randn(R * 14, 3, generator=g)
    e = torch.randn(N, R * 14, 3, generator=g)
    z = torch.empty_like(e)
    z[0] = e[0]
    for t in range(1, N):
        z[t] = 0.95 * z[t - 1] + 0.3122 * e[t]
    return (base + 0.3 * z).reshape(N, R, 14, 3).contiguous()


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


def median_wall_ms(fn):
    fn()
    times = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def dihedral32(pos):
    p = pos.reshape(N, R * 14, 3)[:, quads.astype(np.int64)]
    b1, b2, b3 = p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 1], p[:, :, 3] - p[:, :, 2]
    c1, c2 = np.cross(b2, b3), np.cross(b1, b2)
    return np.arctan2((b1 * c1).sum(-1) * np.linalg.norm(b2, axis=-1), (c1 * c2).sum(-1))


def acovf_fft(x, nlag):
    """sum_{t < n - k} x_t x_{t+k} / (n - k) of every column, by FFT (float64)."""
    n = x.shape[0]
    f = np.fft.rfft(x.astype(np.float64), n=2 * n, axis=0)
    ac = np.fft.irfft(f * np.conj(f), axis=0)[:nlag + 1]
    return (ac / (n - np.arange(nlag + 1))[:, None]).T


with torch.no_grad():
    pos_d, ref_d = trajectory(1).to(dev), trajectory(2).to(dev)
    ref = TorsionStats(quads, labels, pairs=PAIRS)
    ref.update(ref_d)
    ref_c, ref_c2 = ref.counts.cpu().numpy(), ref.counts2.cpu().numpy()
    stats = TorsionStats(quads, labels, pairs=PAIRS)
    ang_d = stats.update(pos_d)
    sc_d = torch.cat([ang_d.sin(), ang_d.cos()], dim=1)

    def device_chain():
        stats.reset()  # (the index and edge tables stay on the device, as in a loop over rollouts)
        ang = stats.update(pos_d)
        d1 = js_distance(ref.counts, stats.counts)
        d2 = js_distance(ref.counts2.reshape(len(PAIRS), -1), stats.counts2.reshape(len(PAIRS), -1))
        return d1, d2, decorrelation(ang, NLAG)

    def host_chain():
        pos = pos_d.cpu().numpy()  # the copy the device path does not need
        ang = dihedral32(pos)
        a64 = ang.astype(np.float64)
        c = [np.histogram(a64[:, q], range=(-np.pi, np.pi), bins=100)[0] for q in range(Q)]
        c2 = [np.histogram2d(a64[:, a], a64[:, b], range=((-np.pi, np.pi), (-np.pi, np.pi)), bins=50)[0] for a, b in PAIRS]
        d1 = [jensenshannon(ref_c[q], c[q]) for q in range(Q)]
        d2 = [jensenshannon(ref_c2[p].reshape(-1), c2[p].reshape(-1)) for p in range(len(PAIRS))]
        s, co = np.sin(a64), np.cos(a64)
        base = s.mean(0) ** 2 + co.mean(0) ** 2
        return d1, d2, (acovf_fft(s, NLAG) + acovf_fft(co, NLAG) - base[:, None]) / (1 - base[:, None])

    lines = [f"Torsion statistics at the evaluation's shape: n = {N} frames, R = {R} ({Q} torsions), 100 bins, {len(PAIRS)} pairs of 50 x 50 bins, nlag = {NLAG}",
             f"measured on {torch.cuda.get_device_name(0)} (torch {torch.__version__}), host side on this box's CPU with numpy {np.__version__}; "
             f"median of {args.runs} runs (min, max)"]
    d_ms = median_ms(device_chain, args.calls)
    h_ms = median_wall_ms(host_chain)
    lines.append("  device path (update + 2 x js_distance + decorrelation):  %9.1f us  (min %.1f, max %.1f)" % tuple(1e3 * v for v in d_ms))
    for name, fn in (("dihedral_angles", lambda: dihedral_angles(pos_d.reshape(N, -1, 3), quads)),
                     ("angle_histograms (1-D + pairs)", lambda: angle_histograms(ang_d, pairs=PAIRS)),
                     ("js_distance (all tables)", lambda: (js_distance(ref.counts, stats.counts), js_distance(ref.counts2.reshape(2, -1), stats.counts2.reshape(2, -1)))),
                     (f"lagged_products ({2 * Q} channels)", lambda: lagged_products(sc_d, NLAG)),
                     ("decorrelation", lambda: decorrelation(ang_d, NLAG))):
        lines.append("    %-34s %9.1f us  (min %.1f, max %.1f)   [binding included: allocations, table copies]" % ((name,) + tuple(1e3 * v for v in median_ms(fn, args.calls))))
    lines.append("  host path (copy to host + numpy + scipy, FFT lagged sums): %9.1f us  (min %.1f, max %.1f)" % tuple(1e3 * v for v in h_ms))
    lines.append("  device / host = %.4f" % (d_ms[0] / h_ms[0]))
    dd, hh = device_chain(), host_chain()
    e_js = max(float(np.abs(dd[0].cpu().numpy() - np.asarray(hh[0])).max()), float(np.abs(dd[1].cpu().numpy() - np.asarray(hh[1])).max()))
    e_dc = float(np.abs(dd[2].cpu().double().numpy() - hh[2]).max())
    lines.append(f"  agreement of the two paths: JS distances to {e_js:.1e} (float32 angles of two operation orders may fall in neighbouring bins), "
                 f"decorrelation curves to {e_dc:.1e}")
    if d_ms[0] >= h_ms[0]:
        lines.append("  THE DEVICE PATH DID NOT WIN AT THIS SHAPE.")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
