#!/usr/bin/env python3
"""Cost of the peptide evaluation's TICA and state statistics at the evaluation's shape: an MD reference of n_ref = 10^6 frames and a sampled
trajectory of n_traj = 10^4 frames of F = 32 cos / sin torsion features, TICA at lag 1000 (kinetic map, 95 % of the kinetic variance:
d = dim columns), 100-bin and 50 x 50 histograms on the joint range, k = 100 centres mapped to 10 states, transition counts at lag 1000.

The reference length 10^6 is a reading of ``nlag=100000`` (eval_peptide.py:233) and of the "lag time 100 ps" comment beside ``lag=1000``
(modules/analysis.py:36-38) - a trajectory at least ten times its longest lag - not a measured fact about the MD data set.

  device path   features on the GPU -> ``TicaModel.fit`` (moments and covariances on the device, two F x F matrices to the host, the
                eigenproblem there) -> ``tica_jsd`` (two projections with the joint range, edges, four histograms, two distances) ->
                ``assign_centers`` of both sides -> ``transition_counts`` -> ``metastable_jsd``; wall clock around the whole chain ending
                in a synchronise (it holds host work), HIP events around each device piece alone
  host path     the same features copied to the host, then numpy / scipy: float64 Gram matrices through BLAS, the same eigenproblem,
                the projection, ``np.histogram`` / ``np.histogram2d``, ``jensenshannon``, ``cdist(...).argmin``, ``np.add.at``; wall
                clock, the copy included
One warm-up, then the median of several runs.  A record, not a gate: the numbers are written to profiles/tica_cost.txt.
Usage (GPU box):  python tools/tica_cost.py [--runs 3] [--calls 3]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import scipy.signal
import torch
from scipy.spatial.distance import cdist, jensenshannon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import (TicaModel, _lib, assign_centers, lagged_moments, metastable_jsd, solve_tica, tica, tica_dimension, tica_jsd,  # noqa: E402
                           transition_counts)

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--n-ref", type=int, default=1000000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tica_cost.txt"))
args = ap.parse_args()

N_REF, N_TRAJ, F, LAG, K, NSTATES = args.n_ref, 10000, 32, 1000, 100, 10
dev = torch.device("cuda:0")


def features(n, seed):
    """Seeded float32 [n, F]: six AR(1) processes (slow to fast) mixed into F columns plus white noise, scaled to |x| <= 1 (the
    statistics' cost does not depend on the values)."""
    rng = np.random.default_rng(seed)
    rho = np.array([0.9999, 0.9997, 0.9995, 0.999, 0.99, 0.5])  # four processes that outlive the lag
    e = rng.standard_normal((n, rho.size))
    e[1:] *= np.sqrt(1.0 - rho * rho)
    z = np.stack([scipy.signal.lfilter([1.0], [1.0, -r], e[:, i]) for i, r in enumerate(rho)], axis=1)
    x = z @ (np.random.default_rng(1).standard_normal((rho.size, F)) / np.sqrt(rho.size)) + 0.3 * rng.standard_normal((n, F))
    return torch.from_numpy((x / np.abs(x).max()).astype(np.float32))


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
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def fit(x):
    """``TicaModel.fit`` at the evaluation's settings; a dimension beyond the device form's 16 columns (noise components of a short
    series) is cut there, so that the record times the device form."""
    m = TicaModel.fit(x, lag=LAG)
    if m.dim > _lib.PROJ_MAX_D:
        m = TicaModel.from_arrays(m.mean, m.eigenvectors, m.eigenvalues, dim=_lib.PROJ_MAX_D)
    return m


with torch.no_grad():
    ref_d, traj_d = features(N_REF, 2).to(dev), features(N_TRAJ, 3).to(dev)
    model = fit(ref_d)
    d = model.dim
    y_ref = model.transform(ref_d)
    centers = y_ref[:: N_REF // K][:K].contiguous()  # K frames of the reference as centres (k-means fitting is the caller's)
    smap = np.arange(K, dtype=np.int32) % NSTATES
    smap_d = torch.from_numpy(smap).to(dev)
    centers_h = centers.cpu().numpy().astype(np.float64)

    def device_chain():
        m = fit(ref_d)
        jsd = tica_jsd(m, ref_d, traj_d)
        yr, yt = m.transform(ref_d), m.transform(traj_d)
        _, cr = assign_centers(yr, centers, state_map=smap_d, nstates=NSTATES)
        lt, ct = assign_centers(yt, centers, state_map=smap_d, nstates=NSTATES)
        return jsd, float(metastable_jsd(cr, ct)), transition_counts(lt, LAG, NSTATES)

    def host_chain():
        ref, traj = ref_d.cpu().numpy().astype(np.float64), traj_d.cpu().numpy().astype(np.float64)  # the copy the device path does not need
        m_ = N_REF - LAG
        a, b = ref[:m_], ref[LAG:]
        mean = (a.sum(0) + b.sum(0)) / (2.0 * m_)
        mm = np.outer(mean, mean)
        xy = a.T @ b
        lam, R = solve_tica((a.T @ a + b.T @ b) / (2.0 * m_) - mm, (xy + xy.T) / (2.0 * m_) - mm)
        dim = min(tica_dimension(lam), _lib.PROJ_MAX_D)
        W = R[:, :dim] * lam[:dim]
        yr, yt = ((ref - mean) @ W).astype(np.float32).astype(np.float64), ((traj - mean) @ W).astype(np.float32).astype(np.float64)
        lo, hi = np.minimum(yr.min(0), yt.min(0)), np.maximum(yr.max(0), yt.max(0))
        jsd = {"TICA-0": jensenshannon(np.histogram(yr[:, 0], range=(lo[0], hi[0]), bins=100)[0], np.histogram(yt[:, 0], range=(lo[0], hi[0]), bins=100)[0])}
        if W.shape[1] > 1:
            rng2 = ((lo[0], hi[0]), (lo[1], hi[1]))
            jsd["TICA-0,1"] = jensenshannon(np.histogram2d(yr[:, 0], yr[:, 1], range=rng2, bins=50)[0].reshape(-1),
                                            np.histogram2d(yt[:, 0], yt[:, 1], range=rng2, bins=50)[0].reshape(-1))
        lr = np.concatenate([smap[cdist(yr[i:i + 65536], centers_h, "sqeuclidean").argmin(1)] for i in range(0, N_REF, 65536)])
        lt = smap[cdist(yt, centers_h, "sqeuclidean").argmin(1)]
        cr, ct = np.bincount(lr, minlength=NSTATES), np.bincount(lt, minlength=NSTATES)
        C = np.zeros((NSTATES, NSTATES), dtype=np.int64)
        np.add.at(C, (lt[:N_TRAJ - LAG], lt[LAG:]), 1)
        return jsd, float(jensenshannon(cr, ct)), C

    lines = [f"TICA and state statistics at the evaluation's shape: n_ref = {N_REF}, n_traj = {N_TRAJ}, F = {F}, lag = {LAG}, d = dim = {d}, "
             f"100 / 50 x 50 bins, k = {K} centres, {NSTATES} states",
             "(n_ref is a reading of nlag=100000 and the \"lag 1000 = 100 ps\" comment of the reference, not a measured fact about its MD data)",
             f"measured on {torch.cuda.get_device_name(0)} (torch {torch.__version__}), host side on this box's CPU with numpy {np.__version__}; "
             f"median of {args.runs} runs (min, max)"]
    d_ms = median_wall_ms(device_chain)
    assert all(tica.last_path[k] == "fused" for k in ("fit", "tica_jsd", "transform", "assign_centers", "transition_counts", "metastable_jsd")), tica.last_path
    h_ms = median_wall_ms(host_chain)
    lines.append("  device path (fit + tica_jsd + 2 x assign_centers + transition_counts + metastable_jsd; wall clock, host eigenproblem and reads included): "
                 "%9.2f ms  (min %.2f, max %.2f)" % d_ms)
    lim = torch.empty(2, d, dtype=torch.float32, device=dev)

    def fresh_lim():
        lim[0], lim[1] = float("inf"), float("-inf")
        return lim

    for name, fn in ((f"lagged_moments (n = {N_REF})", lambda: lagged_moments(ref_d, LAG)),
                     (f"transform with limits (n = {N_REF})", lambda: model.transform(ref_d, fresh_lim())),
                     ("tica_jsd (both sides, the final read included)", lambda: tica_jsd(model, ref_d, traj_d)),
                     (f"assign_centers (n = {N_REF}, k = {K}, d = {d})", lambda: assign_centers(y_ref, centers, state_map=smap_d, nstates=NSTATES)),
                     (f"transition_counts (n = {N_REF}, lag = {LAG})", lambda: transition_counts(assign_centers(y_ref, centers, state_map=smap_d, nstates=NSTATES)[0], LAG, NSTATES))):
        lines.append("    %-52s %9.1f us  (min %.1f, max %.1f)   [HIP events; binding included]" % ((name,) + tuple(1e3 * v for v in median_ms(fn, args.calls))))
    lines.append("  host path (copy to host + numpy / scipy, wall clock):   %9.2f ms  (min %.2f, max %.2f)" % h_ms)
    lines.append("  device / host = %.4f" % (d_ms[0] / h_ms[0]))
    dd, hh = device_chain(), host_chain()
    lines.append("  agreement of the two paths: " + ", ".join(f"{k} {dd[0][k]:.6f} / {hh[0][k]:.6f}" for k in dd[0]) + f", MSMS {dd[1]:.6f} / {hh[1]:.6f}, "
                 f"transition counts differ in {int((dd[2].cpu().numpy() != hh[2]).sum())} cells (another formula of the distance may move a frame that lies near a tie)")
    if d_ms[0] >= h_ms[0]:
        lines.append("  THE DEVICE PATH DID NOT WIN AT THIS SHAPE.")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
