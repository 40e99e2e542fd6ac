#!/usr/bin/env python3
"""The TICA and Markov-state half of the peptide evaluation on one MI355X, on seeded synthetic features: fit a TICA model on the "MD"
features (lagged second moments on the device, the F x F eigenproblem on the host) -> project both trajectories and take the joint ranges
-> TICA-0 / TICA-0,1 Jensen-Shannon distances -> 100 k-means microstates of the projected reference -> nearest-centre labels through a microstate -> state map -> state occupancies and their
distance -> the transition count matrix of the sampled trajectory.  Nothing is read back before the distances.

Mirrors eval_peptide.py:189-288 without pyemma: the features would be ``cossin_features(TorsionStats.update(frames))`` of the sampled
positions (examples/peptide_torsion_stats_on_device.py) and the MD side's stored features; a model pyemma fitted enters through
``TicaModel.from_arrays(tica.mean, tica.eigenvectors, tica.eigenvalues, dim=tica.dimension())``, its k-means centres and
``msm.metastable_assignments`` through ``assign_centers(y, centers, state_map=...)``.

    python examples/peptide_tica_on_device.py [--n-ref 100000] [--n-traj 10000] [--lag 100]
"""
import argparse
import os
import sys

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import TicaModel, assign_centers, fit_microstates, metastable_jsd, summary_metrics, tica, tica_autocovariance, tica_jsd, transition_counts  # noqa: E402


def features(n, F, seed, mix_seed=1):
    """Seeded float32 [n, F]: slow and fast AR(1) processes mixed into F columns plus white noise - stands for cos / sin torsions."""
    rng = np.random.default_rng(seed)
    rho = np.array([0.999, 0.995, 0.98, 0.93, 0.8, 0.5])
    e = rng.standard_normal((n, rho.size))
    e[1:] *= np.sqrt(1.0 - rho * rho)
    z = np.stack([scipy.signal.lfilter([1.0], [1.0, -r], e[:, i]) for i, r in enumerate(rho)], axis=1)
    x = z @ (np.random.default_rng(mix_seed).standard_normal((rho.size, F)) / np.sqrt(rho.size)) + 0.3 * rng.standard_normal((n, F))
    return torch.from_numpy((x / np.abs(x).max()).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ref", type=int, default=100000)
    ap.add_argument("--n-traj", type=int, default=10000)
    ap.add_argument("--F", type=int, default=32)
    ap.add_argument("--lag", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (the package has no CPU path)"
    dev = torch.device("cuda:0")
    ref, traj = features(args.n_ref, args.F, seed=2).to(dev), features(args.n_traj, args.F, seed=3).to(dev)

    model = TicaModel.fit(ref, lag=args.lag)                       # pyemma.coordinates.tica(ref, lag=, kinetic_map=True)
    jsd = tica_jsd(model, ref, traj)                               # {"TICA-0", "TICA-0,1"}: merge into TorsionStats.jsd(...)'s dict
    y_ref, y_traj = model.transform(ref), model.transform(traj)
    centers = fit_microstates(y_ref, k=100, max_iter=100, seed=137)  # analysis.get_kmeans: k-means++ and Lloyd iterations on the device
    state_map = np.arange(100) % 10                                # stands for msm.metastable_assignments
    _, ref_counts = assign_centers(y_ref, centers, state_map=state_map, nstates=10)
    labels, traj_counts = assign_centers(y_traj, centers, state_map=state_map, nstates=10)
    msms = float(metastable_jsd(ref_counts, traj_counts))          # calc_summary_metrics' "MSMS"
    counts = transition_counts(labels, min(args.lag, args.n_traj // 2), 10)  # what estimate_markov_model(traj_discrete, lag) counts
    ac = tica_autocovariance(y_traj, min(1000, args.n_traj - 1))
    print(f"TICA of {args.n_ref} x {args.F} features at lag {args.lag}: dim {model.dim}, eigenvalues {np.round(model.eigenvalues[:model.dim], 4).tolist()}")
    print(f"JSD {jsd}  summary {summary_metrics([{'PHI 1': 0.0, **jsd}])}")
    print(f"MSMS {msms:.4f}  occupancies {traj_counts.tolist()}  transitions counted {int(counts.sum())}  autocovariance at lag 10: {float(ac[10]):.4f}")
    print(f"paths: {tica.last_path}")


if __name__ == "__main__":
    main()
