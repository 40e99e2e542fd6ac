#!/usr/bin/env python3
"""The Markov-state block of the peptide evaluation (eval_peptide.py:245-288) on one MI355X, on seeded synthetic chains: k-means
microstates of the projected "MD" reference -> the reversible maximum-likelihood microstate model -> PCCA+ assignments by the inner simplex
algorithm (host) -> both coarse label series -> the coarse model and the sampled trajectory's model, embedded in the 10 x 10 index space ->
the dict analyze_trajectory stores.  With ``metastable_assignments=`` (e.g. the array a real pyemma produced) nothing is read back before
the dict; without it the one read is the microstate model going into the host PCCA.

Mirrors analysis.get_msm / analysis.discretize without pyemma.  The estimator is stated as mathematics; parity with a
live pyemma was not checked, and pyemma's refinement of the PCCA+ rotation is not reproduced.

    python examples/peptide_msm_on_device.py [--n-ref 200000] [--n-traj 10000] [--lag 100] [--msm-lag 10] [--device cuda:0]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import estimate_markov_model, fit_microstates, markov_state_block, metastable_jsd, msm  # noqa: E402

NSTATES = 10


def wells_series(n, seed, stay=0.995):
    """Seeded float32 [n, 2]: a sticky chain over NSTATES wells on a circle plus Gaussian noise - stands for the two leading TICA columns."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(NSTATES) / NSTATES
    wells = 4.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    jump = rng.random(n) > stay
    step = np.where(jump, rng.choice([-1, 1], n), 0)
    state = np.cumsum(step) % NSTATES
    return torch.from_numpy((wells[state] + 0.35 * rng.standard_normal((n, 2))).astype(np.float32))


def main(device="cuda:0", n_ref=200000, n_traj=10000, lag=100, msm_lag=10, k=100):
    dev = torch.device(device)
    if dev.type == "cuda":
        assert torch.cuda.is_available(), "needs the MI355X"
    y_ref, y_traj = wells_series(n_ref, seed=2).to(dev), wells_series(n_traj, seed=3).to(dev)
    centers = fit_microstates(y_ref, k=k, max_iter=100, seed=137)   # analysis.get_kmeans
    out = markov_state_block(y_ref, y_traj, centers, nstates=NSTATES, lag=lag, msm_lag=msm_lag)  # analysis.get_msm, discretize and the block
    again = markov_state_block(y_ref, y_traj, centers, metastable_assignments=out["metastable_assignments"], nstates=NSTATES, lag=lag, msm_lag=msm_lag)
    assert all(torch.equal(out[key], again[key]) for key in out)     # given assignments: the same block with no read-back
    n_ref_rows, n_traj_rows = y_ref.shape[0], y_traj.shape[0]
    msms = float(metastable_jsd((out["ref_metastable_probs"] * n_ref_rows).round().long(), (out["traj_metastable_probs"] * n_traj_rows).round().long()))
    micro = estimate_markov_model(counts=torch.ones(3, 3, dtype=torch.int64, device=dev), lag=lag)  # a model from a count matrix alone
    print(f"keys: {sorted(out)}")
    print(f"msm_pi {np.round(out['msm_pi'].cpu().numpy(), 4).tolist()}")
    print(f"traj_pi {np.round(out['traj_pi'].cpu().numpy(), 4).tolist()}")
    print(f"diagonal of msm_transition_matrix {np.round(out['msm_transition_matrix'].diagonal().cpu().numpy(), 4).tolist()}")
    print(f"MSMS {msms:.4f}  a 3-state uniform model converged after {int(micro.n_iter)} step  paths: {msm.last_path}")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ref", type=int, default=200000)
    ap.add_argument("--n-traj", type=int, default=10000)
    ap.add_argument("--lag", type=int, default=100)
    ap.add_argument("--msm-lag", type=int, default=10)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    main(a.device, a.n_ref, a.n_traj, a.lag, a.msm_lag)
