#!/usr/bin/env python3
"""`tica_utils.run_tica` and the two TIC keys of the peptide validation on one MI355X, from seeded atom14 positions: a tetrapeptide whose
backbone switches slowly between two conformations -> `tica_features` (pair distances of the C / N / S atoms, sin / cos of phi, psi,
omega: a few hundred columns) -> `run_tica` (Koopman weights, weighted reversible covariances on the device; two small eigenproblems on
the host) -> the projection of the reference and of a "sampled" trajectory -> `traj_analysis(..., tica_lagtime=)`, which does all of that
itself and returns the seven numbers `SIAtom14SampleCallback.log_metrics` logs.

With real data pass the MD frames as `pos_ref`, the sampled frames as `pos_model` and the peptide's own `aatype`.

    python examples/peptide_koopman_tica_on_device.py [--n 4000] [--lag 100]
"""
import argparse
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import StructureTables, koopman_tica, run_tica, structure_stats, tica_features, traj_analysis  # noqa: E402


def positions(n, R, seed, dwell):
    """float32 [n, R, 14, 3], nanometres: a bent C-alpha trace whose bend angle switches between two values with probability 1 / dwell per
    frame, thermal noise on every atom, the other slots at fixed offsets of size 0.15 from their C-alpha (the same peptide for every seed)."""
    rng = np.random.default_rng(seed)
    state = np.where(np.cumsum(rng.random(n) < 1.0 / dwell) % 2 == 0, 1.0, -1.0)
    angle = 0.9 + 0.5 * state  # radians between consecutive bonds
    ca = np.zeros((n, R, 3))
    for k in range(1, R):
        ca[:, k] = ca[:, k - 1] + 0.38 * np.stack([np.cos(k * angle), np.sin(k * angle), 0.05 * k * np.ones(n)], axis=1)
    pos = ca[:, :, None, :] + 0.15 * np.random.default_rng(100).standard_normal((1, R, 14, 3)) + 0.008 * rng.standard_normal((n, R, 14, 3))
    return pos.astype(np.float32), state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--lag", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    # the residue tables are the host application's (residue_constants); here: the copy the test fixtures hold
    tables = {}
    for part in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "f18_peptide_loss*.npz"))):
        tables.update({k[len("tables/"):]: v for k, v in np.load(part).items() if k.startswith("tables/")})
    aatype = [17, 13, 10, 18]  # TRP PHE LEU TYR
    st = StructureTables(aatype, tables)
    st.on(dev)
    ref, state = positions(args.n, 4, seed=0, dwell=400)
    pos_ref = torch.from_numpy(ref).to(dev)
    pos_model = torch.from_numpy(positions(args.n // 4, 4, seed=7, dwell=150)[0]).to(dev)  # a "sampled" trajectory that switches too fast

    feats = tica_features(pos_ref, st)
    t = time.perf_counter()
    model = run_tica(feats, lagtime=args.lag, dim=40)
    y = model.transform(feats)
    torch.cuda.synchronize()
    print(f"tica_features {tuple(feats.shape)}; run_tica ({koopman_tica.last_path['run_tica']}) + projection ({koopman_tica.last_path['transform']}) "
          f"{1e3 * (time.perf_counter() - t):.1f} ms; dim {model.dim}, leading eigenvalues {np.round(model.eigenvalues[:3], 4)}")
    r = abs(np.corrcoef(y[:, 0].cpu().numpy().astype(np.float64), state)[0, 1])
    print(f"|corr(TIC-0, the planted two-state coordinate)| = {r:.4f}")

    out = traj_analysis(pos_model, pos_ref, st, tica_lagtime=args.lag)
    print(f"traj_analysis ({structure_stats.last_path['traj_analysis']}):", ", ".join(f"{k} {float(v):.4f}" for k, v in out.items()))


if __name__ == "__main__":
    main()
