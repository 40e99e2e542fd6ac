#!/usr/bin/env python3
"""Cost of the peptide losses of ``model_step`` at the peptide shape (B = 8, T = 1000, R = 4: 8000 frames of 56 atoms and 28 torsions): the
three launches behind ``peptide_losses`` - ``lsl_geom_loss_sums``, ``lsl_peptide_loss_sums``, ``lsl_peptide_loss_final`` - each alone and all
three (HIP events around back-to-back library calls on preallocated buffers), and the generic torch path of ``PeptideLoss`` (frames,
atom37 gather, torsions, two cdist matrices, five masked reductions) on the same device and inputs.  One warm-up, then the median of
several runs.  A record, not a gate.  The residue tables come from the fixture tests/golden/f18_peptide_loss.npz.
Usage (GPU box):  python tools/peptide_loss_cost.py [--runs 7] [--calls 500]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import _lib  # noqa: E402
from lam_slide_amd import peptide_loss as pl  # noqa: E402
from lam_slide_amd.losses import inter_distance, masked_mse, masked_norm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--calls", type=int, default=500)  # (a timed window of tens of milliseconds, not of one)
ap.add_argument("--B", type=int, default=8)
ap.add_argument("--T", type=int, default=1000)
ap.add_argument("--R", type=int, default=4)
args = ap.parse_args()

dev = torch.device("cuda:0")
lib = _lib.load()
z = {}
for part in ("f18_peptide_loss.npz", "f18_peptide_loss.part2.npz"):
    with np.load(os.path.join(ROOT, "tests", "golden", part)) as f:
        z.update({k[len("tables/"):]: f[k] for k in f.files if k.startswith("tables/")})
tables = pl.residue_tables(z)


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


with torch.no_grad():
    g = torch.Generator().manual_seed(5)
    F_, R = args.B * args.T, args.R
    A = R * 14
    aa = torch.randint(0, 20, (F_, R), generator=g)
    target = torch.randn(F_, R, 14, 3, generator=g)
    pred = (target + 0.3 * torch.randn(F_, R, 14, 3, generator=g)).to(dev)
    target = target.to(dev)
    target_frame = pl.backbone_local(target)
    aa_d = aa.to(dev)
    tors_target = pl.torsion_angles(target, aa_d, tables)
    tm = pl.torsion_mask(aa, tables).to(dev)
    am = torch.ones(F_, R, 14, dtype=torch.bool, device=dev)  # (every slot counted: the most work)
    am8, tm8 = am.to(torch.uint8).contiguous(), (tm != 0).to(torch.uint8).contiguous()
    restab = tables.on(dev)["restab"]
    geom, pept, out = torch.empty(F_, 5, device=dev), torch.empty(F_, 4, device=dev), torch.empty(5, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def k_geom():
        _lib.check(lib.lsl_geom_loss_sums(pred.data_ptr(), target.data_ptr(), am8.data_ptr(), F_, A, 3, geom.data_ptr(), stream))

    def k_pept():
        _lib.check(lib.lsl_peptide_loss_sums(pred.data_ptr(), target_frame.data_ptr(), am8.data_ptr(), tors_target.data_ptr(), tm8.data_ptr(),
                                             aa_d.data_ptr(), restab.data_ptr(), F_, R, 1, pept.data_ptr(), stream))

    def k_final():
        _lib.check(lib.lsl_peptide_loss_final(geom.data_ptr(), pept.data_ptr(), F_, out.data_ptr(), stream))

    def three():
        k_geom(), k_pept(), k_final()

    def generic():
        flat3 = lambda x: x.reshape(-1, 3)  # noqa: E731
        m = am.reshape(-1)
        return (masked_mse(flat3(pred), flat3(target), m), masked_mse(flat3(pl.backbone_local(pred)), flat3(target_frame), m),
                inter_distance(pred.reshape(F_, A, 3), target.reshape(F_, A, 3), am.reshape(F_, A)), masked_norm(flat3(pred), flat3(target), m),
                pl.masked_cosine_v2(pl.torsion_angles(pred, aa_d, tables).reshape(-1, 2), tors_target.reshape(-1, 2), tm.reshape(-1)))

    res = {name: median_ms(fn, args.calls) for name, fn in (("three", three), ("geom", k_geom), ("pept", k_pept), ("final", k_final))}
    t_ms, t_lo, t_hi = median_ms(generic, max(1, args.calls // 10))
    three()
    want = generic()
    worst = max(abs(float(out[i]) - float(want[i])) / abs(float(want[i])) for i in range(5))
    print(f"peptide losses: F = {args.B} x {args.T} = {F_} frames, R = {R} ({A} atoms, {R * 7} torsions per frame); median of {args.runs} runs of {args.calls} calls")
    print(f"  the three launches of peptide_losses:   {res['three'][0] * 1e3:9.1f} us (min {res['three'][1] * 1e3:.1f}, max {res['three'][2] * 1e3:.1f})")
    print(f"    each alone, back to back: lsl_geom_loss_sums {res['geom'][0] * 1e3:.1f} us, lsl_peptide_loss_sums {res['pept'][0] * 1e3:.1f} us, "
          f"lsl_peptide_loss_final {res['final'][0] * 1e3:.1f} us")
    print(f"  generic torch path (same device, inputs): {t_ms * 1e3:9.1f} us (min {t_lo * 1e3:.1f}, max {t_hi * 1e3:.1f}); "
          f"kernels / torch = {res['three'][0] / t_ms:.4f}; the five values agree to {worst:.1e}")
