#!/usr/bin/env python3
"""Cost of the evaluation tail behind the decode: the two kernels behind ``displacement_errors`` (HIP events around back-to-back library
calls on preallocated buffers; as a pair and each alone) and the existing torch path on the same device and inputs - the tail of
``best_of_k_errors`` behind its decode (slice, permute + reshape copy, boolean index, ``min_ade_fde``), which waits for the host once per
batch.  NBA shape (K = 60, num_runs = 20, 64 scenes of 11 agents, 10 future frames of 20) and pedestrian shape (K = 20, 12 future frames
of 20, 3 coordinates).  One warm-up, then the median of several runs.  A record, not a gate.
Usage (GPU box):  python tools/disp_errors_cost.py [--runs 7] [--calls 20]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lam_slide_amd import _lib, displacement_errors, min_ade_fde  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()

SHAPES = {
    # K, num_runs, B, T, c1, A, D
    "nba": (60, 20, 64, 20, 10, 11, 2),
    "pedestrian": (20, 20, 64, 20, 8, 8, 3),
}
dev = torch.device("cuda:0")
lib = _lib.load()


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
    for name, (K, R, B, T, c1, A, D) in SHAPES.items():
        g = torch.Generator().manual_seed(5)
        pos = torch.randn(K * B, T, A, D, generator=g).to(dev)      # what the decoder leaves
        target = torch.randn(B, T - c1, A, D, generator=g).to(dev)  # the true future positions
        mask = (torch.rand(B, A, generator=g) > 0.1).to(dev)
        m8 = mask.view(torch.uint8)
        rows, traj = torch.empty(K, B, A, 2, device=dev), torch.empty(K, B, 2, device=dev)
        agents, totals = torch.empty(B, A, 2, device=dev), torch.empty(5, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def rows_only():
            _lib.check(lib.lsl_disp_error_rows(pos.data_ptr(), target.data_ptr(), K, B, T, c1, T - c1, 0, T - c1, A, D, rows.data_ptr(), traj.data_ptr(),
                                               stream))

        def final_only():
            _lib.check(lib.lsl_disp_error_final(rows.data_ptr(), traj.data_ptr(), m8.data_ptr(), K, R, B, A, agents.data_ptr(), totals.data_ptr(), stream))

        def kernels():
            rows_only()
            final_only()

        def module():
            return displacement_errors(pos.reshape(K, B, T, A, D), target, mask, first_frame=c1, num_runs=R)

        def torch_tail():  # best_of_k_errors behind its decode, as it stands
            p = pos.reshape(K, B, T, A, D)[:, :, c1:]
            tr = p.permute(1, 3, 0, 2, 4).reshape(B * A, K, T - c1, D)
            tg = target.permute(0, 2, 1, 3).reshape(B * A, T - c1, D)
            keep = mask.reshape(-1)
            return min_ade_fde(tr[keep][:, :R], tg[keep])

        k_ms, k_lo, k_hi = median_ms(kernels, args.calls)
        r_ms, _, _ = median_ms(rows_only, args.calls)
        f_ms, _, _ = median_ms(final_only, args.calls)
        m_ms, m_lo, m_hi = median_ms(module, args.calls)
        t_ms, t_lo, t_hi = median_ms(torch_tail, args.calls)
        want, got = torch_tail(), module().real()
        agree = max(float(((a - b).abs() / b.abs()).max()) for a, b in zip(got, want))
        print(f"{name}: K = {K}, num_runs = {R}, B = {B}, A = {A}, D = {D}, Tf = {T - c1} of T = {T}")
        print(f"  lsl_disp_error_rows + lsl_disp_error_final: {k_ms * 1e3:9.1f} us per pair of launches (min {k_lo * 1e3:.1f}, max {k_hi * 1e3:.1f})")
        print(f"    each alone, back to back: k_disp_rows {r_ms * 1e3:.1f} us, k_disp_final {f_ms * 1e3:.1f} us")
        print(f"  displacement_errors (binding, allocations):  {m_ms * 1e3:9.1f} us (min {m_lo * 1e3:.1f}, max {m_hi * 1e3:.1f})")
        print(f"  torch tail of best_of_k_errors:              {t_ms * 1e3:9.1f} us (min {t_lo * 1e3:.1f}, max {t_hi * 1e3:.1f}); "
              f"kernels / torch = {k_ms / t_ms:.3f}; values agree to {agree:.1e}")
