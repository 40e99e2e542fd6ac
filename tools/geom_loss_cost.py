#!/usr/bin/env python3
"""Cost of the geometry losses of ``model_step``: the two kernels behind ``geom_losses`` (HIP events around
back-to-back library calls on preallocated buffers; as a pair and each alone), a torch restatement of the three default loss modules on
the same tensors, and one ``Transport.training_losses`` (one ``lsl_si_loss``) of the same batch for scale.  One warm-up, then the median
of several runs.  A record, not a gate.
Usage (GPU box):  python tools/geom_loss_cost.py [--runs 7] [--calls 20]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lam_slide_amd import CreateTransport, LatentSIV3, _lib  # noqa: E402
from lam_slide_amd.losses import inter_distance, masked_mse, masked_norm  # noqa: E402
from lam_slide_amd.synthetic import seeded_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()

SHAPES = {
    # backbone (bench.py WORKLOADS), B, T, L, A, D
    "nba": (dict(depth=6, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=4, vec_in_dim=256, normalize=True), 1024, 20, 8, 11, 2),
    "md17": (dict(depth=4, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2), 64, 30, 192, 13, 3),
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
    for name, (kw, B, T, L, A, D) in SHAPES.items():
        g = torch.Generator().manual_seed(5)
        F_ = B * T
        pred, target = (torch.randn(F_, A, D, generator=g).to(dev) for _ in range(2))
        mask = (torch.rand(F_, A, generator=g) > 0.1).to(dev)
        m8 = mask.to(torch.uint8)
        sums, out = torch.empty(F_, 5, device=dev), torch.empty(3, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def kernels():
            _lib.check(lib.lsl_geom_loss_sums(pred.data_ptr(), target.data_ptr(), m8.data_ptr(), F_, A, D, sums.data_ptr(), stream))
            _lib.check(lib.lsl_geom_loss_final(sums.data_ptr(), F_, out.data_ptr(), stream))

        def restated():
            return (masked_mse(pred.reshape(-1, D), target.reshape(-1, D), mask.reshape(-1)),
                    masked_norm(pred.reshape(-1, D), target.reshape(-1, D), mask.reshape(-1)), inter_distance(pred, target, mask))

        def frame_only():
            _lib.check(lib.lsl_geom_loss_sums(pred.data_ptr(), target.data_ptr(), m8.data_ptr(), F_, A, D, sums.data_ptr(), stream))

        def final_only():
            _lib.check(lib.lsl_geom_loss_final(sums.data_ptr(), F_, out.data_ptr(), stream))

        k_ms, k_lo, k_hi = median_ms(kernels, args.calls)
        f_ms, _, _ = median_ms(frame_only, args.calls)
        e_ms, _, _ = median_ms(final_only, args.calls)
        t_ms, t_lo, t_hi = median_ms(restated, args.calls)
        want = restated()
        dev_rel = max(abs(float(out[i]) - float(want[j])) / abs(float(want[j])) for i, j in ((0, 0), (1, 1), (2, 2)))
        net = LatentSIV3(reset_parameters=False, **kw)
        net.load_state_dict(seeded_state_dict(net, seed=0))
        net.to(dev).requires_grad_(False)
        x1, x0, xc = (torch.randn(B, T, L, 32, generator=g).to(dev) for _ in range(3))
        cm = torch.zeros(B, T, L, dtype=torch.long, device=dev)
        cm[:, :T // 3] = 1
        mk = {"x_cond": xc, "x_cond_mask": cm}
        if kw.get("vec_in_dim"):
            mk["y"] = torch.randn(B, kw["vec_in_dim"], generator=g).to(dev)
        t = (torch.rand(B, generator=g) * 0.9 + 0.05).to(dev)
        tr = CreateTransport("GVP", "data")()
        s_ms, s_lo, s_hi = median_ms(lambda: tr.training_losses(net, x1, mk, t=t, x0=x0), 1)
        assert tr.last_path == "fused"
        print(f"{name}: F = {B} x {T} = {F_} frames, A = {A}, D = {D}; backbone {kw['hidden_size']} x {kw['depth']}, L = {L}")
        print(f"  lsl_geom_loss_sums + lsl_geom_loss_final: {k_ms * 1e3:9.1f} us per pair of launches (min {k_lo * 1e3:.1f}, max {k_hi * 1e3:.1f})")
        print(f"    each alone, back to back: k_geom_loss_frame {f_ms * 1e3:.1f} us, k_loss_final<5, 0, 3> {e_ms * 1e3:.1f} us")
        print(f"  torch restatement of the three modules:   {t_ms * 1e3:9.1f} us (min {t_lo * 1e3:.1f}, max {t_hi * 1e3:.1f}); "
              f"kernels / torch = {k_ms / t_ms:.3f}; values agree to {dev_rel:.1e}")
        print(f"  one training_losses (one lsl_si_loss):    {s_ms * 1e3:9.1f} us (min {s_lo * 1e3:.1f}, max {s_hi * 1e3:.1f}); "
              f"the two kernels are {100 * k_ms / s_ms:.3f} % of it, the torch form {100 * t_ms / s_ms:.3f} %")
