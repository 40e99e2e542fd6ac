#!/usr/bin/env python3
"""Cost of the first-stage validation additions at the MD17 and NBA first-stage shapes: ``lsl_class_loss_sums`` + ``lsl_class_loss_final``
(HIP events around back-to-back library calls on preallocated buffers; as a pair and each alone) against the reference's formula through
torch on the same tensors, and ``Stage1Decoder.decode_heads`` against one single-head ``decode`` per head.  One warm-up, then the median
(with min and max) of several runs.  A record, not a gate.
Usage (GPU box):  python tools/first_stage_cost.py [--runs 7] [--calls 20]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lam_slide_amd import Stage1Decoder, _lib  # noqa: E402
from lam_slide_amd.first_stage import cross_entropy, masked_cross_entropy  # noqa: E402
from lam_slide_amd.synthetic import seeded_decoder_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()

SHAPES = {
    # frames, latents L, entities A, decoder heads (num_head_cross, dim_head_cross), heads {name: width}, class heads {name: masked?}
    "md17": (64 * 30, 192, 13, (8, 16), {"pos": 3, "atom": 10}, {"atom": True}),
    "nba": (1024 * 20, 8, 11, (2, 16), {"pos": 2, "team": 3, "group": 2}, {"team": False, "group": False}),
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
    for name, (F_, L, A, (hc, dhc), heads, class_heads) in SHAPES.items():
        g = torch.Generator().manual_seed(6)
        first = next(iter(heads))
        sd = seeded_decoder_state_dict(num_head_cross=hc, dim_head_cross=dhc, out_dim=heads[first], seed=1)
        sd = {k.replace("output_layers.pos.", f"output_layers.{first}."): v for k, v in sd.items()}
        for h, w in list(heads.items())[1:]:
            for k in [k for k in sd if k.startswith(f"decoder.output_layers.{first}.0.")]:
                sd[k.replace(f".{first}.", f".{h}.")] = torch.randn(sd[k].shape, generator=g) * 0.05
            sd[f"decoder.output_layers.{h}.2.weight"] = torch.randn(w, 128, generator=g) * 0.05
            sd[f"decoder.output_layers.{h}.2.bias"] = torch.randn(w, generator=g) * 0.05
        kw = dict(num_head_latent=2, dim_head_latent=16, num_head_cross=hc, dim_head_cross=dhc)
        dec = Stage1Decoder(sd, device=dev, output=first, **kw)
        single = [Stage1Decoder(sd, device=dev, output=h, **kw) for h in heads]
        z, ent = torch.randn(F_, L, 32, generator=g).to(dev), torch.randint(0, 32, (F_, A), generator=g).to(dev)
        print(f"{name}: F = {F_} frames, L = {L}, A = {A}, heads {heads}")
        h_ms, h_lo, h_hi = median_ms(lambda: dec.decode_heads(z, ent), 3)
        s_ms, s_lo, s_hi = median_ms(lambda: [d.decode(z, ent) for d in single], 3)
        o_ms, o_lo, o_hi = median_ms(lambda: single[0].decode(z, ent), 3)
        print(f"  decode_heads, {len(heads)} heads from one trunk: {h_ms:9.3f} ms (min {h_lo:.3f}, max {h_hi:.3f})")
        print(f"  {len(heads)} single-head decodes:               {s_ms:9.3f} ms (min {s_lo:.3f}, max {s_hi:.3f}); one: {o_ms:.3f} ms (min {o_lo:.3f}, max {o_hi:.3f}); "
              f"decode_heads / separate = {h_ms / s_ms:.3f}")
        stream = torch.cuda.current_stream(dev).cuda_stream
        for h, masked in class_heads.items():
            K = heads[h]
            logits = (torch.randn(F_, A, K, generator=g) * 3).to(dev)
            target = torch.randint(0, K, (F_, A), generator=g).to(dev)
            mask = (torch.rand(F_, A, generator=g) > 0.1).to(dev)
            m8 = mask.to(torch.uint8)
            mp = m8.data_ptr() if masked else None
            sums, out = torch.empty(F_, 2, device=dev), torch.empty(1, device=dev)

            def frame_only():
                _lib.check(lib.lsl_class_loss_sums(logits.data_ptr(), target.data_ptr(), mp, F_, A, K, 0.0, sums.data_ptr(), None, stream))

            def final_only():
                _lib.check(lib.lsl_class_loss_final(sums.data_ptr(), F_, out.data_ptr(), stream))

            def kernels():
                frame_only()
                final_only()

            lf, tf, mf = logits.reshape(-1, K), target.reshape(-1), mask.reshape(-1)
            restated = (lambda: masked_cross_entropy(lf, tf, mf)) if masked else (lambda: cross_entropy(lf, tf))
            k_ms, k_lo, k_hi = median_ms(kernels, args.calls)
            f_ms, _, _ = median_ms(frame_only, args.calls)
            e_ms, _, _ = median_ms(final_only, args.calls)
            t_ms, t_lo, t_hi = median_ms(restated, args.calls)
            kernels()
            agree = abs(float(out[0]) - float(restated())) / abs(float(restated()))
            print(f"  {h} (K = {K}, {'masked' if masked else 'no mask'}): lsl_class_loss_sums + lsl_class_loss_final {k_ms * 1e3:8.1f} us per pair (min {k_lo * 1e3:.1f}, "
                  f"max {k_hi * 1e3:.1f}); alone: k_class_loss_frame {f_ms * 1e3:.1f} us, k_loss_final<2, 0, 1> {e_ms * 1e3:.1f} us")
            print(f"      the reference's formula through torch: {t_ms * 1e3:8.1f} us (min {t_lo * 1e3:.1f}, max {t_hi * 1e3:.1f}); kernels / torch = {k_ms / t_ms:.3f}; "
                  f"values agree to {agree:.1e}")
