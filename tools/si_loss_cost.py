#!/usr/bin/env python3
"""Cost of the stochastic-interpolant objective next to the network it wraps (profiles/si_loss_cost.txt): one md17_bench-shape
``Transport.training_losses`` (B = 32 by default) against ``net.forward`` alone, HIP-event times; and the share of k_si_mix + k_si_loss_*
in a rocprofv3 kernel trace of the call.
Usage (GPU box):
    python tools/si_loss_cost.py [--batch 32] [--calls 10]                      the two timings
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/si_loss_cost.py --only-loss --calls 3
    python tools/si_loss_cost.py --summary DIR                                  shares from DIR's *kernel_stats.csv"""
import argparse
import csv
import glob
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only-loss", action="store_true")
ap.add_argument("--summary")
args = ap.parse_args()

if args.summary:
    for f in sorted(glob.glob(os.path.join(args.summary, "**", "*kernel_stats.csv"), recursive=True)):
        rows = [r for r in csv.DictReader(open(f)) if not r["Name"].startswith(("at::", "void at::", "__amd_rocclr"))]
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        pick = lambda keys: sum(float(r["TotalDurationNs"]) for r in rows if any(k in r["Name"] for k in keys))  # noqa: E731
        si, emb = pick(("k_si_mix", "k_si_loss")), pick(("k_embed", "k_head"))
        print(f"# {os.path.basename(f)}: library kernels {tot / 1e6:.3f} ms in the trace")
        print(f"k_si_mix + k_si_loss_partial + k_si_loss_final: {si / 1e3:.1f} us = {100 * si / tot:.3f} % of the library's kernel time")
        print(f"embedding + head kernels of the same trace:     {emb / 1e3:.1f} us = {100 * emb / tot:.3f} %")
        for r in rows:
            if any(k in r["Name"] for k in ("k_si_mix", "k_si_loss", "k_embed", "k_head")):
                print(f"  calls {int(r['Calls']):4d}  avg {float(r['AverageNs']) / 1e3:9.2f} us  {r['Name'].split('(')[0][:100]}")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lam_slide_amd import CreateTransport, LatentSIV3  # noqa: E402
from lam_slide_amd.synthetic import seeded_state_dict  # noqa: E402

dev = torch.device("cuda:0")
kw = dict(depth=4, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2)  # md17_bench (bench.py)
B, T, L = args.batch, 30, 256
net = LatentSIV3(reset_parameters=False, **kw)
net.load_state_dict(seeded_state_dict(net, seed=0))
net.to(dev).requires_grad_(False)
g = torch.Generator().manual_seed(1)
x1, x0, xc = (torch.randn(B, T, L, 32, generator=g).to(dev) for _ in range(3))
mask = torch.zeros(B, T, L, dtype=torch.long, device=dev)
mask[:, :10] = 1
t = (torch.rand(B, generator=g) * 0.9 + 0.05).to(dev)
tr = CreateTransport("GVP", "data")()
mk = {"x_cond": xc, "x_cond_mask": mask}


def timed(fn):
    for _ in range(args.warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.calls):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.calls, out


with torch.no_grad():
    ms_loss, out = timed(lambda: tr.training_losses(net, x1, mk, t=t, x0=x0))
    assert tr.last_path == "fused"
    print(f"md17_bench shape B = {B} ({B * T * L} tokens): training_losses (one lsl_si_loss) {ms_loss:.3f} ms per call, "
          f"mean loss {float(out['loss'].mean()):.6f}")
    if not args.only_loss:
        xt = (x1 + x0).contiguous()
        ms_fwd, _ = timed(lambda: net(xt, t, xc, mask))
        print(f"net.forward alone on the same box: {ms_fwd:.3f} ms per call; the objective adds {ms_loss - ms_fwd:+.3f} ms "
              f"({100 * (ms_loss - ms_fwd) / ms_fwd:+.2f} %)")
