#!/usr/bin/env python3
"""Device time of one tangent pass (``LatentSIV3.jvp``: ``lsl_forward_jvp``) against one evaluation (``LatentSIV3.forward``: ``lsl_forward``)
at three shapes, in one process on one box, by HIP events around the library call:

  md17_ref    B = 4, T = 30, L = 192, depth 4, hidden 256
  md17_bench  the headline shape of bench.py at B = 1: T = 30, L = 256, depth 4, hidden 512
  peptide     B = 1, T = 1000, L = 2, depth 7, hidden 384 (heads of 24, padded to 32)
Seeded weights (lam_slide_amd/synthetic.py) and inputs.  Per shape: ``--warmup`` calls of each, then ``--runs`` alternating pairs (forward,
jvp), the median of each side.  The largest new kernel's share of a tangent pass is read from a rocprofv3 kernel trace of this tool, in a
run of its own (``rocprofv3 --kernel-trace --stats -- python tools/likelihood_cost.py --shapes NAME --only-jvp``: jvp calls alone).  A record, not a
gate: the numbers go to profiles/likelihood_cost.txt.
Usage (GPU box):  python tools/likelihood_cost.py [--runs 20] [--warmup 3] [--shapes md17_ref,md17_bench,peptide]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lam_slide_amd import LatentSIV3  # noqa: E402
from lam_slide_amd.synthetic import seeded_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--shapes", default="md17_ref,md17_bench,peptide")
ap.add_argument("--only-jvp", action="store_true", help="run jvp calls alone (for a kernel trace of the tangent pass); writes no record")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_cost.txt"))
args = ap.parse_args()
dev = torch.device("cuda:0")

SHAPES = {
    "md17_ref": (dict(depth=4, in_dim=32, hidden_size=256, num_heads=16, mlp_ratio=2), 4, 30, 192),
    "md17_bench": (dict(depth=4, in_dim=32, hidden_size=512, num_heads=16, mlp_ratio=2), 1, 30, 256),
    "peptide": (dict(depth=7, in_dim=96, hidden_size=384, num_heads=16, mlp_ratio=4), 1, 1000, 2),
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


lines = [f"one tangent pass (LatentSIV3.jvp) against one evaluation (LatentSIV3.forward); measured on {torch.cuda.get_device_name(0)} "
         f"(torch {torch.__version__}); HIP events around the call, median of {args.runs} alternating pairs after {args.warmup} warm-up calls of each"]
for name in args.shapes.split(","):
    netkw, B, T, L = SHAPES[name]
    net = LatentSIV3(reset_parameters=False, **netkw)
    net.load_state_dict(seeded_state_dict(net, seed=0))
    net = net.to(dev)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, T, L, netkw["in_dim"], generator=g).to(dev)
    xc = torch.randn(B, T, L, netkw["in_dim"], generator=g).to(dev)
    mask = (torch.rand(B, T, L, generator=g) < 0.2).long().to(dev)
    t = torch.rand(B, generator=g).to(dev)
    v = (torch.randint(2, x.shape, generator=g).float() * 2 - 1).to(dev)
    fwd = lambda: net(x, t, xc, mask)  # noqa: E731
    jvp = lambda: net.jvp(x, t, xc, mask, tangent=v)  # noqa: E731
    if args.only_jvp:
        for _ in range(args.warmup + args.runs):
            jvp()
        torch.cuda.synchronize()
        continue
    for _ in range(args.warmup):
        fwd()
        jvp()
    torch.cuda.synchronize()
    tf, tj = [], []
    for _ in range(args.runs):
        tf.append(timed(fwd))
        tj.append(timed(jvp))
    out, _ = jvp()
    same = torch.equal(out, fwd())
    mf, mj = statistics.median(tf), statistics.median(tj)
    lines.append(f"{name}: B = {B}, T = {T}, L = {L}, depth {netkw['depth']}, hidden {netkw['hidden_size']}, {B * T * L} tokens: forward {mf:8.3f} ms "
                 f"(min {min(tf):.3f}, max {max(tf):.3f}), jvp {mj:8.3f} ms (min {min(tj):.3f}, max {max(tj):.3f}), jvp / forward {mj / mf:5.2f}x, "
                 f"primal output bit-equal to forward: {same}")
if args.only_jvp:
    sys.exit(0)
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
