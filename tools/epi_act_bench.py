#!/usr/bin/env python3
"""Micro-benchmark of the conv kernel's activation epilogue (hsp_conv1d_args.act = HSP_ACT_ACT1D): the fused launch against the two
launches it replaces, conv then stand-alone Activation1d, on the low-channel AMP shapes (a sibling of tools/conv_bench.py).
Rounds of the two forms alternate; per form the median round and the spread of the rounds are printed, in us per call.
   python tools/epi_act_bench.py                      (the five shapes of profiles/epi_act_bench.txt)
   python tools/epi_act_bench.py --shapes 32,3,1,64000 --batch 32 --reps 20 --rounds 5"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from megatts2_hierspeechpp_amd import activations, hip_layers  # noqa: E402
from megatts2_hierspeechpp_amd.alias_free_torch import Activation1d  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="*", default=["32,3,1,64000", "32,7,1,64000", "32,11,1,64000", "64,3,1,32000", "64,7,1,32000"],
                help="channels,k,dilation,length")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.reps


for spec in a.shapes:
    c, k, d, Lc = (int(v) for v in spec.split(","))

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = hip_layers.Conv1d(c, c, k, dilation=d, padding=(k - 1) * d // 2)
            self.act = Activation1d(activations.SnakeBeta(c, alpha_logscale=True))

    m = M()
    m.conv.weight.data.normal_(0, 0.05)
    m.conv.bias.data.normal_(0, 0.1)
    m.act.act.alpha.data.normal_(0, 0.5)
    m.act.act.beta.data.normal_(0, 0.5)
    hip_layers.finalize(m, dev)
    x = torch.randn(a.batch, c, Lc, device=dev)
    xt, y2, y1 = (torch.empty_like(x) for _ in range(3))
    plan = m.conv.plain_plan(x)
    two = lambda: m.act(m.conv(x, out=xt))
    conv_only = lambda: m.conv(x, out=xt)
    fused = lambda: m.conv(x, out=y1, epi_act=m.act)
    y2 = two()
    fused()
    torch.cuda.synchronize()
    equal = torch.equal(y1, y2)
    for f in (two, fused, conv_only):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {"two": [], "fused": [], "conv": []}
    for _ in range(a.rounds):
        t["two"].append(timed(two))
        t["fused"].append(timed(fused))
        t["conv"].append(timed(conv_only))
    med = {n: statistics.median(v) for n, v in t.items()}
    spread = {n: max(v) - min(v) for n, v in t.items()}
    print(f"C {c} k {k} dil {d} L {Lc} B {a.batch} plan {tuple(plan[:3])}: conv {med['conv']:7.1f} us | conv + act1d {med['two']:7.1f} us "
          f"(spread {spread['two']:.1f}) | fused {med['fused']:7.1f} us (spread {spread['fused']:.1f}) | "
          f"fused - two = {med['fused'] - med['two']:+7.1f} us | bit-equal {equal}")
