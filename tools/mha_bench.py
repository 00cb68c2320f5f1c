#!/usr/bin/env python3
"""Time hsp_mha_f32 (B x H x D, the batch side by side on the columns, the PLM layout) in a hipGraph of --calls calls.
Every row names the kernel hsp_mha_plan gives the launch.

    python tools/mha_bench.py [--batch 16] [--heads 4] [--dim 69] [--lens 16,32,...] [--masked] [--window W]
    python tools/mha_bench.py --per-kernel        one row per kernel at H = 2, D = 96, B = 16

--masked adds factor masks of ones, --window W the relative-position terms: the launches that the latency kernel (TOK)
does not take.  --per-kernel asks hsp_mha_plan, for the plain, the masked and the windowed launch in turn, which kernel
each length of --candidates gets, and times the first length that reaches each of the six kernels; no threshold of
mha_decide is written down here."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from megatts2_hierspeechpp_amd import _lib as L  # noqa: E402
from megatts2_hierspeechpp_amd import functional as Fh  # noqa: E402

KERNELS = ("TOK", "MFMA_WHOLE", "MFMA_SLAB", "MFMA_STREAM", "ROW", "ROW_STREAM")   # HSP_MHA_* of hsp.h

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--heads", type=int, default=4)
ap.add_argument("--dim", type=int, default=69)
ap.add_argument("--lens", default="16,32,64,100,128,160,200")
ap.add_argument("--masked", action="store_true", help="mask_q / mask_k of ones")
ap.add_argument("--window", type=int, default=0, help="rel_k / rel_v of this window")
ap.add_argument("--per-kernel", action="store_true", help="H = 2, D = 96, B = 16: one length per kernel, found by hsp_mha_plan")
ap.add_argument("--candidates", default="64,128,256,320,512,768,960,1024,1280,1536,2048,2304,2560,3072,4096")
ap.add_argument("--calls", type=int, default=50, help="launches per graph")
a = ap.parse_args()
dev = torch.device("cuda:0")


def plan(B, H, D, T, masked, window):
    """Kernel index hsp_mha_plan names for the launch (no launch: the pointers only have to be non-null), or None."""
    s, p = L.MhaArgs(), 0x1000
    s.q = s.k = s.v = s.o = p
    s.B, s.H, s.D, s.Tq, s.Tk, s.qk_scale = B, H, D, T, T, 1.0
    s.q_bs = s.k_bs = s.v_bs = s.o_bs = T
    s.q_cs = s.k_cs = s.v_cs = s.o_cs = B * T
    if masked:
        s.mask_q = s.mask_k = p
    if window:
        s.rel_k, s.rel_v, s.window = p, p, window
    out = (ctypes.c_int32 * 4)()
    return out[0] if L.lib().hsp_mha_plan(ctypes.byref(s), out) == 0 else None


def bench(B, H, D, T, masked, window):
    qkv = torch.randn(3 * H * D, B * T, device=dev)
    o = torch.empty(H * D, B * T, device=dev)
    per = lambda m: m.reshape(-1, B, T).permute(1, 0, 2)
    q, k, v = (per(qkv[i * H * D:(i + 1) * H * D]) for i in range(3))
    kw = {}
    if masked:
        kw.update(mask_q=torch.ones(B, T, device=dev), mask_k=torch.ones(B, T, device=dev))
    if window:
        kw.update(rel_k=torch.randn(2 * window + 1, D, device=dev) * D ** -0.5,
                  rel_v=torch.randn(2 * window + 1, D, device=dev) * D ** -0.5, window=window)
    run = lambda: Fh.mha(q, k, v, H, D ** -0.5, out=per(o), **kw)
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(a.calls):
            run()
    g.replay()
    torch.cuda.synchronize()
    us = float("inf")
    for _ in range(3):                      # the best of three passes of four replays
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        us = min(us, e0.elapsed_time(e1) * 1e3 / (4 * a.calls))
    fl = 4.0 * B * H * T * T * D
    kern = plan(B, H, D, T, masked, window)
    what = "masked" if masked else f"window {window}" if window else "plain"
    print(f"{KERNELS[kern]:11s} T={T:4d} {what:9s}: {us:8.1f} us / call   {fl / us / 1e6:6.2f} TFLOP/s (algorithmic)", flush=True)


if a.per_kernel:
    B, H, D = 16, 2, 96
    rows = {}
    for masked, window in ((False, 0), (True, 0), (False, a.window or 4)):
        for T in [int(t) for t in a.candidates.split(",")]:
            kern = plan(B, H, D, T, masked, window)
            if kern is not None and kern not in rows:
                rows[kern] = (T, masked, window)
    for kern in sorted(rows):
        bench(B, H, D, *rows[kern])
    for kern in set(range(len(KERNELS))) - set(rows):
        print(f"{KERNELS[kern]:11s} not reached by --candidates")
else:
    for T in [int(t) for t in a.lens.split(",")]:
        bench(a.batch, a.heads, a.dim, T, a.masked, a.window)
