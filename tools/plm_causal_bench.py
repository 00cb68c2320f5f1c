#!/usr/bin/env python3
"""Time the prosody-LM loop (Megatts2PLM1.infer) in both decoding modes, each as a captured graph.

    python tools/plm_causal_bench.py [--shapes 16x200,1x200] [--reps 20] [--sampling] [--out profiles/plm_causal_loop.json]

(a) the reference's bidirectional loop (``infer``), (b) K/V-cached causal decoding (``infer(causal=True)``), on the same
synthetic weights and inputs, alternating the two graphs replay by replay; device time between two events around each
replay, median and spread over ``--reps`` replays after 3 warm-up replays.  ``--sampling``: both loops draw their codes
(one fixed PlmSampling, seed 0) instead of taking the argmax.  Prints one JSON line and writes it to
``--out`` when given.  The share of device time the decode kernel takes in (b) comes from a kernel trace of its own
(``--only causal`` under a profiler), not from this run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x200,1x200")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["both", "bidirectional", "causal"], default="both")
    ap.add_argument("--sampling", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plm_causal_bench needs a GPU: a CPU run says nothing about the loop's time")
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import Megatts2PLM1, PlmSampling
    dev = torch.device("cuda:0")
    m = Megatts2PLM1()
    m.load_state_dict({k: torch.from_numpy(synth.synth_tensor("plm." + k, tuple(v.shape), 7))
                       for k, v in m.state_dict().items()})
    m.finalize(dev)
    modes = [("bidirectional", False), ("causal", True)]
    modes = [x for x in modes if args.only in ("both", x[0])]
    how = dict(sampling=PlmSampling(temperature=0.9, top_k=30, top_p=0.95, repetition_penalty=1.2), seeds=0) \
        if args.sampling else {}
    result = {"tool": "plm_causal_bench", "reps": args.reps, "sampling": args.sampling, "shapes": {}}
    for shape in args.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        tc = torch.randn(B, 256, T, generator=torch.Generator().manual_seed(1)).to(dev)
        graphs = {}
        for name, causal in modes:
            m.infer(tc, causal=causal, **how)                # eager once: code objects, LDS limits
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = m.infer(tc, causal=causal, **how)
            graphs[name] = (g, out)
        times = {name: [] for name in graphs}
        for rep in range(args.reps + 3):
            for name, (g, _) in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    times[name].append(e0.elapsed_time(e1))
        result["shapes"][shape] = {name: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                                          "max_ms": round(max(v), 3), "per_step_us": round(1e3 * statistics.median(v) / T, 1)}
                                   for name, v in times.items()}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
