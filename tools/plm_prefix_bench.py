#!/usr/bin/env python3
"""Time prosody-LM decoding behind a given code prefix, and the prefill alone.

    python tools/plm_prefix_bench.py [--T 200] [--prefixes 0,1,2,4,8,50,150] [--reps 20] [--out profiles/plm_prefix.json]

At B = 1 and T frames, for every prefix length P: (a) ``infer(causal=True, prefix_codes=...)`` -- P = 0 is the loop without
a prefix -- and (b) ``Megatts2PLM1.prefill`` alone (embedding, per layer the q/k/v GEMM over P columns and
hsp_plm_prefill_attn_f32, out-proj and feed-forward but for the last layer), both launched eagerly as a session's ``admit``
launches them.  Device time between two events around each call, median and spread over ``--reps`` calls after 3 warm-up
calls, the variants alternating call by call.  The yardstick -- the loop WITHOUT this feature, as a captured graph, and its
time per step -- is the parent commit's tools/plm_causal_bench.py run on the same machine in the same visit; this tool
also times the captured unprefixed loop of its own tree (``loop_graph``) so that the two can be seen to agree.  Prints one
JSON line and writes it to ``--out`` when given.
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
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--prefixes", default="0,1,2,4,8,50,150")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plm_prefix_bench needs a GPU: a CPU run says nothing about the loop's time")
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import Megatts2PLM1
    dev = torch.device("cuda:0")
    m = Megatts2PLM1()
    m.load_state_dict({k: torch.from_numpy(synth.synth_tensor("plm." + k, tuple(v.shape), 7))
                       for k, v in m.state_dict().items()})
    m.finalize(dev)
    T = args.T
    Ps = [int(v) for v in args.prefixes.split(",")]
    if any(p < 0 or p >= T for p in Ps):
        raise SystemExit(f"prefix lengths must lie in [0, {T})")
    tc = torch.randn(1, 256, T, generator=torch.Generator().manual_seed(1)).to(dev)
    own = m.infer(tc, causal=True)                                   # the prefixes: the row's own codes
    D, Tp = m.d_model, (T + 3) & ~3
    kv = [(torch.empty(D, 1, Tp, device=dev), torch.empty(D, 1, Tp, device=dev)) for _ in m.plm.layers]
    rows = [(kc[:, 0], vc[:, 0]) for kc, vc in kv]

    variants = {}
    for P in Ps:
        pre = own[:, :P].contiguous() if P else None
        variants[f"infer_P{P}"] = (lambda pre=pre: m.infer(tc, causal=True, prefix_codes=pre))
        if P:
            variants[f"prefill_P{P}"] = (lambda pre=pre: m.prefill(tc[0], pre[0], rows))
    m.infer(tc, causal=True)                                         # eager once: code objects, LDS limits
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.infer(tc, causal=True)
    variants["loop_graph"] = graph.replay

    times = {name: [] for name in variants}
    for rep in range(args.reps + 3):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 3:
                times[name].append(e0.elapsed_time(e1))
    stat = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    result = {"tool": "plm_prefix_bench", "B": 1, "T": T, "reps": args.reps, "launch": "eager (loop_graph: captured)",
              "infer": {str(P): stat(times[f"infer_P{P}"]) for P in Ps},
              "prefill": {str(P): stat(times[f"prefill_P{P}"]) for P in Ps if P},
              "loop_graph": dict(stat(times["loop_graph"]),
                                 per_step_us=round(1e3 * statistics.median(times["loop_graph"]) / T, 1))}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
