#!/usr/bin/env python3
"""Time ragged prosody-LM decoding: a decode session (Megatts2PLM1.infer_many) against padded batches of infer(causal=True).

    python tools/plm_session_bench.py [--requests 64] [--slots 16] [--reps 10] [--out profiles/plm_session.json]

A seeded request mix (``--requests`` lengths uniform in 60 .. 240) on the synthetic weights, two arms:
 (a) one session of ``--slots`` rows: the step captured once, then PlmDecodeSession.run (admit / replay / copy-out);
 (b) what causal decoding offered before sessions: arrival-order batches of ``--slots`` through ``infer(causal=True)``,
     zero-padded to the batch's longest row, each batch its own captured graph.  Its replay time and its capture time are
     reported separately: the capture is what (b) pays for every new (B, T).
Device time between two events around each run, median and spread over ``--reps`` runs after 3 warm-up runs, the arms
alternating.  The step counts of both arms come from session_plan / the batch maxima: their ratio is arithmetic.
A second measurement puts the session's step (all slots busy, 200 replays) beside the by-value loop at slots x 200 (one
graph of 200 steps), alternating; a third runs the same 200 session steps as graphs of k = 1, 2, 4, 8, 200 steps each, which
separates the cost of one replay per step from the cost of the step's own launches.  ``--only session`` runs arm (a) alone, for a kernel trace under a profiler.
Prints one JSON line and writes it to ``--out`` when given.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v, steps=None):
    d = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    if steps:
        d["steps"] = steps
        d["per_step_us"] = round(1e3 * statistics.median(v) / steps, 1)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", choices=["both", "session"], default="both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plm_session_bench needs a GPU: a CPU run says nothing about the loop's time")
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import Megatts2PLM1, session_plan
    dev = torch.device("cuda:0")
    m = Megatts2PLM1()
    m.load_state_dict({k: torch.from_numpy(synth.synth_tensor("plm." + k, tuple(v.shape), 7))
                       for k, v in m.state_dict().items()})
    m.finalize(dev)
    S = args.slots
    lengths = [int(n) for n in np.random.default_rng(args.seed).integers(60, 241, args.requests)]
    gen = torch.Generator().manual_seed(1)
    reqs = [torch.randn(256, n, generator=gen).to(dev) for n in lengths]
    result = {"tool": "plm_session_bench", "reps": args.reps, "requests": args.requests, "slots": S,
              "lengths": {"min": min(lengths), "max": max(lengths), "sum": sum(lengths)}}

    # (a) the session
    ses = m.decode_session(S, max(lengths))
    t0 = time.perf_counter()
    ses.capture()
    torch.cuda.synchronize()
    capture_a = time.perf_counter() - t0
    steps_a = session_plan(lengths, S)[1]
    out_a = ses.run(reqs)
    torch.cuda.synchronize()

    # (b) padded batches, one graph each
    graphs, capture_b, steps_b = [], 0.0, 0
    if args.only == "both":
        for i in range(0, len(reqs), S):
            part = reqs[i:i + S]
            T = max(q.shape[1] for q in part)
            tc = torch.zeros(len(part), 256, T, device=dev)
            for b, q in enumerate(part):
                tc[b, :, :q.shape[1]] = q
            m.infer(tc, causal=True)                                  # eager once: code objects, LDS limits
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = m.infer(tc, causal=True)
            torch.cuda.synchronize()
            capture_b += time.perf_counter() - t0
            graphs.append((g, out, part, tc))                       # tc: the graph reads it at every replay
            steps_b += T
        for g, _, _, _ in graphs:
            g.replay()
        torch.cuda.synchronize()
        same = all(torch.equal(out[b, :q.shape[1]], out_a[i * S + b])
                   for i, (_, out, part, _) in enumerate(graphs) for b, q in enumerate(part))
        result["arms_agree"] = bool(same)                              # causal rows do not depend on their padding

    ta, tb = [], []
    for rep in range(args.reps + 3):
        a = timed(lambda: ses.run(reqs))
        b = timed(lambda: [g.replay() for g, _, _, _ in graphs]) if graphs else None
        if rep >= 3:
            ta.append(a)
            if graphs:
                tb.append(b)
    result["session"] = dict(stats(ta, steps_a), capture_ms=round(1e3 * capture_a, 1), graphs=1)
    if graphs:
        result["padded_batches"] = dict(stats(tb, steps_b), capture_ms=round(1e3 * capture_b, 1), graphs=len(graphs))
        result["step_ratio"] = round(steps_b / steps_a, 3)
        result["time_ratio"] = round(statistics.median(tb) / statistics.median(ta), 3)

    # the step itself: all slots busy for 200 steps, beside the by-value loop at slots x 200
    if args.only == "both":
        T = 200
        tc = torch.randn(S, 256, T, generator=gen).to(dev)
        ses2 = m.decode_session(S, T)
        ses2.capture()
        m.infer(tc, causal=True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            m.infer(tc, causal=True)

        def session_steps():
            for _ in range(T):
                ses2.step()

        ts, tl = [], []
        for rep in range(args.reps + 3):
            for b in range(S):
                ses2.admit(b, tc[b])
            torch.cuda.synchronize()
            a = timed(session_steps)
            b = timed(g.replay)
            if rep >= 3:
                ts.append(a)
                tl.append(b)
        result[f"step_{S}x{T}"] = {"session": stats(ts, T), "by_value_loop": stats(tl, T)}
        # what one replay per step costs: the same 200 steps as graphs of k steps each
        sweep = {}
        for k in (1, 2, 4, 8, T):
            gk = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gk):
                for _ in range(k):
                    ses2.enqueue_step()
            tk = []
            for rep in range(args.reps + 3):
                for b in range(S):
                    ses2.admit(b, tc[b])
                ses2._left = [0] * S                                   # the graphs below advance the rows, not step()
                torch.cuda.synchronize()
                tk.append(timed(lambda: [gk.replay() for _ in range(T // k)]))
            sweep[str(k)] = stats(tk[3:], T)["per_step_us"]
        result["per_step_us_by_steps_per_graph"] = sweep
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
