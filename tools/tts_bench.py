#!/usr/bin/env python3
"""BASELINE.json configs[2]: full text -> 16 kHz synthesis on one MI355X, batch 16: phone ids
U{12..112} [B, 40], tone U{0..10}, prompt mel [B, 80, 150], durations pinned to 10 frames / phone (-> 200 PLM steps, 4 s
of audio per utterance), synthetic weights.  The workload lives in tools/bench_extra.py (bench.py prints it as
extra_configs.tts_b16); this is its command line.

    python tools/tts_bench.py [--batch 16] [--phones 40] [--steps 3] [--warmup 1] [--no-graph] [--sample] [--rounds 3]

Prints one JSON line with the whole-step rate and the per-stage split (HIP events).  --sample: the PLM loop samples
(top_k 10, top_p 0.9, temperature 0.8, repetition_penalty 1.1) -- greedy and sampled steps alternate on the same models
for --rounds rounds, one JSON line each, then one summary line with the medians of both."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import bench_extra  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--phones", type=int, default=40)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--no-graph", action="store_true", help="launch everything eagerly instead of replaying hipGraphs")
ap.add_argument("--sample", action="store_true", help="time the sampled PLM loop against greedy, alternating")
ap.add_argument("--rounds", type=int, default=3, help="--sample: greedy / sampled rounds")
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
kw = dict(steps=args.steps, warmup=args.warmup, batch=args.batch, phones=args.phones, use_graph=not args.no_graph)
if not args.sample:
    print(json.dumps(bench_extra.tts_b16(dev, **kw)))
    sys.exit(0)

from megatts2_hierspeechpp_amd import inference_plm as IP, synth  # noqa: E402
from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling  # noqa: E402

models = IP.TtsModels(bench_extra.VOC_CFG, bench_extra.TTV_CFG)
models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 0)) for k, v in models.state_dict().items()})
models.finalize(dev)
sp = PlmSampling(temperature=0.8, top_k=10, top_p=0.9, repetition_penalty=1.1)
runs = {"greedy": [], "sampled": []}
for r in range(args.rounds):
    for mode in (("greedy", "sampled") if r % 2 == 0 else ("sampled", "greedy")):
        res = bench_extra.tts_b16(dev, models=models, plm_sampling=sp if mode == "sampled" else None, **kw)
        res["plm_decoding"] = mode
        runs[mode].append(res)
        print(json.dumps(res))


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


print(json.dumps({"summary": "tts_b16 greedy vs sampled PLM loop (" + str(sp) + ")",
                  **{f"{m}_ms_per_step": med([x["ms_per_step"] for x in runs[m]]) for m in runs},
                  **{f"{m}_plm_loop_ms": med([x["stage_ms"]["plm_loop(A18)"] for x in runs[m]]) for m in runs}}))
