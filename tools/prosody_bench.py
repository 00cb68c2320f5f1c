#!/usr/bin/env python3
"""Kernel time of the prosody codes of one mel: the single hsp_prosody_encode_f32 launch against the launches the legacy
path issued for the same mel before it (PLMConv as mask_mul + two direct convs, hsp_maxpool1d_f32, the pooled mask,
PLMConv again, hsp_vq_nearest_f32), from a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/prosody_prof -- python3 tools/prosody_bench.py run --out OUT
    python3 tools/prosody_bench.py summarize OUT

``run`` alternates the two paths in one process, ``--calls`` times per mel length, and launches a marker kernel
(hsp_zero_below_f32 on one element, which neither path uses) between them; ``summarize`` cuts the trace at the markers,
sums the kernel durations of every segment and prints the median per path and length (and writes OUT/prosody_bench.json).
The prompt's mel mask is made outside the segments: the legacy infer() shared it with the style encoder.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MARKER = "zero_below_kernel"


def legacy_codes(ttv, mel, lens, mel_mask):
    """The launches SynthesizerTrn.infer issued for its prompt codes before prosody_codes (T a multiple of 8)."""
    import torch
    from megatts2_hierspeechpp_amd import _lib as L, functional as Fh
    B, _, Tm = mel.shape
    q_in = ttv.plm_conv1(mel[:, :20], mel_mask)
    pooled = torch.empty(B, 20, Tm // 8, dtype=torch.float32, device=mel.device)
    L.check(L.lib().hsp_maxpool1d_f32(L.fptr(q_in), q_in.stride(0), q_in.stride(1), L.fptr(pooled), B, 20, Tm, 8,
                                      L.stream_ptr()), "hsp_maxpool1d_f32")
    pool_len = torch.div(lens + 7, 8, rounding_mode="floor")
    q_in = ttv.plm_conv2(pooled, Fh.sequence_mask(pool_len, Tm // 8))
    codes = torch.empty(B, Tm, dtype=torch.int64, device=mel.device)
    cb = ttv.quantizer.vq.layers[0]._codebook
    L.check(L.lib().hsp_vq_nearest_f32(L.fptr(q_in), q_in.stride(0), q_in.stride(1), L.fptr(cb._w), L.ptr(codes),
                                       codes.stride(0), B, 20, Tm // 8, ttv.quantizer.bins, 8, Tm, L.stream_ptr()),
            "hsp_vq_nearest_f32")
    return codes


def run(args):
    import torch
    import helpers as H
    from megatts2_hierspeechpp_amd import functional as Fh, synth
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    from megatts2_hierspeechpp_amd.inference_plm import zero_below
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import SynthesizerTrn
    dev = torch.device("cuda:0")
    ttv = SynthesizerTrn(126, 11, 4, 641, 320, 16000, 60, **H.TTV_MODEL)
    ttv.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7)) for k, v in ttv.state_dict().items()})
    finalize(ttv, dev)
    one = torch.ones(1, device=dev)
    plan = []
    for T in args.T:
        assert T % 8 == 0, "the legacy path needs a mel length that is a multiple of 8"
        mel = torch.from_numpy(synth.synth_inputs(1, T, seed=900 + T)["mel"]).to(dev)
        lens = torch.full((1,), T, dtype=torch.int64, device=dev)
        mask = Fh.sequence_mask(lens, T)
        for _ in range(3):                                              # warm both paths at this shape
            a, b = legacy_codes(ttv, mel, lens, mask), ttv.prosody_codes(mel, lens)
        torch.cuda.synchronize()
        same = bool(torch.equal(a, b))
        print(f"T = {T}: legacy and fused codes equal: {same} ({int((a != b).sum())} of {T} frames differ)")
        zero_below(one, 0.0)
        for _ in range(args.calls):
            legacy_codes(ttv, mel, lens, mask)
            zero_below(one, 0.0)
            ttv.prosody_codes(mel, lens)
            zero_below(one, 0.0)
            plan += [[T, "legacy"], [T, "fused"]]
        torch.cuda.synchronize()
    os.makedirs(args.out, exist_ok=True)
    json.dump(plan, open(os.path.join(args.out, "prosody_bench_plan.json"), "w"))


def summarize(args):
    plan = json.load(open(os.path.join(args.out, "prosody_bench_plan.json")))
    files = glob.glob(os.path.join(args.out, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    # segments between consecutive markers; per length the warm-up precedes the first marker, so a segment that is no
    # call (warm-up of the next length) is longer than a call's launches and is found by its position in the plan
    segs, cur = [], None
    for r in rows:
        if MARKER in r["Kernel_Name"]:
            if cur is not None:
                segs.append(cur)
            cur = []
        elif cur is not None:
            cur.append(r)
    calls = len(plan) // len({t for t, _ in plan})
    per_len = calls + 1                                                # + the warm-up segment between two lengths
    out, k = {}, 0
    for i, seg in enumerate(segs):
        if i % per_len == calls:
            continue
        T, path = plan[k]
        k += 1
        d = out.setdefault(f"{path}_T{T}", dict(us=[], launches=[], kernels={}))
        d["us"].append(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in seg) / 1e3)
        d["launches"].append(len(seg))
        for r in seg:
            m = re.search(r"(\w*_kernel\w*)", r["Kernel_Name"])
            name = m.group(1) if m else r["Kernel_Name"][:60]
            d["kernels"].setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    assert k == len(plan), (k, len(plan), len(segs))
    res = {}
    for key, d in out.items():
        res[key] = dict(median_us=statistics.median(d["us"]), min_us=min(d["us"]), max_us=max(d["us"]), calls=len(d["us"]),
                        launches=statistics.median(d["launches"]),
                        kernels_median_us={n: round(statistics.median(v) * len(v) / len(d["us"]), 3) for n, v in d["kernels"].items()})
        print(key, json.dumps(res[key]))
    json.dump(res, open(os.path.join(args.out, "prosody_bench.json"), "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--out", required=True)
    r.add_argument("--T", type=int, nargs="+", default=[152, 3000])
    r.add_argument("--calls", type=int, default=24)
    s = sub.add_parser("summarize")
    s.add_argument("out")
    args = ap.parse_args()
    run(args) if args.cmd == "run" else summarize(args)


if __name__ == "__main__":
    main()
