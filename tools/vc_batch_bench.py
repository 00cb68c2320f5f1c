#!/usr/bin/env python3
"""Batched voice conversion (inference_vc.vc_batch) on the synthetic-weight model of bench.py's vc_b1_4s line:
B in {1, 4, 16, 32} x 4 s sources at equal length, and one ragged mix of 1-8 s sources sharing one 3-s prompt.
hipGraph replay per fixed shape (median of HIP-event pairs), a per-stage split from one eager pass with events
(inference_vc.STAGE_HOOK; host submission included), and for the ragged mix the solo-versus-batch deviation of every
row (contract item 3).  Prints one JSON line.
    python tools/vc_batch_bench.py [--steps N] [--batches 1,4,16,32] [--row-exact]
--row-exact adds, in the same process: the ragged mix with row_exact=True (and its deviation), the mix as
length-grouped batches (vc_batch_files' default: one batch per padded length, times summed), and 16 x 4 s with
row_exact=True against the default."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_extra import VOC_CFG, _speechlike, event_median_ms  # noqa: E402


def setup(dev):
    from megatts2_hierspeechpp_amd import inference_vc as IV, synth
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    models = IV.VcModels(VOC_CFG)
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 0)) for k, v in models.state_dict().items()})
    models.finalize(dev)
    mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                                 n_mels=80, window_fn=torch.hann_window).finalize(dev)
    return models, mel_fn


def batch(dev, raw_lengths, prompt_seconds=3.0, seed=11):
    """sources of the given raw lengths (padded by pad_source), their tracks, one shared prompt, noise; tensor form"""
    from megatts2_hierspeechpp_amd import inference_vc as IV
    r = np.random.default_rng(seed + 2)
    srcs = [IV.pad_source(torch.from_numpy(_speechlike(n, seed + b)).to(dev)) for b, n in enumerate(raw_lengths)]
    mk_f0 = lambda n: torch.from_numpy(np.where(r.random(n) < 0.3, 0, r.uniform(90, 300, n)).astype(np.float32)).to(dev)
    f0s = [mk_f0(s.shape[-1] // 80) for s in srcs]
    trg = torch.from_numpy(_speechlike(int(prompt_seconds * 16000), 12)).to(dev)
    f0t = mk_f0(trg.shape[-1] // 80)
    x, xl = IV._stack(srcs, dev)
    fs, fl = IV._stack(f0s, dev)
    T = x.shape[1] // 320
    noise = torch.from_numpy(r.standard_normal((len(srcs), 192, T)).astype(np.float32)).to(dev)
    return dict(srcs=srcs, f0s=f0s, trg=trg, f0t=f0t, x=x, xl=torch.tensor(xl, device=dev), fs=fs,
                fl=torch.tensor(fl, device=dev), noise=noise, seconds=sum(s.shape[-1] for s in srcs) / 16000.0)


def measure(models, mel_fn, d, steps, row_exact=False):
    from megatts2_hierspeechpp_amd import inference_vc as IV
    run = lambda: IV.vc_batch(models, mel_fn, (d["x"], d["xl"]), (d["fs"], d["fl"]), d["trg"], d["f0t"], noise=d["noise"],
                              row_exact=row_exact)
    run()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    torch.cuda.synchronize()
    ms = event_median_ms(g.replay, steps)
    ev = []
    IV.STAGE_HOOK = lambda name: ev.append((name, torch.cuda.Event(enable_timing=True))) or ev[-1][1].record()
    try:
        run()
    finally:
        IV.STAGE_HOOK = None
    torch.cuda.synchronize()
    stage = {ev[i][0]: ev[i][1].elapsed_time(ev[i + 1][1]) for i in range(len(ev) - 1)}
    return {"B": d["x"].shape[0], "audio_s": d["seconds"], "ms_per_batch": ms, "rtf": ms * 1e-3 / d["seconds"],
            "stage_ms_eager": stage}


def ragged_deviation(models, mel_fn, d, row_exact=False):
    """Solo vc() per row against the batch's float row (same noise slice): max |diff| / row peak over the whole row and
    over all but the last 0.5 s, and the distance from the row end beyond which |diff| stays below 1e-4 of the peak."""
    from megatts2_hierspeechpp_amd import inference_vc as IV
    _, n_out, audio = IV.vc_batch(models, mel_fn, d["srcs"], d["f0s"], d["trg"], d["f0t"], noise=d["noise"],
                                  return_float=True, row_exact=row_exact)
    rows = []
    for b, s in enumerate(d["srcs"]):
        n = int(n_out[b])
        T = n // 320
        _, a1 = IV.vc(models, mel_fn, s, d["f0s"][b].reshape(1, -1), d["trg"], d["f0t"].reshape(1, -1),
                      noise=d["noise"][b:b + 1, :, :T].contiguous(), return_float=True)
        solo = a1.reshape(-1).double()
        diff = (audio[b, 0, :n].double() - solo).abs()
        peak = float(solo.abs().max())
        over = torch.nonzero(diff > 1e-4 * peak)
        rows.append({"seconds": n / 16000.0, "max_rel": float(diff.max()) / peak,
                     "max_rel_excl_last_0.5s": float(diff[:max(n - 8000, 0)].max()) / peak if n > 8000 else None,
                     "below_1e-4_from_end_s": (n - int(over[0])) / 16000.0 if len(over) else 0.0})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", default="1,4,16,32")
    ap.add_argument("--row-exact", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    models, mel_fn = setup(dev)
    out = {"metric": "vc_batch latency per batch (hipGraph replay) and RTF, synthetic weights", "equal_4s": [],
           "unit": "ms"}
    n4 = 4 * 16000 - 640                                      # 4 s after pad_source, as vc_b1_4s
    with torch.no_grad():
        for B in [int(b) for b in a.batches.split(",")]:
            out["equal_4s"].append(measure(models, mel_fn, batch(dev, [n4] * B), a.steps))
            torch.cuda.empty_cache()
        mix = [16000 * s - 640 for s in (1, 8, 3, 5, 2, 7, 4, 6)]
        d = batch(dev, mix)
        out["ragged_1_8s"] = measure(models, mel_fn, d, a.steps)
        out["ragged_1_8s"]["solo_vs_batch"] = ragged_deviation(models, mel_fn, d)
        if a.row_exact:
            from megatts2_hierspeechpp_amd import inference_vc as IV
            out["ragged_1_8s_row_exact"] = measure(models, mel_fn, d, a.steps, row_exact=True)
            out["ragged_1_8s_row_exact"]["solo_vs_batch"] = ragged_deviation(models, mel_fn, d, row_exact=True)
            groups = IV.length_groups([s.shape[-1] for s in d["srcs"]])
            parts = [measure(models, mel_fn, batch(dev, [mix[b] for b in g]), a.steps) for g in groups]
            out["ragged_1_8s_length_grouped"] = {"batches": len(groups), "ms_per_mix": sum(p["ms_per_batch"] for p in parts),
                                                 "ms_per_batch": [p["ms_per_batch"] for p in parts]}
            d16 = batch(dev, [n4] * 16)
            out["equal_16x4s_default_vs_row_exact"] = {"default": measure(models, mel_fn, d16, a.steps)["ms_per_batch"],
                                                       "row_exact": measure(models, mel_fn, d16, a.steps, row_exact=True)["ms_per_batch"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
