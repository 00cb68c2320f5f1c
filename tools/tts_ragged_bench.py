#!/usr/bin/env python3
"""A page of 8 different lines, three ways, on one MI355X: eight `tts_from_prompt` calls (the loop a user writes
today), `tts_batch(row_exact=True)` and `tts_batch(row_exact=False)`.  Lines of 10, 20, ... 80 phones with durations
pinned to 10 frames / phone (50, 100, ... 400 vocoder frames: 1 to 8 s of audio, 36 s in all), one shared prompt of
48000 samples, causal greedy prosody LM, 16 kHz, synthetic weights, explicit noise.

    python tools/tts_ragged_bench.py [--rounds 5] [--warmup 1] [--out profiles/tts_ragged.json]

Per round the three ways run once each in alternating order; a timing is a host clock around the call, closed by a
device synchronise.  The figures are medians over the rounds.  The per-stage split of the two batched ways comes from
further rounds of their own with a synchronise at every stage boundary (inference_plm.STAGE_HOOK), which is why its
parts add up to a little more than the whole.  Prints one JSON line and writes it to --out when given."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from megatts2_hierspeechpp_amd import inference_plm as IP, synth  # noqa: E402
from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed  # noqa: E402
from tools import bench_extra  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "this is a GPU measurement: no device, no number"
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)

PHONES = [10 * (k + 1) for k in range(8)]
FRAMES = [5 * n for n in PHONES]
models = IP.TtsModels(bench_extra.VOC_CFG, bench_extra.TTV_CFG)
models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 0)) for k, v in models.state_dict().items()})
models.finalize(dev)
mel_fn = MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                             n_mels=80, window_fn=torch.hann_window).finalize(dev)
r = np.random.default_rng(0)
lines = []
for n in PHONES:
    ids = torch.from_numpy(r.integers(12, 113, n)).to(dev)
    lines.append((ids, torch.from_numpy(r.integers(0, 11, n)).to(dev), torch.where(ids < 74, 1, 2)))
t = np.arange(48000) / 16000.0
prompt = torch.from_numpy((0.3 * np.sin(2 * np.pi * 140 * t) + 0.05 * r.standard_normal(48000)).astype(np.float32)[None]).to(dev)
dur = [torch.full((n,), 10.0, device=dev) for n in PHONES]
noise = torch.from_numpy(r.standard_normal((8, 192, max(FRAMES))).astype(np.float32)).to(dev)
solo_noise = [noise[b:b + 1, :, :FRAMES[b]].contiguous() for b in range(8)]


def loop():
    return [IP.tts_from_prompt(models, mel_fn, *(x.reshape(1, -1) for x in lines[b]), prompt, dur=dur[b].reshape(1, -1),
                               noise=solo_noise[b], plm_causal=True) for b in range(8)]


def batch(row_exact):
    return IP.tts_batch(models, mel_fn, lines, prompt, dur=dur, noise=noise, plm_causal=True, row_exact=row_exact)


WAYS = {"loop_of_8_one_line_calls": loop, "tts_batch_row_exact": lambda: batch(True),
        "tts_batch_padded": lambda: batch(False)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


for _ in range(max(1, args.warmup)):
    outs = {name: timed(fn)[1] for name, fn in WAYS.items()}
# what the batches compute against the loop: the largest int16 difference of any row (row-exact: 5 LSB is the contract)
lsb = {name: max((outs[name][0][b, :320 * FRAMES[b]].to(torch.int32) - solo.to(torch.int32)).abs().max().item()
                 for b, solo in enumerate(outs["loop_of_8_one_line_calls"]))
       for name in ("tts_batch_row_exact", "tts_batch_padded")}
ms = {name: [] for name in WAYS}
names = list(WAYS)
for rnd in range(args.rounds):
    for name in (names if rnd % 2 == 0 else names[::-1]):
        ms[name].append(timed(WAYS[name])[0])

stage_ms = {}
for name in ("tts_batch_row_exact", "tts_batch_padded"):
    parts = {}
    marks = []

    def hook(stage):
        torch.cuda.synchronize()
        marks.append((stage, time.perf_counter()))

    IP.STAGE_HOOK = hook
    for _ in range(args.rounds):
        del marks[:]
        WAYS[name]()
        for (s0, t0), (_, t1) in zip(marks, marks[1:]):
            parts.setdefault(s0, []).append((t1 - t0) * 1e3)
    IP.STAGE_HOOK = None
    stage_ms[name] = {k: round(med(v), 3) for k, v in parts.items()}

audio_s = sum(FRAMES) * 320 / 16000.0
res = {"workload": "8 lines of 10..80 phones (50..400 frames, 36 s of audio), one prompt, causal greedy PLM, 16 kHz",
       "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
       "ms": {k: round(med(v), 3) for k, v in ms.items()},
       "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
       "audio_seconds_per_second": {k: round(audio_s / (med(v) / 1e3), 1) for k, v in ms.items()},
       "stage_ms": stage_ms, "max_int16_diff_vs_loop": lsb}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
