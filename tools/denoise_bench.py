#!/usr/bin/env python3
"""Batched prompt denoiser (denoiser.infer.denoise_batch) against the loop of solo ``denoise`` calls, on
the MP-SENet mirror with synthetic weights: P prompts of mixed 3-10 s.  Three sides, timed wall-clock around a device
synchronise (the solo call reads its norm factor back, so host time is part of what it costs): the solo loop, one eager
``denoise_batch``, and the replay of that batch captured in a hipGraph.  The sides alternate round by round in one
process, after a warm-up of every shape; the medians and the spread (min / max) of each side are printed as one JSON
line.
    python tools/denoise_bench.py [--prompts 8] [--rounds 15] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HPS = types.SimpleNamespace(dense_channel=64, compress_factor=0.3, num_tsconformers=4, beta=2.0, sampling_rate=16000,
                            n_fft=400, hop_size=100, win_size=400)


def prompt(n, seed):
    r = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.2 * np.sin(t * r.uniform(0.03, 0.09)) + 0.1 * np.sin(t * r.uniform(0.2, 0.5)) + 0.05 * r.standard_normal(n)
    return x.astype(np.float32)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.denoiser.generator import MPNet
    from megatts2_hierspeechpp_amd.denoiser.infer import denoise, denoise_batch, mag_pha_istft
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    net = MPNet(HPS)
    net.load_state_dict({k: torch.from_numpy(synth.synth_tensor("den." + k, tuple(v.shape), 7))
                         for k, v in net.state_dict().items()})
    net.finalize(dev)
    seconds = np.linspace(3.0, 10.0, a.prompts) if a.prompts > 1 else np.array([5.0])
    lens = [int(s * 16000) + 37 * i for i, s in enumerate(seconds)]              # off the hop grid
    wavs = [torch.from_numpy(prompt(n, i)).to(dev) for i, n in enumerate(lens)]
    padded = torch.zeros(len(lens), max(lens), device=dev)
    for b, w in enumerate(wavs):
        padded[b, :lens[b]] = w
    solo = lambda: [denoise(w, net, HPS) for w in wavs]
    batch = lambda: denoise_batch(padded, net, HPS, lengths=lens, max_rows=1 << 20)
    with torch.no_grad():
        for _ in range(a.warmup):                                                # every shape of all three sides
            solo()
            batch()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            batch()
        for _ in range(a.warmup):
            g.replay()
        torch.cuda.synchronize()
        sides = {"solo_loop": solo, "batch_eager": batch, "batch_graph": g.replay}
        ms = {k: [] for k in sides}
        for _ in range(a.rounds):                                                # the sides alternate
            for k, fn in sides.items():
                ms[k].append(wall_ms(fn))
        # deviation of the batch from the solo calls, and from the solo NETWORK given the batch's own spectrogram of the
        # row: the first is dominated by the +-pi phase branch of the edge frames' real bins, which differs between DFT
        # summation orders and is an input feature of the network; the second is the packed pass itself
        out_b, n_out, (mag, pha) = denoise_batch(padded, net, HPS, lengths=lens, max_rows=1 << 20, return_spectrogram=True)
        dev_call, dev_net = [], []
        for b, w in enumerate(wavs):
            ref = denoise(w, net, HPS)[0]
            peak = max(float(ref.abs().max()), 1e-30)
            dev_call.append(float((out_b[b, :n_out[b]] - ref).abs().max()) / peak)
            T = 1 + lens[b] // HPS.hop_size
            norm = float(np.sqrt(lens[b] / float((w.double() ** 2).sum())))
            ag, pg, _ = net(mag[b:b + 1, :, :T].contiguous(), pha[b:b + 1, :, :T].contiguous())
            same = mag_pha_istft(ag, pg, HPS.n_fft, HPS.hop_size, HPS.win_size, HPS.compress_factor, scale=1.0 / norm)[0]
            dev_net.append(float((out_b[b, :n_out[b]] - same).abs().max()) / peak)
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out = {"metric": "prompt denoiser: P solo calls vs one packed batch, wall ms around a synchronise, synthetic weights",
           "unit": "ms", "prompts": a.prompts, "seconds": [n / 16000.0 for n in lens], "audio_s": sum(lens) / 16000.0,
           "rounds": a.rounds, "warmup": a.warmup, **{k: stat(v) for k, v in ms.items()},
           "batch_vs_solo_call_max_rel": max(dev_call),
           "batch_vs_solo_network_on_same_spectrogram_max_rel": max(dev_net)}
    out["speedup_eager"] = out["solo_loop"]["median"] / out["batch_eager"]["median"]
    out["speedup_graph"] = out["solo_loop"]["median"] / out["batch_graph"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
