"""Cost of the int16 stage with the limiter against the plain one: functional.lufs_limit_int16
(passes = 2) and functional.lufs_int16 on 32 rows x 4 s at 48 kHz, each captured in a graph, warmed, and timed as the
median of N replays between device events.  Prints one JSON line; needs the GPU.

    python tools/limiter_bench.py [--rows 32] [--seconds 4] [--rate 48000] [--replays 30] [--passes 2]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from megatts2_hierspeechpp_amd import functional as Fh  # noqa: E402


def signal(rows, n, rate, seed=0):
    """speech-like rows with bursts: a high crest factor, so that the limiter works on every row"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = 0.05 * np.sin(2 * np.pi * 140.0 * t)[None, :] * (0.6 + 0.4 * np.sin(2 * np.pi * 1.7 * t) ** 2)[None, :] \
        + 0.004 * r.standard_normal((rows, n))
    for start in range(rate // 20, n - rate // 100, rate // 3):
        m = rate // 250
        x[:, start:start + m] += 0.8 * r.standard_normal((rows, m)) * np.exp(-4.0 * np.arange(m) / m)[None, :]
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def timed_graph(fn, replays):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--target", type=float, default=-16.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("limiter_bench needs the GPU")
    n = int(a.seconds * a.rate)
    x = torch.from_numpy(signal(a.rows, n, a.rate)).cuda()
    (_, stats), lim_ms, lim_lo, lim_hi = timed_graph(
        lambda: Fh.lufs_limit_int16(x, None, a.rate, a.target, passes=a.passes), a.replays)
    _, old_ms, old_lo, old_hi = timed_graph(lambda: Fh.lufs_int16(x, None, a.rate, a.target), a.replays)
    samples = a.rows * n
    # fp32 passes over the rows: the meter reads twice; every limiter pass reads x and writes z; the true peak reads z;
    # the int16 stage reads z and writes half a pass
    passes_lim = 2 + a.passes * (2 + 2) + 1 + 1.5
    passes_old = 2 + 2 + 0.5                      # meter; peak_int16_gains reads twice (row peak, then the conversion)
    print(json.dumps({
        "rows": a.rows, "samples_per_row": n, "rate": a.rate, "passes": a.passes, "replays": a.replays,
        "lufs_limit_int16_ms": round(lim_ms, 4), "lufs_limit_int16_ms_min_max": [round(lim_lo, 4), round(lim_hi, 4)],
        "lufs_int16_ms": round(old_ms, 4), "lufs_int16_ms_min_max": [round(old_lo, 4), round(old_hi, 4)],
        "bytes_limit": int(passes_lim * 4 * samples), "bytes_plain": int(passes_old * 4 * samples),
        "achieved_lufs_mean": float(stats["achieved_lufs"].mean()), "min_gain_min": float(stats["min_gain"].min()),
        "true_peak_max": float(stats["true_peak"].max()),
    }))


if __name__ == "__main__":
    main()
