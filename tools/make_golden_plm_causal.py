#!/usr/bin/env python3
"""Generate tests/golden/causal/plm_causal_b2_t24.npz by running the REFERENCE's Megatts2PLM1.forward (CPU).

    python tools/make_golden_plm_causal.py [--ref /path/to/reference/checkout]

``forward(tc_latent, p_codes, lens)`` (ttv_v1/t2w2v_transformer.py:679-700) is the model's training pass: the codes
shifted right behind the go token, the encoder under ``causal=True`` with ``lens``, the predict layer.  Its logits are
what Megatts2PLM1.score mirrors and what a K/V-cached decode reproduces step by step.  The reference is imported from
its read-only checkout behind the stubs of tools/make_golden.py (monotonic_align, torchmetrics: built or imported by
the module, never used by the logits); nothing of it is copied: the fixture holds a JSON ``meta`` record (weight seed,
the (key, shape) list of the module's state dict), the inputs and the logits.  Weights are regenerated on the consumer
side from ``megatts2_hierspeechpp_amd.synth`` with the same seed.  The loss and the accuracy forward also returns are
training-time values and are not stored (the accuracy metric is a stub, so forward's last line is caught).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEED_W, SEED_IN, LENS = 7, 324, [24, 17]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("HSP_REFERENCE", "/root/reference"))
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import make_golden as MG
    MG.install_stubs()
    MG.install_ttv_stubs()
    import logging
    logging.getLogger("matplotlib").setLevel(logging.WARNING)
    from ttv_v1 import t2w2v_transformer as TT

    mod = TT.Megatts2PLM1()
    shapes, _ = MG.load_synth(mod, SEED_W, "plm.")
    # forward ends with the accuracy metric (a stub here): give it a callable whose result has .item()
    mod.ar_accuracy_metric.forward = lambda *a, **k: torch.zeros(())
    B, T = len(LENS), max(LENS)
    r = np.random.default_rng(SEED_IN)
    tc = r.standard_normal((B, 256, T)).astype(np.float32)
    p_codes = r.integers(0, 1024, (B, T)).astype(np.int64)
    for b, n in enumerate(LENS):
        p_codes[b, n:] = 1025                    # the reference's padding id (ignore_index = vq_bins + 1)
    lens = np.array(LENS, np.int64)
    with torch.no_grad():
        logits = mod(torch.from_numpy(tc), torch.from_numpy(p_codes), torch.from_numpy(lens))[0]   # [B, vq_bins, T]
    logits = logits.transpose(1, 2).contiguous().numpy().astype(np.float32)                        # [B, T, vq_bins]
    meta = dict(kind="plm_causal", prefix="plm", seed=SEED_W, shapes=shapes)
    out = os.path.join(ROOT, "tests", "golden", "causal", "plm_causal_b2_t24.npz")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, tc=tc, p_codes=p_codes, lens=lens, logits=logits,
                        meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
    print(out, os.path.getsize(out), "bytes; logits", logits.shape, "max|logits|", float(np.abs(logits).max()))


if __name__ == "__main__":
    main()
