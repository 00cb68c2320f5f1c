#!/usr/bin/env python3
"""Generate tests/golden/prosody/*.npz: SynthesizerTrn.extract_tc_latent_code of the REFERENCE, run on the CPU.

Run from the repo root:  python tools/make_golden_prosody.py --ref /path/to/reference/checkout

The reference's own class (ttv_v1/t2w2v_transformer.py:887-930) with the synthetic weights (synth seed 7, no prefix:
the keys of the ttv_* fixtures).  Nothing of the reference is copied: a fixture holds inputs and recorded results only.

tc_code_t40 / tc_code_t64 -- B = 1, a mel of 40 / 64 frames at its full length: the only form the reference's front
    part runs in (RangePredictor's .squeeze()).
tc_code_b3 / tc_code_b2 -- ragged rows (64, 41, 9) and (136, 130).  The reference's max-pool is floor mode and its masks
    want a mel length that is a multiple of 8, so every row is ONE reference call on that row alone, its mel padded
    with zeros to the next multiple of 8 and mel_spk_lengths = the row's length; rows are then stacked, zero-padded.
    ``x_frame`` of a row likewise comes from the B = 1 call.

Saved per fixture: ids / tone / language / text lengths / dur, mel_spk + lengths, mrte_mel + lengths, x_frame (rows
zero-padded to the longest) + its frame counts, lr_codes, and ``margin``: for every pooled frame j < ceil(len / 8) the
float64 distance between the best and the second-best code, from the reference's own plm_conv2 output (a forward
hook); NaN elsewhere.  A fixture whose smallest margin is below 1e-3 is refused.
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
from megatts2_hierspeechpp_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "prosody")   # not *.npz of golden/: those are module fixtures
W = 7
MIN_MARGIN = 1e-3


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def one_row(net, captured, r, n, d, mel, tm, mrte):
    """One utterance through the reference: n phones of duration d, prompt mel [80, tm], MRTE mel [80, tr]."""
    ids = r.integers(1, 126, (1, n))
    tone, lang = r.integers(0, 11, (1, n)), np.where(ids < 74, 1, np.where(ids < 113, 2, 0))
    dur = np.full((1, n), d, np.float32)
    tpad = -(-tm // 8) * 8
    mel_p = np.zeros((1, 80, tpad), np.float32)
    mel_p[0, :, :tm] = mel
    captured.clear()
    xf, codes = net.extract_tc_latent_code(t(ids), t(np.array([n])), t(mel_p), t(np.array([tm])), t(tone), t(lang), t(dur),
                                           t(mrte[None]), t(np.array([mrte.shape[1]])))
    q = captured[-1][0].double().numpy()                               # [20, tpad / 8]
    e = net.quantizer.vq.layers[0]._codebook.embed.double().numpy()
    dist = ((q.T[:, None, :] - e[None]) ** 2).sum(-1)
    best = dist.min(-1, keepdims=True)
    margin = np.where(dist > best, dist, np.inf).min(-1) - best[:, 0]
    margin[-(-tm // 8):] = np.nan
    assert codes.shape == (1, tpad) and (codes[0, tm:] == 0).all()
    return dict(ids=ids[0], tone=tone[0], language=lang[0], dur=dur[0], x_frame=xf[0].numpy(),
                lr_codes=codes[0, :tm].numpy(), margin=margin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import tools.make_golden as MG
    MG.install_stubs()
    MG.install_ttv_stubs()
    import logging
    logging.getLogger("matplotlib").setLevel(logging.WARNING)
    from ttv_v1 import t2w2v_transformer as TT
    import utils as ref_utils
    hps = ref_utils.get_hparams_from_file(os.path.join(os.path.dirname(TT.__file__), "config.json"))
    net = TT.SynthesizerTrn(126, 11, 4, 641, 320, 16000, 60, **hps.model)
    MG.load_synth(net, W, "")
    captured = []
    net.plm_conv2.register_forward_hook(lambda m, i, o: captured.append(o.clone()))
    os.makedirs(OUT, exist_ok=True)
    r = np.random.default_rng(79)
    # name -> rows of (phones, duration per phone, prompt mel frames, MRTE mel frames)
    plan = {"tc_code_t40": [(8, 10.0, 40, 52)], "tc_code_t64": [(16, 8.0, 64, 64)],
            "tc_code_b3": [(12, 10.0, 64, 60), (9, 9.0, 41, 48), (4, 5.0, 9, 40)],
            "tc_code_b2": [(20, 13.0, 136, 70), (17, 15.0, 130, 56)]}
    for name, rows in plan.items():
        per = []
        for b, (n, d, tm, tr) in enumerate(rows):
            seed = 900 + 10 * len(name) + b + tm
            mel = synth.synth_inputs(1, tm, seed=seed)["mel"][0]
            mrte = synth.synth_inputs(1, tr, seed=seed + 5000)["mel"][0]
            row = one_row(net, captured, r, n, d, mel, tm, mrte)
            row.update(mel=mel, mrte=mrte)
            per.append(row)
        B = len(per)
        pad = lambda key, shape, dtype: np.zeros((B,) + shape, dtype)  # noqa: E731
        N, Tm, Tr = (max(p[k].shape[-1] for p in per) for k in ("ids", "mel", "mrte"))
        T2 = max(p["x_frame"].shape[1] for p in per)
        arr = dict(ids=pad("ids", (N,), np.int64), tone=pad("tone", (N,), np.int64), language=pad("language", (N,), np.int64),
                   dur=pad("dur", (N,), np.float32), mel_spk=pad("mel", (80, Tm), np.float32),
                   mrte_mel=pad("mrte", (80, Tr), np.float32), x_frame=pad("x_frame", (256, T2), np.float32),
                   lr_codes=pad("lr_codes", (Tm,), np.int64), margin=np.full((B, -(-Tm // 8)), np.nan))
        for b, p in enumerate(per):
            n = p["ids"].shape[0]
            for k in ("ids", "tone", "language", "dur"):
                arr[k][b, :n] = p[k]
            arr["mel_spk"][b, :, :p["mel"].shape[1]] = p["mel"]
            arr["mrte_mel"][b, :, :p["mrte"].shape[1]] = p["mrte"]
            arr["x_frame"][b, :, :p["x_frame"].shape[1]] = p["x_frame"]
            arr["lr_codes"][b, :p["lr_codes"].shape[0]] = p["lr_codes"]
            arr["margin"][b, :p["margin"].shape[0]] = p["margin"]
        arr["lengths"] = np.array([p["ids"].shape[0] for p in per], np.int64)
        arr["mel_spk_lengths"] = np.array([p["mel"].shape[1] for p in per], np.int64)
        arr["mrte_mel_lengths"] = np.array([p["mrte"].shape[1] for p in per], np.int64)
        arr["frames"] = np.array([p["x_frame"].shape[1] for p in per], np.int64)
        lo = float(np.nanmin(arr["margin"]))
        assert lo >= MIN_MARGIN, f"{name}: smallest code margin {lo:g} is below {MIN_MARGIN:g}"
        meta = dict(kind="ttv_tc_code", prefix="", seed=W, min_margin=lo)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), meta=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arr)
        print(f"{name}: lengths {arr['mel_spk_lengths'].tolist()} frames {arr['frames'].tolist()} min margin {lo:.4f} "
              f"codes {arr['lr_codes'][0, ::8][:8].tolist()} ...")


if __name__ == "__main__":
    main()
