#!/usr/bin/env python3
"""Generate tests/golden/sampling/plm_sample_*.npz: fixtures of the sampled PLM decision from the REFERENCE's own sampler.

Run from the repo root:  python tools/make_golden_sampling.py [--ref /path/to/reference/checkout]

``logits_to_probs`` of the reference's ttv_v1/utils_gptsovits.py gives every distribution; the token is the exponential
race of multinomial_sample_one_no_sync with the Philox draws of include/hsp.h (tests/plm_sampling_ref.exp_draws).
Nothing of the reference is copied: a fixture holds inputs, parameters and recorded results only.

plm_sample_cases.npz -- (a) single decisions: random-normal logit rows, previous-token lists, parameter sets, the
    reference's probs and the race token at a stated (seed, j).  Seeds are chosen so that the best race score beats the
    second by more than GAP (relative): float32 rounding cannot flip the token.
plm_sample_loop.npz -- (b) a whole sampled loop: the reference's Megatts2PLM1 modules with the plm_b3_t40 synthetic
    weights (synth seed 7), B = 3, T = 40; every step runs the reference loop body and then logits_to_probs + the race
    in place of argmax.  Per-row seeds are chosen so that no decision of the row is within GAP of flipping (race,
    top-k pivot, top-p boundary); the smallest margins are recorded.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plm_sampling_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sampling")   # not *.npz of golden/: those are module fixtures
V = 1024
GAP = 1e-4


def ref_probs(logits_to_probs, logits, prev, **kw):
    """The reference's probs of one row.  It gets a clone (logits_to_probs scatters into its input) and always a
    tensor (it calls previous_tokens.squeeze() before its None check).  A single previous token squeezes to a 0-d
    index that gather rejects when the penalty is on, so that case passes the token twice: the penalty is applied once
    per distinct token either way (the scatter writes the same value twice)."""
    p = torch.tensor(list(prev), dtype=torch.int64)
    if len(prev) == 1:
        p = p.repeat(2)
    return logits_to_probs(torch.from_numpy(logits).clone(), previous_tokens=p, **kw)


def margins(x, top_k=None, top_p=None, pen=None, **_):
    """Relative distance of the top-k pivot from its neighbour below and of the top-p cut from p (1 = no such cut)."""
    mk = mp = 1.0
    if top_k is not None and top_k < V:
        s = np.sort(x[np.isfinite(x)])[::-1]
        if top_k < len(s):
            mk = abs(float(s[top_k - 1]) - float(s[top_k])) / max(1.0, abs(float(s[top_k - 1])))
    if top_p is not None and top_p < 1.0:
        order = np.argsort(-pen, kind="stable")
        e = np.exp((pen[order] - pen[order[0]]).astype(np.float64))
        cum = np.cumsum(e) / e.sum()
        mp = float(np.abs(cum - top_p).min())
    return mk, mp


def decision_cases(logits_to_probs):
    rng = np.random.default_rng(1234)
    P = lambda **k: dict(dict(temperature=1.0, top_k=None, top_p=None, repetition_penalty=1.0), **k)  # noqa: E731
    rep = [5, 17, 5, 900, 17, 5, 33]
    plan = [
        (P(), []),
        (P(repetition_penalty=1.3), rep),
        (P(repetition_penalty=0.7), [3]),
        (P(repetition_penalty=1.5), []),
        (P(top_p=0.9), [1, 2]),
        (P(top_p=0.02), []),
        (P(top_p=0.99), rep),
        (P(top_k=1, temperature=1.5), []),
        (P(top_k=V), [7]),
        (P(top_k=10), []),
        (P(temperature=1e-6), rep),
        (P(temperature=0.7, top_k=50), []),
        (P(temperature=1.5), [8]),
        (P(temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.2), rep),
        (P(temperature=1.5, top_k=V, top_p=0.97, repetition_penalty=1.1), [42]),
    ]
    out = dict(logits=[], probs=[], prev=[], token=[], seed=[], j=[])
    meta = []
    for c, (pr, prev) in enumerate(plan):
        while True:
            logits = (rng.standard_normal(V) * 2.0).astype(np.float32)
            # the penalised tokens get large logits of both signs, so that the penalty matters
            for t in prev:
                logits[t] = np.float32(rng.choice([-1, 1]) * (3.0 + rng.random()))
            if len(np.unique(logits)) != V:                   # no exact ties
                continue
            probs = ref_probs(logits_to_probs, logits, prev, **pr).numpy()
            mine, x = R.decide_probs(logits, prev, **pr)
            pen, _ = R.decide_probs(logits, prev, repetition_penalty=pr["repetition_penalty"])
            pen = np.log(np.maximum(pen.astype(np.float64), 1e-300))
            mk, mp = margins(x, pen=pen, **pr)
            if mk > 1e-3 and mp > 2e-5:                        # no cut within float32 rounding of flipping
                break
        assert np.abs(mine - probs).max() < 1e-6, (c, np.abs(mine - probs).max())
        j = len(prev) + 1
        seed = (0x1234_5678_9ABC * (c + 1)) & 0x7FFF_FFFF_FFFF_FFFF
        while True:
            tok, gap = R.race(np.where(probs > 0, np.log(np.maximum(probs.astype(np.float64), 1e-300)), -np.inf),
                              seed, j)
            if gap > GAP:
                break
            seed += 1
        assert tok == R.race(x, seed, j)[0]
        out["logits"].append(logits)
        out["probs"].append(probs)
        out["prev"].append(np.array(prev + [-1] * (8 - len(prev)), np.int64))
        out["token"].append(tok)
        out["seed"].append(seed)
        out["j"].append(j)
        meta.append(dict(pr, n_prev=len(prev), gap=gap))
        print(f"case {c:2d} {pr} prev {len(prev)} -> token {tok} (gap {gap:.2e}, kept {(probs > 0).sum()})")
    arrays = {k: np.array(v) for k, v in out.items()}
    np.savez_compressed(os.path.join(OUT, "plm_sample_cases.npz"), meta=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)


LOOP = dict(temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.1)


def loop_fixture(logits_to_probs):
    import tools.make_golden as MG
    MG.install_stubs()
    MG.install_ttv_stubs()
    from ttv_v1 import t2w2v_transformer as TT
    mod = TT.Megatts2PLM1()
    shapes, _ = MG.load_synth(mod, 7, "plm.")
    B, T = 3, 40
    tc = (np.random.default_rng(440).standard_normal((B, 256, T))).astype(np.float32)
    codes = np.zeros((B, T), np.int64)
    gaps = np.zeros((B, T))
    seeds = []
    with torch.no_grad():
        for b in range(B):
            seed = 1000 + 7919 * b
            while True:
                ok, row, g = run_row(mod, logits_to_probs, torch.from_numpy(tc[b:b + 1]), seed, T)
                if ok:
                    break
                seed += 1
            seeds.append(seed)
            codes[b], gaps[b] = row, g
            print(f"loop row {b}: seed {seed}, min race gap {g.min():.2e}, codes {row[:12].tolist()} ...")
    np.savez_compressed(os.path.join(OUT, "plm_sample_loop.npz"), tc=tc, seeds=np.array(seeds, np.int64), codes=codes,
                        gaps=gaps, meta=np.frombuffer(json.dumps(dict(params=LOOP, weight_seed=7, prefix="plm.", shapes=shapes,
                                                                      min_gap=float(gaps.min()))).encode(), np.uint8))


def run_row(mod, logits_to_probs, tc, seed, T):
    """The reference loop (ttv_v1/t2w2v_transformer.py Megatts2PLM1.infer) at B = 1 with the sampled choice; returns
    (all margins above GAP, codes, race gaps)."""
    tcl = tc.transpose(-1, -2)
    p_code = torch.tensor([[1024]], dtype=torch.int64)
    gaps = []
    for t in range(T):
        pc_emb = mod.pc_embedding(p_code)
        x_emb = torch.cat([tcl[:, 0:t + 1, :], pc_emb], dim=-1)
        x = mod.plm(mod.pos_emb(x_emb))
        logits = mod.predict_layer(x)[:, -1:, :][0, 0].numpy()
        prev = p_code[0, 1:].tolist()
        probs = ref_probs(logits_to_probs, logits, prev, **LOOP).numpy()
        _, xs = R.decide_probs(logits, prev, **LOOP)
        pen, _ = R.decide_probs(logits, prev, repetition_penalty=LOOP["repetition_penalty"])
        mk, mp = margins(xs, pen=np.log(np.maximum(pen.astype(np.float64), 1e-300)), **LOOP)
        tok, gap = R.race(np.where(probs > 0, np.log(np.maximum(probs.astype(np.float64), 1e-300)), -np.inf), seed,
                          t + 1)
        if gap <= GAP or mk <= GAP or mp <= 2e-5 or tok != R.race(xs, seed, t + 1)[0]:
            print(f"  seed {seed} rejected at step {t}: race gap {gap:.1e}, top-k margin {mk:.1e}, top-p margin {mp:.1e}")
            return False, None, None
        gaps.append(gap)
        p_code = torch.cat([p_code, torch.tensor([[tok]])], dim=1)
    return True, p_code[0, 1:].numpy(), np.array(gaps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    torch.manual_seed(0)
    from ttv_v1.utils_gptsovits import logits_to_probs
    decision_cases(logits_to_probs)
    loop_fixture(logits_to_probs)


if __name__ == "__main__":
    main()
