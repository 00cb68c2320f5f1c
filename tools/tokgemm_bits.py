#!/usr/bin/env python3
"""One `case plan sha256` line per output buffer of a 1x1 token-GEMM launch of hsp_conv1d_mfma_f32, for the library
HSP_LIB names (default: the built one): every case of tests/tokgemm_ref.py, every token-GEMM case of tests/fold_cases.py
(folded and not), then the PLM / DiT / WN shapes (K 192 / 276 / 1104, M 276 / 384 / 828 / 1104, 16 / 200 / 1 600 / 3 200
columns) and two launches whose mask values are not powers of two (there a contracted `v * mask + y` and a rounded
product differ).  Two libraries compute the same bits when their listings are equal:
    HSP_LIB=/path/to/other/libhsp.so python tools/tokgemm_bits.py > a.txt;  python tools/tokgemm_bits.py > b.txt;  cmp a.txt b.txt"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import conv_ref as R  # noqa: E402
import fold_cases as FC  # noqa: E402
import tokgemm_ref as T  # noqa: E402
from megatts2_hierspeechpp_amd import _lib as L  # noqa: E402

dev = torch.device("cuda:0")


def run(id, a, a2, split, fold=0):
    host = {n: np.ascontiguousarray(a[n], dtype=np.float32) for n in T.POINTERS if a.get(n) is not None}
    if a2 is not None:
        host["y2"] = np.ascontiguousarray(a2["y"], dtype=np.float32)
    d = {n: torch.from_numpy(v).to(dev) for n, v in host.items()}
    d["zeros"] = torch.zeros(64, dtype=torch.float32, device=dev)
    s = T.to_struct(a, a2, split, {n: t.data_ptr() for n, t in d.items()})
    s.fold_cols = fold
    plan = (ctypes.c_int32 * 4)()
    if L.lib().hsp_conv1d_mfma_plan(ctypes.byref(s), plan) != 0:
        print(f"{id} fold{fold} (refused)", flush=True)
        return
    rc = L.lib().hsp_conv1d_mfma_f32(ctypes.byref(s), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (id, rc)
    for n in ("y", "y2")[:2 if a2 is not None else 1]:
        print(f"{id} fold{fold} {n} plan {plan[0]}x{plan[1]}/{plan[2]}", hashlib.sha256(d[n].cpu().numpy().tobytes()).hexdigest(),
              flush=True)


def launch_of(spec):
    a = T.build(spec)
    split = spec.get("split")
    a2 = T.second_half(a, *split, np.random.default_rng(spec["seed"] + 1)) if split else None
    return a, a2, split


for spec in T.SPECS:
    run(spec["id"], *launch_of(spec))
for id in FC.IDS:
    if id.startswith("gemm_"):
        a, a2, split, _ = FC.case(id)
        for fold in (0, 1):               # (T = 50: the register path takes the 1x1 and refuses the field: one "(refused)" line)
            run(id, a, a2, split, fold)
# ---- model shapes: the PLM layer's four GEMMs over `cols` token columns, the WN res_skip / DiT 1x1s over B x 200 frames
model = []
for cols in (16, 200, 1600, 3200):
    g = dict(K=1, B=1, L=cols, bias=True)
    model += [dict(g, id=f"plm_qkv_ln_cols{cols}", Cin=276, Cout=828, ln=True),
              dict(g, id=f"plm_out_proj_res_cols{cols}", Cin=276, Cout=276, res=True),
              dict(g, id=f"plm_ff0_ln_relu_cols{cols}", Cin=276, Cout=1104, ln=True, act=R.ACT_RELU),
              dict(g, id=f"plm_ff3_res_cols{cols}", Cin=1104, Cout=276, res=True)]
for B in (1, 8):
    g = dict(K=1, B=B, L=200, bias=True, Cin=192)
    model += [dict(g, id=f"wn_res_skip_split192_b{B}", Cout=384, res=True, mask_mode=R.MASK_POST, split=(192, R.MASK_NONE, True)),
              dict(g, id=f"dit_proj_res_cscale_b{B}", Cout=192, res=True, cscale=True),
              dict(g, id=f"dit_fc2_gelu_cbias_b{B}", Cout=384, cbias=True, act=R.ACT_GELU_TANH)]
oddmask = [dict(K=1, B=8, L=200, Cin=192, Cout=384, id="bg64_ext_everything_mask_not_pow2", **T.EXT_ALL),
           dict(K=1, B=2, L=33, Cin=38, Cout=36, id="rg32_chain_mask_not_pow2", **T.EXT_ALL)]
for i, spec in enumerate(model + oddmask):
    spec.update(entry="mfma", tile=None, seed=9000 + i)
    a, a2, split = launch_of(spec)
    if spec in oddmask:
        a["mask"] = np.random.default_rng(1).uniform(0.1, 0.9, a["mask"].shape).astype(np.float32)
    for fold in (0, 1) if (a["B"] > 1 and spec not in oddmask[1:]) else (0,):
        run(spec["id"], a, a2, split, fold)
