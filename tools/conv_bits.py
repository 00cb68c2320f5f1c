#!/usr/bin/env python3
"""One `case plan sha256` line per output buffer of a conv-tile launch of hsp_conv1d_mfma_f32, for the library HSP_LIB
names (default: the built one): every MFMA case of tests/conv_ref.py, every case of tests/fold_cases.py (folded and
not), then the Generator's stages at B = 2 -- the direct k = 3 convs of the AMP blocks (d = 1 / 3 / 5 at C / L = 512 /
800, 256 / 4 000, 128 / 16 000, 64 / 32 000, 32 / 32 000), each once on the accumulator-init epilogue with residual,
running sum and post_scale and once behind the fused Activation1d prologue, and each stage's ConvTranspose.  Two
libraries compute the same bits when their listings are equal:
    HSP_LIB=/path/to/other/libhsp.so python tools/conv_bits.py > a.txt;  python tools/conv_bits.py > b.txt;  cmp a.txt b.txt"""
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


def run(id, a, a2=None, split=None, fold=0):
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


for spec in R.SPECS:
    if spec["entry"] == "mfma":
        run(spec["id"], R.build(spec))
for id in FC.IDS:
    a, a2, split, _ = FC.case(id)
    for fold in (0, 1):
        run(id, a, a2, split, fold)
# ---- the Generator at B = 2: channels and length behind each up-sampling stage, and the ConvTranspose that leads there
model = []
for C, Lc in ((512, 800), (256, 4000), (128, 16000), (64, 32000), (32, 32000)):
    for d in (1, 3, 5):
        g = dict(Cin=C, Cout=C, K=3, dil=d, L=Lc, B=2, bias=True, res=True)
        model.append(dict(g, id=f"amp_k3_d{d}_c{C}_l{Lc}_init_res_acc_ps", accumulate=True, post_scale=0.5))
        model.append(dict(g, id=f"amp_k3_d{d}_c{C}_l{Lc}_act1d", prologue=R.PRO_ACT1D))
for Cin, Lc, up, kt in ((1024, 200, 4, 8), (512, 800, 5, 11), (256, 4000, 4, 8), (128, 16000, 2, 4), (64, 32000, 2, 4)):
    model.append(dict(id=f"ups_c{Cin}_l{Lc}_up{up}_k{kt}", rows=R.ROWS_SHUFFLE, Cin=Cin, Cout=Cin // 2, L=Lc, B=2, up=up, kt=kt,
                      tp=(kt - up) // 2, bias=True, prologue=R.PRO_LRELU))
for i, spec in enumerate(model):
    spec.update(entry="mfma", tile=None, seed=11000 + i)
    run(spec["id"], R.build(spec))
