#!/usr/bin/env python3
"""One `case sha256` line per output buffer of the three transform entry points (hsp_dftseg_fwd_f32, hsp_dftseg_inv_f32,
hsp_dftseg_pair_f32) for the library HSP_LIB names (default: the built one): every case of tests/dftseg_ref.py, then the
Generator's stage shapes at B = 2 (C / L = 512 / 800, 256 / 4 000, 128 / 16 000, 64 / 32 000; k = 7, 11; d = 1, 3, 5).
Two libraries compute the same bits when their listings are equal:
    HSP_LIB=/path/to/other/libhsp.so python tools/dftseg_bits.py > a.txt;  python tools/dftseg_bits.py > b.txt;  cmp a.txt b.txt"""
import ctypes
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import dftseg_ref as R  # noqa: E402
from megatts2_hierspeechpp_amd import _lib as L  # noqa: E402

dev = torch.device("cuda:0")
specs = list(R.SPECS)
for n, (C_, L_) in enumerate(((512, 800), (256, 4000), (128, 16000), (64, 32000))):
    for k in (7, 11):
        for d in (1, 3, 5):
            g = dict(B=2, C=C_, L=L_, k=k, d=d, seed=9000 + 100 * n + 10 * k + d)
            specs += [dict(g, id=f"gen_fwd_act_C{C_}_L{L_}_k{k}_d{d}", kind="fwd", act=True, prod3=1),
                      dict(g, id=f"gen_inv_res_C{C_}_L{L_}_k{k}_d{d}", kind="inv", res=True, bias=True),
                      dict(g, id=f"gen_pair_C{C_}_L{L_}_k{k}_d{d}", kind="pair", bias=True, prod3=1)]
for s in specs:
    ai, af = R.build(s)
    if s["kind"] == "pair":
        si, sf = R.to_struct(ai, R.fake_base()), R.to_struct(af, R.fake_base())
        if not L.lib().hsp_dftseg_pair_supported(ctypes.byref(si), ctypes.byref(sf)):
            print(f"{s['id']} (no pair launch at this geometry)", flush=True)
            continue
    print(s["id"], hashlib.sha256(R.run_case(ai, af, dev).tobytes()).hexdigest(), flush=True)
