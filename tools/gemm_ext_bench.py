#!/usr/bin/env python3
"""Per-launch time of the token-GEMM launches tools/gemm_bench.py cannot express -- the block GEMM's extended epilogue
(masks, cscale, scales, running sum), split rows, folded columns -- and of the register path's full chain, for the
library HSP_LIB names (default: the built one): hsp_conv1d_mfma_f32 through the C ABI on operands of
tests/tokgemm_ref.py, 200 back-to-back launches between two events, median of 7.  Section 3 of
profiles/tokgemm_refactor_ab.txt is this tool, one process per library and round.
    HSP_LIB=/path/to/libhsp.so python tools/gemm_ext_bench.py"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import conv_ref as R  # noqa: E402
import tokgemm_ref as T  # noqa: E402
from megatts2_hierspeechpp_amd import _lib as L  # noqa: E402

dev = torch.device("cuda:0")
EXT = {k: v for k, v in T.EXT_ALL.items() if k != "bias"}
g = dict(K=1, B=32, L=200, bias=True, Cin=192)          # the DiT / WN 1x1s of the 32-utterance step
split = dict(Cout=384, res=True, mask_mode=R.MASK_POST, split=(192, R.MASK_NONE, True))
specs = [dict(g, id="wn_res_skip_split192_b32_fold", **split, fold=1),
         dict(g, id="wn_res_skip_split192_b32", **split),
         dict(g, id="ext_everything_192x384_b32_fold", Cout=384, fold=1, **EXT),
         dict(g, id="ext_everything_192x384_b32", Cout=384, **EXT),
         dict(g, id="ext_scale_gelu_768x192_b32_fold", Cin=768, Cout=192, res=True, scale=0.75, act=R.ACT_GELU_TANH, fold=1),
         dict(K=1, B=1, L=3200, bias=True, id="ext_everything_276x1104_cols3200_128x128", Cin=276, Cout=1104, **EXT),
         dict(K=1, B=1, L=200, bias=True, id="rg_chain_276x276_cols200", Cin=276, Cout=276, **EXT)]
for i, spec in enumerate(specs):
    spec.update(entry="mfma", tile=None, seed=100 + i)
    a = T.build(spec)
    sp = spec.get("split")
    a2 = T.second_half(a, *sp, np.random.default_rng(1)) if sp else None
    host = {n: np.ascontiguousarray(a[n], dtype=np.float32) for n in T.POINTERS if a.get(n) is not None}
    if a2 is not None:
        host["y2"] = np.ascontiguousarray(a2["y"], dtype=np.float32)
    d = {n: torch.from_numpy(v).to(dev) for n, v in host.items()}
    d["zeros"] = torch.zeros(64, dtype=torch.float32, device=dev)
    s = T.to_struct(a, a2, sp, {n: t.data_ptr() for n, t in d.items()})
    s.fold_cols = spec.get("fold", 0)
    plan = (ctypes.c_int32 * 4)()
    assert L.lib().hsp_conv1d_mfma_plan(ctypes.byref(s), plan) == 0, spec["id"]
    fn, stream = L.lib().hsp_conv1d_mfma_f32, L.stream_ptr()
    for _ in range(20):
        assert fn(ctypes.byref(s), stream) == 0
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            fn(ctypes.byref(s), stream)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 200 * 1e3)
    print(f"{spec['id']} plan {plan[0]}x{plan[1]}/{plan[2]}: {sorted(ts)[3]:.2f} us", flush=True)
