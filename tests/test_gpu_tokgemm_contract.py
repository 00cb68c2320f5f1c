"""GPU (-m gpu): the two 1x1 token GEMMs behind hsp_conv1d_mfma_f32 -- register path (csrc/hsp_rgemm.hip) and block GEMM
(csrc/hsp_bgemm.hip) -- called through the C ABI with a hand-filled hsp_conv1d_args, one launch per case of
tests/tokgemm_ref.py, against the float64 statement of the header contract on the same packed operands: both K-split
forms and group depths of the register path, its odd-K tail and strided x / res, the block GEMM's two tile shapes, short
last stage, slot reuse, LayerNorm partner exchange, plain and extended epilogue and the second output.

Every case meets helpers.tol_for(reference) (1e-4 x max(1, peak)); a linear case without LayerNorm also meets, element by
element, conv_ref.derived_bound = 2 (Cin + 8) 2^-24 |contract|.  y and y2 live inside canary buffers: every element the
contract does not write keeps its bits; every written one is finite.  tests/test_tokgemm_ref_host.py pins the reference
and the plan of every case on a CPU.

    python -m pytest tests/test_gpu_tokgemm_contract.py -q -m gpu -s        (-s shows the measured errors)
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as R
import helpers as H
import tokgemm_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib as L
    return L


def upload(a, a2, device):
    """Host and device copies of the operand buffers of a case and the device base addresses."""
    host = {n: np.ascontiguousarray(a[n], dtype=np.float32) for n in T.POINTERS if a.get(n) is not None}
    if a2 is not None:
        host["y2"] = np.ascontiguousarray(a2["y"], dtype=np.float32)
    dev = {n: torch.from_numpy(v).to(device) for n, v in host.items()}
    dev["zeros"] = torch.zeros(64, dtype=torch.float32, device=device)
    return host, dev, {n: t.data_ptr() for n, t in dev.items()}


@pytest.mark.parametrize("id", T.IDS)
def test_tokgemm_contract(id, device, lib):
    a, a2, split, refs = T.case(id)
    host, dev, base = upload(a, a2, device)
    code = lib.lib().hsp_conv1d_mfma_f32(ctypes.byref(T.to_struct(a, a2, split, base)), lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0, (id, code)
    linear = R.is_linear(a) and a.get("ln_c1") is None
    for (name, ref, written), h in zip(refs, (dict(a, M=split[0], Cout=split[0]) if split else a, a2)):
        got = dev[name].cpu().numpy()
        same = got.view(np.uint32)[~written] == host[name].view(np.uint32)[~written]
        assert same.all(), f"{id}: {int((~same).sum())} elements of {name} outside the contract's output were written"
        g, r = got.astype(np.float64)[written], ref[written]
        assert np.isfinite(g).all(), (id, name)
        err, tol = float(np.abs(g - r).max()), H.tol_for(r)
        line = f"tokgemm_contract {id} {name}: max|hip - float64| = {err:.3e} (bar {tol:.1e}, ratio {err / tol:.3f})"
        if linear:
            bound = R.derived_bound(h)[written]
            ratio = float(np.max(np.abs(g - r) / np.maximum(bound, 1e-300) * (np.abs(g - r) > 0)))
            line += f", derived-bound ratio {ratio:.3f}"
        print(line)
        assert err <= tol, f"{id}: {name}: max|hip - ref| = {err:.3e} > {tol:.1e}"
        if linear:
            bad = np.abs(g - r) > bound
            assert not bad.any(), f"{id}: {name}: {int(bad.sum())} elements beyond 2 (Cin + 8) 2^-24 |contract| (worst ratio {ratio:.2f})"
