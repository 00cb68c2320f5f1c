"""GPU (-m gpu): hsp_conv1d_mfma_f32 and hsp_conv1d_direct_f32 called through the C ABI with a hand-filled
hsp_conv1d_args, one launch per case of tests/conv_ref.py, against the float64 statement of the header contract
(conv_ref.conv_contract) on the same packed operands -- every tile shape and epilogue kind of the MFMA kernel, the three
direct kernels, at the edges listed in conv_ref's table.

Every case meets helpers.tol_for(reference) (1e-4 x max(1, peak)); a case whose epilogue is linear also meets, element
by element, the derived bound 2 (Cin K + 8) 2^-24 conv_contract_abs.  The output lives inside a canary buffer: every
element the contract does not write -- outside [B, Cout, Lout] at the given strides, the padding rows Cout .. M, the
SHUFFLE positions outside [0, Lout) -- must keep its bits.  tests/test_conv_ref_host.py pins the reference and the
claims of the case ids on a CPU.

    python -m pytest tests/test_gpu_conv_contract.py -q -m gpu -s        (-s shows the measured errors)
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as R
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib as L
    return L


def _upload(a, device):
    """Device copies of the operand buffers of a case and their base addresses (16-B aligned: to_struct asserts it)."""
    dev = {n: torch.from_numpy(np.ascontiguousarray(a[n], dtype=np.float32)).to(device) for n in R.POINTERS
           if a.get(n) is not None}
    dev["zeros"] = torch.zeros(64, dtype=torch.float32, device=device)
    return dev, {n: t.data_ptr() for n, t in dev.items()}


def _launch(lib, a, base):
    fn = lib.lib().hsp_conv1d_mfma_f32 if a["entry"] == "mfma" else lib.lib().hsp_conv1d_direct_f32
    s = R.to_struct(a, base)
    code = fn(ctypes.byref(s), lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0, (a["id"], code)


def _kind(a):
    return R.EPI_NAMES[R.epilogue_kind(a)] if a["entry"] == "mfma" else R.direct_kernel(a)


@pytest.mark.parametrize("id", R.IDS)
def test_conv_contract(id, device, lib):
    a, ref, written = R.case(id)
    dev, base = _upload(a, device)
    _launch(lib, a, base)
    got = dev["y"].cpu().numpy()
    # what the contract does not write keeps its bits
    before = np.asarray(a["y"], np.float32)
    same = got.view(np.uint32)[~written] == before.view(np.uint32)[~written]
    assert same.all(), f"{id}: {int((~same).sum())} elements outside the contract's output were written " \
                       f"(first at buffer offset {int(np.flatnonzero(~written)[np.argmin(same)])}, y at {a['y_off']})"
    g, r = got.astype(np.float64)[written], ref[written]
    assert np.isfinite(g).all(), id
    err, tol = float(np.abs(g - r).max()), H.tol_for(r)
    line = f"conv_contract {a['entry']} {_kind(a)} {id}: max|hip - float64| = {err:.3e} (bar {tol:.1e}, ratio {err / tol:.3f})"
    if R.is_linear(a):
        bound = R.derived_bound(a)[written]
        ratio = float(np.max(np.abs(g - r) / np.maximum(bound, 1e-300) * (np.abs(g - r) > 0)))
        line += f", derived-bound ratio {ratio:.3f}"
    print(line)
    assert err <= tol, f"{id}: max|hip - ref| = {err:.3e} > {tol:.1e}"
    if R.is_linear(a):
        bad = np.abs(g - r) > bound
        assert not bad.any(), f"{id}: {int(bad.sum())} elements beyond 2 (Cin K + 8) 2^-24 |contract| (worst ratio {ratio:.2f})"


# ------------------------------------------------------------------------------------------------ the wrappers
def _tv(dev, a, name, shape, strides):
    return torch.as_strided(dev[name], shape, strides, int(a.get(name + "_off", 0)))


def _operands(dev, a):
    B, Cout, Lout = a["B"], a["Cout"], a["Lout"]
    kw = dict(out=_tv(dev, a, "y", (B, Cout, Lout), (a["y_bs"], a["y_cs"], 1)))
    if a.get("res") is not None:
        kw["res"] = _tv(dev, a, "res", (B, Cout, Lout), (a["res_bs"], a["res_cs"], 1))
    if a.get("cbias") is not None:
        kw["cbias"] = _tv(dev, a, "cbias", (B, Cout), (a["cbias_bs"], 1))
    if a.get("cscale") is not None:
        kw["cscale"] = _tv(dev, a, "cscale", (B, Cout), (a["cscale_bs"], 1))
    if a["mask_mode"]:
        kw["mask"] = _tv(dev, a, "mask", (B, Lout), (a["mask_bs"], 1))
    x = _tv(dev, a, "x", (B, a["Cin"], a["Lin"]), (a["x_bs"], a["x_cs"], a["x_ts"]))
    return x, kw


@pytest.mark.parametrize("id", ["S64_VEC_chain_both_mish", "S64_GEN_chain_both_mish", "generic_stride2_dil2_chain",
                                "S64_SHUF_up2_lrelu_clip"])
def test_wrapper_fills_the_struct_the_same_way(id, device, lib):
    """hip_layers.Conv1d.forward / ConvTranspose1d.forward on the operands of a case (the layer packs the un-packed
    weight itself): the whole output buffer is torch.equal to the raw call's."""
    from megatts2_hierspeechpp_amd import hip_layers as HL
    a, _, _ = R.case(id)
    dev, base = _upload(a, device)
    _launch(lib, a, base)
    raw = dev["y"].clone()
    dev["y"].copy_(torch.from_numpy(np.asarray(a["y"], np.float32)))
    x, kw = _operands(dev, a)
    W = torch.from_numpy(np.asarray(a["layer_w"], np.float32))
    if a["rows"] == R.ROWS_SHUFFLE:
        layer = HL.ConvTranspose1d(a["Cin"], a["Cout"], W.shape[2], a["up"], padding=a["shuf_pad"])
        call = lambda: layer(x, lrelu=float(a["slope"]) if a["prologue"] == R.PRO_LRELU else None, **kw)
    else:
        layer = HL.Conv1d(a["Cin"], a["Cout"], a["K"], stride=a["stride"], padding=a["pad"], dilation=a["dil"])
        call = lambda: layer(x, act=a["act"], mask_mode=a["mask_mode"], scale=a["scale"], accumulate=bool(a["accumulate"]),
                             post_scale=a["post_scale"], **kw)
    layer.weight.data.copy_(W)
    layer.bias.data.copy_(torch.from_numpy(np.asarray(a["layer_b"][:a["Cout"]], np.float32)))
    HL.finalize(layer, device)
    out = call()
    torch.cuda.synchronize()
    assert out.data_ptr() == kw["out"].data_ptr()
    assert torch.equal(dev["y"], raw), id
