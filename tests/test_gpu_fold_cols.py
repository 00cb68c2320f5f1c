"""GPU (-m gpu): the folded-columns form of hsp_conv1d_mfma_f32 (hsp_conv1d_args.fold_cols) on the cases of
tests/fold_cases.py.  Per case: the launch with the field set is torch.equal -- whole buffers, canaries included -- to the
same launch with the field 0, and both meet the float64 contract of tests/conv_ref.py at helpers.tol_for(reference), the
bar of tests/test_gpu_conv_contract.py; what the contract does not write keeps its bits.  A launch whose kernel does not
implement the form refuses the field with HSP_EINVAL, and hip_layers.Conv1d does not set it there; a kernel that does
implement it keeps the per-utterance tiling where the geometry does not fit (T % 4 != 0, 9 x 8 on the conv tiles).  One model-level case:
SynthesizerTrn.infer at B = 3, T = 40 with the form on and off, padded and row-exact.

    python -m pytest tests/test_gpu_fold_cols.py -q -m gpu -s        (-s shows the measured errors)
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as R
import fold_cases as FC
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib as L
    return L


def _upload(id, device):
    a, a2, _, _ = FC.case(id)
    host = {n: np.ascontiguousarray(a[n], dtype=np.float32) for n in R.POINTERS if a.get(n) is not None}
    if a2 is not None:
        host["y2"] = np.ascontiguousarray(a2["y"], dtype=np.float32)
    dev = {n: torch.from_numpy(v).to(device) for n, v in host.items()}
    dev["zeros"] = torch.zeros(64, dtype=torch.float32, device=device)
    return host, dev, {n: t.data_ptr() for n, t in dev.items()}


def _run(lib, id, dev, base, fold):
    rc = lib.lib().hsp_conv1d_mfma_f32(ctypes.byref(FC.to_struct(id, base, fold)), lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _plan(lib, id, base):
    out = (ctypes.c_int32 * 4)()
    assert lib.lib().hsp_conv1d_mfma_plan(ctypes.byref(FC.to_struct(id, base, 0)), out) == 0, id
    return tuple(out)


@pytest.mark.parametrize("id", FC.IDS)
def test_folded_launch_is_the_unfolded_launch(id, device, lib):
    from megatts2_hierspeechpp_amd import hip_layers as HL
    a, a2, split, refs = FC.case(id)
    host, dev, base = _upload(id, device)
    outs = [n for n, _, _ in refs]
    assert _run(lib, id, dev, base, 0) == 0, id
    plain = {n: dev[n].clone() for n in outs}
    for n in outs:
        dev[n].copy_(torch.from_numpy(host[n]))
    plan = _plan(lib, id, base)
    rc = _run(lib, id, dev, base, 1)
    kind = dict(gated=a["rows"] in (R.ROWS_GATE_WN, R.ROWS_GATE_GLU), halo=(a["K"] - 1) * a["dil"])
    if not HL.fold_cols_kernel(plan, **kind):
        # not a kernel that implements the form: the field is refused, and the layer would not have set it
        assert rc == lib.EINVAL, (id, plan, rc)
        assert not HL.fold_cols_wanted(plan, a["B"], a["ncols"], **kind), (id, plan)
        return
    assert rc == 0, (id, plan, rc)      # (where the geometry does not fit, the launch keeps the per-utterance tiling)
    for n, ref, written in refs:
        assert torch.equal(dev[n], plain[n]), f"{id}: {n} of the folded launch differs from the unfolded launch"
        got = dev[n].cpu().numpy()
        same = got.view(np.uint32)[~written] == host[n].view(np.uint32)[~written]
        assert same.all(), f"{id}: {int((~same).sum())} elements of {n} outside the contract's output were written"
        g, r = got.astype(np.float64)[written], ref[written]
        assert np.isfinite(g).all(), id
        err, tol = float(np.abs(g - r).max()), H.tol_for(r)
        print(f"fold_cols {id} {n} plan {plan[:3]}: max|hip - float64| = {err:.3e} (bar {tol:.1e})")
        assert err <= tol, f"{id}: {n}: max|hip - ref| = {err:.3e} > {tol:.1e}"


def test_fused_layernorm_gemm_folds_bit_identically(device, lib):
    """The block GEMM's fused input LayerNorm (ln_c1) takes its column statistics from the staged tile: the folded tile
    holds other columns, every column's own statistics are unchanged.  conv_ref has no LayerNorm: equality only."""
    id = "gemm_plain_res_b3_t200"
    a = FC.case(id)[0]
    host, dev, base = _upload(id, device)
    c1 = torch.from_numpy(np.asarray(a["w"], np.float32).reshape(a["Cin"], a["w_ld"]).sum(0)).to(device)
    got = []
    for fold in (0, 1):
        dev["y"].copy_(torch.from_numpy(host["y"]))
        s = FC.to_struct(id, base, fold)
        s.ln_c1, s.ln_eps = c1.data_ptr(), 1e-5
        assert lib.lib().hsp_conv1d_mfma_f32(ctypes.byref(s), lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        got.append(dev["y"].clone())
    assert torch.isfinite(got[0]).all() and not torch.equal(got[0], torch.from_numpy(host["y"]).to(device))
    assert torch.equal(got[0], got[1])


def test_other_values_and_other_kernels_refuse_the_field(device, lib):
    id = "gemm_plain_res_b3_t200"
    host, dev, base = _upload(id, device)
    s = FC.to_struct(id, base, 0)
    s.fold_cols = 2
    assert lib.lib().hsp_conv1d_mfma_f32(ctypes.byref(s), lib.stream_ptr()) == lib.EINVAL
    s.fold_cols = 1
    assert lib.lib().hsp_conv1d_direct_f32(ctypes.byref(s), lib.stream_ptr()) == lib.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(dev["y"], torch.from_numpy(host["y"]).to(device))
    s.fold_cols = 0          # (the VALU entry point takes the same struct without the field)
    assert lib.lib().hsp_conv1d_direct_f32(ctypes.byref(s), lib.stream_ptr()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,T", [(3, 200), (3, 50)])
def test_layer_sets_the_field_only_where_it_applies(B, T, device, monkeypatch):
    """hip_layers.Conv1d on a split-row 1x1 (always the block GEMM): T = 200 folds, T = 50 (T % 4 != 0) silently keeps the
    per-utterance tiling; either way the outputs equal those with the form switched off."""
    from megatts2_hierspeechpp_amd import hip_layers as HL
    torch.manual_seed(B * 1000 + T)
    layer = HL.Conv1d(192, 384, 1)
    HL.finalize(layer, device)
    x = torch.randn(B, 192, T, device=device)
    res = torch.randn(B, 192, T, device=device)
    mask = (torch.rand(B, 1, T, device=device) > 0.2).float()
    seen = []
    monkeypatch.setattr(HL, "LAUNCH_HOOK", lambda kind, flops, nbytes, e0, e1, arg:
                        seen.append(int(getattr(arg, "fold_cols", 0))))
    outs = []
    for on in (False, True):
        monkeypatch.setattr(HL, "FOLD_COLS", "1" if on else "0")
        r = layer(x, mask=mask, mask_mode=HL.L.MASK_POST, res=res, split_out=(192, None, False))
        if r is None:      # no fused kernel for the shape (T % 4 != 0): the caller launches the halves separately
            r = (layer(x, mask=mask, mask_mode=HL.L.MASK_POST, res=res, row_range=(0, 192)),
                 layer(x, row_range=(192, 384)))
        torch.cuda.synchronize()
        outs.append(r)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    n = len(seen) // 2
    assert not any(seen[:n])
    assert any(seen[n:]) == (T % 4 == 0), (T, seen)


# ------------------------------------------------------------------------------------------------ the model
def _model(meta, device):
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    mod = H.build_module(meta)
    sd = H.synth_sd(meta)
    pre = meta["prefix"] + "." if meta["prefix"] else ""
    for k, v in mod.state_dict().items():
        if k not in sd:
            sd[k] = torch.from_numpy(synth.synth_tensor(pre + k, tuple(v.shape), meta["seed"]))
    mod.load_state_dict(sd, strict=True)
    finalize(mod, device)
    return mod


def test_synthesizer_infer_is_unchanged_by_the_form(device, monkeypatch):
    """SynthesizerTrn.infer at B = 3, T = 40, the form on against off: torch.equal on both outputs, as a padded batch and
    with row_exact=True over ragged lengths; and the run with the form on did set the field on some launches."""
    from megatts2_hierspeechpp_amd import hip_layers as HL
    meta, a = H.load_fixture("infer_config1")
    mod = _model(meta, device)
    B, T = 3, 40
    r = np.random.default_rng(11)
    d = lambda shape, scale=1.0: torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32)).to(device)
    per = a["f0"].shape[-1] // a["w2v"].shape[2]
    mel, w2v = d((B,) + a["mel"].shape[1:-1] + (T,)), d((B,) + a["w2v"].shape[1:-1] + (T,))
    f0, noise = d((B,) + a["f0"].shape[1:-1] + (per * T,), 0.5), d((B,) + a["noise"].shape[1:-1] + (T,))
    folded = []
    shapes = set()

    def hook(kind, flops, nbytes, e0, e1, arg):
        folded.append(int(getattr(arg, "fold_cols", 0)))
        if hasattr(arg, "fold_cols"):
            shapes.add((arg.B, arg.Cin, arg.K, arg.M, arg.ncols, arg.rows, arg.fold_cols))
    monkeypatch.setattr(HL, "LAUNCH_HOOK", hook)
    for lengths, kw in (([T, T, T], {}), ([28, T, 36], dict(row_exact=True))):
        outs = []
        for on in (False, True):
            monkeypatch.setattr(HL, "FOLD_COLS", "1" if on else "0")
            del folded[:]
            with torch.no_grad():
                o, e_ = mod.infer(mel, w2v, torch.tensor(lengths, device=device), f0, noise=noise, **kw)
            torch.cuda.synchronize()
            outs.append((o.clone(), e_.clone()))
            assert any(folded) == on, (lengths, on, sorted(shapes))
        assert torch.isfinite(outs[0][0]).all()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), lengths
