"""GPU (-m gpu): hsp_mha_f32 and hsp_mha_proj_f32 called through the C ABI with a hand-filled struct, one launch per
case of tests/attn_ref.py, against the float64 statement of the header contract (attn_ref.contract) on the same flat
buffers -- every (kernel, NDB) the decision function of hsp_mha_f32 returns and the four instantiations of the fused
kernel, at the tile edges, layouts, masks and numerical regimes of attn_ref's table.

Every case meets helpers.tol_for(reference) (1e-4 x max(1, peak)) and, element by element, attn_ref.derived_bound (first
order in 2^-24, derived in attn_ref's docstring).  The output lives inside a canary buffer: every element the contract
does not write -- padding columns up to the row pitch, other utterances' columns, beyond o_cs, y at general strides --
must keep its bits.  Every input lives inside a NaN-poisoned buffer (the gaps of a stride, the columns wt_ld - M, the
mask tails, the dense mask's gap, the keys past key_len[b]); the poison stays inside the allocation, and the assertion is
only that the output is finite and within the bars.  tests/test_attn_ref_host.py pins the reference, the plan of every
case id and the admission of every case to the two bars on a CPU.

    python -m pytest tests/test_gpu_attn_contract.py -q -m gpu -s        (-s shows the measured errors)
"""
import ctypes

import numpy as np
import pytest
import torch

import attn_ref as R
import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from megatts2_hierspeechpp_amd import _lib as L
    return L


def _upload(a, device):
    """Device copies of the operand buffers of a case and their base addresses."""
    names = R.MHA_POINTERS if a["entry"] == "mha" else R.PROJ_POINTERS
    dev = {}
    for n in names:
        if a.get(n) is None or (n == "res" and a.get("res_is_y")):
            continue
        dev[n] = torch.from_numpy(np.ascontiguousarray(a[n])).to(device)
    return dev, {n: t.data_ptr() for n, t in dev.items()}


def _launch(lib, a, base):
    fn = lib.lib().hsp_mha_f32 if a["entry"] == "mha" else lib.lib().hsp_mha_proj_f32
    s = R.to_struct(a, base)
    code = fn(ctypes.byref(s), lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0, (a["id"], code)


def _kind(a):
    if a["entry"] == "mha":
        return "%s%d" % (R.KERNEL_NAMES[R.named_kernel(a["id"])[0]], R.named_kernel(a["id"])[1])
    return "MpCfg<%d,%d>%s" % (a["H"], a["D"], "+key_len" if a.get("key_len") is not None else "")


@pytest.mark.parametrize("id", R.IDS)
def test_attn_contract(id, device, lib):
    a, ref, written = R.case(id)
    dev, base = _upload(a, device)
    _launch(lib, a, base)
    name = R.out_name(a)
    got = dev[name].cpu().numpy()
    # what the contract does not write keeps its bits
    before = np.asarray(a[name], np.float32)
    same = got.view(np.uint32)[~written] == before.view(np.uint32)[~written]
    assert same.all(), f"{id}: {int((~same).sum())} elements outside the contract's output were written " \
                       f"(first at buffer offset {int(np.flatnonzero(~written)[np.argmin(same)])})"
    g, r = got.astype(np.float64)[written], ref[written]
    assert np.isfinite(g).all(), f"{id}: {int((~np.isfinite(g)).sum())} non-finite outputs (poison reached a sum)"
    err, tol = np.abs(g - r), H.tol_for(r)
    bound = R.derived_bound(a)[written]
    ratio = float(np.max(err / np.maximum(bound, 1e-300) * (err > 0)))
    print(f"attn_contract {_kind(a)} {id}: max|hip - float64| = {err.max():.3e} (bar {tol:.1e}, ratio {err.max() / tol:.3f}), "
          f"derived-bound ratio {ratio:.3f}")
    assert err.max() <= tol, f"{id}: max|hip - ref| = {err.max():.3e} > {tol:.1e}"
    bad = err > bound
    assert not bad.any(), f"{id}: {int(bad.sum())} elements beyond the derived bound (worst ratio {ratio:.2f})"


# ------------------------------------------------------------------------------------------------ the wrappers
def _tv(dev, a, name, shape, strides):
    return torch.as_strided(dev[name], shape, tuple(int(s) for s in strides), int(a.get(name + "_off", 0)))


def _qkv_views(dev, a):
    B, C, Tq, Tk = a["B"], a["H"] * a["D"], a["Tq"], a["Tk"]
    _, _, qcs, kcs, vcs, _ = R.eff(a)
    return (_tv(dev, a, "q", (B, C, Tq), (a["q_bs"], qcs, 1)), _tv(dev, a, "k", (B, C, Tk), (a["k_bs"], kcs, 1)),
            _tv(dev, a, "v", (B, C, Tk), (a["v_bs"], vcs, 1)))


@pytest.mark.parametrize("id", ["TOK3_d69_tq17_tk255_side1", "WHOLE2_d64_tq17_tk65_side1_factor+irreg", "SLAB4_d128_tq33_tk300_contig",
                                "MSTR4_d128_tq33_tk257_own_factor+irreg", "ROW2_d160_t31_w10_own_factor+irreg+gap",
                                "RSTR2_d160_t257_w3_side4_causal"])
def test_mha_wrapper_fills_the_struct_the_same_way(id, device, lib):
    """functional.mha on views of the same device buffers: the whole output buffer is torch.equal to the raw call's."""
    from megatts2_hierspeechpp_amd import functional as Fh
    a, _, _ = R.case(id)
    dev, base = _upload(a, device)
    _launch(lib, a, base)
    raw = dev["o"].clone()
    dev["o"].fill_(R.SENT)
    B, C, Tq, Tk = a["B"], a["H"] * a["D"], a["Tq"], a["Tk"]
    q, k, v = _qkv_views(dev, a)
    out = _tv(dev, a, "o", (B, C, Tq), (a["o_bs"], R.eff(a)[5], 1))
    w, force = R.eff(a)[:2]
    kw = {}
    if a.get("mask_q") is not None:
        kw.update(mask_q=dev["mask_q"][:B * Tq].view(B, Tq), mask_k=dev["mask_k"][:B * Tk].view(B, Tk))
    if a.get("rel_k") is not None:
        kw.update(rel_k=dev["rel_k"], rel_v=dev["rel_v"], window=w)
    if a.get("mask_dense") is not None:      # the wrapper takes a contiguous [B, Tq, Tk] mask (batch stride Tq Tk)
        kw.update(mask_dense=_tv(dev, a, "mask_dense", (B, Tq, Tk), (a["mask_dense_bs"], Tk, 1)).contiguous())
    Fh.mha(q, k, v, a["H"], a["qk_scale"], out=out, force_stream=force, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dev["o"], raw), id


@pytest.mark.parametrize("id", ["P_tq15_tk5_side4", "D_tq16_tk63_dit", "Pkl_edges_tk70", "D_wide_strides", "P_last_token",
                                "Dkl_inplace_btm_kl"])
def test_mha_proj_wrapper_fills_the_struct_the_same_way(id, device, lib):
    from megatts2_hierspeechpp_amd import functional as Fh
    a, _, _ = R.case(id)
    dev, base = _upload(a, device)
    _launch(lib, a, base)
    raw = dev["y"].clone()
    dev["y"].copy_(torch.from_numpy(a["y"]))
    B, M, Tq = a["B"], a["M"], a["Tq"]
    q, k, v = _qkv_views(dev, a)
    y = _tv(dev, a, "y", (B, M, Tq), (a["y_bs"], a["y_cs"], a["y_ts"]))
    kw = {}
    if a.get("bias") is not None:
        kw["bias"] = dev["bias"][:M]
    if a.get("mask") is not None:
        kw["mask"] = _tv(dev, a, "mask", (B, Tq), (a["mask_bs"], 1))
    if a.get("cscale") is not None:
        kw["cscale"] = _tv(dev, a, "cscale", (B, M), (a["cscale_bs"], 1))
    if a.get("res") is not None:
        kw["res"] = y if a.get("res_is_y") else _tv(dev, a, "res", (B, M, Tq), (a["res_bs"], a["res_cs"], a["res_ts"]))
    if a.get("key_len") is not None:
        kw["key_len"] = dev["key_len"]
    Fh.mha_proj(q, k, v, a["H"], a["qk_scale"], _tv(dev, a, "wt", (M, M), (a["wt_ld"], 1)), out=y, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dev["y"], raw), id
