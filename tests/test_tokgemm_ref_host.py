"""CPU: pins tests/tokgemm_ref.py, the float64 statement that tests/test_gpu_tokgemm_contract.py holds the two token GEMMs
to -- against torch's float64 layer_norm -> conv1d (two conv1d calls for the split form), the plan of every case
against the kernel its id names, and the refusals of the fields only the token GEMMs take (hsp_conv1d_mfma_plan:
validation + selection, no launch, no memory read)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import tokgemm_ref as T

# every reference of the big 128 x 128 cases is ~0.3 G float64 multiply-adds: the torch comparison takes one of each kind
TORCH_IDS = [i for i in T.IDS if not i.startswith("bg128")] + ["bg128_ln_cin100_partner_exchange", "bg128_ext_cin100_everything"]


@pytest.fixture(scope="module")
def L():
    from megatts2_hierspeechpp_amd import _lib
    return _lib


def _plan(L, s):
    out = (ctypes.c_int32 * 4)()
    return L.lib().hsp_conv1d_mfma_plan(ctypes.byref(s), out), tuple(out)


def _t(a, name, shape, strides):
    return torch.from_numpy(R.view(a, name, shape, strides)[0])


def _torch_half(a, rows):
    """rows [0, rows) of the launch ``a`` by torch in float64 from the un-packed layer parameters."""
    B, Cin, Cout, N = a["B"], a["Cin"], rows, a["ncols"]
    x = _t(a, "x", (B, Cin, N), (a["x_bs"], a["x_cs"], a["x_ts"]))
    w0 = a["w_off"]
    W = torch.from_numpy(np.asarray(a["w"], np.float64).reshape(Cin, a["w_ld"])[:, w0:w0 + Cout].T.copy())[:, :, None]
    bias = _t(a, "bias", (Cout,), (1,))
    if a.get("ln_c1") is not None:
        x = F.layer_norm(x.transpose(1, 2), (Cin,), eps=float(np.float32(a["ln_eps"]))).transpose(1, 2)
    v = F.conv1d(x, W, bias)
    if a.get("cbias") is not None:
        v = v + _t(a, "cbias", (B, Cout), (a["cbias_bs"], 1))[:, :, None]
    v = torch.from_numpy(R.pointwise_act(v.numpy(), a["act"]))
    mk = _t(a, "mask", (B, N), (a["mask_bs"], 1))[:, None, :] if a["mask_mode"] else None
    if a["mask_mode"] & R.MASK_PRE:
        v = v * mk
    if a.get("cscale") is not None:
        v = v * _t(a, "cscale", (B, Cout), (a["cscale_bs"], 1))[:, :, None]
    v = v * float(np.float32(a["scale"]))
    if a.get("res") is not None:
        v = v + _t(a, "res", (B, Cout, N), (a["res_bs"], a["res_cs"], max(1, a.get("res_ts", 1))))
    if a["mask_mode"] & R.MASK_POST:
        v = v * mk
    if a["accumulate"]:
        v = v + _t(a, "y", (B, Cout, N), (a["y_bs"], a["y_cs"], 1))
    return (v * float(np.float32(a["post_scale"]))).numpy()


@pytest.mark.parametrize("id", TORCH_IDS)
def test_statement_is_torch_float64(id):
    a, a2, split, refs = T.case(id)
    halves = [(a, split[0] if split else a["Cout"])] + ([(a2, a2["Cout"])] if split else [])
    for (h, rows), (name, ref, written) in zip(halves, refs):
        want = _torch_half(h, rows)
        _, idx = R.view(h, "y", (h["B"], rows, h["ncols"]), (h["y_bs"], h["y_cs"], 1))
        assert written.sum() == idx.size and written[idx].all(), (id, name)         # exactly [B, rows, ncols] is written
        before = np.asarray(h["y"], np.float64)
        assert np.array_equal(ref[~written], before[~written]), (id, name)
        err = float(np.abs(ref[idx] - want).max())
        # ln_c1 is rounded to fp32 where torch subtracts the exact mean: <= 2^-24 |mean| sum|w| rstd, well under 1e-5 here
        assert err <= (1e-5 if a.get("ln_c1") is not None else 1e-10) * max(1.0, float(np.abs(want).max())), (id, name, err)


@pytest.mark.parametrize("id", [i for i in T.IDS if "_ln_" in i])
def test_layernorm_inputs_stay_away_from_cancellation(id):
    a = T.case(id)[0]
    x, _ = R.view(a, "x", (a["B"], a["Cin"], a["ncols"]), (a["x_bs"], a["x_cs"], a["x_ts"]))
    assert x.std(axis=1).min() >= 0.5 and np.abs(x.mean(axis=1)).max() <= 2.0


@pytest.mark.parametrize("id", T.IDS)
def test_plan_is_the_kernel_the_id_names(id, L):
    a, a2, split, _ = T.case(id)
    rc, plan = _plan(L, T.to_struct(a, a2, split, T.fake_base()))
    assert rc == 0 and plan[:3] == T.plan_of(id), (id, rc, plan)


def test_table_reaches_what_it_claims():
    """The properties of the ids that are arithmetic on Cin: k-steps per wave of the register path (K split 8 / 4 ways,
    groups of 18 k-steps up to Cin = 512 and of 36 beyond) and 48-channel stages of the block GEMM."""
    by = {s["id"]: s for s in T.SPECS}
    per = lambda cin, split: -(-((cin + 1) // 2) // split)
    assert per(32, 8) == 2 and per(276, 8) == 18 and 18 < per(512, 8) <= 36 and 36 < per(1104, 8) <= 72
    assert 7 * per(34, 8) >= (34 + 1) // 2                      # the eighth wave's share is empty
    assert by["rg32_cin33_odd_k_tail"]["Cin"] % 2 == 1 and by["rg32_ln_cin33_odd_k_tail"]["Cin"] % 2 == 1
    assert -(-196 // 48) == 5 and 100 % 48 != 0 and 96 % 48 == 0
    assert {s.get("act", 0) for s in T.SPECS if s["id"].startswith("rg32_act_")} == set(range(8))
    g = by["bg128_cin96_two_stages"]
    assert -(-g["Cout"] // 128) * -(-g["L"] // 128) * g["B"] == 245 and -(-g["Cout"] // 64) * -(-g["L"] // 64) * g["B"] == 819


def _rc(L, id, **fields):
    """Return code of hsp_conv1d_mfma_plan for case ``id`` (itself taken) with some struct fields replaced."""
    a, a2, split, _ = T.case(id)
    s = T.to_struct(a, a2, split, T.fake_base())
    assert _plan(L, s)[0] == 0, id
    for k, v in fields.items():
        setattr(s, k, v)
    return _plan(L, s)[0]


def test_refusals(L):
    """Each refusal stands next to a launch that differs in the named field alone and is taken."""
    no, ok = L.EINVAL, 0
    y2 = dict(y2=T.fake_base()["y2"], y2_bs=1 << 20, y2_cs=256)
    ln, sp, plain, rts = "bg64_ln_cin96", "bg64_split64_mask2_acc2", "bg64_cin96_two_stages", "rg32_res_ts5"
    for id in (ln, "rg32_ln_cin276"):                                     # ln_c1: 1x1 only -- the k = 3 conv without it is taken
        assert _rc(L, id, K=3, pad=1) == no and _rc(L, id, K=3, pad=1, ln_c1=None) == ok
        assert _rc(L, id, ln_eps=0.0) == no and _rc(L, id, ln_eps=-1e-5) == no and _rc(L, id, ln_eps=1e-12) == ok
    # ln_c1 with split_row: either alone is taken
    assert _rc(L, ln, split_row=64, **y2) == no and _rc(L, ln, split_row=64, ln_c1=None, **y2) == ok and _rc(L, ln) == ok
    # either with per-batch weights: the same weights without the field are taken (by a conv tile)
    assert _rc(L, ln, w_bs=96 * 132) == no and _rc(L, ln, w_bs=96 * 132, ln_c1=None) == ok
    assert _rc(L, sp, w_bs=100 * 132) == no and _rc(L, sp, w_bs=100 * 132, split_row=0, y2=None) == ok
    # split_row: a multiple of 64 inside (0, Cout = 132), with a y2
    assert _rc(L, sp, split_row=32) == no and _rc(L, sp, split_row=96) == no and _rc(L, sp, split_row=128) == ok
    assert _rc(L, sp, split_row=192) == no and _rc(L, sp, split_row=-64) == no
    assert _rc(L, sp, y2=None) == no and _rc(L, sp) == ok
    # res_ts > 1: the register path only -- no folded columns (which the block GEMM takes at unit stride), Cin >= 32, one
    # weight matrix
    assert _rc(L, plain, fold_cols=1, res_ts=5) == no and _rc(L, plain, fold_cols=1) == ok and _rc(L, plain, res_ts=5) == ok
    assert _rc(L, rts, fold_cols=1) == no
    assert _rc(L, rts, Cin=28) == no and _rc(L, rts, Cin=32) == ok and _rc(L, rts, Cin=28, res_ts=1) == ok
    assert _rc(L, rts, w_bs=38 * 36) == no and _rc(L, rts, w_bs=38 * 36, res_ts=1) == ok
