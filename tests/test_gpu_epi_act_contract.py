"""GPU (-m gpu): the activation epilogue of hsp_conv1d_mfma_f32 (hsp_conv1d_args.act = HSP_ACT_ACT1D, include/hsp.h) through
the C ABI, on the cases of tests/epi_act_cases.py: the fused launch against the plain conv launch followed by
hsp_act1d_snakebeta_f32 on the same operands, bit for bit.

Equality is expected: the fused kernel starts its accumulators at the bias and walks K like the plain launch on the same
tile shape, and the activation is the stand-alone kernel's arithmetic (csrc/hsp_act1d_arith.h).  The reference conv launch
is epi_act_cases.reference_batch(L) utterances -- the case's two and zero ones -- so that the dispatcher gives it the tile
shape the form lives on (asserted through hsp_conv1d_mfma_plan: same BM, BN and chunk depth as the fused launch); at two
short utterances it would take a short-sequence shape, whose chunk order is another.  The comparison is over whole
buffers: the output sits between 64 sentinel floats on either side, which must keep their bits.  No shape is off the
bit-equal list.

    python -m pytest tests/test_gpu_epi_act_contract.py -q -m gpu
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as R
import epi_act_cases as EC

pytestmark = pytest.mark.gpu


def _dev(a, device):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    assert t.data_ptr() % 16 == 0
    return t


def _filt(device):
    import act1d_ref
    return _dev(act1d_ref.filt24(), device)


def _zeros(device):
    from megatts2_hierspeechpp_amd import hip_layers
    return hip_layers._zeros(device)


def _args(L, x, w, y_ptr, bias, cout, M, k, d, zeros, nb=None):
    """A plain "same" conv of x [nb, cin, Lc] with packed weights w[k][cin][M] into a contiguous [nb, cout, Lc] at y_ptr."""
    nb_, cin, Lc = x.shape
    nb = nb_ if nb is None else nb
    s = L.Conv1dArgs()
    s.x, s.x_bs, s.x_cs, s.x_ts = x.data_ptr(), cin * Lc, Lc, 1
    s.B, s.Cin, s.Lin = nb, cin, Lc
    s.w, s.K, s.M, s.dil, s.pad, s.stride = w.data_ptr(), k, M, d, (k - 1) * d // 2, 1
    s.zeros, s.w_ld = zeros.data_ptr(), M
    s.y, s.y_bs, s.y_cs = y_ptr, cout * Lc, Lc
    s.Cout, s.Lout, s.ncols = cout, Lc, Lc
    s.bias = bias.data_ptr() if bias is not None else None
    s.scale, s.post_scale = 1.0, 1.0
    return s


def _plan(L, s):
    out = (ctypes.c_int32 * 4)()
    return L.lib().hsp_conv1d_mfma_plan(ctypes.byref(s), out), tuple(out)


def _guarded(n, device):
    return torch.full((n + 2 * EC.GUARD,), EC.SENT, dtype=torch.float32, device=device)


@pytest.mark.parametrize("c,Lc,k,d", EC.SHAPES, ids=EC.IDS)
def test_fused_is_conv_then_activation(c, Lc, k, d, device):
    from megatts2_hierspeechpp_amd import _lib as L
    x_h, W, bias_h, ea_h, bi_h = EC.operands(c, Lc, k, d)
    nb = EC.reference_batch(Lc)
    xr_h = np.zeros((nb, c, Lc), np.float32)
    xr_h[:EC.B] = x_h
    x, xr, w, bias = _dev(x_h, device), _dev(xr_h, device), _dev(R.pack_plain(W, c), device), _dev(bias_h, device)
    ea, bi, filt, zeros = _dev(ea_h, device), _dev(bi_h, device), _filt(device), _zeros(device)
    n = EC.B * c * Lc
    st = L.stream_ptr()

    # the two launches: conv on the padded batch, the activation of its first two utterances into a guarded buffer
    xt = torch.empty(nb, c, Lc, dtype=torch.float32, device=device)
    plain = _args(L, xr, w, xt.data_ptr(), bias, c, c, k, d, zeros)
    rc_p, plan_p = _plan(L, plain)
    assert rc_p == 0 and plan_p[:2] == EC.TILE_OF[c] and plan_p[2] > 0, plan_p
    assert L.lib().hsp_conv1d_mfma_f32(ctypes.byref(plain), st) == 0
    want = _guarded(n, device)
    assert L.lib().hsp_act1d_snakebeta_f32(xt.data_ptr(), want.data_ptr() + 4 * EC.GUARD, EC.B, c, Lc, ea.data_ptr(),
                                           bi.data_ptr(), filt.data_ptr(), st) == 0

    # the fused launch on the case's own two utterances
    got = _guarded(n, device)
    fused = _args(L, x, w, got.data_ptr() + 4 * EC.GUARD, bias, c, c, k, d, zeros)
    fused.act, fused.alpha_exp, fused.beta_inv, fused.filt = L.ACT_ACT1D, ea.data_ptr(), bi.data_ptr(), filt.data_ptr()
    rc_f, plan_f = _plan(L, fused)
    assert rc_f == 0 and plan_f[:3] == plan_p[:3], (plan_f, plan_p)      # same tile, same chunk depth: same order of K
    assert plan_f[3] <= 80 * 1024, plan_f                                 # two workgroups per CU
    assert L.lib().hsp_conv1d_mfma_f32(ctypes.byref(fused), st) == 0
    torch.cuda.synchronize()

    assert torch.isfinite(want[EC.GUARD:EC.GUARD + n]).all()
    same = got.view(torch.int32) == want.view(torch.int32)
    if not bool(same.all()):
        bad = torch.nonzero(~same).flatten()
        first = int(bad[0]) - EC.GUARD
        diff = float((got - want).abs().max())
        raise AssertionError(f"{int(bad.numel())} of {n} floats differ (first at flat index {first} = row "
                             f"{first // Lc}, column {first % Lc}; max |diff| {diff:.3e}; guards included)")
    assert torch.equal(x.cpu(), torch.from_numpy(x_h))                    # the input keeps its bits


def test_refusals_write_nothing(device):
    """HSP_EINVAL for act = HSP_ACT_ACT1D wherever the form is not implemented: 128 channels, gated rows, ConvTranspose rows,
    folded columns, a residual, a row length that is no multiple of 4, a partial set of the activation's operands, and the VALU entry point."""
    from megatts2_hierspeechpp_amd import _lib as L
    c, Lc, k, d = 32, 496, 3, 1
    x_h, W, bias_h, ea_h, bi_h = EC.operands(c, Lc, k, d)
    x, w, bias = _dev(x_h, device), _dev(R.pack_plain(W, c), device), _dev(bias_h, device)
    ea, bi, filt, zeros = _dev(ea_h, device), _dev(bi_h, device), _filt(device), _zeros(device)
    # operands large enough for every variant below (M up to 128, 2 x as many output columns)
    wbig = torch.zeros(k * c * 128, dtype=torch.float32, device=device)
    big = torch.zeros(128, dtype=torch.float32, device=device)
    y = _guarded(EC.B * 128 * 2 * Lc, device)
    yp = y.data_ptr() + 4 * EC.GUARD

    def base(**over):
        s = _args(L, x, w, yp, bias, c, c, k, d, zeros)
        s.act, s.alpha_exp, s.beta_inv, s.filt = L.ACT_ACT1D, ea.data_ptr(), bi.data_ptr(), filt.data_ptr()
        for key, v in over.items():
            setattr(s, key, v)
        return s

    wide = dict(w=wbig.data_ptr(), M=128, w_ld=128, Cout=128, y_bs=128 * Lc, bias=big.data_ptr(),
                alpha_exp=big.data_ptr(), beta_inv=big.data_ptr())
    variants = {
        "Cout = 128": base(**wide),
        "gated rows": base(w=wbig.data_ptr(), M=64, w_ld=64, rows=L.ROWS_GATE_WN, gate_half=32, bias=big.data_ptr()),
        "ConvTranspose rows": base(w=wbig.data_ptr(), M=64, w_ld=64, rows=L.ROWS_SHUFFLE, up=2, shuf_pad=0, Lout=2 * Lc,
                                   y_cs=2 * Lc, y_bs=c * 2 * Lc, bias=big.data_ptr()),
        "fold_cols": base(fold_cols=1),
        "residual": base(res=x.data_ptr(), res_bs=c * Lc, res_cs=Lc),
        "alpha only": base(beta_inv=None, filt=None),
        "filt only": base(alpha_exp=None, beta_inv=None),
        "leaky-ReLU prologue": base(prologue=L.PRO_LRELU, slope=0.1),
        "post_scale": base(post_scale=0.5),
    }
    st = L.stream_ptr()
    for name, s in variants.items():
        assert L.lib().hsp_conv1d_mfma_f32(ctypes.byref(s), st) == L.EINVAL, name
        assert _plan(L, s)[0] == L.EINVAL, name
    assert L.lib().hsp_conv1d_direct_f32(ctypes.byref(base()), st) == L.EINVAL
    assert L.lib().hsp_conv1d_direct_f32(ctypes.byref(base(alpha_exp=None, beta_inv=None)), st) == L.EINVAL
    # L % 4 != 0 (operands of their own: the row stride changes)
    odd = _args(L, x[:, :, :494].contiguous(), w, yp, bias, c, c, k, d, zeros)
    odd.act, odd.alpha_exp, odd.beta_inv, odd.filt = L.ACT_ACT1D, ea.data_ptr(), bi.data_ptr(), filt.data_ptr()
    assert L.lib().hsp_conv1d_mfma_f32(ctypes.byref(odd), st) == L.EINVAL
    # the same struct without the value is a launch the library takes (so the refusals above are the value's)
    ok = base(act=L.ACT_NONE)
    assert _plan(L, ok)[0] == 0
    torch.cuda.synchronize()
    assert bool((y == EC.SENT).all()), "a refused launch wrote to y"
