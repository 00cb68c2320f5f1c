"""CPU: the host side of the conv kernel's activation epilogue (hsp_conv1d_args.act = HSP_ACT_ACT1D): the struct mirror, the
overlapping column tiles, amp_pair's eligibility rule against the pure-Python model of tests/epi_act_cases.py, and what
hsp_conv1d_mfma_plan (validation + selection, never a launch: it reads no memory) makes of the value."""
import ctypes
import itertools

import pytest

import conv_ref as R
import epi_act_cases as EC
import helpers


@pytest.fixture(scope="module")
def L():
    from megatts2_hierspeechpp_amd import _lib
    return _lib


def _plan(L, s):
    out = (ctypes.c_int32 * 4)()
    return L.lib().hsp_conv1d_mfma_plan(ctypes.byref(s), out), tuple(out)


def _struct(L, c, Lc, k, d, nb=EC.B, fused=True):
    base = R.fake_base()
    s = L.Conv1dArgs()
    s.x, s.x_bs, s.x_cs, s.x_ts = base["x"], c * Lc, Lc, 1
    s.B, s.Cin, s.Lin = nb, c, Lc
    s.w, s.K, s.M, s.dil, s.pad, s.stride = base["w"], k, c, d, (k - 1) * d // 2, 1
    s.zeros, s.w_ld = base["zeros"], c
    s.y, s.y_bs, s.y_cs = base["y"], c * Lc, Lc
    s.Cout, s.Lout, s.ncols = c, Lc, Lc
    s.bias, s.scale, s.post_scale = base["bias"], 1.0, 1.0
    if fused:
        s.act, s.alpha_exp, s.beta_inv, s.filt = L.ACT_ACT1D, base["alpha_exp"], base["beta_inv"], base["filt"]
    return s


def test_struct_mirror(L, tmp_path):
    """The form adds no field: the struct is the parent's, the value is the header's HSP_ACT_ACT1D and a default struct
    does not ask for it."""
    assert L.Conv1dArgs().act == L.ACT_NONE != L.ACT_ACT1D
    assert not any(n.startswith("epi_act") for n, _ in L.Conv1dArgs._fields_)
    val, size = helpers.header_values(tmp_path, ["HSP_ACT_ACT1D", "sizeof(hsp_conv1d_args)"])
    assert val == L.ACT_ACT1D and size == ctypes.sizeof(L.Conv1dArgs)


@pytest.mark.parametrize("bn", [512, 256])
@pytest.mark.parametrize("ncols", [4, 8, 12, 236, 240, 244, 484, 492, 496, 500, 1000, 64000])
def test_column_tiles(ncols, bn):
    """hip_layers.epi_act_tiling == the model; the stored ranges partition [0, ncols); every tile's conv window holds the
    8 halo columns of the activation on either side of what it stores, starts on a float4 and is BN wide."""
    from megatts2_hierspeechpp_amd.hip_layers import epi_act_tiling
    tiles = epi_act_tiling(ncols, bn)
    assert tiles == EC.tiling(ncols, bn)
    assert len(tiles) == -(-ncols // (bn - 16))
    pos = 0
    for first_conv, first_out, n_out in tiles:
        assert first_out == pos and n_out > 0 and n_out % 4 == 0 and first_conv % 4 == 0
        assert first_conv == first_out - 8 and first_out + n_out + 8 <= first_conv + bn
        pos += n_out
    assert pos == ncols


def test_eligibility_rule():
    from megatts2_hierspeechpp_amd import hip_layers as HL
    plans = [None, (32, 512, 8, 44032), (64, 256, 8, 40000), (128, 128, 16, 70000), (32, 128, 32, 60000), (64, 64, 64, 81920),
             (64, 64, -2, 73728), (32, 32, -1, 0)]
    saved = HL.EPI_ACT
    try:
        for enabled in (True, False):
            HL.EPI_ACT = enabled
            for (cin, Lc, w1, w2, rows, plan) in itertools.product((32, 64, 128), (64000, 63999, 63998, 8), (False, True),
                                                                   (False, True), (False, True), plans):
                got = HL.epi_act_eligible(cin, cin, Lc, fft_first=w1, fft_second=w2, row_exact=rows, plan=plan)
                assert got == EC.eligible_model(cin, cin, Lc, w1, w2, rows, plan, enabled), (cin, Lc, w1, w2, rows, plan)
    finally:
        HL.EPI_ACT = saved
    assert HL.epi_act_eligible(32, 32, 64000, fft_first=False, fft_second=False, row_exact=False, plan=(32, 512, 8, 1)) == bool(saved)


@pytest.mark.parametrize("c,Lc,k,d", EC.SHAPES, ids=EC.IDS)
def test_plan_of_every_case(c, Lc, k, d, L):
    """The fused launch takes the form's shape at any size; the reference launch of the GPU test (padded batch) takes
    the same shape at the same chunk depth, and the LDS request leaves room for two workgroups per CU."""
    rc, fused = _plan(L, _struct(L, c, Lc, k, d))
    assert rc == 0 and fused[:2] == EC.TILE_OF[c] and fused[2] > 0, (rc, fused)
    assert fused[3] <= 80 * 1024 and fused[3] >= 4 * (16 * fused[1] + 8 * (2 * fused[1] + 16))
    rc, plain = _plan(L, _struct(L, c, Lc, k, d, nb=EC.reference_batch(Lc), fused=False))
    assert rc == 0 and plain[:3] == fused[:3], (plain, fused)
    rc, short = _plan(L, _struct(L, c, Lc, k, d, fused=False))
    assert rc == 0 and short[:2] != EC.TILE_OF[c]            # why the reference batch is padded: two short utterances go elsewhere


def test_refusals_by_plan(L):
    ok = _struct(L, 32, 496, 3, 1)
    assert _plan(L, ok)[0] == 0
    for over in (dict(fold_cols=1), dict(rows=L.ROWS_GATE_WN, gate_half=32, M=64, w_ld=64), dict(rows=L.ROWS_SHUFFLE, up=2),
                 dict(M=128, w_ld=128, Cout=128), dict(filt=None), dict(alpha_exp=None), dict(beta_inv=None), dict(post_scale=0.5),
                 dict(scale=2.0), dict(accumulate=1), dict(res=ok.x), dict(prologue=L.PRO_LRELU), dict(prologue=L.PRO_ACT1D),
                 dict(pad=0), dict(Lin=500), dict(y=ok.y + 4), dict(y_cs=498), dict(cbias=ok.bias), dict(w_bs=4096)):
        s = _struct(L, 32, 496, 3, 1)
        for key, v in over.items():
            setattr(s, key, v)
        assert _plan(L, s)[0] == L.EINVAL, over
        assert L.lib().hsp_conv1d_direct_f32(ctypes.byref(s), None) == L.EINVAL, over   # (refused before any launch)
    odd = _struct(L, 32, 494, 3, 1)
    assert _plan(L, odd)[0] == L.EINVAL
    wide_halo = _struct(L, 32, 496, 11, 7)      # (K - 1) dil = 70 > 61
    assert _plan(L, wide_halo)[0] == L.EINVAL
