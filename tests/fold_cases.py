"""Case table of the folded-columns form (hsp_conv1d_args.fold_cols) shared by tests/test_fold_cols_host.py (CPU) and
tests/test_gpu_fold_cols.py (GPU): operands and float64 references come from tests/conv_ref.py (batch and channel
strides wider than the dense ones: x_bs > Cin T, as the batch groups of the front part are passed).

Geometries B x T: 3 x 200 (seams inside tiles), 5 x 72 (a seam in nearly every 64-column tile), 9 x 8 (many seams per
tile), 1 x 200 (no seam), 3 x 52 (partial last tile), 3 x 50 (T % 4 != 0: the form does not apply).

The gated conv cases run two more geometries, 5 x 200 and 9 x 72: at 384 gated rows the six above have at most 48 tiles
of 64 x 128 (except 9 x 8) and take the K-split tile, which does not implement the form and refuses the field.

A case is (spec for conv_ref.build, split) with split = None or (split_row, mask_mode2, accumulate2): the two-output form
of a 1x1 token GEMM, which conv_ref does not know, is stated as two launches of its contract (rows [0, split_row) with
the case's epilogue, rows [split_row, Cout) into y2): tokgemm_ref.evaluate.
"""
import conv_ref as R
import tokgemm_ref as T

GEOMETRIES = ((3, 200), (5, 72), (9, 8), (1, 200), (3, 52), (3, 50))

# the 1x1 token GEMMs of the front part on the block GEMM (Cin >= 96; from 96 tiles of 64 x 64 per launch, or the
# split-row form at any size).  704 rows: 11 row tiles x (12 | 10 | 9 column tiles) >= 96 at the first three geometries.
_GEMM = dict(K=1, Cin=192)
_BIG = dict(_GEMM, Cout=704)
_SPLIT = dict(_GEMM, Cout=128, bias=True, res=True)
# the k = 5 convs of the front part on the short-sequence conv tiles: 64 x 64 plain rows, 64 x 128 gated rows
_K5 = dict(K=5, dil=1, pad=2)
GATED_GEOMETRIES = GEOMETRIES + ((5, 200), (9, 72))


def _specs():
    s = []
    for B, T in GEOMETRIES:
        g = f"b{B}_t{T}"
        geo = dict(B=B, L=T)
        if T % 4 == 0:
            # split-row two-output form (WN res_skip): first half (x + rs[:H]) * mask, second half out += rs[H:]
            s.append((dict(id=f"gemm_split_post_acc2_{g}", **_SPLIT, **geo, mask_mode=R.MASK_POST), (64, R.MASK_NONE, True)))
            s.append((dict(id=f"gemm_split_both_mask2_{g}", **_SPLIT, **geo, mask_mode=R.MASK_BOTH, accumulate=True),
                      (64, R.MASK_POST, False)))
        if (B, T) in ((3, 200), (5, 72), (9, 8), (3, 50)):   # (T = 50: no 16-B groups, so another kernel than the block GEMM)
            # plain epilogue: bias + conditioning bias + GELU + residual
            s.append((dict(id=f"gemm_plain_cbias_gelu_res_{g}", **_BIG, **geo, bias=True, cbias=True, res=True,
                           act=R.ACT_GELU_TANH), None))
            # k = 1 with res alone (INIT-like plain epilogue)
            s.append((dict(id=f"gemm_plain_res_{g}", **_BIG, **geo, bias=True, res=True), None))
        if (B, T) in ((3, 200), (5, 72)):
            # extended epilogue: every per-(b, .) operand -- masks, cscale, scale, accumulate, post_scale
            s.append((dict(id=f"gemm_ext_pre_cscale_scale_acc_{g}", **_BIG, **geo, bias=True, cbias=True, cscale=True,
                           res=True, mask_mode=R.MASK_PRE, scale=0.75, accumulate=True, post_scale=0.5, act=R.ACT_RELU), None))
            s.append((dict(id=f"gemm_ext_post_{g}", **_BIG, **geo, bias=True, res=True, mask_mode=R.MASK_POST), None))
            s.append((dict(id=f"gemm_ext_both_cscale_{g}", **_BIG, **geo, bias=True, cscale=True, mask_mode=R.MASK_BOTH,
                           act=R.ACT_GELU_TANH), None))
    for B, T in GATED_GEOMETRIES:
        g, geo = f"b{B}_t{T}", dict(B=B, L=T)
        # WN in-layer: gated rows (M = 384) with the conditioning bias, written into a wider output tensor
        s.append((dict(id=f"conv_k5_gated_wn_cbias_{g}", **_K5, **geo, Cin=192, H=192, rows=R.ROWS_GATE_WN, bias=True,
                       cbias=True), None))
    for B, T in GEOMETRIES:
        g, geo = f"b{B}_t{T}", dict(B=B, L=T)
        # FFN fc1: k = 5 with GELU (vector epilogue)
        s.append((dict(id=f"conv_k5_gelu_{g}", **_K5, **geo, Cin=192, Cout=128, bias=True, act=R.ACT_GELU_TANH), None))
        # accumulator-init epilogue: bias + cbias + residual + running sum
        s.append((dict(id=f"conv_k5_init_res_acc_{g}", **_K5, **geo, Cin=32, Cout=64, bias=True, cbias=True, res=True,
                       accumulate=True, post_scale=0.5), None))
    for B, T in ((3, 200), (5, 72)):
        g, geo = f"b{B}_t{T}", dict(B=B, L=T)
        small = dict(_K5, **geo, Cin=32, Cout=64, bias=True)
        s.append((dict(id=f"conv_k5_vec_pre_cscale_scale_{g}", **small, cbias=True, cscale=True, scale=0.75, res=True,
                       mask_mode=R.MASK_PRE), None))
        s.append((dict(id=f"conv_k5_vec_post_acc_{g}", **small, res=True, accumulate=True, mask_mode=R.MASK_POST), None))
        s.append((dict(id=f"conv_k5_vec_both_gelu_{g}", **small, act=R.ACT_GELU_TANH, mask_mode=R.MASK_BOTH), None))
        s.append((dict(id=f"conv_k5_gen_y_off1_{g}", **small, res=True, scale=0.75, mask_mode=R.MASK_BOTH, y_shift=1), None))
        s.append((dict(id=f"conv_k3_lrelu_{g}", K=3, **geo, Cin=32, Cout=128, bias=True, prologue=R.PRO_LRELU, scale=0.75), None))
        s.append((dict(id=f"conv_k5_gated_glu_chain_{g}", **_K5, B=B + 4, L=T, Cin=32, H=192, rows=R.ROWS_GATE_GLU, bias=True,
                       cbias=True, cscale=True, res=True, scale=0.75, accumulate=True, mask_mode=R.MASK_BOTH), None))
    for i, (spec, _) in enumerate(s):
        spec.update(entry="mfma", tile=None, seed=7000 + i)
    return s


SPECS = _specs()
IDS = [spec["id"] for spec, _ in SPECS]
assert len(set(IDS)) == len(IDS)
_CACHE = {}


def case(id):
    """-> (a, a2 or None, split, refs) as tokgemm_ref.evaluate gives them: ``a`` the args of the launch (of its first half
    when split), ``a2`` those of the second half, refs = [(buffer name, float64 reference buffer, written mask), ...].
    Computed once, never modified."""
    if id not in _CACHE:
        spec, split = SPECS[IDS.index(id)]
        _CACHE[id] = T.evaluate(R.build(spec), split, spec["seed"])
    return _CACHE[id]


def to_struct(id, base, fold):
    """hsp_conv1d_args of a case; ``base`` as conv_ref.to_struct, plus 'y2' for the split form."""
    a, a2, split, _ = case(id)
    s = T.to_struct(a, a2, split, base)
    s.fold_cols = int(fold)
    return s


def fake_base():
    return dict(R.fake_base(), y2=0x100000 * 30)
