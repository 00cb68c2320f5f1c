"""The 1x1 token GEMMs behind hsp_conv1d_mfma_f32 (csrc/hsp_rgemm.hip, plan KC = -1; csrc/hsp_bgemm.hip, plan KC = -2)
against the header contract in float64: the case table that tests/test_tokgemm_ref_host.py (CPU) and
tests/test_gpu_tokgemm_contract.py (GPU) both walk, and tools/tokgemm_bits.py hashes.

Operands, views and the float64 statement are those of tests/conv_ref.py (its `_evaluate` knows `ln_c1` and `res_ts`);
this module adds what conv_ref's case builder does not make -- a LayerNorm operand, column-strided `x` and `res` -- and
the one statement of the two-output form (hsp_conv1d_args.split_row) as two launches of the contract: rows
[0, split_row) with the case's epilogue into y, rows [split_row, Cout) into a y2 canary buffer with bias, mask_mode2
and accumulate2 alone.  tests/fold_cases.py imports that statement.

A case id names the kernel and tile (rg32 / rg64: register path 32 x 32 / 64 x 32; bg64 / bg128: block GEMM 64 x 64 /
128 x 128) and the property; the host test checks the name against hsp_conv1d_mfma_plan.  Shapes follow the
eligibility code: ncols = 33 or 99 (ncols % 4 != 0) keeps the block GEMM out; 3 x 3 x 11 = 99 tiles of 64 x 64 is just
past its threshold of 96; 772 x 516 x 7 is 245 tiles of 128 x 128, one round of 256.
"""
import numpy as np

import conv_ref as R

LN_EPS = 1e-5
PLANS = dict(rg32=(32, 32, -1), rg64=(64, 32, -1), bg64=(64, 64, -2), bg128=(128, 128, -2))
EXT_ALL = dict(bias=True, cbias=True, cscale=True, res=True, accumulate=True, scale=0.75, post_scale=0.5,
               mask_mode=R.MASK_BOTH)


def _specs():
    s = []

    def c(id, **kw):
        s.append(dict(dict(K=1, bias=True), id=id, **kw))
    # ---- register path, 32 x 32 tile, K split eight ways: k-steps = ceil(Cin / 2), ceil(k-steps / 8) per wave
    rg32 = dict(Cout=36, L=33, B=2)
    c("rg32_cin32_two_ksteps_per_wave", **rg32, Cin=32, res=True)
    c("rg32_cin33_odd_k_tail", **rg32, Cin=33, res=True)
    c("rg32_cin34_wave_with_empty_k_share", **rg32, Cin=34, res=True)
    c("rg32_cin38_ragged_k_share", **rg32, Cin=38, res=True)
    c("rg32_cin276_one_group_of_18", **rg32, Cin=276, res=True)
    c("rg32_cin512_two_groups_of_18", **rg32, Cin=512)
    c("rg32_cin1104_two_groups_of_36", **rg32, Cin=1104, res=True)
    c("rg32_ln_cin276", **rg32, Cin=276, ln=True, act=R.ACT_RELU)
    c("rg32_ln_cin33_odd_k_tail", **rg32, Cin=33, ln=True, cbias=True)
    c("rg32_x_ts3", **rg32, Cin=38, x_ts=3, res=True)
    c("rg32_res_ts5", **rg32, Cin=38, res=True, res_ts=5)
    c("rg32_chain_both_masks_cscale_acc_scales", **rg32, Cin=38, **EXT_ALL)
    for act, name in enumerate(R.ACT_NAMES):
        c(f"rg32_act_{name}", **rg32, Cin=38, act=act, res=True)
    # ---- register path, 64 x 32 tile, K split four ways: 2 x 4 x 25 = 200 tiles; Cin < 96 keeps the block GEMM out too
    rg64 = dict(Cout=128, L=99, B=25, Cin=64)
    c("rg64_cin64", **rg64, res=True)
    c("rg64_ln_cin64", **rg64, ln=True)
    c("rg64_chain_both_masks_cscale_acc_scales", **rg64, **EXT_ALL, act=R.ACT_GELU_TANH)
    # ---- block GEMM, 64 x 64: 48-channel stages, three resident; interior tiles on the fast DMA path, edge tiles (132 =
    # 2 x 64 + 4 rows and columns) on the general one
    bg64 = dict(Cout=132, L=132, B=11)
    c("bg64_cin96_two_stages", **bg64, Cin=96, res=True)
    c("bg64_cin100_short_last_stage", **bg64, Cin=100, cbias=True)
    c("bg64_cin196_five_stages_slot_reuse", **bg64, Cin=196, res=True)
    c("bg64_ln_cin96", **bg64, Cin=96, ln=True)
    c("bg64_ln_cin100_short_last_stage", **bg64, Cin=100, ln=True, res=True, act=R.ACT_GELU_TANH)
    for act in (R.ACT_RELU, R.ACT_GELU_TANH, R.ACT_NONE):
        c(f"bg64_plain_{R.ACT_NAMES[act]}", **bg64, Cin=100, act=act, res=True, cbias=True)
        c(f"bg64_ext_{R.ACT_NAMES[act]}", **bg64, Cin=100, act=act, res=True, scale=0.75)
    c("bg64_ext_everything", **bg64, Cin=100, **EXT_ALL, act=R.ACT_GELU_TANH)
    # the second output: admitted below 96 tiles (3 x 3 x 1 = 9)
    c("bg64_split64_mask2_acc2", Cout=132, L=132, B=1, Cin=100, res=True, mask_mode=R.MASK_POST,
      split=(64, R.MASK_POST, True))
    # ---- block GEMM, 128 x 128: two column blocks per wave, LayerNorm statistics exchanged between partner waves
    bg128 = dict(Cout=772, L=516, B=7)
    for cin, what in ((96, "two_stages"), (100, "short_last_stage")):
        c(f"bg128_cin{cin}_{what}", **bg128, Cin=cin, res=True)
        c(f"bg128_ln_cin{cin}_partner_exchange", **bg128, Cin=cin, ln=True, act=R.ACT_RELU)
        c(f"bg128_ext_cin{cin}_everything", **bg128, Cin=cin, **EXT_ALL)
    for i, spec in enumerate(s):
        spec.update(entry="mfma", tile=None, seed=8000 + i)
    return s


SPECS = _specs()
IDS = [s["id"] for s in SPECS]
assert len(set(IDS)) == len(IDS)
_CACHE = {}


def build(spec):
    """conv_ref.build, then the operands it does not make.  ln: x = standard-normal columns plus a per-column offset of
    at most 1 (the header formula's own cancellation stays small), ln_c1[row] = sum_ci w[ci][row] in fp32 as the caller
    packs it.  x_ts / res_ts: the same logical tensors re-laid at a column stride, inside wider buffers."""
    a = R.build({k: v for k, v in spec.items() if k not in ("x_ts", "res_ts")})
    r = np.random.default_rng(spec["seed"] + 500)
    B, Cin, L, Cout = a["B"], a["Cin"], a["Lin"], a["Cout"]
    ts = spec.get("x_ts", 1)
    if spec.get("ln") or ts > 1:
        xcs = R._round_up((L + 3) * ts, 4) + 4
        buf = r.standard_normal((B, Cin + 1, xcs)).astype(R.F32)
        if spec.get("ln"):
            buf += r.uniform(-1.0, 1.0, (B, 1, xcs)).astype(R.F32)
        a.update(x=buf.reshape(-1), x_off=4, x_bs=(Cin + 1) * xcs, x_cs=xcs, x_ts=ts)
    if spec.get("ln"):
        c1 = np.asarray(a["w"], R.F32).reshape(Cin, a["w_ld"]).astype(R.F64).sum(0).astype(R.F32)
        a.update(ln_c1=np.concatenate([r.standard_normal(4).astype(R.F32), c1]), ln_c1_off=4, ln_eps=LN_EPS)
    rts = spec.get("res_ts", 1)
    if rts > 1:
        rcs = (L + 2) * rts + 3
        a.update(res=r.standard_normal((B, Cout + 1, rcs)).astype(R.F32).reshape(-1), res_off=2, res_bs=(Cout + 1) * rcs,
                 res_cs=rcs, res_ts=rts)
    return a


def second_half(a, split_row, mode2, acc2, r):
    """The args dict of rows [split_row, Cout) written to a y2 canary buffer: bias only, mask per mask_mode2."""
    B, rows2, Lout = a["B"], a["Cout"] - split_row, a["Lout"]
    y2cs = a["y_cs"] + 12
    buf = np.full((B, rows2 + 3, y2cs), R.SENT, R.F32)
    if acc2:
        buf[:, 1:rows2 + 1, 8:8 + Lout] = r.standard_normal((B, rows2, Lout)).astype(R.F32)
    a2 = dict(a, M=rows2, Cout=rows2, w_off=a["w_off"] + split_row, bias_off=a["bias_off"] + split_row,
              y=buf.reshape(-1), y_off=y2cs + 8, y_bs=(rows2 + 3) * y2cs, y_cs=y2cs, mask_mode=mode2,
              accumulate=int(acc2), scale=1.0, post_scale=1.0, act=R.ACT_NONE)
    for k in ("res", "res_off", "res_bs", "res_cs", "cbias", "cbias_off", "cbias_bs", "cscale", "cscale_off", "cscale_bs"):
        a2.pop(k, None)
    return a2


def evaluate(full, split, seed):
    """-> (a, a2 or None, split, refs) of a launch with args ``full`` and split = None or (split_row, mask_mode2,
    accumulate2): ``a`` the args of the launch, ``a2`` those of the second half, refs = [(buffer name, float64 reference
    buffer, written mask), ...], never to be modified."""
    if split is None:
        ref, written = R._evaluate(full)
        out = (full, None, None, [("y", ref, written)])
    else:
        split_row, mode2, acc2 = split
        a1 = dict(full, M=split_row, Cout=split_row)
        a2 = second_half(full, split_row, mode2, acc2, np.random.default_rng(seed + 1))
        r1, w1 = R._evaluate(a1)
        r2, w2 = R._evaluate(a2)
        out = (full, a2, split, [("y", r1, w1), ("y2", r2, w2)])
    for _, ref, written in out[3]:
        ref.setflags(write=False)
        written.setflags(write=False)
    return out


def case(id):
    """(a, a2, split, refs) as `evaluate` gives them, computed once per process."""
    if id not in _CACHE:
        spec = SPECS[IDS.index(id)]
        _CACHE[id] = evaluate(build(spec), spec.get("split"), spec["seed"])
    return _CACHE[id]


def plan_of(id):
    """(BM, BN, KC) the id names."""
    return PLANS[id.split("_")[0]]


POINTERS = R.POINTERS + ("ln_c1", "y2")


def to_struct(a, a2, split, base):
    """hsp_conv1d_args of a launch; ``base`` as conv_ref.to_struct, plus 'ln_c1' and 'y2' where the case has them."""
    s = R.to_struct(a, base)
    if a.get("ln_c1") is not None:
        s.ln_c1, s.ln_eps = base["ln_c1"] + 4 * a["ln_c1_off"], a["ln_eps"]
    s.res_ts = a.get("res_ts", 0)
    if split is not None:
        s.split_row, s.mask_mode2, s.accumulate2 = split[0], split[1], int(split[2])
        s.y2, s.y2_bs, s.y2_cs = base["y2"] + 4 * a2["y_off"], a2["y_bs"], a2["y_cs"]
    return s


def fake_base():
    return dict(R.fake_base(), ln_c1=0x100000 * 29, y2=0x100000 * 30)
