"""CPU, no device: the float64 contract of tests/conv_ref.py against torch's CPU conv1d / conv_transpose1d in float64,
and what the GPU comparisons of tests/test_gpu_conv_contract.py rely on for the same case table:

  * the packed weights of every case are what hip_layers' packing maps make of the layer's torch-layout weight,
  * hsp_conv1d_mfma_plan (validation + selection, no launch) returns the conv tile shape each MFMA case id names, and
    the table reaches all eleven tile shapes, every (shape, epilogue kind) the library instantiates, all eight
    activations on the vector and the scalar epilogue, both window DMA widths, the narrow-tail schedule from both
    sides and the three direct kernels,
  * the mask values tell NONE / PRE / POST / BOTH apart by at least 100 x the GPU bar,
  * the refusals of both entry points (those tests/test_host_logic.py does not already hold).

    python -m pytest tests/test_conv_ref_host.py -q
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import conv_ref as R
import helpers as H

RTOL = 1e-12
MFMA = [s["id"] for s in R.SPECS if s["entry"] == "mfma"]
DIRECT = [s["id"] for s in R.SPECS if s["entry"] == "direct"]


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.fixture(scope="module")
def L():
    from megatts2_hierspeechpp_amd import _lib
    _lib.lib()
    return _lib


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _plan(L, a):
    out = (ctypes.c_int32 * 4)()
    rc = L.lib().hsp_conv1d_mfma_plan(ctypes.byref(R.to_struct(a, R.fake_base())), out)
    return rc, tuple(out)


# ------------------------------------------------------------------------------------------------ contract == torch
def _torch_reference(a):
    """[B, Cout, Lout] float64: the layer through torch's CPU convolutions on the UN-packed weight, then the epilogue of
    include/hsp.h spelled out."""
    B, Cin, Lin, Cout, Lout = a["B"], a["Cin"], a["Lin"], a["Cout"], a["Lout"]
    x = _t(R.view(a, "x", (B, Cin, Lin), (a["x_bs"], a["x_cs"], a["x_ts"]))[0])
    if a["prologue"] == R.PRO_LRELU:
        x = TF.leaky_relu(x, float(np.float32(a["slope"])))
    elif a["prologue"] == R.PRO_SILU:
        x = TF.silu(x)
    elif a["prologue"] == R.PRO_ACT1D:
        x = _t(R.act1d(x.numpy(), a["alpha_exp"], a["beta_inv"], a["filt"]))     # pinned on its own below
    rows, gated = a["rows"], a["rows"] in (R.ROWS_GATE_WN, R.ROWS_GATE_GLU)
    r0 = a.get("w_off", 0)
    nb = 2 * a["gate_half"] if gated else Cout
    bias = _t(a["layer_b"][r0:r0 + nb]) if a.get("bias") is not None else None
    W = _t(a["layer_w"])
    if rows == R.ROWS_SHUFFLE:
        v = TF.conv_transpose1d(x, W, bias, stride=a["up"], padding=a["shuf_pad"])
    else:
        Wb = W if a["w_bs"] else W[None].expand(B, *W.shape)
        v = torch.cat([TF.conv1d(x[b:b + 1], Wb[b][r0:r0 + nb], bias, stride=a["stride"], padding=a["pad"],
                                 dilation=a["dil"]) for b in range(B)])
    assert v.shape == (B, nb, Lout), (v.shape, (B, nb, Lout))
    if a.get("cbias") is not None:
        v = v + _t(R.view(a, "cbias", (B, nb), (a["cbias_bs"], 1))[0])[:, :, None]
    if gated:
        Hh = a["gate_half"]
        v = (torch.tanh(v[:, :Hh]) if rows == R.ROWS_GATE_WN else v[:, :Hh]) * torch.sigmoid(v[:, Hh:])
    else:
        act = {R.ACT_NONE: lambda t: t, R.ACT_TANH: torch.tanh, R.ACT_GELU_TANH: lambda t: TF.gelu(t, approximate="tanh"),
               R.ACT_RELU: torch.relu, R.ACT_MISH: TF.mish, R.ACT_SILU: TF.silu, R.ACT_SOFTPLUS: TF.softplus,
               R.ACT_GELU_ERF: TF.gelu}[a["act"]]
        v = act(v)
    mk = _t(R.view(a, "mask", (B, Lout), (a["mask_bs"], 1))[0])[:, None, :] if a["mask_mode"] else None
    if a["mask_mode"] & R.MASK_PRE:
        v = v * mk
    if a.get("cscale") is not None:
        v = v * _t(R.view(a, "cscale", (B, Cout), (a["cscale_bs"], 1))[0])[:, :, None]
    v = v * float(np.float32(a["scale"]))
    if a.get("res") is not None:
        v = v + _t(R.view(a, "res", (B, Cout, Lout), (a["res_bs"], a["res_cs"], 1))[0])
    if a["mask_mode"] & R.MASK_POST:
        v = v * mk
    if a["accumulate"]:
        v = v + _t(R.view(a, "y", (B, Cout, Lout), (a["y_bs"], a["y_cs"], 1))[0])
    return (v * float(np.float32(a["post_scale"]))).numpy()


@pytest.mark.parametrize("id", R.IDS)
def test_contract_equals_torch_float64(id):
    a, ref, written = R.case(id)
    _, yidx = R.view(a, "y", (a["B"], a["Cout"], a["Lout"]), (a["y_bs"], a["y_cs"], 1))
    want = _torch_reference(a)
    got = ref[yidx]
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert float(err.max()) <= RTOL, f"{id}: relative difference {err.max():.2e}"
    # a conv writes its whole [B, Cout, Lout] tensor and nothing else; the rest of the buffer keeps its canaries
    own = np.zeros(ref.shape, bool)
    own[yidx.reshape(-1)] = True
    assert np.array_equal(own, written), id
    assert np.array_equal(ref[~own], a["y"].astype(np.float64)[~own]) and (a["y"][~own] == R.SENT).all()
    if not a["accumulate"]:
        assert (a["y"] == R.SENT).all()


def test_act1d_restatement_equals_the_closed_form_of_the_oracle():
    """The oracle's loop keeps its 2x-rate signal in a float32 tensor, so the two agree to fp32 rounding of O(1) values
    (5e-7), not to 1e-12; an index or tap slip would show at 1e-3 and above."""
    from oracle import hsp_oracle as O
    from megatts2_hierspeechpp_amd.synth import kaiser_sinc_filter12
    r = np.random.default_rng(41)
    h = kaiser_sinc_filter12()
    for Lx in (1, 2, 7, 23):
        x, al, be = r.standard_normal((2, 3, Lx)), r.uniform(-1, 1, 3), r.uniform(-1, 1, 3)
        want = O.act1d_closed_form(_t(x), _t(al), _t(be), h=[float(v) for v in h]).numpy()
        got = R.act1d(x, np.exp(al), 1.0 / (np.exp(be) + 1e-9), np.concatenate([h, h]))
        assert np.abs(got - want).max() <= 5e-7, Lx


@pytest.mark.parametrize("id", R.IDS)
def test_packed_weights_are_what_hip_layers_packs(id):
    from megatts2_hierspeechpp_amd import hip_layers as HL
    a, _, _ = R.case(id)
    W = np.asarray(a["layer_w"], np.float32)
    if a["rows"] == R.ROWS_SHUFFLE:
        mp, kp, M = HL.convtr_pack_map(a["Cin"], a["Cout"], W.shape[2], a["up"])
        assert (kp, M) == (a["K"], a["M"])
        Ws = [W]
    else:
        Ws = W if a["w_bs"] else [W]
        gated = a["rows"] != R.ROWS_PLAIN
        rows = HL.gated_rows(a["gate_half"]) if gated else HL.plain_rows(Ws[0].shape[0])
        assert len(rows) == a["w_ld"]
        mp = HL.conv_pack_map(Ws[0].shape[0], a["Cin"], a["K"], rows)
    packed = np.concatenate([np.where(mp >= 0, Wb.reshape(-1)[np.maximum(mp, 0)], np.float32(0)) for Wb in Ws])
    assert np.array_equal(packed.astype(np.float32), a["w"]), id


# ------------------------------------------------------------------------------------------------ plans and coverage
@pytest.mark.parametrize("id", MFMA)
def test_mfma_case_takes_the_conv_tile_its_id_names(id, L):
    a, _, _ = R.case(id)
    rc, (bm, bn, kc, lds) = _plan(L, a)
    assert rc == 0, (id, rc)
    assert kc > 0, f"{id}: not a conv tile (KC = {kc})"
    tile, epi = id.split("_")[:2]
    assert tile == a["tile"] and (bm, bn) == R.TILES[tile], (id, bm, bn)
    assert R.tile_of(a, bm, bn) == tile, (id, R.tile_of(a, bm, bn))
    # (BM, BN) is shared by S64 / S64W / S64G2 and by M64 / M64P, M32 / M32P: the plan's LDS byte count is the named
    # shape's, and every other shape of that (BM, BN) either needs another byte count or is not instantiated for this
    # case's epilogue and prologue (so the library cannot have meant it)
    kind, act = R.EPI_NAMES[R.epilogue_kind(a)], a["prologue"] == R.PRO_ACT1D
    assert lds == R.lds_bytes(tile, a, kc), (id, lds, R.lds_bytes(tile, a, kc))
    assert (tile, kind, act) in EXISTS, (id, kind, act)
    for other, shape in R.TILES.items():
        if other != tile and shape == (bm, bn):
            assert R.lds_bytes(other, a, kc) != lds or (other, kind, act) not in EXISTS, (id, other)
    assert R.EPI_NAMES[R.epilogue_kind(a)] == epi.replace("SHUFGEN", "GEN"), (id, R.EPI_NAMES[R.epilogue_kind(a)])
    assert a["K"] >= 2
    assert a["B"] * a["Cout"] * a["Lout"] <= 1_300_000


CHUNKS3 = [id for id in MFMA if "chunks3" in id]


def test_chunks3_cases_stage_at_least_three_chunks(L):
    """The chunk depth KC is the library's own (third number of the plan): a `chunks3` case walks its input channels in
    at least three chunks, so the producers refill both halves of the double buffer and the consumers' fragment pipeline
    crosses two chunk barriers; under ACT1D the raw-row look-ahead to chunk c + 2 runs."""
    assert len(CHUNKS3) == 7
    for id in CHUNKS3:
        a, _, _ = R.case(id)
        rc, (_, _, kc, _) = _plan(L, a)
        assert rc == 0 and kc > 0, (id, rc, kc)
        assert -(-a["Cin"] // kc) >= 3, f"{id}: Cin {a['Cin']} at KC {kc} is {-(-a['Cin'] // kc)} chunk(s)"
    by = {id: R.case(id)[0] for id in CHUNKS3}
    assert sum(a["prologue"] == R.PRO_ACT1D for a in by.values()) == 2
    fast = by["S64_INIT_chunks3_fast"]   # the fast staging's preconditions: no channel tail, 16-B window, full row tiles
    assert fast["Cin"] % _plan(L, fast)[1][2] == 0 and R.xvec(fast) and fast["Cout"] % R.TILES["S64"][0] == 0
    assert by["S64_VEC_chunks3_cin_tail"]["Cin"] % _plan(L, by["S64_VEC_chunks3_cin_tail"])[1][2] == 8
    assert R.xvec(by["S64_VEC_chunks3_cin_tail"]) and not R.xvec(by["S64_GEN_chunks3_dma4"])
    assert R.tail_schedule(by["M128_INIT_chunks3_tail_rem1"], "M128")


# (shape, epilogue kind, ACT1D prologue) the library instantiates: supported<>() of csrc/hsp_conv1d_tile.hip
PLAIN_SHAPES = ("M128", "M64P", "M32P", "S64", "S64W", "S32")
EXISTS = {(t, e, False) for t in PLAIN_SHAPES for e in ("INIT", "VEC", "SHUF", "GEN")} | \
         {(t, e, True) for t in ("M128", "M64", "M32", "S64", "S64W", "S32") for e in ("INIT", "GEN")} | \
         {(t, "GATE", False) for t in ("M128", "S64G", "S64GW", "S64G2")}


def test_table_covers_shapes_epilogues_activations_and_direct_kernels():
    cases = [R.case(id)[0] for id in R.IDS]
    mf = [a for a in cases if a["entry"] == "mfma"]
    seen = {(a["tile"], R.EPI_NAMES[R.epilogue_kind(a)], a["prologue"] == R.PRO_ACT1D) for a in mf}
    assert {t for t, _, _ in seen} == set(R.TILES)                         # eleven shapes
    assert {e for _, e, _ in seen} == set(R.EPI_NAMES)                     # five epilogue kinds
    assert seen == EXISTS, (EXISTS - seen, seen - EXISTS)
    for epi in (R.EPI_VEC, R.EPI_GEN):
        assert {a["act"] for a in mf if R.epilogue_kind(a) == epi} == set(range(8)), epi
        for mm in range(4):                                                # the full chain per mask mode
            assert any(R.epilogue_kind(a) == epi and a["mask_mode"] == mm and a["accumulate"] and a["act"] and
                       all(a.get(k) is not None for k in ("cbias", "cscale", "res")) and a["scale"] != 1 and
                       a["post_scale"] != 1 for a in mf), (epi, mm)
    for mm in range(4):
        assert any(R.epilogue_kind(a) == R.EPI_GATE and a["mask_mode"] == mm and a.get("cbias") is not None and
                   a.get("cscale") is not None and a.get("res") is not None for a in mf), mm
    assert {a["gate_half"] for a in mf if a["gate_half"]} >= {32, 96}
    assert {a["rows"] for a in mf} == {0, 1, 2, 3}
    tails = {(a["ncols"] % 128, R.tail_schedule(a, a["tile"])) for a in mf if a["id"].startswith("M128_INIT_tail")}
    assert tails == {(1, True), (32, True), (33, False)}
    assert {R.xvec(a) for a in mf} == {True, False}
    assert any(a["x_ts"] != 1 for a in mf) and any(a["w_bs"] for a in mf) and any(a["w_off"] == 4 for a in mf) and \
        any(a["w_off"] == 64 for a in mf)
    ups = {a["up"] for a in mf if a["rows"] == R.ROWS_SHUFFLE}
    assert ups >= {2, 3, 4, 5, 8}
    # padding rows Cout up .. M on each SHUFFLE route: 8-B vector stores, scalar stores, the scalar epilogue with cscale
    padded = [a for a in mf if a["rows"] == R.ROWS_SHUFFLE and a["M"] > a["Cout"] * a["up"]]
    assert any(a["up"] == 2 and R.epilogue_kind(a) == R.EPI_SHUF for a in padded)
    assert any(a["up"] not in (2, 4) and R.epilogue_kind(a) == R.EPI_SHUF for a in padded)
    assert any(R.epilogue_kind(a) == R.EPI_GEN and a.get("cscale") is not None and a.get("cbias") is not None
               for a in padded)
    assert any(a["rows"] == R.ROWS_SHUFFLE and a["Lout"] % a["up"] for a in mf)
    assert {a["Cin"] for a in mf} >= {5, 12, 40}
    di = [a for a in cases if a["entry"] == "direct"]
    kinds = {R.direct_kernel(a) for a in di}
    assert kinds == {"generic", "cout1", "linear_vec"}
    for a in di:
        assert a["id"].startswith(R.direct_kernel(a)), (a["id"], R.direct_kernel(a))
    c1 = [a for a in di if R.direct_kernel(a) == "cout1"]
    assert {a["K"] for a in c1} == {1, 3, 5, 7, 9} and {a["Cin"] for a in c1} >= {1, 4, 6}
    assert {a["Lin"] for a in c1} >= {4, 1024, 1028, 2052}
    lv = [a for a in di if R.direct_kernel(a) == "linear_vec"]
    assert {a["Cin"] for a in lv} >= {64, 100, 1000, 1024} and {a["Cout"] for a in lv} >= {64, 65, 200}
    assert {a["B"] for a in lv} >= {1, 8, 9, 17}
    assert {a["prologue"] for a in lv} >= {R.PRO_SILU, R.PRO_LRELU}
    assert {a["prologue"] for a in di if R.direct_kernel(a) == "generic"} >= {R.PRO_SILU, R.PRO_LRELU}
    assert {a["stride"] for a in di} >= {2, 4}


def test_neighbours_of_the_cout1_conditions_compute_the_same_contract():
    """The cases next to cout1_base_k7_l1028 that fail one cout1_fast condition each and so run on the generic kernel."""
    base = R.case("cout1_base_k7_l1028")[0]
    assert R.cout1_fast(base)
    for id in ("generic_cout1_l_mod4_1", "generic_cout1_x_off1", "generic_cout1_res", "generic_cout1_k11"):
        a = R.case(id)[0]
        assert not R.cout1_fast(a) and a["Cout"] == 1 and a["Cin"] == base["Cin"], id


@pytest.mark.parametrize("id", ["S64_VEC_chain_both_mish", "S64_GEN_chain_both_mish", "S64G2_GATE_wn_h32_chain_pre",
                                "generic_stride2_dil2_chain"])
def test_mask_modes_are_told_apart(id):
    """Non-idempotent mask values: with a residual NONE, PRE, POST and BOTH give four references that differ pairwise
    by at least 100 x the bar of the GPU comparison.  Without one PRE and POST are the same product in another order
    (equal to rounding), and the three classes NONE, PRE = POST, BOTH differ by as much."""
    a = R.case(id)[0]
    assert a.get("res") is not None
    own = R.conv_written(a)
    for drop_res in (False, True):
        outs = [R.conv_contract(dict(a, mask_mode=mm, res=None if drop_res else a["res"]))[own] for mm in range(4)]
        bar = max(H.tol_for(o) for o in outs)
        for p, q in itertools.combinations(range(4), 2):
            gap = float(np.abs(outs[p] - outs[q]).max())
            if drop_res and (p, q) == (R.MASK_PRE, R.MASK_POST):
                assert gap <= 1e-12 * max(1.0, float(np.abs(outs[p]).max()))
            else:
                assert gap >= 100 * bar, (id, drop_res, p, q, gap, bar)


def test_derived_bound_scale_dominates_the_reference():
    """conv_contract_abs >= |conv_contract| element-wise on the linear cases (the triangle inequality, term by term)."""
    n = 0
    for id in R.IDS:
        a, ref, written = R.case(id)
        if R.is_linear(a) and a["B"] * a["Cout"] * a["Lout"] < 100_000:
            ab = R.conv_contract_abs(a)
            assert (ab[written] >= np.abs(ref[written]) * (1 - 1e-12)).all(), id
            n += 1
    assert n >= 20


# ------------------------------------------------------------------------------------------------ refusals
def _plan_code(L, a, **change):
    """Return code of hsp_conv1d_mfma_plan (validation and selection, never a launch) for the case with fields replaced."""
    s = R.to_struct(a, R.fake_base())
    for k, v in change.items():
        setattr(s, k, v)
    return L.lib().hsp_conv1d_mfma_plan(ctypes.byref(s), (ctypes.c_int32 * 4)())


def _direct_refused(L, a, **change):
    """hsp_conv1d_direct_f32 has no plan form, so this calls the LAUNCHING entry point on made-up addresses (fake_base)
    and a null stream: only a struct that one of the checks in front of the three launches refuses may come here -- were
    such a check to go missing on a machine with a device, a kernel would run on those addresses.  Do not extend this
    list with a struct whose refusal is not one of those checks, and never call it expecting 0."""
    s = R.to_struct(a, R.fake_base())
    for k, v in change.items():
        setattr(s, k, v)
    return L.lib().hsp_conv1d_direct_f32(ctypes.byref(s), None) == L.EINVAL


def test_mfma_refusals(L):
    """Every refused struct breaks ONE rule of validate() / pick_lkc (all its other fields satisfy theirs); where the rule
    is a bound or a divisibility, the nearest struct on the allowed side of it is accepted."""
    fb = R.fake_base()
    a = R.case("S64_VEC_boundary_base")[0]
    M = a["M"]
    assert _plan_code(L, a) == 0 and (M, a["w_ld"], a["Cout"], a["dil"], a["K"]) == (40, 40, 40, 1, 3)
    for change in (dict(stride=2),
                   dict(M=M + 2, w_ld=M + 4),                     # M % 4 alone: w_ld is a multiple of 4 and >= M
                   dict(w_ld=M + 2),                              # w_ld % 4 alone
                   dict(w_ld=M - 4),                              # w_ld < M alone
                   dict(w=fb["w"] + 4), dict(zeros=fb["zeros"] + 4), dict(zeros=None), dict(mask=None),
                   dict(prologue=R.PRO_SILU),
                   dict(prologue=R.PRO_ACT1D),                    # without alpha_exp / beta_inv / filt
                   dict(w_bs=2), dict(dil=0),
                   dict(K=2, dil=126, pad=63)):                   # a halo (K - 1) dil of 126 columns
        assert _plan_code(L, a, **change) == L.EINVAL, change
    for change in (dict(M=M + 4, w_ld=M + 4), dict(w_ld=M + 4), dict(w_bs=a["K"] * a["Cin"] * a["w_ld"]),
                   dict(K=2, dil=125, pad=63)):                   # 125: the widest the S64W pitch holds
        assert _plan_code(L, a, **change) == 0, change
    g = R.case("S64G2_GATE_wn_h32_chain_pre")[0]
    assert _plan_code(L, g) == 0 and (g["gate_half"], g["w_ld"]) == (32, 64)
    for change in (dict(gate_half=48, M=96, Cout=48, w_ld=96),    # gate_half % 32 alone, above 32 ...
                   dict(gate_half=16, M=32, Cout=16),             # ... and below
                   dict(Cout=31),                                 # Cout != gate_half
                   dict(M=128, w_ld=128),                         # M != 2 gate_half
                   dict(prologue=R.PRO_ACT1D, alpha_exp=fb["alpha_exp"], beta_inv=fb["beta_inv"], filt=fb["filt"])):
        assert _plan_code(L, g, **change) == L.EINVAL, change
    assert _plan_code(L, g, gate_half=64, M=128, Cout=64, w_ld=128) == 0
    # the same ACT1D operands are accepted on plain rows: the refusal above is the one for gated rows
    p = R.case("S64_INIT_lin_x4_dma16")[0]
    assert _plan_code(L, p, prologue=R.PRO_ACT1D, alpha_exp=fb["alpha_exp"], beta_inv=fb["beta_inv"], filt=fb["filt"]) == 0
    u = R.case("S64_SHUF_up4_clip_both_ends")[0]
    Cu = u["Cout"]
    assert _plan_code(L, u) == 0 and (Cu, u["up"], u["M"], u["w_ld"]) == (11, 4, 44, 44)
    for change in (dict(up=17, M=188, w_ld=188),                  # up > 16 alone: M = 17 Cout + 1 is what up = 17 asks for
                   dict(up=0),
                   dict(M=48, w_ld=48),                           # four padding rows
                   dict(M=40)):                                   # fewer rows than Cout up
        assert _plan_code(L, u, **change) == L.EINVAL, change
    assert 17 * Cu <= 188 <= 17 * Cu + 3 and 16 * Cu == 176
    assert _plan_code(L, u, up=16, M=176, w_ld=176) == 0


def test_direct_refusals(L):
    a = R.case("generic_linear_chain_post")[0]
    fb = R.fake_base()
    for change in (dict(rows=R.ROWS_GATE_WN, gate_half=32), dict(rows=R.ROWS_GATE_GLU, gate_half=32),
                   dict(rows=R.ROWS_SHUFFLE, up=2), dict(w_bs=4), dict(ln_c1=fb["bias"]), dict(split_row=64),
                   dict(prologue=R.PRO_ACT1D), dict(mask=None), dict(Cout=a["M"] + 1), dict(w_ld=a["M"] - 4),
                   dict(stride=0), dict(dil=0), dict(res_ts=2), dict(x=None), dict(B=0)):
        assert _direct_refused(L, a, **change), change
