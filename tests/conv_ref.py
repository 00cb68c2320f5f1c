"""The contract of hsp_conv1d_args (include/hsp.h, "conv:" / "epilogue:") in numpy float64, on the PACKED operands
the two entry points see -- w[K][Cin][w_ld], element strides, the `rows` mode -- plus the seeded case table that
tests/test_conv_ref_host.py (CPU) and tests/test_gpu_conv_contract.py (GPU) both walk.

Nothing here calls the library or a torch module.  An operand is a flat float32 buffer, an element offset into it and
element strides: exactly what the struct carries, with every buffer wider than its view so that batch and channel
strides differ from the dense ones and from one another.  test_conv_ref_host.py pins `conv_contract` against torch's
CPU conv1d / conv_transpose1d in float64 through the packing maps of hip_layers, and checks for every case that the
library's own plan is the tile shape the case id names.

`_evaluate` also states the two fields only the 1x1 token GEMMs take, `ln_c1` (fused input LayerNorm) and `res_ts`
(column stride of the residual); their case table and the two-output form are in tests/tokgemm_ref.py.

Activation1d (HSP_PRO_ACT1D) is the index statement of oracle.hsp_oracle.act1d_closed_form, vectorised and taking the
operands the kernel takes (exp(alpha), 1 / (exp(beta) + 1e-9), the 12 + 12 taps); the host test pins one against the
other.
"""
from __future__ import annotations

import math

import numpy as np

from glue_ref import _erf, softplus

F32, F64 = np.float32, np.float64
SENT = 1234.5          # canary of the output buffers

# enums of include/hsp.h
PRO_NONE, PRO_LRELU, PRO_ACT1D, PRO_SILU = range(4)
ACT_NONE, ACT_TANH, ACT_GELU_TANH, ACT_RELU, ACT_MISH, ACT_SILU, ACT_SOFTPLUS, ACT_GELU_ERF = range(8)
ACT_NAMES = ("none", "tanh", "gelutanh", "relu", "mish", "silu", "softplus", "geluerf")
ROWS_PLAIN, ROWS_GATE_WN, ROWS_GATE_GLU, ROWS_SHUFFLE = range(4)
MASK_NONE, MASK_PRE, MASK_POST, MASK_BOTH = range(4)
MASK_NAMES = ("none", "pre", "post", "both")
EPI_INIT, EPI_VEC, EPI_GATE, EPI_SHUF, EPI_GEN = range(5)
EPI_NAMES = ("INIT", "VEC", "GATE", "SHUF", "GEN")

# tile shapes of csrc/hsp_conv1d_mfma_kernel.h (bottom of the file): name -> (BM, BN)
TILES = dict(M128=(128, 128), M64=(64, 256), M32=(32, 512), M64P=(64, 256), M32P=(32, 512), S64=(64, 64),
             S64G=(64, 128), S32=(32, 128), S64W=(64, 64), S64GW=(64, 128), S64G2=(64, 64))


def _round_up(x, m):
    return (x + m - 1) // m * m


def _sigmoid(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def pointwise_act(v, kind):
    """HSP_ACT_* of include/hsp.h on float64 values (glue_ref.act rounds its argument to fp32 first)."""
    if kind == ACT_NONE:
        return v
    if kind == ACT_TANH:
        return np.tanh(v)
    if kind == ACT_GELU_TANH:
        return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    if kind == ACT_RELU:
        return np.maximum(v, 0.0)
    if kind == ACT_MISH:
        return v * np.tanh(softplus(v))
    if kind == ACT_SILU:
        return v * _sigmoid(v)
    if kind == ACT_SOFTPLUS:
        return softplus(v)
    if kind == ACT_GELU_ERF:
        return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------ operand views
def view(a, name, shape, strides):
    """float64 copy of the strided view ``name`` of the args dict (buffer a[name], offset a[name + '_off'])."""
    buf = np.asarray(a[name], F32)
    idx = np.full(shape, int(a.get(name + "_off", 0)), np.int64)
    for ax, (n, s) in enumerate(zip(shape, strides)):
        sh = [1] * len(shape)
        sh[ax] = n
        idx = idx + (np.arange(n, dtype=np.int64) * int(s)).reshape(sh)
    assert idx.min() >= 0 and idx.max() < buf.size, (name, shape, strides)
    return buf.astype(F64)[idx], idx


def act1d(x, alpha_exp, beta_inv, filt):
    """DownSample2x(SnakeBeta(UpSample2x(x))) along the last axis of [B, C, L], replicate-padded at both ends:
    up[2q] = 2 sum_i x[q - 3 + i] fu[11 - 2i], up[2q + 1] = 2 sum_i x[q - 2 + i] fu[10 - 2i] (i < 6, indices clamped),
    a = up + beta_inv sin(up alpha_exp)^2, y[n] = sum_k fd[k] a[clamp(2n + k - 5)] -- act1d_closed_form of the oracle."""
    x = np.asarray(x, F64)
    L = x.shape[-1]
    fu, fd = np.asarray(filt[:12], F32).astype(F64), np.asarray(filt[12:], F32).astype(F64)
    ea = np.asarray(alpha_exp, F32).astype(F64)[None, :, None]
    bi = np.asarray(beta_inv, F32).astype(F64)[None, :, None]
    q = np.arange(L)
    e = sum(x[..., np.clip(q - 3 + i, 0, L - 1)] * fu[11 - 2 * i] for i in range(6)) * 2.0
    o = sum(x[..., np.clip(q - 2 + i, 0, L - 1)] * fu[10 - 2 * i] for i in range(6)) * 2.0
    up = np.empty(x.shape[:-1] + (2 * L,), F64)
    up[..., 0::2], up[..., 1::2] = e, o
    a2 = up + bi * np.sin(up * ea) ** 2
    return sum(fd[k] * a2[..., np.clip(2 * q + k - 5, 0, 2 * L - 1)] for k in range(12))


def _prologue(a, x, absolute):
    if absolute:
        return np.abs(x)                      # |lrelu(x)| <= |x|: the linear cases carry NONE or LRELU only
    p = a["prologue"]
    if p == PRO_LRELU:
        return np.where(x > 0, x, x * float(F32(a["slope"])))
    if p == PRO_SILU:
        return x * _sigmoid(x)
    if p == PRO_ACT1D:
        return act1d(x, a["alpha_exp"], a["beta_inv"], a["filt"])
    assert p == PRO_NONE
    return x


def _evaluate(a, absolute=False):
    """-> (y buffer after the call as float64, bool mask of the elements the call writes)."""
    B, Cin, Lin, K, M, ncols = a["B"], a["Cin"], a["Lin"], a["K"], a["M"], a["ncols"]
    Cout, Lout, stride, dil, pad = a["Cout"], a["Lout"], a["stride"], a["dil"], a["pad"]
    fix = np.abs if absolute else (lambda v: v)
    x, _ = view(a, "x", (B, Cin, Lin), (a["x_bs"], a["x_cs"], a["x_ts"]))
    xin = _prologue(a, x, absolute)
    # zero padding applies to prologue(x): positions outside [0, Lin) are 0 whatever the prologue makes of 0
    lo = pad
    hi = max(0, (ncols - 1) * stride + (K - 1) * dil - pad - (Lin - 1))
    xp = np.zeros((B, Cin, lo + Lin + hi), F64)
    xp[:, :, lo:lo + Lin] = xin
    w, _ = view(a, "w", (B, K, Cin, M), (a.get("w_bs", 0), Cin * a["w_ld"], a["w_ld"], 1))
    w = fix(w)
    acc = np.zeros((B, M, ncols), F64)
    for j in range(K):
        xs = xp[:, :, j * dil: j * dil + (ncols - 1) * stride + 1: stride]
        acc += np.matmul(w[:, j].transpose(0, 2, 1), xs)
    if a.get("ln_c1") is not None:
        # fused input LayerNorm of the 1x1 token GEMMs, as the header writes it: column mean and biased variance over the
        # Cin inputs, rstd = 1 / sqrt(var + ln_eps), acc <- rstd (acc - mean ln_c1[row])
        assert K == 1 and pad == 0 and stride == 1 and a["prologue"] == PRO_NONE
        c1 = fix(view(a, "ln_c1", (M,), (1,))[0])
        mean, var = x.mean(axis=1), x.var(axis=1)
        rstd = 1.0 / np.sqrt(var + float(F32(a["ln_eps"])))
        mean = fix(mean)
        acc = rstd[:, None, :] * (acc + mean[:, None, :] * c1[None, :, None] * (1.0 if absolute else -1.0))

    rows = a["rows"]
    gated = rows in (ROWS_GATE_WN, ROWS_GATE_GLU)
    nb = 2 * a["gate_half"] if gated else Cout              # bias / cbias hold one value per channel of the un-packed layer
    bias = fix(view(a, "bias", (nb,), (1,))[0]) if a.get("bias") is not None else np.zeros(nb)
    cb = fix(view(a, "cbias", (B, nb), (a["cbias_bs"], 1))[0]) if a.get("cbias") is not None else np.zeros((B, nb))
    add = bias[None, :] + cb                                  # [B, nb]
    if gated:
        H = a["gate_half"]
        m = np.arange(M)
        blk = m >> 5                                          # 32-row blocks alternate a, b (hip_layers.gated_rows)
        co_m, is_b = (blk >> 1) * 32 + (m & 31), (blk & 1).astype(bool)
        va = np.zeros((B, H, ncols), F64)
        vb = np.zeros((B, H, ncols), F64)
        va[:, co_m[~is_b]] = acc[:, ~is_b] + add[:, co_m[~is_b], None]
        vb[:, co_m[is_b]] = acc[:, is_b] + add[:, H + co_m[is_b], None]
        if absolute:
            v = va + vb
        else:
            v = (np.tanh(va) if rows == ROWS_GATE_WN else va) * _sigmoid(vb)
        co_i = np.arange(Cout)[:, None] + np.zeros((1, ncols), np.int64)
        to_i = np.zeros((Cout, 1), np.int64) + np.arange(ncols)[None, :]
        ok = np.ones((Cout, ncols), bool)
    elif rows == ROWS_SHUFFLE:
        up = a["up"]
        m = np.arange(M)
        co_m, ph = m // up, m % up
        rowok = co_m < Cout
        v = acc + np.where(rowok, add[:, np.minimum(co_m, Cout - 1)], 0.0)[:, :, None]
        co_i = co_m[:, None] + np.zeros((1, ncols), np.int64)
        to_i = up * np.arange(ncols)[None, :] + ph[:, None] - a["shuf_pad"]
        ok = rowok[:, None] & (to_i >= 0) & (to_i < Lout)
    else:
        assert rows == ROWS_PLAIN
        v = acc[:, :Cout] + add[:, :, None]
        co_i = np.arange(Cout)[:, None] + np.zeros((1, ncols), np.int64)
        to_i = np.zeros((Cout, 1), np.int64) + np.arange(ncols)[None, :]
        ok = np.ones((Cout, ncols), bool)
    if not gated and not absolute:
        v = pointwise_act(v, a["act"])

    co_c, to_c = np.where(ok, co_i, 0), np.where(ok, to_i, 0)
    bI = np.arange(B)[:, None, None]
    mm = a["mask_mode"]
    mk = None
    if mm != MASK_NONE:
        mfull, _ = view(a, "mask", (B, Lout), (a["mask_bs"], 1))
        mk = fix(mfull)[bI, to_c[None]]
    if mm & MASK_PRE:
        v = v * mk
    if a.get("cscale") is not None:
        cs = fix(view(a, "cscale", (B, Cout), (a["cscale_bs"], 1))[0])
        v = v * cs[bI, co_c[None]]
    v = v * abs(float(F32(a["scale"]))) if absolute else v * float(F32(a["scale"]))
    if a.get("res") is not None:
        r, _ = view(a, "res", (B, Cout, Lout), (a["res_bs"], a["res_cs"], max(1, a.get("res_ts", 1))))   # res_ts: 0 or 1 = unit
        v = v + fix(r)[bI, co_c[None], to_c[None]]
    if mm & MASK_POST:
        v = v * mk
    yv, yidx = view(a, "y", (B, Cout, Lout), (a["y_bs"], a["y_cs"], 1))
    if a["accumulate"]:
        v = v + fix(yv)[bI, co_c[None], to_c[None]]
    v = v * abs(float(F32(a["post_scale"]))) if absolute else v * float(F32(a["post_scale"]))
    out = np.asarray(a["y"], F32).astype(F64).copy()
    written = np.zeros(out.shape, bool)
    okb = np.broadcast_to(ok[None], v.shape)
    flat = yidx[bI, co_c[None], to_c[None]][okb]
    assert len(np.unique(flat)) == len(flat), "two rows of the launch write one output element"
    out[flat] = v[okb]
    written[flat] = True
    return out, written


def conv_contract(a):
    """The y BUFFER after the call, float64: elements the contract does not write keep their value."""
    return _evaluate(a)[0]


def conv_written(a):
    """Which elements of the y buffer the contract writes."""
    return _evaluate(a, absolute=True)[1]


def conv_contract_abs(a):
    """The same formula with every operand replaced by its absolute value and act = identity (gates: |a| + |b| rows
    summed): the error scale of the derived bound."""
    return _evaluate(a, absolute=True)[0]


def is_linear(a):
    return a["act"] == ACT_NONE and a["rows"] in (ROWS_PLAIN, ROWS_SHUFFLE) and a["prologue"] in (PRO_NONE, PRO_LRELU)


def derived_bound(a):
    """Per element: 2 (Cin K + 8) 2^-24 conv_contract_abs -- the forward error of an fp32 sum of Cin K products plus at
    most eight epilogue operations in any order, with a factor 2."""
    return 2.0 * (a["Cin"] * a["K"] + 8) * 2.0 ** -24 * conv_contract_abs(a)


# ------------------------------------------------------------------------------------------------ predicates (restated)
def _al16(a, name):
    """16-B addressability of an operand: every buffer is allocated 16-B aligned (both tests assert it)."""
    return a.get(name + "_off", 0) % 4 == 0


def epilogue_kind(a):
    """select_epilogue of csrc/hsp_conv1d_mfma_kernel.h and the ACT1D rule of dispatch() in hsp_conv1d_mfma.hip."""
    if a["rows"] in (ROWS_GATE_WN, ROWS_GATE_GLU):
        return EPI_GATE
    pointwise = a["act"] != ACT_NONE or a["mask_mode"] != MASK_NONE or a.get("cscale") is not None
    has_res, has_cb = a.get("res") is not None, a.get("cbias") is not None
    if a["rows"] == ROWS_SHUFFLE:
        epi = EPI_SHUF if not (pointwise or has_cb or has_res or a["accumulate"]) else EPI_GEN
    elif not pointwise and float(F32(a["scale"])) == 1.0:
        epi = EPI_INIT
    else:
        vec = (a["ncols"] % 4 == 0 and _al16(a, "y") and a["y_bs"] % 4 == 0 and a["y_cs"] % 4 == 0 and
               (not has_res or (_al16(a, "res") and a["res_bs"] % 4 == 0 and a["res_cs"] % 4 == 0)) and
               (a["mask_mode"] == MASK_NONE or (_al16(a, "mask") and a["mask_bs"] % 4 == 0)))
        epi = EPI_VEC if vec else EPI_GEN
    if a["prologue"] == PRO_ACT1D and epi != EPI_INIT:
        epi = EPI_GEN
    return epi


def xvec(a):
    """The 16-B window DMA: window_dma16 of hsp_conv1d_mfma_kernel.h; the 4-B one otherwise."""
    return (a["prologue"] != PRO_ACT1D and a["x_ts"] == 1 and a["Lin"] % 4 == 0 and a["x_cs"] % 4 == 0 and
            a["x_bs"] % 4 == 0 and _al16(a, "x"))


# what tells two shapes of one (BM, BN) apart: name -> (gated rows, ACT1D prologue, halo (K - 1) dil + 3 > 64), None =
# either.  dispatch() of hsp_conv1d_mfma.hip and supported<>() of hsp_conv1d_tile.hip (M64 / M32 exist with the
# ACT1D prologue only, M64P / M32P without it only; gated rows exist on M128, S64G, S64GW and S64G2 only)
TILE_RULES = dict(M128=(None, None, False), M64=(False, True, False), M64P=(False, False, False), M32=(False, True, False),
                  M32P=(False, False, False), S32=(False, None, False), S64=(False, None, False), S64W=(False, None, True),
                  S64G=(True, False, False), S64GW=(True, False, True), S64G2=(True, False, False))

# the tile shapes (Cfg<>) at the bottom of hsp_conv1d_mfma_kernel.h: name -> (producer waves NPW, window row pitch XWP = BN + slack)
TILE_CFG = dict(M128=(4, 192), M64=(8, 320), M32=(8, 576), M64P=(4, 320), M32P=(4, 576), S64=(4, 128), S64G=(4, 192),
                S32=(4, 192), S64W=(4, 192), S64GW=(4, 256), S64G2=(4, 128))


def tile_of(a, bm, bn):
    """The one tile shape of (BM, BN) whose TILE_RULES the case meets."""
    have = (a["rows"] in (ROWS_GATE_WN, ROWS_GATE_GLU), a["prologue"] == PRO_ACT1D, (a["K"] - 1) * a["dil"] + 3 > 64)
    hit = [n for n, s in TILES.items() if s == (bm, bn) and
           all(want is None or want == h for want, h in zip(TILE_RULES[n], have))]
    assert len(hit) == 1, (a["id"], bm, bn, hit)
    return hit[0]


def lds_bytes(tile, a, kc):
    """Dynamic LDS of a launch of ``tile`` at chunk depth kc: make_plan of hsp_conv1d_mfma_kernel.h -- two weight
    slabs K kc BM, two windows kc XWP and, under ACT1D, one scratch per producer wave.  The fourth number of
    hsp_conv1d_mfma_plan; it depends on the shape's pitch and producer count, which (BM, BN) alone do not give."""
    (bm, bn), (npw, xwp) = TILES[tile], TILE_CFG[tile]
    K, xw = a["K"], bn + (a["K"] - 1) * a["dil"]
    rpw = -(-kc // npw)
    scr = 2 * rpw * _round_up(xw + 10, 64) + _round_up(2 * xw + 10, 4) if a["prologue"] == PRO_ACT1D else 0
    return 4 * (2 * K * kc * bm + 2 * kc * xwp + npw * scr)


def tail_schedule(a, tile):
    """`tail` of launch_one (hsp_conv1d_mfma_kernel.h): the narrow last column tile of the 128 x 128 INIT shape."""
    n_nt = -(-a["ncols"] // 128)
    rem = a["ncols"] - (n_nt - 1) * 128
    return tile == "M128" and epilogue_kind(a) == EPI_INIT and a["prologue"] != PRO_ACT1D and n_nt >= 2 and rem <= 32


def linear_vec_fast(a):
    """linear_vec_fast of csrc/hsp_conv1d_direct.hip."""
    return (a["K"] == 1 and a["Lin"] == 1 and a["Lout"] == 1 and a["stride"] == 1 and a["pad"] == 0 and
            64 <= a["Cin"] <= 1024 and a["Cout"] >= 64)


def cout1_fast(a):
    """cout1_fast of csrc/hsp_conv1d_direct.hip."""
    K = a["K"]
    return (a["Cout"] == 1 and a["stride"] == 1 and a["dil"] == 1 and K <= 9 and K % 2 == 1 and a["pad"] == (K - 1) // 2 and
            a["x_ts"] == 1 and a["Lin"] == a["Lout"] and a["Lin"] % 4 == 0 and a["x_cs"] % 4 == 0 and a["x_bs"] % 4 == 0 and
            a["y_bs"] % 4 == 0 and _al16(a, "x") and _al16(a, "y") and a["prologue"] == PRO_NONE and
            a.get("cbias") is None and a.get("cscale") is None and a.get("res") is None and not a["accumulate"] and
            a["mask_mode"] == MASK_NONE and a["Cin"] * K <= 4096)


def direct_kernel(a):
    """Which of the three kernels hsp_conv1d_direct_f32 launches (the order in that entry point)."""
    return "linear_vec" if linear_vec_fast(a) else ("cout1" if cout1_fast(a) else "generic")


# ------------------------------------------------------------------------------------------------ packing (restated)
def pack_plain(W, M):
    """W [Cout, Cin, K] -> w[K][Cin][M], rows beyond Cout zero."""
    cout, cin, k = W.shape
    w = np.zeros((k, cin, M), F32)
    w[:, :, :cout] = W.transpose(2, 1, 0)
    return w


def pack_gated(W):
    """W [2H, Cin, K] (a half then b half) -> w[K][Cin][2H] in 32-row blocks a, b, a, b, ..."""
    H = W.shape[0] // 2
    m = np.arange(2 * H)
    src = ((m >> 5) & 1) * H + (m >> 6) * 32 + (m & 31)
    return np.ascontiguousarray(W[src].transpose(2, 1, 0))


def pack_convtr(Wt, up):
    """Wt [Cin, Cout, k] of a ConvTranspose1d(stride = up) -> (w[K'][Cin][M], K', M): packed row m = co up + r and tap j'
    hold source tap r + (K' - 1 - j') up, absent taps and the rows beyond Cout up are zero."""
    cin, cout, k = Wt.shape
    kp, M = -(-k // up), _round_up(cout * up, 4)
    w = np.zeros((kp, cin, M), F32)
    for m in range(cout * up):
        co, r = divmod(m, up)
        for jp in range(kp):
            tap = r + (kp - 1 - jp) * up
            if tap < k:
                w[jp, :, m] = Wt[:, co, tap]
    return w, kp, M


# ------------------------------------------------------------------------------------------------ the case table
def _c(id, tile=None, **kw):
    return dict(id=id, tile=tile, **kw)


FULL = dict(bias=True, cbias=True, cscale=True, res=True, accumulate=True, scale=0.75, post_scale=0.5)   # + act + mask
LONG = 16385          # 129 column tiles of 128: the first length past `short_seq` at B = 1 and M <= 128


def _mfma_specs():
    s = []
    # ---- plain shapes x INIT / VEC / SHUF / GEN.  Short sequences: S32 (M <= 32), S64, S64W (halo (K-1) dil + 3 > 64)
    short = (("S32", dict(Cout=30, Cin=5)), ("S64", dict(Cout=37, Cin=12)),
             ("S64W", dict(Cout=68, Cin=12, K=11, dil=7, L=132)))
    long_ = (("M32P", dict(Cout=6, Cin=5, B=1, L=LONG + 3)), ("M64P", dict(Cout=36, Cin=5, B=1, L=LONG + 3)),
             ("M128", dict(Cout=68, Cin=8, B=1, L=LONG + 35)))
    for tile, kw in short + long_:
        L = kw.get("L", 70)
        s.append(_c(f"{tile}_INIT_res_acc_cbias_ps", tile, **dict(kw, bias=True, cbias=True, res=True, accumulate=True,
                                                                   post_scale=0.5, L=L)))
        s.append(_c(f"{tile}_VEC_chain_both_tanh", tile, **dict(kw, **FULL, act=ACT_TANH, mask_mode=MASK_BOTH,
                                                                 L=_round_up(L, 4))))
        s.append(_c(f"{tile}_GEN_chain_both_none", tile, **dict(kw, **FULL, mask_mode=MASK_BOTH, L=_round_up(L, 4) + 1)))
    # ConvTranspose (SHUFFLE rows): kt = transposed kernel, tp = its padding
    for tile, kw in (("S32", dict(Cout=7, up=4, kt=8, tp=2)), ("S64", dict(Cout=12, up=5, kt=11, tp=3)),
                     ("S64W", dict(Cout=18, up=2, kt=140, tp=1, L=40)),
                     ("M32P", dict(Cout=4, up=2, kt=4, tp=1, B=1, L=LONG, Cin=5)),
                     ("M64P", dict(Cout=5, up=8, kt=16, tp=4, B=1, L=LONG, Cin=5)),
                     ("M128", dict(Cout=24, up=3, kt=7, tp=2, B=1, L=LONG, Cin=5))):
        s.append(_c(f"{tile}_SHUF_up{kw['up']}", tile, **dict(kw, rows=ROWS_SHUFFLE, bias=True, scale=0.75, post_scale=0.5)))
    s += [
        _c("S64_SHUF_up2_lrelu_clip", "S64", rows=ROWS_SHUFFLE, Cout=22, up=2, kt=4, tp=1, bias=True, prologue=PRO_LRELU),
        _c("S64_SHUF_up4_clip_both_ends", "S64", rows=ROWS_SHUFFLE, Cout=11, up=4, kt=9, tp=3, bias=True),
        _c("S32_SHUF_up3_rows_not_x4", "S32", rows=ROWS_SHUFFLE, Cout=3, up=3, kt=7, tp=2, bias=True),
        _c("S64_SHUFGEN_up4_res_acc_relu", "S64", rows=ROWS_SHUFFLE, Cout=11, up=4, kt=8, tp=2, bias=True, res=True,
           accumulate=True, act=ACT_RELU, cbias=True, post_scale=0.5),
        _c("S64_SHUFGEN_up5_res", "S64", rows=ROWS_SHUFFLE, Cout=12, up=5, kt=11, tp=3, bias=True, res=True, scale=0.75),
        # padding rows (Cout up not a multiple of 4) on the other two routes: the 8-B vector stores, and the scalar
        # epilogue with bias, cbias and cscale all read at co = m / up
        _c("S32_SHUF_up2_odd_cout_pad_rows", "S32", rows=ROWS_SHUFFLE, Cout=7, up=2, kt=4, tp=1, bias=True, scale=0.75),
        _c("S64_SHUFGEN_up3_cscale_cbias_pad_rows", "S64", rows=ROWS_SHUFFLE, Cout=11, up=3, kt=7, tp=2, bias=True,
           cbias=True, cscale=True, mask_mode=MASK_BOTH, scale=0.75),
    ]
    # ---- the 128 x 128 narrow-tail schedule from both sides: ncols % 128 = 1, 32 (tail) and 33 (no tail)
    for rem in (1, 32, 33):
        s.append(_c(f"M128_INIT_tail_rem{rem}", "M128", Cout=68, Cin=8, B=1, L=LONG - 1 + rem, bias=True, res=True))
    # ---- ACT1D prologue: INIT and GEN on every shape that carries it
    for tile, kw in (("S32", dict(Cout=30, Cin=5)), ("S64", dict(Cout=37, Cin=12)),
                     ("S64W", dict(Cout=37, Cin=12, K=11, dil=7, L=132)),
                     ("M32", dict(Cout=6, Cin=5, B=1, L=LONG + 3)), ("M64", dict(Cout=36, Cin=5, B=1, L=LONG + 3)),
                     ("M128", dict(Cout=68, Cin=8, B=1, L=LONG + 35))):
        s.append(_c(f"{tile}_INIT_act1d", tile, **dict(kw, prologue=PRO_ACT1D, bias=True, res=True)))
        s.append(_c(f"{tile}_GEN_act1d_tanh", tile, **dict(kw, prologue=PRO_ACT1D, bias=True, act=ACT_TANH, post_scale=0.5)))
    s.append(_c("S64_INIT_act1d_L7", "S64", Cout=37, Cin=12, L=7, prologue=PRO_ACT1D, bias=True))
    s.append(_c("S32_GEN_act1d_L7", "S32", Cout=30, Cin=5, L=7, prologue=PRO_ACT1D, bias=True, scale=0.75))
    # ---- gated rows: S64G2 (<= 48 tiles of 64 x 128), S64G above, S64GW (wide halo), M128 (long)
    gfull = dict(bias=True, cbias=True, cscale=True, res=True, scale=0.75, post_scale=0.5, accumulate=True)
    for tile, kw in (("S64G2", dict(H=32, Cin=12)), ("S64G2", dict(H=96, Cin=40)),
                     ("S64G", dict(H=96, Cin=12, B=3, L=1100)), ("S64GW", dict(H=32, Cin=12, K=5, dil=16, L=140)),
                     ("M128", dict(H=32, Cin=8, B=1, L=LONG + 3))):
        for rows, nm in ((ROWS_GATE_WN, "wn"), (ROWS_GATE_GLU, "glu")):
            mm = MASK_BOTH if rows == ROWS_GATE_WN else MASK_POST
            s.append(_c(f"{tile}_GATE_{nm}_h{kw['H']}_chain_{MASK_NAMES[mm]}", tile, **dict(kw, rows=rows, mask_mode=mm, **gfull)))
    s.append(_c("S64G2_GATE_wn_h32_chain_pre", "S64G2", H=32, Cin=12, rows=ROWS_GATE_WN, mask_mode=MASK_PRE, **gfull))
    s.append(_c("S64G2_GATE_glu_h32_chain_none", "S64G2", H=32, Cin=12, rows=ROWS_GATE_GLU, **gfull))
    s.append(_c("S64G2_GATE_wn_h64_lrelu", "S64G2", H=64, Cin=12, rows=ROWS_GATE_WN, prologue=PRO_LRELU, bias=True))
    # ---- the full pointwise chain per mask mode on VEC and GEN, and every activation once on each
    acts_a = (ACT_TANH, ACT_GELU_TANH, ACT_RELU, ACT_MISH)
    acts_b = (ACT_NONE, ACT_SILU, ACT_SOFTPLUS, ACT_GELU_ERF)
    for mm in range(4):
        for epi, L in (("VEC", 72), ("GEN", 73)):
            s.append(_c(f"S64_{epi}_chain_{MASK_NAMES[mm]}_{ACT_NAMES[acts_a[mm]]}", "S64", Cout=37, L=L, **FULL,
                        act=acts_a[mm], mask_mode=mm))
            s.append(_c(f"S32_{epi}_{ACT_NAMES[acts_b[mm]]}_{MASK_NAMES[mm]}", "S32", Cout=30, Cin=5, L=L, bias=True,
                        act=acts_b[mm], mask_mode=mm, scale=0.75, res=True))
    # ---- VEC <-> GEN: the same case on both sides of each documented condition
    vb = dict(Cout=40, L=72, **FULL, mask_mode=MASK_POST)
    s += [_c("S64_VEC_boundary_base", "S64", **vb), _c("S64_GEN_boundary_y_off1", "S64", **vb, y_shift=1),
          _c("S64_GEN_boundary_mask_bs_odd", "S64", **vb, mask_bs_odd=True),
          _c("S64_GEN_boundary_res_off1", "S64", **vb, res_shift=1),
          _c("S64_GEN_boundary_ncols_4n1", "S64", **dict(vb, L=73))]
    # ---- ragged rows, columns and windows (scale 0.75 without an activation: VEC when everything is 16-B addressable)
    lin = dict(bias=True, scale=0.75)
    s += [
        _c("S64_VEC_cin40_cout130", "S64", Cout=130, Cin=40, L=72, **lin),          # three row tiles, the last with 2 rows
        _c("S64_INIT_lin_mod4_dma4", "S64", Cout=40, L=70, bias=True),               # Lin % 4 != 0: 4-B window DMA
        _c("S64_INIT_lin_x4_dma16", "S64", Cout=40, L=72, bias=True),
        _c("S64_INIT_x_off1_dma4", "S64", Cout=40, L=72, bias=True, x_shift=1),
        _c("S64_INIT_x_transposed", "S64", Cout=40, L=72, bias=True, x_layout="t"),
        _c("S32_GEN_x_transposed_lrelu", "S32", Cout=30, Cin=5, L=71, prologue=PRO_LRELU, x_layout="t", **lin),
        _c("S64_GEN_L3_k11_d5", "S64", Cout=40, L=3, K=11, dil=5, **lin),
        _c("S64_INIT_pad0_lout_lt_lin", "S64", Cout=40, L=70, K=5, pad=0, bias=True),
        _c("S64_VEC_even_k_lout_lin1", "S64", Cout=40, L=71, K=4, pad=2, **lin),
        _c("S64_GEN_pad_beyond_halo", "S64", Cout=40, L=69, K=3, pad=5, **lin),
        _c("S64_VEC_lrelu_two_col_tiles", "S64", Cout=40, L=132, prologue=PRO_LRELU, **lin),
        _c("S64_INIT_rows_r4", "S64", Cout=40, L=70, r0=4, Cfull=100, bias=True, res=True),
        _c("S64_VEC_rows_r64", "S64", Cout=36, L=72, r0=64, Cfull=100, **lin),
        _c("S64_INIT_w_bs_b3", "S64", Cout=40, L=70, B=3, w_bs=True, bias=True, res=True),
        _c("S32_VEC_w_bs_b3", "S32", Cout=30, Cin=5, L=72, B=3, w_bs=True, **lin),
    ]
    return s


def _chunk_specs():
    """MFMA cases that stage at least three chunks (every case of _mfma_specs stages one, its ACT1D ones at Cin = 12 two):
    the producers' "stage c + 1 while c is multiplied" with its buffer flip, the consumers' fragment pipeline across the
    chunk barrier, the ACT1D raw-row look-ahead to c + 2.  test_conv_ref_host.py reads each case's chunk depth from the
    library's plan.  (Behind the direct cases in SPECS: a case's seed is its index there.)"""
    lin = dict(bias=True, scale=0.75)
    gfull = dict(bias=True, cbias=True, cscale=True, res=True, scale=0.75, post_scale=0.5, accumulate=True)
    return [
        _c("S64_INIT_chunks3_fast", "S64", Cin=192, Cout=64, L=72, bias=True, res=True),   # full row tile, Cin % KC == 0
        _c("S64_VEC_chunks3_cin_tail", "S64", Cin=136, Cout=40, L=72, **lin),              # partial row tile, 8-channel tail
        _c("S64_GEN_chunks3_dma4", "S64", Cin=136, Cout=40, L=73, **lin),                  # the same on the 4-B window DMA
        _c("S64_INIT_act1d_chunks3", "S64", Cin=20, Cout=37, L=72, prologue=PRO_ACT1D, bias=True, res=True),
        _c("S64G2_GATE_wn_h32_chunks3", "S64G2", H=32, Cin=136, L=72, rows=ROWS_GATE_WN, mask_mode=MASK_BOTH, **gfull),
        _c("M128_INIT_chunks3_tail_rem1", "M128", Cin=40, Cout=68, B=1, L=LONG, bias=True, res=True),
        _c("M128_INIT_act1d_chunks3", "M128", Cin=20, Cout=68, B=1, L=LONG + 35, prologue=PRO_ACT1D, bias=True, res=True),
    ]


def _direct_specs():
    chain = dict(FULL, mask_mode=MASK_BOTH, act=ACT_GELU_TANH)
    s = [
        _c("generic_stride2_dil2_chain", Cout=7, Cin=9, L=61, K=5, dil=2, stride=2, pad=4, **chain),
        _c("generic_stride4_dil2_cin1", Cout=10, Cin=1, L=64, K=9, dil=2, stride=4, pad=8, bias=True, mask_mode=MASK_PRE),
        _c("generic_lrelu_cin9_cout_lt_m", Cout=6, Cin=9, L=33, K=3, prologue=PRO_LRELU, bias=True, scale=0.75),
        _c("generic_silu_x_transposed", Cout=5, Cin=9, L=33, K=3, prologue=PRO_SILU, x_layout="t", bias=True, res=True),
        _c("generic_linear_chain_post", Cout=6, Cin=17, L=40, K=3, **dict(FULL, mask_mode=MASK_POST)),
    ]
    for K, Cin, L, kw in ((1, 1, 4, {}), (3, 4, 1024, {}), (5, 6, 1028, {}),
                          (7, 6, 2052, dict(act=ACT_TANH, scale=0.75, post_scale=0.5)), (9, 4, 2052, {}), (7, 1, 1028, {})):
        s.append(_c(f"cout1_k{K}_cin{Cin}_l{L}" + ("_tanh" if kw else ""), Cout=1, Cin=Cin, L=L, K=K, B=3, bias=True, **kw))
    nb = dict(Cout=1, Cin=6, B=3, bias=True, scale=0.75, post_scale=0.5)
    s += [_c("cout1_base_k7_l1028", K=7, L=1028, **nb),
          _c("generic_cout1_l_mod4_1", K=7, L=1029, **nb), _c("generic_cout1_x_off1", K=7, L=1028, x_shift=1, **nb),
          _c("generic_cout1_res", K=7, L=1028, res=True, **nb), _c("generic_cout1_k11", K=11, L=1028, **nb)]
    lv = dict(K=1, L=1, bias=True)
    s += [
        _c("linear_vec_cin64_cout64_b1", Cin=64, Cout=64, B=1, **lv),
        _c("linear_vec_cin100_cout65_b8_silu", Cin=100, Cout=65, B=8, prologue=PRO_SILU, cbias=True, cscale=True, **lv),
        _c("linear_vec_cin1000_cout200_b9_lrelu", Cin=1000, Cout=200, B=9, prologue=PRO_LRELU, res=True, accumulate=True,
           post_scale=0.5, **lv),
        _c("linear_vec_cin1024_cout65_b17_chain", Cin=1024, Cout=65, B=17, cbias=True, cscale=True, res=True,
           accumulate=True, scale=0.75, post_scale=0.5, act=ACT_SILU, **lv),
        _c("linear_vec_cin100_cout200_b17", Cin=100, Cout=200, B=17, scale=0.75, **lv),
        _c("generic_linear_cin63", Cin=63, Cout=64, B=9, scale=0.75, **lv),
        _c("generic_linear_cout63", Cin=64, Cout=63, B=9, scale=0.75, **lv),
        _c("generic_linear_cin1025", Cin=1025, Cout=64, B=2, scale=0.75, **lv),
    ]
    for c in s:
        c["entry"] = "direct"
    return s


SPECS = _mfma_specs() + _direct_specs() + _chunk_specs()
for _i, _s in enumerate(SPECS):
    _s.setdefault("entry", "mfma")
    _s["seed"] = 5000 + _i
assert len({s["id"] for s in SPECS}) == len(SPECS)
IDS = [s["id"] for s in SPECS]

MASK_VALUES = np.array([0.0, 0.25, 0.5, 1.0], F32)


def _wide(r, shape, sl, fill=None):
    """A buffer of ``shape`` and (offset, strides) of its sub-view ``sl`` (one slice per axis), in elements."""
    buf = r.standard_normal(shape).astype(F32) if fill is None else np.full(shape, fill, F32)
    strides = [int(np.prod(shape[i + 1:])) for i in range(len(shape))]
    off = sum(s.start * st for s, st in zip(sl, strides))
    return buf, off, strides


def build(spec):
    """The args dict of one case: every field of hsp_conv1d_args the case sets, device pointers replaced by (flat float32
    buffer, element offset).  Also 'layer_w' / 'layer_b': the un-packed torch-layout parameters the packed ones came from."""
    s = dict(B=2, Cin=12, L=70, K=3, dil=1, stride=1, rows=ROWS_PLAIN, prologue=PRO_NONE, act=ACT_NONE,
             mask_mode=MASK_NONE, scale=1.0, post_scale=1.0, accumulate=False, bias=False, cbias=False, cscale=False,
             res=False, x_layout="d", x_shift=0, y_shift=0, res_shift=0, mask_bs_odd=False, r0=0, w_bs=False)
    s.update(spec)
    r = np.random.default_rng(s["seed"])
    B, Cin, Lin, rows = s["B"], s["Cin"], s["L"], s["rows"]
    a = dict(id=s["id"], entry=s["entry"], tile=s["tile"], B=B, Cin=Cin, Lin=Lin, dil=s["dil"], stride=s["stride"],
             rows=rows, prologue=s["prologue"], slope=0.1, act=s["act"], mask_mode=s["mask_mode"], scale=s["scale"],
             post_scale=s["post_scale"], accumulate=int(s["accumulate"]), gate_half=0, up=0, shuf_pad=0, w_off=0, w_bs=0)
    gated = rows in (ROWS_GATE_WN, ROWS_GATE_GLU)
    # ---- weights: torch-layout layer parameters, then packed
    if rows == ROWS_SHUFFLE:
        up, kt, tp, Cout = s["up"], s["kt"], s["tp"], s["Cout"]
        Wt = (r.standard_normal((Cin, Cout, kt)) / math.sqrt(Cin * -(-kt // up))).astype(F32)
        w, K, M = pack_convtr(Wt, up)
        a.update(K=K, M=M, w_ld=M, pad=K - 1, up=up, shuf_pad=tp, Cout=Cout, Lout=(Lin - 1) * up - 2 * tp + kt)
        a["ncols"] = (a["Lout"] - 1 + tp) // up + 1
        a["layer_w"], nb = Wt, Cout
    else:
        K = s["K"]
        pad = s.get("pad", (K - 1) * s["dil"] // 2)
        Cl = 2 * s["H"] if gated else s.get("Cfull", s["Cout"])              # channels of the un-packed layer
        nW = B if s["w_bs"] else 1
        W = (r.standard_normal((nW, Cl, Cin, K)) / math.sqrt(Cin * K)).astype(F32)
        w_ld = Cl if gated else _round_up(Cl, 4)
        w = np.stack([pack_gated(Wb) if gated else pack_plain(Wb, w_ld) for Wb in W])
        Cout = s["H"] if gated else s["Cout"]
        M = 2 * s["H"] if gated else (w_ld if not s["r0"] and "Cfull" not in s else _round_up(Cout, 4))
        Lout = (Lin + 2 * pad - s["dil"] * (K - 1) - 1) // s["stride"] + 1
        a.update(K=K, M=M, w_ld=w_ld, pad=pad, Cout=Cout, Lout=Lout, ncols=Lout, gate_half=s["H"] if gated else 0,
                 w_off=s["r0"], w_bs=K * Cin * w_ld if s["w_bs"] else 0)
        a["layer_w"], nb = (W if s["w_bs"] else W[0]), Cl
    a["w"] = np.ascontiguousarray(w).reshape(-1)
    Cout, Lout = a["Cout"], a["Lout"]
    bs_used, cs_used = set(), set()

    def fresh(used, v, step):
        while v in used:
            v += step
        used.add(v)
        return v
    # ---- x: [B, Cin, Lin] inside [B, Cin + 1, x_cs] (16-B addressable unless shifted), or the transposed view
    if s["x_layout"] == "t":
        ts = Cin + 3
        buf, off, st = _wide(r, (B, Lin + 2, ts), (slice(0, B), slice(1, Lin + 1), slice(2, Cin + 2)))
        a.update(x=buf.reshape(-1), x_off=off, x_bs=st[0], x_cs=1, x_ts=ts)
        bs_used.add(st[0])
    else:
        xcs = fresh(cs_used, _round_up(Lin, 4) + 8, 4)
        c0 = 4 + s["x_shift"]
        buf, off, st = _wide(r, (B, Cin + 1, xcs), (slice(0, B), slice(0, Cin), slice(c0, c0 + Lin)))
        a.update(x=buf.reshape(-1), x_off=off, x_bs=st[0], x_cs=xcs, x_ts=1)
        bs_used.add(st[0])
    # ---- y: [B, Cout, Lout] inside a canary buffer [B, 1 + Cout + 4, y_cs], 16 (+ shift) canary columns in front
    ycs = fresh(cs_used, _round_up(Lout, 4) + 48, 4)
    c0 = 16 + s["y_shift"]
    sl = (slice(0, B), slice(1, Cout + 1), slice(c0, c0 + Lout))
    rows_y = Cout + 5
    while rows_y * ycs in bs_used:
        rows_y += 1
    ybuf, off, st = _wide(r, (B, rows_y, ycs), sl, fill=SENT)
    bs_used.add(st[0])
    if s["accumulate"]:
        ybuf[sl] = r.standard_normal((B, Cout, Lout)).astype(F32)
    guard = 64
    a.update(y=np.concatenate([np.full(guard, SENT, F32), ybuf.reshape(-1), np.full(guard, SENT, F32)]),
             y_off=off + guard, y_bs=st[0], y_cs=ycs)
    if s["res"]:
        rcs = fresh(cs_used, _round_up(Lout, 4) + 12, 4)
        c0 = 4 + s["res_shift"]
        rows_r = Cout + 1
        while rows_r * rcs in bs_used:
            rows_r += 1
        buf, off, st = _wide(r, (B, rows_r, rcs), (slice(0, B), slice(0, Cout), slice(c0, c0 + Lout)))
        bs_used.add(st[0])
        a.update(res=buf.reshape(-1), res_off=off, res_bs=st[0], res_cs=rcs)
    if s["mask_mode"] != MASK_NONE:
        mbs = _round_up(Lout, 4) + 8 + (1 if s["mask_bs_odd"] else 0)
        while mbs in bs_used:
            mbs += 4
        bs_used.add(mbs)
        a.update(mask=r.choice(MASK_VALUES, (B, mbs)).astype(F32).reshape(-1), mask_off=4, mask_bs=mbs)
    if s["bias"]:
        bfull = r.standard_normal(nb + 8).astype(F32)
        a.update(bias=bfull, bias_off=s["r0"])
        a["layer_b"] = bfull[:nb]
    if s["cbias"]:
        ncb = 2 * s["H"] if gated else Cout
        cbs = fresh(bs_used, ncb + 3, 1)
        a.update(cbias=r.standard_normal((B, cbs)).astype(F32).reshape(-1), cbias_off=2, cbias_bs=cbs)
    if s["cscale"]:
        css = fresh(bs_used, Cout + 5, 1)
        a.update(cscale=r.standard_normal((B, css)).astype(F32).reshape(-1), cscale_off=1, cscale_bs=css)
    if s["prologue"] == PRO_ACT1D:
        from megatts2_hierspeechpp_amd.synth import kaiser_sinc_filter12
        h = kaiser_sinc_filter12()
        al, be = r.uniform(-1.0, 1.0, Cin), r.uniform(-1.0, 1.0, Cin)
        a.update(alpha_exp=np.exp(al).astype(F32), beta_inv=(1.0 / (np.exp(be) + 1e-9)).astype(F32),
                 filt=np.concatenate([h, h]).astype(F32), alpha_log=al.astype(F32), beta_log=be.astype(F32))
    strides_b = [a[k] for k in ("x_bs", "y_bs", "res_bs", "mask_bs", "cbias_bs", "cscale_bs") if k in a]
    assert len(set(strides_b)) == len(strides_b), (s["id"], strides_b)
    return a


_CACHE = {}


def case(id):
    """(args, reference y buffer, written mask) of a case, computed once per process and never modified."""
    if id not in _CACHE:
        a = build(SPECS[IDS.index(id)])
        ref, written = _evaluate(a)
        ref.setflags(write=False)
        written.setflags(write=False)
        _CACHE[id] = (a, ref, written)
    return _CACHE[id]


# ------------------------------------------------------------------------------------------------ the struct
POINTERS = ("x", "w", "y", "bias", "cbias", "mask", "cscale", "res", "alpha_exp", "beta_inv", "filt")


def to_struct(a, base):
    """hsp_conv1d_args of a case.  ``base``: operand name -> address of its buffer's first element ('zeros' included);
    the struct gets base + 4 * offset.  Used with device addresses by the GPU test and with made-up 16-B aligned ones by
    the host test (hsp_conv1d_mfma_plan and the refusals read no memory)."""
    from megatts2_hierspeechpp_amd import _lib as L
    s = L.Conv1dArgs()
    for name in POINTERS:
        if a.get(name) is not None:
            assert base[name] % 16 == 0, name
            setattr(s, name, base[name] + 4 * int(a.get(name + "_off", 0)))
    s.zeros = base["zeros"]
    for k in ("x_bs", "x_cs", "x_ts", "B", "Cin", "Lin", "K", "M", "dil", "pad", "stride", "w_ld", "y_bs", "y_cs", "Cout",
              "Lout", "ncols", "prologue", "slope", "rows", "gate_half", "up", "shuf_pad", "act", "mask_mode", "scale",
              "accumulate", "post_scale", "w_bs"):
        setattr(s, k, a[k])
    for k in ("cbias_bs", "mask_bs", "cscale_bs", "res_bs", "res_cs"):
        if k in a:
            setattr(s, k, a[k])
    return s


def fake_base():
    return dict({n: 0x100000 * (i + 1) for i, n in enumerate(POINTERS)}, zeros=0x100000 * 20)
