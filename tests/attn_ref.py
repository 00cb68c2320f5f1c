"""The contracts of hsp_mha_args and hsp_mha_proj_args (include/hsp.h) in numpy float64, on the flat buffers, element
offsets and element strides the structs carry, plus the seeded case table that tests/test_attn_ref_host.py (CPU) and
tests/test_gpu_attn_contract.py (GPU) both walk.

Nothing here calls the library or a torch module.  An operand is a flat float32 buffer that is NaN everywhere except at
the elements (b, c, t) the contract reads (the gaps where a stride exceeds T, the columns wt_ld - M of the weight, the
mask's tail, the dense mask's gap and the keys past key_len[b] are poison); the output buffer holds the canary SENT
everywhere the contract does not write.

    hsp_mha_f32       s[b,h,i,j] = sum_d (qk_scale q[b,hD+d,i]) k[b,hD+d,j]
                                   + sum_d (qk_scale q[b,hD+d,i]) rel_k[j-i+w, d]          for |j - i| <= w
                      s = -1e4 (assigned) where mask_q[b,i] * mask_k[b,j] == 0 or mask_dense[b,i,j] == 0
                      p = softmax_j(s);  o[b,hD+d,i] = sum_j p v[b,hD+d,j] + sum_{|j-i|<=w} p rel_v[j-i+w, d]
    hsp_mha_proj_f32  the same o without masks or window over the keys [0, clamp(key_len[b], 1, Tk)), then
                      y[b,m,i] = ((sum_c wt[m,c] o[b,c,i] + bias[m]) * mask[b,i]) * cscale[b,m] + res[b,m,i]

The derived bound (first order in u = 2^-24, gamma(n) = n u / (1 - n u); no constant comes from the code under test)
------------------------------------------------------------------------------------------------------------------
A dot product of n terms in any order, with or without fused multiply-adds, errs by at most gamma(n) sum |terms|.  The
scaled query is one more rounding and the relative-key term one more addition, so a score errs by
    |ds_ij| <= E_i = max_j gamma(D + 2) (sum_d |scale q_di k_dj| + sum_d |scale q_di rel_k[j-i+w]_d|).
The row maximum m_i is the maximum of the computed scores and only shifts the exponent, so it cancels in the quotient.
An un-normalised weight w_ij = exp(s_ij - m_i) then carries the relative error
    eps_ij = E_i + u (3 |s_ij - m_i| + (C_EXP + 1) n_blk):
the subtraction, the product with log2(e) and that constant's own rounding perturb the argument by 3 u |s - m|, and an
evaluation that walks the keys in blocks reaches the final weight through at most n_blk = ceil(Tk / 64) + 1 exponentials
(64 keys is the smallest block of any kernel; the arguments of the rescale factors telescope to m_i - s_ij) of C_EXP ulp
each plus one multiplication.  C_EXP = 4 is ASSUMED: no accuracy statement for v_exp_f32 / expf was found next to the
compiler the library is built with (both are commonly documented at 1 ulp).
With p = w / sum w,  |dp_ij| <= p_ij (eps_ij + ebar_i),  ebar_i = sum_j p_ij eps_ij, and the P V product adds
gamma(Tk + 2) (sum, the 1 / sum factor, the final product), so that
    |do_id| <= sum_j p_ij (eps_ij + ebar_i + gamma(Tk + 2)) |v_dj|        (+ the same over the window with |rel_v|)
which is the issue's (2 E_i + c_exp(i) + gamma(Tk + 2)) sum_j p_ij |v_dj| with c_exp kept inside the sum, where a key
of negligible weight does not pay for its large argument.  The fused form propagates it:
    |dy_mi| <= (sum_c |wt_mc| |do_ci| + gamma(C + 4) (sum_c |wt_mc o_ci| + |bias_m|)) |mask| |cscale| + u |res| + u |y|.
`derived_bound` returns TWICE these (the slack the conv bound has).  tests/test_attn_ref_host.py admits a case only if
the plain float32 numpy evaluation of the contract stays inside this bound and inside helpers.tol_for.
"""
from __future__ import annotations

import ctypes
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
SENT = 1234.5          # canary of the output buffers
U = 2.0 ** -24
C_EXP = 4.0            # ulp of one exponential: assumed (module docstring)

# hsp_mha_plan kernel ids (include/hsp.h) and the id prefixes that name them
TOK, WHOLE, SLAB, MSTR, ROW, RSTR = range(6)
KERNEL_NAMES = ("TOK", "WHOLE", "SLAB", "MSTR", "ROW", "RSTR")
MASKED_CAPABLE = (WHOLE, SLAB, MSTR, ROW, RSTR)
MHA_POINTERS = ("q", "k", "v", "o", "mask_q", "mask_k", "rel_k", "rel_v", "mask_dense")
PROJ_POINTERS = ("q", "k", "v", "wt", "bias", "mask", "cscale", "res", "y", "key_len")
PROJ_CFG = {"P": (4, 69), "D": (2, 96)}          # the PLM layer and the DiT block


def gamma(n):
    return n * U / (1.0 - n * U)


def _round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ operand views
def index(a, name, shape, strides):
    idx = np.full(shape, int(a.get(name + "_off", 0)), np.int64)
    for ax, (n, s) in enumerate(zip(shape, strides)):
        sh = [1] * len(shape)
        sh[ax] = n
        idx = idx + (np.arange(n, dtype=np.int64) * int(s)).reshape(sh)
    assert idx.min() >= 0 and idx.max() < a[name].size, (a["id"], name, shape, strides)
    return idx


def view(a, name, shape, strides, dt=F64, dead=None):
    """Copy of the strided view ``name`` of the args dict (buffer a[name], offset a[name + '_off']) in ``dt``.  Every
    element of a view is finite; ``dead`` (bool, broadcastable) marks the elements that must be poison and read as 0."""
    v = np.asarray(a[name], F32)[index(a, name, shape, strides)]
    if dead is not None:
        dead = np.broadcast_to(dead, v.shape)
        assert np.isnan(v[dead]).all(), (a["id"], name)
        v = np.where(dead, F32(0), v)
    assert np.isfinite(v).all(), (a["id"], name)
    return v.astype(dt)


def eff(a):
    """(window, force_stream, q_cs, k_cs, v_cs, o_cs) with the struct's defaults applied."""
    w = a.get("window", 0)
    force = w < 0
    w = -(w + 1) if force else w
    cs = [a.get(n + "_cs", 0) or (a["Tq"] if n in ("q", "o") else a["Tk"]) for n in ("q", "k", "v", "o")]
    return (w, force, *cs)


# ------------------------------------------------------------------------------------------------ the softmax core
def _core(a, q, k, v, dt, lens=None, want_bound=False):
    """q [B,H,D,Tq], k / v [B,H,D,Tk] in dt -> o [B,H,D,Tq] (and the first-order bound on it when asked)."""
    B, H, D, Tq, Tk = a["B"], a["H"], a["D"], a["Tq"], a["Tk"]
    w = eff(a)[0]
    qs = q * dt(a["qk_scale"])             # a float32 value in every case of the table
    s = np.matmul(qs.transpose(0, 1, 3, 2), k)                                   # [B,H,Tq,Tk]
    sabs = np.matmul(np.abs(qs).transpose(0, 1, 3, 2), np.abs(k)) if want_bound else None
    rel = a.get("rel_k") is not None
    if rel:
        ii, jj = np.nonzero(np.abs(np.arange(Tk)[None, :] - np.arange(Tq)[:, None]) <= w)
        rk = np.asarray(a["rel_k"], F32).astype(dt).reshape(2 * w + 1, D)
        rv = np.asarray(a["rel_v"], F32).astype(dt).reshape(2 * w + 1, D)
        qe = np.einsum("bhdi,rd->bhir", qs, rk)
        s[:, :, ii, jj] += qe[:, :, ii, jj - ii + w]
        if want_bound:
            sabs[:, :, ii, jj] += np.einsum("bhdi,rd->bhir", np.abs(qs), np.abs(rk))[:, :, ii, jj - ii + w]
    neg = dt(F32(-1e4))
    if a.get("mask_q") is not None:
        mq = np.asarray(a["mask_q"], F32)[:B * Tq].reshape(B, Tq)
        mk = np.asarray(a["mask_k"], F32)[:B * Tk].reshape(B, Tk)
        s = np.where(((mq[:, :, None] * mk[:, None, :]) == 0)[:, None], neg, s)
    if a.get("mask_dense") is not None:
        md = view(a, "mask_dense", (B, Tq, Tk), (a["mask_dense_bs"], Tk, 1), F32)
        s = np.where((md == 0)[:, None], neg, s)
    live = np.ones((B, 1, 1, Tk), bool)
    if lens is not None:
        live = (np.arange(Tk)[None, :] < np.asarray(lens)[:, None])[:, None, None, :]
        s = np.where(live, s, dt(-np.inf))
    m = s.max(axis=-1, keepdims=True)
    e = np.exp(s - m)
    p = e / e.sum(axis=-1, keepdims=True)
    o = np.matmul(v, p.transpose(0, 1, 3, 2))                                    # [B,H,D,Tq]
    if rel:
        pw = np.zeros((B, H, Tq, 2 * w + 1), dt)
        pw[:, :, ii, jj - ii + w] = p[:, :, ii, jj]
        o = o + np.einsum("bhir,rd->bhdi", pw, rv)
    if not want_bound:
        return o
    E = gamma(D + 2) * np.where(live, sabs, 0.0).max(axis=-1, keepdims=True)
    arg = np.where(p > 0, np.abs(np.where(live, s, 0.0) - m), 0.0)
    eps = E + U * (3.0 * arg + (C_EXP + 1.0) * (-(-Tk // 64) + 1))
    pe = p * eps
    W = pe + (pe.sum(axis=-1, keepdims=True) + gamma(Tk + 2)) * p
    bo = np.matmul(np.abs(v), W.transpose(0, 1, 3, 2))
    if rel:
        Ww = np.zeros((B, H, Tq, 2 * w + 1), dt)
        Ww[:, :, ii, jj - ii + w] = W[:, :, ii, jj]
        bo = bo + np.einsum("bhir,rd->bhdi", Ww, np.abs(rv))
    return o, bo


def _qkv(a, dt):
    B, H, D, Tq, Tk = a["B"], a["H"], a["D"], a["Tq"], a["Tk"]
    _, _, qcs, kcs, vcs, _ = eff(a)
    q = view(a, "q", (B, H * D, Tq), (a["q_bs"], qcs, 1), dt).reshape(B, H, D, Tq)
    dead = None
    if a.get("key_len") is not None:           # the keys past key_len[b] are poison and carry no weight
        dead = (np.arange(Tk)[None, :] >= proj_lens(a)[:, None])[:, None, :]
    k = view(a, "k", (B, H * D, Tk), (a["k_bs"], kcs, 1), dt, dead).reshape(B, H, D, Tk)
    v = view(a, "v", (B, H * D, Tk), (a["v_bs"], vcs, 1), dt, dead).reshape(B, H, D, Tk)
    return q, k, v


def _scatter(a, name, vals, idx):
    out = np.asarray(a[name], F32).astype(F64).copy()
    written = np.zeros(out.shape, bool)
    out[idx.reshape(-1)] = vals.reshape(-1)
    written[idx.reshape(-1)] = True
    assert int(written.sum()) == idx.size, (a["id"], "output elements overlap")
    return out, written


def mha_values(a, dt=F64, want_bound=False):
    """[B, H*D, Tq] of the contract in dt (and the bound)."""
    B, C, Tq = a["B"], a["H"] * a["D"], a["Tq"]
    r = _core(a, *_qkv(a, dt), dt, want_bound=want_bound)
    if want_bound:
        return r[0].reshape(B, C, Tq), 2.0 * r[1].reshape(B, C, Tq)
    return r.reshape(B, C, Tq)


def proj_lens(a):
    return None if a.get("key_len") is None else np.clip(np.asarray(a["key_len"], np.int64), 1, a["Tk"])


def proj_values(a, dt=F64, want_bound=False):
    """[B, M, Tq] of the fused contract in dt (and the bound)."""
    B, C, Tq, M = a["B"], a["H"] * a["D"], a["Tq"], a["M"]
    r = _core(a, *_qkv(a, dt), dt, lens=proj_lens(a), want_bound=want_bound)
    o = (r[0] if want_bound else r).reshape(B, C, Tq)
    wt = view(a, "wt", (M, C), (a["wt_ld"], 1), dt)
    opt = lambda n, shape, st: view(a, n, shape, st, dt) if a.get(n) is not None else None
    bias = opt("bias", (M,), (1,))
    mask = opt("mask", (B, Tq), (a.get("mask_bs", 0), 1))
    cs = opt("cscale", (B, M), (a.get("cscale_bs", 0), 1))
    res = opt("res", (B, M, Tq), (a.get("res_bs", 0), a.get("res_cs", 0), a.get("res_ts", 0)))
    y = np.einsum("mc,bci->bmi", wt, o)
    if bias is not None:
        y = y + bias[None, :, None]
    if mask is not None:
        y = y * mask[:, None, :]
    if cs is not None:
        y = y * cs[:, :, None]
    pre = y
    if res is not None:
        y = y + res
    if not want_bound:
        return y
    by = np.einsum("mc,bci->bmi", np.abs(wt), r[1].reshape(B, C, Tq))
    mag = np.einsum("mc,bci->bmi", np.abs(wt), np.abs(o)) + (0.0 if bias is None else np.abs(bias)[None, :, None])
    by = by + gamma(C + 4) * mag
    if mask is not None:
        by = by * np.abs(mask)[:, None, :]
    if cs is not None:
        by = by * np.abs(cs)[:, :, None]
    by = by + U * np.abs(pre) + U * np.abs(y) + (0.0 if res is None else U * np.abs(res))
    return y, 2.0 * by


def out_index(a):
    if a["entry"] == "mha":
        return index(a, "o", (a["B"], a["H"] * a["D"], a["Tq"]), (a["o_bs"], eff(a)[5], 1))
    return index(a, "y", (a["B"], a["M"], a["Tq"]), (a["y_bs"], a["y_cs"], a["y_ts"]))


def out_name(a):
    return "o" if a["entry"] == "mha" else "y"


def contract(a, dt=F64):
    """-> (output buffer after the call, bool mask of the elements the call writes)."""
    vals = mha_values(a, dt) if a["entry"] == "mha" else proj_values(a, dt)
    return _scatter(a, out_name(a), vals.astype(F64), out_index(a))


def derived_bound(a):
    """The bound of the module docstring on every element of the output buffer (0 outside `written`)."""
    _, b = mha_values(a, want_bound=True) if a["entry"] == "mha" else proj_values(a, want_bound=True)
    out = np.zeros(a[out_name(a)].shape, F64)
    out[out_index(a).reshape(-1)] = b.reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------ building a case
def _seed(id):
    return zlib.crc32(id.encode())


_EXTRA = dict(q=(3, 7, 1), k=(0, 0, 2), v=(1, 3, 5), o=(2, 11, 3))      # "own": (offset, batch slack, pitch slack)


def _strides(layout, which, B, C, T):
    """(offset, batch stride, channel stride as the struct holds it) of one operand."""
    if layout == "side4":                      # side by side on the columns of one [C][pitch] matrix, pitch % 4 == 0
        return 0, T, _round_up(B * T, 4) + 4
    if layout == "side1":                      # rows only 4-byte aligned
        return 1, T, (B * T + 3) | 1
    if layout == "own":
        off, bx, cx = _EXTRA[which]
        return off, C * (T + cx) + bx, T + cx
    if layout == "ocs" and which == "o":
        return 0, C * (T + 6) + 2, T + 6
    if layout == "dit":                        # rows [0, C) of a batch-major [B][3 C][T] tensor
        return 0, 3 * C * T, T
    return 0, C * T, 0                         # contiguous, channel stride left to the default


def _place(a, name, vals, layout, fill):
    B, C, T = vals.shape
    off, bs, cs = _strides(layout, name, B, C, T)
    a[name + "_off"], a[name + "_bs"], a[name + "_cs"] = off, bs, cs
    buf = np.full(off + (B - 1) * bs + (C - 1) * (cs or T) + T + 5, fill, F32)
    a[name] = buf
    buf[index(a, name, (B, C, T), (bs, cs or T, 1))] = vals


def _regime(reg, blk, r, q, k, v, H, D, scale):
    """Shapes the logits through channel 0 of every head (module docstring of the host test); the other channels stay
    randn.  1 / scale is a float32, so qk_scale * q is 1 to rounding."""
    if reg == "ctl":
        return
    B, C, Tq = q.shape
    Tk = k.shape[2]
    ch = np.arange(H) * D
    inv = F32(1.0) / F32(scale)
    if reg == "v1":
        v[:] = 1.0
    elif reg == "off":                         # common row offset +-50..200: float64 softmax unchanged
        c = r.uniform(50.0, 200.0, Tq) * np.where(np.arange(Tq) & 1, -1.0, 1.0)
        q[:, ch, :] = (c * inv).astype(F32)[None, None, :]
        k[:, ch, :] = 1.0
    elif reg == "dom":                         # one dominant key
        q[:, ch, :] = inv
        k[:, ch, :] = 0.0
        k[:, ch, (2 * Tk) // 3] = 40.0
    else:                                      # staircase: stairup3 / stairdn3 / stairup30 / stairdn30
        step = float(reg[7:])
        nb = np.arange(Tk) // blk
        lvl = nb if reg[5:7] == "up" else nb.max() - nb
        q[:, ch, :] = inv
        k[:, ch, :] = (step * lvl).astype(F32)[None, None, :]


def _masks(a, kind, r):
    B, Tq, Tk = a["B"], a["Tq"], a["Tk"]
    kinds = kind.split("+")
    if "factor" in kinds or "nonbin" in kinds:
        lq = r.integers(max(1, Tq // 2), Tq + 1, B)
        lk = r.integers(max(1, Tk // 2), Tk + 1, B)
        mq = (np.arange(Tq)[None] < lq[:, None]).astype(F32)          # fully masked query rows past lq
        mk = (np.arange(Tk)[None] < lk[:, None]).astype(F32)
        if B > 1:
            mk[B - 1] = 0.0                                           # a batch row whose keys are all masked
        if "nonbin" in kinds:                                         # 0.5 and -1 are NOT masked: the contract is == 0
            mq = mq * np.where(np.arange(Tq) & 1, F32(0.5), F32(-1.0))[None]
            mk = mk * np.where(np.arange(Tk) % 3 == 0, F32(-1.0), F32(0.5))[None]
        a["mask_q"] = np.concatenate([mq.reshape(-1), np.full(3, np.nan, F32)])
        a["mask_k"] = np.concatenate([mk.reshape(-1), np.full(3, np.nan, F32)])
    dense = [x for x in kinds if x in ("causal", "irreg")]
    if dense:
        if dense[0] == "causal":
            md = (np.arange(Tk)[None, :] <= np.arange(Tq)[:, None] + max(0, Tk - Tq)).astype(F32)[None].repeat(B, 0)
        else:
            md = (r.random((B, Tq, Tk)) > 0.4).astype(F32)
            md[:, Tq // 2] = 0.0                                      # a fully masked row
        if "nonbin" in kinds:
            md = md * np.where(r.random((B, Tq, Tk)) > 0.5, F32(0.5), F32(-1.0))
        a["mask_dense_bs"] = Tq * Tk + (5 if "gap" in kinds else 0)
        a["mask_dense_off"] = 2 if "gap" in kinds else 0
        buf = np.full(a["mask_dense_off"] + B * a["mask_dense_bs"] + 3, np.nan, F32)
        a["mask_dense"] = buf
        buf[index(a, "mask_dense", (B, Tq, Tk), (a["mask_dense_bs"], Tk, 1))] = md


def _build_mha(s):
    r = np.random.default_rng(_seed(s["id"]))
    B, H, D, Tq, Tk = s["B"], s["H"], s["D"], s["Tq"], s["Tk"]
    C = H * D
    scale = float(F32(D ** -0.5))
    a = dict(entry="mha", id=s["id"], B=B, H=H, D=D, Tq=Tq, Tk=Tk, qk_scale=scale, layout=s["lay"], mask=s["mask"],
             reg=s["reg"])
    q, k, v = (r.standard_normal((B, C, T)).astype(F32) for T in (Tq, Tk, Tk))
    _regime(s["reg"], s["blk"], r, q, k, v, H, D, scale)
    for n, t in (("q", q), ("k", k), ("v", v)):
        _place(a, n, t, s["lay"], np.nan)
    _place(a, "o", np.full((B, C, Tq), SENT, F32), s["lay"], SENT)
    w = s["w"]
    if w:
        a["rel_k"] = (r.standard_normal((2 * w + 1) * D) * D ** -0.5).astype(F32)
        a["rel_v"] = (r.standard_normal((2 * w + 1) * D) * D ** -0.5).astype(F32)
    a["window"] = -(w + 1) if s["force"] else w
    if s["mask"]:
        _masks(a, s["mask"], r)
    return a


def _build_proj(s):
    r = np.random.default_rng(_seed(s["id"]))
    H, D = PROJ_CFG[s["cfg"]]
    B, Tq, Tk = s["B"], s["Tq"], s["Tk"]
    C = M = H * D
    scale = float(F32(D ** -0.5))
    a = dict(entry="proj", id=s["id"], B=B, H=H, D=D, Tq=Tq, Tk=Tk, M=M, qk_scale=scale, layout=s["lay"], reg=s["reg"],
             form=s["form"])
    q, k, v = (r.standard_normal((B, C, T)).astype(F32) for T in (Tq, Tk, Tk))
    _regime(s["reg"], 64, r, q, k, v, H, D, scale)
    if s.get("key_len") is not None:
        a["key_len"] = np.asarray(s["key_len"], np.int64)
        assert a["key_len"].shape == (B,)
        dead = np.arange(Tk)[None, :] >= proj_lens(a)[:, None]        # keys past key_len[b]: poison
        k[np.broadcast_to(dead[:, None, :], k.shape)] = np.nan
        v[np.broadcast_to(dead[:, None, :], v.shape)] = np.nan
    for n, t in (("q", q), ("k", k), ("v", v)):
        _place(a, n, t, s["lay"], np.nan)
        if not a[n + "_cs"]:
            a[n + "_cs"] = t.shape[2]                                 # the fused struct has no default
    wide = "wide" in s["opt"]
    a["wt_ld"] = M + 4 if wide else M
    wt = np.full(M * a["wt_ld"] + 3, np.nan, F32)
    a["wt"] = wt
    wt[index(a, "wt", (M, C), (a["wt_ld"], 1))] = (r.standard_normal((M, C)) * C ** -0.5).astype(F32)
    if "bias" in s["opt"]:
        a["bias"] = np.concatenate([(0.1 * r.standard_normal(M)).astype(F32), np.full(3, np.nan, F32)])
    if "mask" in s["opt"]:
        a["mask_bs"] = Tq + 3 if wide else Tq
        a["mask"] = np.full(B * a["mask_bs"] + 3, np.nan, F32)
        mv = (r.random((B, Tq)) > 0.3).astype(F32) * F32(-0.75)       # sign-sensitive, not idempotent
        a["mask"][index(a, "mask", (B, Tq), (a["mask_bs"], 1))] = mv
    if "cscale" in s["opt"]:
        a["cscale_bs"] = M + 1 if wide else M
        a["cscale"] = np.full(B * a["cscale_bs"] + 3, np.nan, F32)
        a["cscale"][index(a, "cscale", (B, M), (a["cscale_bs"], 1))] = r.standard_normal((B, M)).astype(F32)
    form = s["form"]
    if form == "bmt":                          # [B][M][Tq] with a row pitch
        ycs = Tq + 2
        a["y_off"], a["y_bs"], a["y_cs"], a["y_ts"] = 1, M * ycs + 3, ycs, 1
    elif form == "btm":                        # [B][Tq][M]
        a["y_off"], a["y_bs"], a["y_cs"], a["y_ts"] = 0, Tq * M + 5, 1, M
    elif form == "gen":                        # general strides: time stride 3 inside a channel row
        ycs = 3 * Tq + 1
        a["y_off"], a["y_bs"], a["y_cs"], a["y_ts"] = 2, M * ycs + 1, ycs, 3
    else:                                      # "last": Tq = 1, a [M][B] matrix with a pitch
        assert Tq == 1
        a["y_off"], a["y_bs"], a["y_cs"], a["y_ts"] = 0, 1, B + 2, 1
    n = a["y_off"] + (B - 1) * a["y_bs"] + (M - 1) * a["y_cs"] + (Tq - 1) * a["y_ts"] + 1 + 4
    a["y"] = np.full(n, SENT, F32)
    if "res" in s["opt"] or "inplace" in s["opt"]:
        rv = r.standard_normal((B, M, Tq)).astype(F32)
        if "inplace" in s["opt"]:              # res == y: the residual is read where the output goes
            a["res"], a["res_is_y"] = a["y"], True
            a["res_off"], a["res_bs"], a["res_cs"], a["res_ts"] = a["y_off"], a["y_bs"], a["y_cs"], a["y_ts"]
            a["y"][out_index(a)] = rv
        else:                                  # its own strides: the PLM's last layer reads it at column stride T
            rts = 1 if form != "last" else 7
            rcs = Tq * rts + 3
            a["res_off"], a["res_bs"], a["res_cs"], a["res_ts"] = 3, M * rcs + 2, rcs, rts
            a["res"] = np.full(3 + B * a["res_bs"] + 4, np.nan, F32)
            a["res"][index(a, "res", (B, M, Tq), (a["res_bs"], rcs, rts))] = rv
    return a


# ------------------------------------------------------------------------------------------------ the case table
SPECS = []


def _m(id, B, H, D, Tq, Tk, lay="contig", mask="", reg="ctl", w=0, force=False, blk=64):
    SPECS.append(dict(entry="mha", id=id, B=B, H=H, D=D, Tq=Tq, Tk=Tk, lay=lay, mask=mask, reg=reg, w=w, force=force,
                      blk=blk))


def _p(id, cfg, B, Tq, Tk, key_len=None, opt=("bias", "mask", "cscale", "res"), form="bmt", lay="contig", reg="ctl"):
    SPECS.append(dict(entry="proj", id=("%s%s_" % (cfg, "kl" if key_len is not None else "")) + id, cfg=cfg, B=B, Tq=Tq,
                      Tk=Tk, key_len=key_len, opt=tuple(opt), form=form, lay=lay, reg=reg))


REGS = ("off", "stairup3", "stairdn3", "stairup30", "stairdn30", "dom", "v1")
LAYS = ("side4", "side1", "own", "ocs")

# ---- TOK <1..3>: no mask, no window, 4 <= Tk <= 256, D <= 96 (key blocks of 32, PV groups of 8)
for n, (D, Tq, Tk, lay) in enumerate([(20, 1, 4, "contig"), (32, 15, 5, "side4"), (33, 16, 7, "side1"),
                                      (64, 17, 8, "own"), (69, 31, 9, "ocs"), (96, 32, 31, "contig"),
                                      (20, 33, 32, "side1"), (64, 33, 33, "side4"), (69, 17, 255, "side1"),
                                      (96, 33, 256, "own"), (69, 33, 45, "side4"), (20, 16, 12, "own")]):
    _m("TOK%d_d%d_tq%d_tk%d_%s" % ((D + 31) // 32, D, Tq, Tk, lay), 3 if Tk < 200 else 2, 2, D, Tq, Tk, lay)
for n, reg in enumerate(REGS):
    D, Tk = ((69, 255), (96, 130), (20, 97), (64, 256))[n % 4]
    _m("TOK%d_d%d_tk%d_%s" % ((D + 31) // 32, D, Tk, reg), 2, 2, D, 33, Tk, ("contig", "side1")[n % 2], reg=reg, blk=32)

# ---- MFMA_WHOLE <1..4>: masked, or D in 97 .. 128, or fewer than 4 keys, or more than 256 (64-key V pitch)
for D, Tq, Tk, lay, mask in [(20, 17, 1, "contig", ""), (33, 15, 2, "side1", "factor"), (69, 16, 3, "side4", ""),
                             (97, 31, 63, "own", ""), (128, 33, 65, "side1", ""), (128, 32, 64, "ocs", "factor"),
                             (97, 33, 100, "side4", "causal"), (20, 33, 63, "own", "irreg+gap"),
                             (64, 17, 65, "side1", "factor+irreg"), (69, 33, 64, "contig", "factor+causal+gap"),
                             (32, 31, 70, "side4", "nonbin"), (32, 33, 257, "contig", ""),
                             (64, 16, 33, "ocs", "nonbin+irreg")]:
    _m("WHOLE%d_d%d_tq%d_tk%d_%s_%s" % ((D + 31) // 32, D, Tq, Tk, lay, mask or "nomask"), 3, 2, D, Tq, Tk, lay, mask)
for n, reg in enumerate(REGS):
    D = (128, 97, 20, 64, 69)[n % 5]
    _m("WHOLE%d_d%d_%s" % ((D + 31) // 32, D, reg), 2, 2, D, 33, 150, ("contig", "side1")[n % 2],
       "factor" if D <= 96 else "", reg)

# ---- MFMA_SLAB <1..4>: whole-V above 160 KB (NDB 3, 4), or above 80 KB with more than 256 workgroups (NDB 1, 2)
_m("SLAB4_d128_tq33_tk300_contig", 2, 1, 128, 33, 300)
_m("SLAB4_d97_tq17_tk320_side1_factor", 2, 1, 97, 17, 320, "side1", "factor")
_m("SLAB3_d69_tq33_tk300_side4_causal", 2, 2, 69, 33, 300, "side4", "causal")
_m("SLAB3_d96_tq31_tk321_own_factor+irreg+gap", 2, 1, 96, 31, 321, "own", "factor+irreg+gap")
_m("SLAB2_d64_tq300_tk270_contig", 13, 2, 64, 300, 270)
_m("SLAB2_d33_tq65_tk300_ocs_factor", 43, 2, 33, 65, 300, "ocs", "factor")
_m("SLAB1_d32_tq300_tk270_side1", 13, 2, 32, 300, 270, "side1")
_m("SLAB1_d20_tq65_tk257_own_nonbin+causal", 43, 2, 20, 65, 257, "own", "nonbin+causal")
for n, reg in enumerate(REGS):
    D = (128, 69)[n % 2]
    _m("SLAB%d_d%d_%s" % ((D + 31) // 32, D, reg), 1, 2, D, 33, 300, ("contig", "side4")[n % 2], reg=reg)

# ---- MFMA_STREAM <1..4>: forced (window = -1), and naturally where the slab no longer fits (128-key blocks)
for D, Tq, Tk, lay, mask in [(20, 17, 127, "contig", ""), (64, 33, 128, "side1", "factor"), (69, 31, 129, "side4", "causal"),
                             (128, 33, 257, "own", "factor+irreg"), (97, 16, 1, "ocs", ""), (33, 15, 3, "side1", "nonbin"),
                             (96, 1, 130, "contig", "irreg+gap")]:
    _m("MSTR%d_d%d_tq%d_tk%d_%s_%s" % ((D + 31) // 32, D, Tq, Tk, lay, mask or "nomask"), 2, 2, D, Tq, Tk, lay, mask,
       force=True)
_m("MSTR4_d128_tq17_tk870_natural", 1, 1, 128, 17, 870)
for n, reg in enumerate(REGS):
    D = (128, 20, 69, 64)[n % 4]
    _m("MSTR%d_d%d_%s" % ((D + 31) // 32, D, reg), 1, 2, D, 33, 400, ("contig", "side1")[n % 2],
       "factor" if n % 3 == 1 else "", reg, force=True, blk=128)

# ---- ROW (mha_kernel): a window at any D <= 256, no window at D in 129 .. 256
for D, T, w, lay, mask in [(20, 17, 4, "contig", "factor"), (64, 33, 4, "side1", ""), (129, 16, 2, "side4", "causal"),
                           (160, 31, 10, "own", "factor+irreg+gap"), (256, 15, 4, "ocs", ""), (64, 3, 4, "contig", ""),
                           (20, 70, 4, "side4", "nonbin")]:
    _m("ROW%d_d%d_t%d_w%d_%s_%s" % ((D + 127) // 128, D, T, w, lay, mask or "nomask"), 2, 2, D, T, T, lay, mask, w=w)
for D, Tq, Tk, lay, mask in [(129, 17, 1, "contig", ""), (256, 16, 2, "side1", ""), (129, 33, 65, "own", "factor"),
                             (256, 15, 100, "side4", "irreg"), (200, 32, 3, "ocs", "factor+causal")]:
    _m("ROW2_d%d_tq%d_tk%d_%s_%s" % (D, Tq, Tk, lay, mask or "nomask"), 2, 1, D, Tq, Tk, lay, mask)
for n, reg in enumerate(REGS):
    D, w = ((64, 4), (160, 0), (20, 4), (256, 0))[n % 4]
    _m("ROW%d_d%d_w%d_%s" % ((D + 127) // 128, D, w, reg), 1, 2, D, 33 if w == 0 else 150, 150,
       ("contig", "side1")[n % 2], reg=reg, w=w)

# ---- ROW_STREAM (mha_stream_kernel): forced, and naturally at D = 256 with ~1 800 keys (256-key blocks)
for D, T, w, lay, mask in [(20, 255, 4, "contig", "factor"), (64, 256, 4, "side1", ""), (160, 257, 3, "side4", "causal"),
                           (129, 513, 4, "own", ""), (64, 3, 4, "ocs", ""), (256, 17, 2, "contig", "factor+irreg+gap")]:
    _m("RSTR%d_d%d_t%d_w%d_%s_%s" % ((D + 127) // 128, D, T, w, lay, mask or "nomask"), 1, 2, D, T, T, lay, mask, w=w,
       force=True)
SPECS[-6:] = [dict(s, B=2) for s in SPECS[-6:]]
_m("RSTR2_d129_tq17_tk300_nowin_nonbin", 2, 1, 129, 17, 300, "side1", "nonbin", force=True)
_m("RSTR2_d256_tq17_tk1800_natural", 1, 1, 256, 17, 1800)
for n, reg in enumerate(REGS):
    D, w = ((64, 4), (160, 0), (256, 0), (20, 4))[n % 4]
    _m("RSTR%d_d%d_w%d_%s" % ((D + 127) // 128, D, w, reg), 1, 1, D, 33 if w == 0 else 600, 600,
       ("contig", "side4")[n % 2], "factor" if n % 3 == 2 else "", reg, w=w, force=True, blk=256)

# ---- hsp_mha_proj_f32: MpCfg<4, 69> ("P", two key splits per head) and <2, 96> ("D", four), 64-key groups
for n, (Tq, Tk) in enumerate([(1, 4), (15, 5), (16, 63), (17, 64), (33, 65), (15, 128), (16, 255), (17, 256),
                              (33, 257), (1, 515)]):
    for cfg in "PD":
        lay = ("contig", "side4", "side1", "dit", "own")[(n + (cfg == "D")) % 5]
        _p("tq%d_tk%d_%s" % (Tq, Tk, lay), cfg, 2, Tq, Tk, lay=lay, form=("bmt", "btm", "gen")[n % 3])
# key_len below 1, below 4, above Tk and on the 64-key group edges; rows most of whose key splits see no key
for cfg in "PD":
    _p("edges_tk70", cfg, 9, 17, 70, key_len=[-3, 0, 1, 3, 63, 64, 65, 70, 79])
    _p("edges_tk515_side1", cfg, 5, 16, 515, key_len=[5, 64, 515, 129, 257], lay="side1")
    _p("edges_tk300_plm", cfg, 4, 15, 300, key_len=[300, 1, 65, 4], lay="side4", opt=("bias", "res"))
# each optional operand NULL alone, all four NULL; wide strides; output forms; res == y
for n, drop in enumerate(("bias", "mask", "cscale", "res", "all")):
    opt = () if drop == "all" else tuple(x for x in ("bias", "mask", "cscale", "res") if x != drop)
    _p("no_%s" % drop, "PD"[n % 2], 2, 17, 70, opt=opt, key_len=[70, 33] if n % 2 else None)
for cfg in "PD":
    _p("wide_strides", cfg, 3, 17, 100, opt=("bias", "mask", "cscale", "res", "wide"), form="gen")
    _p("last_token", cfg, 5, 1, 37, opt=("bias", "res"), form="last", lay="side4")
    _p("inplace_bmt", cfg, 2, 33, 66, opt=("bias", "mask", "cscale", "inplace"))
    _p("inplace_btm_kl", cfg, 3, 16, 130, key_len=[130, 7, 64], opt=("bias", "inplace", "wide"), form="btm")
for cfg in "PD":
    _p("self_t33", cfg, 2, 33, 33, opt=("bias",))
for n, reg in enumerate(REGS):
    for cfg in "PD":
        kl = [515, 70, 200] if (n + (cfg == "D")) % 2 else None
        _p(reg, cfg, 3, 17, 515, key_len=kl, reg=reg, lay=("contig", "side1")[n % 2], opt=("bias", "res"))

# a staircase of 100 per 64-key group whose top group belongs to the LAST key split of a head: the merge of the per-split
# (max, sum, O) must scale by the maximum over ALL splits, or exp(100) overflows (the 30-per-group staircases above
# leave any common reference inside the exponent range, so a merge that forgets one split's maximum survives them)
_p("stairup100_tk128", "P", 2, 17, 128, reg="stairup100", opt=("bias", "res"))
_p("stairup100_tk256", "D", 2, 17, 256, reg="stairup100", opt=("bias", "res"))

IDS = [s["id"] for s in SPECS]
MHA_IDS = [s["id"] for s in SPECS if s["entry"] == "mha"]
PROJ_IDS = [s["id"] for s in SPECS if s["entry"] == "proj"]
assert len(set(IDS)) == len(IDS)
_BY_ID = {s["id"]: s for s in SPECS}
_CACHE = {}


def args(id):
    s = _BY_ID[id]
    return _build_mha(s) if s["entry"] == "mha" else _build_proj(s)


def case(id):
    """-> (args, float64 output buffer after the call, bool mask of the elements the contract writes); computed once
    per process and shared (nobody may change what it returns)."""
    if id not in _CACHE:
        a = args(id)
        ref, written = contract(a)
        _CACHE[id] = (a, ref, written)
    return _CACHE[id]


def named_kernel(id):
    """(kernel id, NDB) an hsp_mha_f32 case id names: 'SLAB3_...' -> (SLAB, 3)."""
    head = id.split("_")[0]
    name = head.rstrip("0123456789")
    return KERNEL_NAMES.index(name), int(head[len(name):])


# ------------------------------------------------------------------------------------------------ ctypes
def fake_base(a=None):
    """Made-up 16-B aligned addresses for calls that never launch (hsp_mha_plan, refusals)."""
    return {n: 0x10000000 * (i + 1) for i, n in enumerate(dict.fromkeys(MHA_POINTERS + PROJ_POINTERS))}


def to_struct(a, base):
    """hsp_mha_args / hsp_mha_proj_args over the ctypes mirrors of _lib.py; base[name] = address of buffer a[name]."""
    from megatts2_hierspeechpp_amd import _lib as L

    def p(n):
        if a.get(n) is None:
            return None
        if n == "res" and a.get("res_is_y"):
            return base["y"] + 4 * a["res_off"]
        return base[n] + (8 if n == "key_len" else 4) * a.get(n + "_off", 0)
    if a["entry"] == "mha":
        s = L.MhaArgs()
        for n in MHA_POINTERS:
            setattr(s, n, p(n))
        for n in ("q_bs", "k_bs", "v_bs", "o_bs", "q_cs", "k_cs", "v_cs", "o_cs", "B", "H", "D", "Tq", "Tk", "window"):
            setattr(s, n, int(a[n]))
        s.qk_scale = a["qk_scale"]
        s.mask_dense_bs = int(a.get("mask_dense_bs", 0))
        return s
    s = L.MhaProjArgs()
    for n in PROJ_POINTERS:
        setattr(s, n, p(n))
    for n in ("q_bs", "q_cs", "k_bs", "k_cs", "v_bs", "v_cs", "B", "H", "D", "Tq", "Tk", "M", "wt_ld", "y_bs", "y_cs", "y_ts"):
        setattr(s, n, int(a[n]))
    for n in ("mask_bs", "cscale_bs", "res_bs", "res_cs", "res_ts"):
        setattr(s, n, int(a.get(n, 0)))
    s.qk_scale = a["qk_scale"]
    s.debug = 0
    return s
