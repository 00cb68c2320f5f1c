"""The contract of hsp_dftseg_args (include/hsp.h, "frequency-domain form of a long dilated Conv1d") in numpy float64,
one statement per entry point -- fwd_contract (hsp_dftseg_fwd_f32), inv_contract (hsp_dftseg_inv_f32), pair_contract
(hsp_dftseg_pair_f32) -- plus the seeded case table that tests/test_dftseg_ref_host.py (CPU) and
tests/test_gpu_dftseg_contract.py (GPU) both walk.

Nothing here calls the library or hip_layers.  An operand is a flat float32 buffer, an element offset into it and element
strides: what the struct carries.  Every buffer is wider than its view (x_bs, x_cs, y_bs, y_cs, res_bs, res_cs and
xf_bs > 2 C Np all differ from the dense strides) and has a guard band on both sides; output buffers are filled with
the sentinel SENT, so whatever the contract does not write must keep those bits.

The geometry the kernels derive on the host (ds_geom / dp_geom of csrc/hsp_dftseg.hip: rows per item, chunking, the
one-or-two operand buffers of the inverse) is restated at the bottom: the case ids name what a case exercises and the host
test checks those claims against the restatement.
"""
from __future__ import annotations

import numpy as np

from conv_ref import act1d

F32, F64 = np.float32, np.float64
SENT = 1234.5
GUARD = 64
DS_N = 128


def hop_of(k):
    return DS_N - (k - 1)


def nseg_of(L, k, d):
    return -(-(-(-L // d)) // hop_of(k))


# ------------------------------------------------------------------------------------------------ operand views
def _rows_idx(a, name, B, C, L):
    idx = (int(a[name + "_off"]) + np.arange(B)[:, None, None] * int(a[name + "_bs"]) +
           np.arange(C)[None, :, None] * int(a[name + "_cs"]) + np.arange(L)[None, None, :])
    assert idx.min() >= 0 and idx.max() < a[name].size, name
    return idx


def rows(a, name):
    """float64 copy of the [B][C][L] view ``name`` (x, y, res) and its indices into the flat buffer."""
    idx = _rows_idx(a, name, a["B"], a["C"], a["L"])
    return np.asarray(a[name], F32).astype(F64)[idx], idx


def _spec_idx(a):
    """indices [64][2 C][B d nseg] of the spectrum columns a launch reads / writes (the padding columns up to Np are not)"""
    C, Np, n = a["C"], a["Np"], a["B"] * a["dil"] * a["nseg"]
    idx = (int(a["xf_off"]) + np.arange(64)[:, None, None] * int(a["xf_bs"]) + np.arange(2 * C)[None, :, None] * Np +
           np.arange(n)[None, None, :])
    assert idx.min() >= 0 and idx.max() < a["xf"].size
    return idx


# ------------------------------------------------------------------------------------------------ the three contracts
def _activate(a, x):
    """Activation1d in front of the transform (act_*), row b cut to act_len[b] (clamped to [1, L]) and zero from there on."""
    if a.get("act_alpha_exp") is None:
        return x
    if a.get("act_len") is None:
        return act1d(x, a["act_alpha_exp"], a["act_beta_inv"], a["act_filt"])
    out = np.zeros_like(x)
    for b, n in enumerate(a["act_len"]):
        n = int(min(max(int(n), 1), a["L"]))
        out[b:b + 1, :, :n] = act1d(x[b:b + 1, :, :n], a["act_alpha_exp"], a["act_beta_inv"], a["act_filt"])
    return out


def segments(a, xin):
    """[B][C][d][nseg][128]: segment s of phase p holds xpad[p + d (s hop + j)], j < 128, xpad = xin behind `pad` zeros."""
    B, C, L = xin.shape
    d, nseg, hop = a["dil"], a["nseg"], hop_of(a["k"])
    xp = np.zeros((B, C, d * ((nseg - 1) * hop + DS_N)), F64)
    xp[:, :, a["pad"]:a["pad"] + L] = xin
    t = (np.arange(d)[:, None, None] + d * (np.arange(nseg)[None, :, None] * hop + np.arange(DS_N)[None, None, :]))
    return xp[:, :, t]


def spectrum_of(a, xin):
    """xin [B][C][L] float64 -> dense [64][2 C][B d nseg]: row part C + c of bin j = Re / Im of bin j of the 128-point real
    DFT of a segment, column n = (b d + p) nseg + s; slot 0: (DC, Nyquist), or (-E0, -O0) with prod3."""
    seg = segments(a, xin)
    B, C = xin.shape[:2]
    X = np.fft.rfft(seg, axis=-1).transpose(4, 1, 0, 2, 3).reshape(65, C, -1)
    re, im = X.real[:64].copy(), X.imag[:64].copy()
    if a["prod3"]:
        col = lambda v: v.transpose(1, 0, 2, 3).reshape(C, -1)
        re[0], im[0] = -col(seg[..., 0::2].sum(-1)), -col(seg[..., 1::2].sum(-1))
    else:
        im[0] = X.real[64]
    return np.concatenate([re, im], axis=1)


def correlation_of(a, Y):
    """dense spectrum [64][2 C][B d nseg] (slot 0 = DC, Nyquist) -> [B][C][L]: the first hop samples of every segment's
    128-point inverse transform are the outputs t = p + d (s hop + j)."""
    B, C, L, d, nseg, hop = a["B"], a["C"], a["L"], a["dil"], a["nseg"], hop_of(a["k"])
    Z = np.zeros((65, C, Y.shape[2]), np.complex128)
    Z[:64] = Y[:, :C] + 1j * Y[:, C:]
    Z[0] = Y[0, :C]
    Z[64] = Y[0, C:]
    v = np.fft.irfft(Z, n=DS_N, axis=0)[:hop].reshape(hop, C, B, d, nseg)
    return v.transpose(2, 1, 4, 0, 3).reshape(B, C, nseg * hop * d)[:, :, :L]


def _write_spectrum(a, dense):
    out = np.asarray(a["xf"], F32).astype(F64)
    idx = _spec_idx(a)
    written = np.zeros(out.shape, bool)
    out[idx] = dense
    written[idx] = True
    return out, written


def fwd_contract(a):
    """-> (the xf buffer after hsp_dftseg_fwd_f32 as float64, bool mask of what the call writes)."""
    return _write_spectrum(a, spectrum_of(a, _activate(a, rows(a, "x")[0])))


def _corr_bias(a):
    v = correlation_of(a, np.asarray(a["xf"], F32).astype(F64)[_spec_idx(a)])
    if a.get("bias") is not None:
        v = v + np.asarray(a["bias"], F32).astype(F64)[None, :a["C"], None]
    return v


def inv_contract(a):
    """-> (the y buffer after hsp_dftseg_inv_f32, written mask): y = ((corr + bias + res) [+ y]) * post_scale on [0, L)."""
    v = _corr_bias(a)
    if a.get("res") is not None:
        v = v + rows(a, "res")[0]
    yv, yidx = rows(a, "y")
    if a["accumulate"]:
        v = v + yv
    v = v * float(F32(a["post_scale"]))
    out = np.asarray(a["y"], F32).astype(F64)
    written = np.zeros(out.shape, bool)
    out[yidx] = v
    written[yidx] = True
    return out, written


def pair_contract(ai, af):
    """hsp_dftseg_pair_f32: inverse of `ai` + bias -> the activation of `af` -> forward of `af` (its xf buffer)."""
    return _write_spectrum(af, spectrum_of(af, _activate(af, _corr_bias(ai))))


def product(dense, w):
    """The channel product between the transforms, float64: dense [64][2 C][n] in the prod3 = 0 layout, w [C][C][k] ->
    conj(rfft(w, 128)) X per bin (slot 0: W_dc DC, W_nyquist Nyquist)."""
    C = w.shape[0]
    W = np.conj(np.fft.rfft(np.asarray(w, F64), n=DS_N, axis=-1))
    X = dense[:, :C] + 1j * dense[:, C:]
    Y = np.einsum("oij,jin->jon", W[:, :, :64], X)
    out = np.concatenate([Y.real, Y.imag], axis=1)
    out[0, :C] = W[:, :, 0].real @ dense[0, :C]
    out[0, C:] = W[:, :, 64].real @ dense[0, C:]
    return out


# ------------------------------------------------------------------------------------------------ the case table
def _f(id, **kw):
    return dict(id=id, kind="fwd", **kw)


def _i(id, **kw):
    return dict(id=id, kind="inv", **kw)


def _p(id, **kw):
    return dict(id=id, kind="pair", **kw)


PERSIST = dict(B=48, C=768, L=100, k=11, d=1)      # items > 2 x resident workgroups on 256 CUs (host test)
RAGGED = (720, 1, 243, 718, 477)                   # L, 1, three past a 240 boundary, not a multiple of 4, three short of 480

SPECS = [
    # ---- forward: staging paths x dilations x taps x segment grid
    _f("fwd_vec_k11_d1_L472_ongrid", C=40, L=472, k=11, d=1),
    _f("fwd_vec_k7_d3_L800_prod3", C=20, L=800, k=7, d=3, prod3=1),
    _f("fwd_scalar_k11_d5_L333", C=30, L=333, k=11, d=5),
    _f("fwd_scalar_xoff1_k7_d1_L400_prod3", C=36, L=400, k=7, d=1, x_shift=1, prod3=1),
    _f("fwd_vec_k11_d1_L60_one_segment", C=37, L=60, k=11, d=1),
    _f("fwd_scalar_k7_d5_L37_uneven_phases", C=37, L=37, k=7, d=5),
    _f("fwd_vec_k11_d2_L600", C=28, L=600, k=11, d=2),
    _f("fwd_vec_k33_d1_L576_ongrid", C=36, L=576, k=33, d=1),
    _f("fwd_scalar_k63_d1_L301", C=40, L=301, k=63, d=1),
    _f("fwd_act_k11_d1_L800", C=24, L=800, k=11, d=1, act=True),
    _f("fwd_act_k7_d3_L472_prod3", C=22, L=472, k=7, d=3, act=True, prod3=1),
    _f("fwd_act_ragged_k7_d5_L720", B=5, C=16, L=720, k=7, d=5, act=True, act_len=RAGGED),
    _f("fwd_act_ragged_k11_d1_L720_prod3", B=5, C=25, L=720, k=11, d=1, act=True, act_len=RAGGED, prod3=1),
    _f("fwd_act_ragged_chunked_k11_d1_L20000_items_past_end", B=3, C=3, L=20000, k=11, d=1, act=True,
       act_len=(20000, 5000, 17)),
    _f("fwd_chunked_vec_k7_d3_L40000", B=1, C=5, L=40000, k=7, d=3),
    _f("fwd_chunked_scalar_k11_d1_L17501", B=2, C=3, L=17501, k=11, d=1),
    _f("fwd_persistent_k11_d1_L100", **PERSIST),
    # ---- inverse: {res} x {accumulate}, post_scale, bias; immediate (1, 3, 5) and generic (2) scatter; hop on either side
    # of the scatter's uniform tests (k = 33: hop 96, k = 35: hop 94, k = 63: hop 66); vector and scalar epilogue
    _i("inv_vec_k11_d1_L472_ongrid_res_acc_ps3", C=40, L=472, k=11, d=1, res=True, acc=True, ps=1 / 3, bias=True),
    _i("inv_vec_k7_d3_L800_res", C=20, L=800, k=7, d=3, res=True, bias=True),
    _i("inv_scalar_k11_d5_L333_acc", C=30, L=333, k=11, d=5, acc=True),
    _i("inv_scalar_yoff1_k7_d1_L400_ps3", C=36, L=400, k=7, d=1, y_shift=1, ps=1 / 3, bias=True),
    _i("inv_vec_k11_d1_L60_one_segment", C=37, L=60, k=11, d=1, bias=True),
    _i("inv_scalar_k7_d5_L37_uneven_phases_res", C=37, L=37, k=7, d=5, res=True),
    _i("inv_vec_k11_d2_L600_acc", C=28, L=600, k=11, d=2, acc=True, bias=True),
    _i("inv_vec_k33_d1_L576_ongrid", C=36, L=576, k=33, d=1, bias=True),
    _i("inv_vec_k35_d3_L564_ongrid_res", C=20, L=564, k=35, d=3, res=True),
    _i("inv_scalar_k63_d1_L301_res_acc", C=40, L=301, k=63, d=1, res=True, acc=True, bias=True),
    _i("inv_scalar_resoff1_k11_d1_L480", C=24, L=480, k=11, d=1, res=True, res_shift=1, bias=True),
    _i("inv_vec_k11_d1_L800_res_acc", C=20, L=800, k=11, d=1, res=True, acc=True),
    _i("inv_chunked_vec_k7_d3_L40000_res", B=1, C=5, L=40000, k=7, d=3, res=True, bias=True),
    _i("inv_chunked_scalar_k11_d1_L17501_acc_ps3", B=2, C=3, L=17501, k=11, d=1, acc=True, ps=1 / 3, bias=True),
    _i("inv_chunked_vec_k11_d1_L40000", B=1, C=3, L=40000, k=11, d=1),
    _i("inv_persistent_k11_d1_L100_res", **PERSIST, res=True, bias=True),
    # ---- pair: (d1, k) -> (1, k) of the AMP blocks
    _p("pair_k7_d1_L800", C=40, L=800, k=7, d=1, bias=True),
    _p("pair_k7_d3_L720_ragged_prod3", B=5, C=40, L=720, k=7, d=3, bias=True, act_len=RAGGED, prod3=1),
    _p("pair_k7_d5_L472_prod3", C=40, L=472, k=7, d=5, prod3=1),
    _p("pair_k11_d1_L720_ragged", B=5, C=40, L=720, k=11, d=1, act_len=RAGGED),
    _p("pair_k11_d3_L800_prod3", C=40, L=800, k=11, d=3, bias=True, prod3=1),
    _p("pair_k11_d5_L720_ragged", B=5, C=40, L=720, k=11, d=5, bias=True, act_len=RAGGED),
    _p("pair_persistent_k11_d1_L100", **PERSIST, bias=True),
]


def _round_up(x, m):
    return (x + m - 1) // m * m


def _row_buffer(r, B, C, L, shift, extra, fill=None):
    """A [B][C + 1][cs] buffer between two guard bands, the view at column 8 + shift of rows 0 .. C - 1."""
    cs = _round_up(L, 4) + extra
    shape = (B, C + 1, cs)
    body = r.standard_normal(shape).astype(F32) if fill is None else np.full(shape, fill, F32)
    buf = np.concatenate([np.full(GUARD, SENT, F32), body.reshape(-1), np.full(GUARD, SENT, F32)])
    return buf, GUARD + 8 + shift, (C + 1) * cs, cs


def _geometry(s, k, d):
    B, C, L = s["B"], s["C"], s["L"]
    nseg = nseg_of(L, k, d)
    Np = _round_up(B * d * nseg, 4) + 4                       # always some padding columns
    return dict(B=B, C=C, L=L, k=k, dil=d, pad=(k - 1) * d // 2, nseg=nseg, Np=Np, xf_bs=2 * C * Np + 8, xf_off=GUARD,
                accumulate=0, post_scale=1.0, prod3=0)


def _spectrum_buffer(a, r=None):
    """[64][xf_bs] between guard bands: random (an inverse's input, time samples of O(1)) or the sentinel (an output)"""
    n = 64 * a["xf_bs"]
    body = np.full(n, SENT, F32) if r is None else (8.0 * r.standard_normal(n)).astype(F32)
    return np.concatenate([np.full(GUARD, SENT, F32), body, np.full(GUARD, SENT, F32)])


def _act_params(a, s, r):
    from megatts2_hierspeechpp_amd.synth import kaiser_sinc_filter12
    h = kaiser_sinc_filter12()
    al, be = r.uniform(-1.0, 1.0, a["C"]), r.uniform(-1.0, 1.0, a["C"])
    a.update(act_alpha_exp=np.exp(al).astype(F32), act_beta_inv=(1.0 / (np.exp(be) + 1e-9)).astype(F32),
             act_filt=np.concatenate([h, h]).astype(F32))
    if s.get("act_len") is not None:
        a["act_len"] = np.asarray(s["act_len"], np.int64)
        assert a["act_len"].shape == (a["B"],)


def _build_fwd(s, r):
    a = _geometry(s, s["k"], s["d"])
    a["prod3"] = int(s.get("prod3", 0))
    a["x"], a["x_off"], a["x_bs"], a["x_cs"] = _row_buffer(r, a["B"], a["C"], a["L"], s.get("x_shift", 0), 12)
    if s.get("act"):
        _act_params(a, s, r)
    a["xf"] = _spectrum_buffer(a)
    return a


def _build_inv(s, r):
    a = _geometry(s, s["k"], s["d"])
    a["xf"] = _spectrum_buffer(a, r)
    B, C, L = a["B"], a["C"], a["L"]
    if s["kind"] == "inv":
        a["y"], a["y_off"], a["y_bs"], a["y_cs"] = _row_buffer(r, B, C, L, s.get("y_shift", 0), 24, fill=SENT)
        if s.get("acc"):
            a["y"][_rows_idx(a, "y", B, C, L)] = r.standard_normal((B, C, L)).astype(F32)
        if s.get("res"):
            a["res"], a["res_off"], a["res_bs"], a["res_cs"] = _row_buffer(r, B, C, L, s.get("res_shift", 0), 16)
        a["accumulate"], a["post_scale"] = int(bool(s.get("acc"))), float(F32(s.get("ps", 1.0)))
    if s.get("bias"):
        a["bias"] = r.standard_normal(C + 4).astype(F32)
    return a


def build(spec):
    """The args of one case: (inverse args or None, forward args or None); device pointers are (flat float32 buffer, element
    offset) pairs.  The random draws do not depend on prod3 or act_len: variants of a spec share their inputs."""
    s = dict(B=2)
    s.update(spec)
    r = np.random.default_rng(s["seed"])
    if s["kind"] == "fwd":
        return None, _build_fwd(s, r)
    if s["kind"] == "inv":
        return _build_inv(s, r), None
    ai = _build_inv(s, r)
    af = _geometry(s, s["k"], 1)
    af["prod3"] = int(s.get("prod3", 0))
    _act_params(af, s, r)
    af["xf"] = _spectrum_buffer(af)
    return ai, af


def spec_of(id):
    return SPECS[IDS.index(id)]


def evaluate(spec):
    ai, af = build(spec)
    ref, written = {"fwd": lambda: fwd_contract(af), "inv": lambda: inv_contract(ai),
                    "pair": lambda: pair_contract(ai, af)}[spec["kind"]]()
    ref.setflags(write=False)
    written.setflags(write=False)
    return ai, af, ref, written


_CACHE = {}


def case(id):
    """(inverse args, forward args, reference output buffer, written mask), computed once per process, never modified."""
    if id not in _CACHE:
        _CACHE[id] = evaluate(spec_of(id))
    return _CACHE[id]


def output_of(ai, af):
    """(args dict, name) of the buffer a case's launch writes"""
    return (af, "xf") if af is not None else (ai, "y")


# ------------------------------------------------------------------------------------------------ the struct
POINTERS = ("x", "y", "xf", "bias", "res", "act_alpha_exp", "act_beta_inv", "act_filt", "act_len")
SCALARS = ("B", "C", "L", "k", "dil", "pad", "nseg", "Np", "xf_bs", "accumulate", "post_scale", "prod3")


def to_struct(a, base):
    """hsp_dftseg_args of one side of a case.  ``base``: operand name -> address of its buffer's first element (16-B
    aligned), 'dft' the table's; the struct gets base + 4 (8 for act_len) * offset."""
    from megatts2_hierspeechpp_amd import _lib as L
    s = L.DftSegArgs()
    for name in POINTERS:
        if a.get(name) is not None:
            assert base[name] % 16 == 0, name
            setattr(s, name, base[name] + 4 * int(a.get(name + "_off", 0)))
    s.dft = base["dft"]
    for k in SCALARS:
        setattr(s, k, a[k])
    for k in ("x_bs", "x_cs", "y_bs", "y_cs", "res_bs", "res_cs"):
        if k in a:
            setattr(s, k, a[k])
    return s


def fake_base():
    return dict({n: 0x1000000 * (i + 1) for i, n in enumerate(POINTERS)}, dft=0x1000000 * 20)


def run_case(ai, af, device, expect=0):
    """Upload the operands of a case, call its entry point once through the C ABI (hsp_dftseg_inv_f32, hsp_dftseg_fwd_f32,
    or hsp_dftseg_pair_f32 when both sides are given) and return the output buffer as float32."""
    import ctypes

    import torch
    from megatts2_hierspeechpp_amd import _lib as L
    tabs = [np.zeros(4160, F32), np.zeros(4160, F32)]
    assert L.lib().hsp_dftseg_tables_f32(tabs[0].ctypes.data, tabs[1].ctypes.data) == 0
    structs, keep = [], []
    for a, tab in ((ai, tabs[1]), (af, tabs[0])):
        if a is None:
            continue
        dev = {n: torch.from_numpy(np.ascontiguousarray(a[n])).to(device) for n in POINTERS if a.get(n) is not None}
        dev["dft"] = torch.from_numpy(tab).to(device)
        keep.append(dev)
        structs.append(to_struct(a, {n: t.data_ptr() for n, t in dev.items()}))
    lib, st = L.lib(), L.stream_ptr()
    if ai is not None and af is not None:
        code = lib.hsp_dftseg_pair_f32(ctypes.byref(structs[0]), ctypes.byref(structs[1]), st)
    elif af is not None:
        code = lib.hsp_dftseg_fwd_f32(ctypes.byref(structs[0]), st)
    else:
        code = lib.hsp_dftseg_inv_f32(ctypes.byref(structs[0]), st)
    torch.cuda.synchronize()
    assert code == expect, code
    a, name = output_of(ai, af)
    return keep[-1][name].cpu().numpy()


# ------------------------------------------------------------------------------------------------ geometry (restated)
LDS_LIMIT = 160 * 1024
OPERAND = 128 * 32                       # floats of one operand buffer of the inverse
DA_SLICE = 256 + 496


def resident(lds_bytes, cus=256):
    """ds_resident: two workgroups per CU while two footprints fit the 160 KB"""
    return cus * min(2, max(1, LDS_LIMIT // max(lds_bytes, 1)))


def fwd_lds(cg_pitch, act=True):
    return 4 * (cg_pitch + 64 + (32 + 4 * DA_SLICE if act else 0))


def ds_geom(a, inverse, cus=256):
    """ds_geom of csrc/hsp_dftseg.hip -> dict(cg, S, pitch, ngrp, nchunk, bufsz)"""
    hop, d, nseg, C, B = hop_of(a["k"]), a["dil"], a["nseg"], a["C"], a["B"]
    budget = 16384 if inverse else 17408
    row_of = (lambda S: (d * S * hop + 3) & ~3) if inverse else (lambda S: (d * ((S - 1) * hop + DS_N) + 12 + 3) & ~3)
    S = nseg
    if row_of(S) > budget:
        smax = budget // (d * hop) if inverse else ((budget - 15) // d - DS_N) // hop + 1
        smax = max(smax & ~1, 2)
        nch = -(-nseg // smax)
        S = min((-(-nseg // nch) + 1) & ~1, smax)
    pitch = row_of(S)
    cmax = min(max(budget // pitch, 1), 32, C)
    quantum = 32 if inverse else 64
    nchunk = -(-nseg // S)
    best, best_score = cmax, 0.0
    for cg in range(cmax, (cmax + 1) // 2 - 1, -1):
        ncols = cg * d * S
        fill = ncols / (quantum * (-(-ncols // quantum)))
        lds = 4 * (cg * pitch + OPERAND) if inverse else fwd_lds(cg * pitch)
        res, items = resident(lds, cus), B * (-(-C // cg)) * nchunk
        score = fill * (items / ((-(-items // res)) * res))
        if score > best_score + 1e-9:
            best_score, best = score, cg
    return dict(cg=best, S=S, pitch=pitch, ngrp=-(-C // best), nchunk=nchunk, bufsz=(best * pitch + 3) & ~3)


def inv_nbuf(a, cus=256):
    """hsp_dftseg_inv_f32: two 16-KB operand buffers while stretch + both stay within 80 KB (two workgroups per CU)"""
    return 2 if 4 * (ds_geom(a, True, cus)["bufsz"] + 2 * OPERAND) <= 80 * 1024 else 1


def dp_geom(ai, af, cus=256):
    """dp_geom: rows per item and item count of the pair launch (one workgroup per CU)"""
    hop1, hop2 = hop_of(ai["k"]), hop_of(af["k"])
    pA = (ai["dil"] * ai["nseg"] * hop1 + 3) & ~3
    pB = (af["dil"] * ((af["nseg"] - 1) * hop2 + DS_N) + 12 + 3) & ~3
    cg = min((LDS_LIMIT // 4 - 2 * OPERAND - 96) // (pA + pB), 32, ai["C"])
    assert cg >= 1
    res = resident(LDS_LIMIT, cus)
    best, best_score = cg, 0.0
    for c in range(cg, (cg + 1) // 2 - 1, -1):
        n1, n2 = c * ai["dil"] * ai["nseg"], c * af["dil"] * af["nseg"]
        fill = 0.5 * (n1 / (64 * (-(-n1 // 64))) + n2 / (128 * (-(-n2 // 128))))
        items = ai["B"] * (-(-ai["C"] // c))
        score = fill * items / ((-(-items // res)) * res)
        if score > best_score + 1e-9:
            best_score, best = score, c
    return dict(cg=best, ngrp=-(-ai["C"] // best))


def launch_shape(spec, cus=256):
    """(rows per item, items, resident workgroups) of a case's launch"""
    ai, af = build(spec) if spec["id"] not in _CACHE else _CACHE[spec["id"]][:2]
    if spec["kind"] == "pair":
        g = dp_geom(ai, af, cus)
        return g["cg"], ai["B"] * g["ngrp"], resident(LDS_LIMIT, cus)
    a, inverse = (ai, True) if spec["kind"] == "inv" else (af, False)
    g = ds_geom(a, inverse, cus)
    lds = 4 * (g["bufsz"] + inv_nbuf(a, cus) * OPERAND) if inverse else fwd_lds(g["bufsz"], a.get("act_alpha_exp") is not None)
    return g["cg"], a["B"] * g["ngrp"] * g["nchunk"], resident(lds, cus)


for _n, _s in enumerate(SPECS):
    _s["seed"] = 7000 + _n
    if _s["kind"] == "inv":                # which of the two operand-buffer counts the launch takes (at 256 CUs)
        _s["id"] += "_nbuf%d" % inv_nbuf(_geometry(dict(B=2, **_s) if "B" not in _s else _s, _s["k"], _s["d"]))
assert len({s["id"] for s in SPECS}) == len(SPECS)
IDS = [s["id"] for s in SPECS]
ACT_FAMILY = [s["id"] for s in SPECS if s.get("act") or s["kind"] == "pair"]      # through the fused activation
