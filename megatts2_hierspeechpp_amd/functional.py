"""Thin Python wrappers (torch tensors in/out) over the pointwise / reduction entry
points of libhsp.so.  No torch arithmetic happens here: every op is one HIP launch."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib as L


def _new_like(x):
    return torch.empty(x.shape, dtype=torch.float32, device=x.device)


def _c(x: torch.Tensor) -> torch.Tensor:
    return x if x.is_contiguous() else x.contiguous()


def _lengths(lengths, B=None):
    """Row lengths as the kernels read them -- device int64 [B], contiguous -- or None (NULL: every row is whole).
    Without ``B`` the tensor is cast and compacted as needed; with ``B`` it must already be so (checked, never copied:
    the launches of the vocoder's row-exact path)."""
    if lengths is None or B is None:
        return lengths if lengths is None else _c(lengths.to(torch.int64))
    assert lengths.dtype == torch.int64 and lengths.is_contiguous() and lengths.numel() == B
    return lengths


def _rows2d(audio):
    """[B, 1, n] / [B, n] audio as the [B, n] view the row kernels read: unit stride in time, any row stride."""
    a = audio.reshape(audio.shape[0], -1) if audio.dim() == 3 else audio
    assert a.dim() == 2 and a.stride(1) == 1
    return a


def _pick(plain: str, ragged: str, *lengths):
    """All that a plain / ragged pair of entry points differs in: (the entry point, its length arguments) -- ``ragged``
    with the device pointers of ``lengths``, or ``plain`` with none when there are no lengths."""
    return (plain, ()) if lengths[0] is None else (ragged, tuple(L.ptr(t) for t in lengths))


def sequence_mask(length: torch.Tensor, max_length: int) -> torch.Tensor:
    """commons.sequence_mask (reference commons.py:128-132) as a float mask [B, 1, T]."""
    length = _c(length.to(torch.int64))
    B = length.shape[0]
    mask = torch.empty(B, 1, max_length, dtype=torch.float32, device=length.device)
    L.call("hsp_sequence_mask_f32", L.ptr(length), L.fptr(mask), B, max_length)
    return mask


# measurement hook (bench.py): hook(algorithmic_bytes, ev_start, ev_end) around every stand-alone activation
ACT_HOOK = None


def act1d(x, ea, binv, filt, out=None, lens=None):
    """``lens`` (device int64 [B]): ragged form (hsp_act1d_snakebeta_ragged_f32) -- row b is the call on the row cut
    to lens[b], zero beyond it."""
    x = _c(x)
    B, Cc, T = x.shape
    out = _new_like(x) if out is None else out
    name, rag = _pick("hsp_act1d_snakebeta_f32", "hsp_act1d_snakebeta_ragged_f32", _lengths(lens, B))
    args = (L.fptr(x), L.fptr(out), B, Cc, T, *rag, L.fptr(ea), L.fptr(binv), L.fptr(filt), L.stream_ptr())
    hook = ACT_HOOK
    _, e0, e1 = L.timed(hook, name, lambda: getattr(L.lib(), name)(*args))
    if hook is not None:
        hook(8 * B * Cc * T, e0, e1)   # one fp32 read + one fp32 write per element
    return out


def flip_channels(x):
    x = _c(x)
    B, Cc, T = x.shape
    y = _new_like(x)
    L.call("hsp_flip_channels_f32", L.fptr(x), L.fptr(y), B, Cc, T)
    return y


def row_seeds(seeds, B: int, device) -> torch.Tensor:
    """int64 [B] seeds on ``device``, THE rule of every seed argument (the prosody LM's ``seeds``, the prior noise's
    ``noise_seeds``): an int s gives row b the seed s + b (one fill kernel, capturable); a tensor is used
    as it is when it already is a contiguous int64 [B] device tensor -- so a captured loop replays with the values
    a later ``seeds.copy_()`` put there."""
    if isinstance(seeds, torch.Tensor):
        if seeds.shape != (B,):
            raise L.HspError(f"seeds must have shape ({B},), got {tuple(seeds.shape)}")
        if seeds.dtype == torch.int64 and seeds.device == torch.device(device) and seeds.is_contiguous():
            return seeds
        return seeds.to(device=device, dtype=torch.int64).contiguous()
    s = int(0 if seeds is None else seeds)
    return torch.arange(s, s + B, dtype=torch.int64, device=device)


def check_noise_seeds(noise, noise_seeds, B: Optional[int] = None, what: str = "noise_seeds") -> None:
    """The argument check of every call that takes ``noise`` and ``noise_seeds`` (from shapes alone, no device work):
    the tensor and the seeds that would draw it exclude each other; the seeds are an int or a 1-D integer tensor, of
    ``B`` entries where the caller knows its rows."""
    if noise_seeds is None:
        return
    if noise is not None:
        raise L.HspError(f"give noise or {what}, not both: the seeds draw the tensor that noise would replace")
    if isinstance(noise_seeds, torch.Tensor):
        if noise_seeds.dim() != 1 or noise_seeds.dtype.is_floating_point or \
                (B is not None and noise_seeds.shape[0] != B):
            raise L.HspError(f"{what} must be an int or an int64 [{'B' if B is None else B}] tensor, got "
                             f"{noise_seeds.dtype} {tuple(noise_seeds.shape)}")
    elif isinstance(noise_seeds, bool) or not isinstance(noise_seeds, int):
        raise L.HspError(f"{what} must be an int or an int64 [B] tensor, got {type(noise_seeds).__name__}")


def randn_rows(seeds, C: int, T: int, device=None):
    """The seeded prior noise [B, C, T] (include/hsp.h "seeded prior noise"): row b is a function of (seeds[b], c, t)
    alone.  ``seeds``: an int64 [B] tensor (B from its length; a CPU tensor goes to ``device``, default the current
    GPU), read in place when it lives on the device."""
    if not isinstance(seeds, torch.Tensor) or seeds.dim() != 1:
        raise L.HspError("randn_rows takes its seeds as an int64 [B] tensor")
    if device is None:
        device = seeds.device if seeds.is_cuda else torch.device("cuda", torch.cuda.current_device())
    seeds = row_seeds(seeds, seeds.shape[0], device)
    out = torch.empty(seeds.shape[0], int(C), int(T), dtype=torch.float32, device=seeds.device)
    L.call("hsp_randn_rows_f32", L.ptr(seeds), L.fptr(out), seeds.shape[0], int(C), int(T))
    return out


def sample_prior(stats, noise, mask, noise_scale: float, seeds=None):
    """z = (m + noise * exp(logs) * noise_scale) * mask; stats = [B, 2C, T].  Exactly one of ``noise`` ([B, C, T]) and
    ``seeds`` (an int or an int64 [B] tensor, `row_seeds`): with seeds the noise of `randn_rows` is drawn inside the
    launch and no noise tensor exists; the result is the same bit for bit."""
    B, C2, T = stats.shape
    check_noise_seeds(noise, seeds, B, "seeds")
    if noise is None and seeds is None:
        raise L.HspError("sample_prior needs noise or seeds")
    stats, mask = _c(stats), _c(mask)
    z = torch.empty(B, C2 // 2, T, dtype=torch.float32, device=stats.device)
    if seeds is not None:
        seeds = row_seeds(seeds, B, stats.device)
        L.call("hsp_sample_prior_seeded_f32", L.fptr(stats), L.ptr(seeds), L.fptr(mask), L.fptr(z), B, C2 // 2, T,
               float(noise_scale))
        return z
    noise = _c(noise)
    assert noise.shape == z.shape, (noise.shape, z.shape)
    L.call("hsp_sample_prior_f32", L.fptr(stats), L.fptr(noise), L.fptr(mask), L.fptr(z), B, C2 // 2, T,
           float(noise_scale))
    return z


def layernorm_mod(x, eps: float, mask=None, shift=None, scale=None, gamma=None, beta=None):
    """LayerNorm over C of [B, C, T] (+ optional affine), * mask, then * (1 + scale) + shift."""
    x = _c(x)
    B, Cc, T = x.shape
    y = _new_like(x)
    mod_bs = 0
    if shift is not None:
        assert shift.stride(1) == 1 and scale.stride(1) == 1 and shift.stride(0) == scale.stride(0)
        mod_bs = shift.stride(0)
    from . import hip_layers
    if hip_layers.SURVEY_ABI and gamma is None and beta is None:   # SURVEY.md §8(b) name of the same launch
        L.call("hsp_layernorm_modulate_f32", L.fptr(x), L.fptr(y), B, Cc, T, float(eps),
               L.fptr(_c(mask)) if mask is not None else None, L.fptr(shift), L.fptr(scale), mod_bs)
        return y
    L.call("hsp_layernorm_mod_f32", L.fptr(x), L.fptr(y), B, Cc, T, float(eps),
           L.fptr(_c(mask)) if mask is not None else None, L.fptr(shift), L.fptr(scale), mod_bs, L.fptr(gamma),
           L.fptr(beta))
    return y


def _mha_qkv(a, q, k, v, n_heads: int, qk_scale: float):
    """What MhaArgs and MhaProjArgs share: q [B, H*D, Tq], k / v [B, H*D, Tk] with unit time stride, their batch and
    channel strides, the sizes and the scale.  Returns (B, H*D, Tq, Tk)."""
    B, HD, Tq = q.shape
    Tk = k.shape[2]
    for t_, T_ in ((q, Tq), (k, Tk), (v, Tk)):
        assert (t_.stride(2) == 1 or T_ == 1), "attention operands need unit time stride"
    a.q, a.k, a.v = L.fptr(q), L.fptr(k), L.fptr(v)
    a.q_bs, a.k_bs, a.v_bs = q.stride(0), k.stride(0), v.stride(0)
    a.q_cs, a.k_cs, a.v_cs = q.stride(1), k.stride(1), v.stride(1)
    a.B, a.H, a.D, a.Tq, a.Tk = B, n_heads, HD // n_heads, Tq, Tk
    a.qk_scale = float(qk_scale)
    return B, HD, Tq, Tk


def mha(q, k, v, n_heads: int, qk_scale: float, mask_q=None, mask_k=None, rel_k=None, rel_v=None, window=0,
        out=None, mask_dense=None, force_stream=False):
    """q [B, H*D, Tq], k/v [B, H*D, Tk] (any batch / channel strides, unit time stride) -> [B, H*D, Tq].
    Strided views let a batch live side by side on the column axis of one [C, B*T] matrix
    (``x.view(C, B, T).permute(1, 0, 2)``), the layout of the PLM loop."""
    a = L.MhaArgs()
    B, HD, Tq, Tk = _mha_qkv(a, q, k, v, n_heads, qk_scale)
    o = torch.empty(B, HD, Tq, dtype=torch.float32, device=q.device) if out is None else out
    assert o.stride(2) == 1 or Tq == 1, "attention operands need unit time stride"
    for t_, T_ in ((q, Tq), (k, Tk), (v, Tk), (o, Tq)):
        assert t_.stride(1) >= T_, "attention operands need unit time stride"
    a.o, a.o_bs, a.o_cs = L.fptr(o), o.stride(0), o.stride(1)
    if mask_q is not None:
        a.mask_q, a.mask_k = L.fptr(_c(mask_q)), L.fptr(_c(mask_k))
    if rel_k is not None:
        a.rel_k, a.rel_v, a.window = L.fptr(_c(rel_k)), L.fptr(_c(rel_v)), window
    if mask_dense is not None:
        # the reference's general attn_mask [B, 1, Tq, Tk] / [B, Tq, Tk] (attentions.py:147-155): 0 -> -1e4
        md = mask_dense.reshape(B, Tq, Tk)
        if md.dtype != torch.float32:
            md = md.to(torch.float32)            # a dtype cast of the caller's bool mask, no arithmetic
        md = _c(md)
        a.mask_dense, a.mask_dense_bs = L.fptr(md), md.stride(0)
    if force_stream:                              # tests: the key-streaming kernels at any length (hsp.h)
        a.window = -(a.window + 1)
    L.call("hsp_mha_f32", C.byref(a))
    return o


# HSP_FUSE_MHA_PROJ=0: attention and its output projection as two launches again (same-box A/B, tests of both paths)
FUSE_MHA_PROJ = os.environ.get("HSP_FUSE_MHA_PROJ", "1") == "1"


def mha_proj_supported(n_heads: int, head_dim: int, m: int, tk: int) -> bool:
    return FUSE_MHA_PROJ and bool(L.lib().hsp_mha_proj_supported(n_heads, head_dim, m, tk))


def mha_proj(q, k, v, n_heads: int, qk_scale: float, wt, bias=None, mask=None, cscale=None, res=None, out=None,
             key_len=None):
    """Attention over all heads + output projection + epilogue in one launch (hsp_mha_proj_f32):
    y = ((wt @ attention(q, k, v) + bias) * mask) * cscale + res.  q [B, H*D, Tq], k / v [B, H*D, Tk] with unit time
    stride (strided views as for ``mha``); ``wt`` [M, H*D] row-major (the nn.Linear weight as stored); ``res`` / ``out``
    [B, M, Tq] with ANY strides; ``mask`` [B, 1, Tq] or [B, Tq]; ``cscale`` [B, M]; ``key_len`` (device int64 [B]): the
    softmax of row b covers keys [0, key_len[b]) only."""
    a = L.MhaProjArgs()
    B, HD, Tq, Tk = _mha_qkv(a, q, k, v, n_heads, qk_scale)
    M = wt.shape[0]
    y = torch.empty(B, M, Tq, dtype=torch.float32, device=q.device) if out is None else out
    assert y.shape == (B, M, Tq) and wt.shape == (M, HD) and wt.stride(1) == 1
    a.wt, a.M, a.wt_ld = L.fptr(wt), M, wt.stride(0)
    if bias is not None:
        a.bias = L.fptr(bias)
    if mask is not None:
        mk = mask.reshape(B, -1)
        assert mk.shape[1] == Tq and (mk.stride(1) == 1 or Tq == 1)
        a.mask, a.mask_bs = L.fptr(mk), mk.stride(0)
    if cscale is not None:
        assert cscale.shape[:2] == (B, M) and cscale.stride(1) == 1
        a.cscale, a.cscale_bs = L.fptr(cscale), cscale.stride(0)
    if res is not None:
        assert res.shape == y.shape
        a.res, a.res_bs, a.res_cs, a.res_ts = L.fptr(res), res.stride(0), res.stride(1), max(res.stride(2), 1)
    a.y, a.y_bs, a.y_cs, a.y_ts = L.fptr(y), y.stride(0), y.stride(1), max(y.stride(2), 1)
    if key_len is not None:
        assert key_len.dtype == torch.int64 and key_len.is_contiguous() and key_len.numel() == B
        a.key_len = L.ptr(key_len)
    L.call("hsp_mha_proj_f32", C.byref(a))
    return y


def masked_mean(x, mask):
    x, mask = _c(x), _c(mask)
    B, Cc, T = x.shape
    out = torch.empty(B, Cc, dtype=torch.float32, device=x.device)
    L.call("hsp_masked_mean_f32", L.fptr(x), L.fptr(mask), L.fptr(out), B, Cc, T)
    return out


def mask_mul(x, mask):
    x, mask = _c(x), _c(mask)
    B, Cc, T = x.shape
    y = _new_like(x)
    L.call("hsp_mask_mul_f32", L.fptr(x), L.fptr(mask), L.fptr(y), B, Cc, T)
    return y


def axpby(x, z, a: float, b: float):
    x, z = _c(x), _c(z)
    assert x.shape == z.shape
    y = _new_like(x)
    L.call("hsp_axpby_f32", L.fptr(x), L.fptr(z), L.fptr(y), float(a), float(b), x.numel())
    return y


def linear_interp(x, out_len: int, lens_in=None, lens_out=None):
    """F.interpolate(x, out_len, mode='linear') along the last axis of [B, C, L].  ``lens_in`` / ``lens_out`` (device
    int64 [B]): ragged form (hsp_linear_interp_ragged_f32) -- row b is the call on its first lens_in[b] samples to
    lens_out[b] outputs, zero after."""
    x = _c(x)
    B, Cc, Lin = x.shape
    y = torch.empty(B, Cc, out_len, dtype=torch.float32, device=x.device)
    name, rag = _pick("hsp_linear_interp_f32", "hsp_linear_interp_ragged_f32", _lengths(lens_in, B),
                      _lengths(lens_out, B))
    L.call(name, L.fptr(x), L.fptr(y), B, Cc, Lin, out_len, *rag)
    return y


def copy_strided(x):
    """Contiguous copy of a strided [B, C, T] view (one launch, no torch arithmetic)."""
    B, Cc, T = x.shape
    y = torch.empty(B, Cc, T, dtype=torch.float32, device=x.device)
    L.call("hsp_copy_strided_f32", L.fptr(x), x.stride(0), x.stride(1), x.stride(2), L.fptr(y), B, Cc, T)
    return y


def add_cbias(x, cb):
    """x [B, C, T] (strided ok) + cb [B, C(, 1)] broadcast over T -> contiguous [B, C, T]."""
    B, Cc, T = x.shape
    assert x.stride(2) == 1 and cb.stride(1) == 1 and cb.shape[:2] == (B, Cc)
    y = torch.empty(B, Cc, T, dtype=torch.float32, device=x.device)
    L.call("hsp_add_cbias_f32", L.fptr(x), x.stride(0), x.stride(1), L.fptr(cb), cb.stride(0), L.fptr(y), B, Cc, T)
    return y


def embedding_sum(ids, tables, n_rows, scale: float, channels: int, out=None):
    """Channel-major sum of up to three embedding lookups: ids = list of int64 [B, T], tables = list of
    flat fp32 tables [rows * channels] -> [B, channels, T]."""
    B, T = ids[0].shape
    if out is None:
        out = torch.empty(B, channels, T, dtype=torch.float32, device=ids[0].device)
    ids = [_c(i.to(torch.int64)) for i in ids] + [None] * (3 - len(ids))
    tables = list(tables) + [None] * (3 - len(tables))
    n_rows = list(n_rows) + [0] * (3 - len(n_rows))
    L.call("hsp_embedding_sum_f32", L.ptr(ids[0]), L.ptr(ids[1]), L.ptr(ids[2]), L.fptr(tables[0]), L.fptr(tables[1]),
           L.fptr(tables[2]), n_rows[0], n_rows[1], n_rows[2], float(scale), L.fptr(out), out.stride(0), out.stride(1),
           B, channels, T)
    return out


def act(x, kind: int):
    """y = act(x) elementwise (HSP_ACT_*)."""
    x = _c(x)
    y = torch.empty_like(x)
    L.call("hsp_act_f32", L.fptr(x), L.fptr(y), x.numel(), kind)
    return y


def reflect_pad(x, pad: int, lengths=None):
    """F.pad(x, (pad, pad), "reflect") on the last axis of [B, L] / [B, 1, L] audio.  ``lengths`` (int64 [B]): row b is
    F.pad(x[b, :lengths[b]], ...), zero after lengths[b] + 2 pad (hsp_reflect_pad_ragged_f32)."""
    shp = x.shape
    x2 = x.reshape(-1, shp[-1])
    assert x2.stride(1) == 1
    B, Lx = x2.shape
    y = torch.empty(B, Lx + 2 * pad, dtype=torch.float32, device=x.device)
    if lengths is None:
        L.call("hsp_reflect_pad_f32", L.fptr(x2), x2.stride(0), L.fptr(y), B, Lx, pad)
    else:
        L.call("hsp_reflect_pad_ragged_f32", L.fptr(x2), x2.stride(0), L.ptr(_lengths(lengths)), L.fptr(y), y.stride(0),
               B, Lx, pad, Lx + 2 * pad)
    return y.reshape(*shp[:-1], Lx + 2 * pad)


def f0_convert(f0_src, f0_trg):
    """inference_vc.py:80-81,104-105 for one utterance: -> log(f0' + 1) with the source's voiced frames moved to the
    target speaker's voiced mean / std."""
    s, t = _c(f0_src.reshape(-1)), _c(f0_trg.reshape(-1))
    out = torch.empty_like(s)
    L.call("hsp_f0_convert_f32", L.fptr(s), s.numel(), L.fptr(t), t.numel(), L.fptr(out))
    return out.reshape(f0_src.shape)


def f0_edit(lf0, lengths=None, shift=None, range=None, target_hz=None, offsets=None, f_min: float = 55.0,
            f_max: float = 1100.0, out=None, return_mean: bool = False):
    """The pitch edit of include/hsp.h (hsp_f0_edit_rows_f32) on the rows of ``lf0`` fp32 [B, n] (log(f0 + 1), 0 =
    unvoiced; unit stride in time, any row stride), row b over ``lengths[b]`` frames (device int64 [B]; None: all n):
    ``shift`` (semitones), ``range``, ``target_hz`` device fp32 [B] or None (0, 1, no target), ``offsets`` (semitones)
    device fp32 [B, n] or None.  One launch.  -> the edited track [B, n] (``out``: written there; it may be ``lf0``),
    zeros from a row's length on; with ``return_mean`` also mean_hz fp32 [B], the geometric mean of every row's voiced
    frames in Hz BEFORE the edit (0 for a row without one).  `prosody_controls.PitchEdit` is the validated form."""
    if lf0.dim() != 2 or lf0.stride(1) != 1:
        raise L.HspError(f"f0_edit takes lf0 as fp32 [B, n] with unit stride in time, got {tuple(lf0.shape)}")
    B, n = lf0.shape
    out = torch.empty(B, n, dtype=torch.float32, device=lf0.device) if out is None else out
    if out.shape != lf0.shape or out.stride(1) != 1:
        raise L.HspError(f"f0_edit: out must be fp32 {tuple(lf0.shape)} with unit stride in time")
    for name, v in (("shift", shift), ("range", range), ("target_hz", target_hz)):
        if v is not None and (v.shape != (B,) or not v.is_contiguous()):
            raise L.HspError(f"f0_edit: {name} must be a contiguous fp32 [{B}] tensor, got {tuple(v.shape)}")
    if offsets is not None and (offsets.shape != lf0.shape or offsets.stride(1) != 1):
        raise L.HspError(f"f0_edit: offsets must be fp32 {tuple(lf0.shape)} with unit stride in time, got "
                         f"{tuple(offsets.shape)}")
    mean = torch.empty(B, dtype=torch.float32, device=lf0.device) if return_mean else None
    a = L.F0EditArgs()
    a.lf0, a.lf0_bs, a.lengths, a.B, a.n = L.fptr(lf0), lf0.stride(0) if B > 1 else n, L.ptr(_lengths(lengths)), B, n
    a.shift, a.range, a.target_hz = L.fptr(shift), L.fptr(range), L.fptr(target_hz)
    a.offsets, a.off_bs = L.fptr(offsets), 0 if offsets is None else (offsets.stride(0) if B > 1 else n)
    a.f_min, a.f_max = float(f_min), float(f_max)
    a.out, a.out_bs, a.mean_hz = L.fptr(out), out.stride(0) if B > 1 else n, L.fptr(mean)
    L.call("hsp_f0_edit_rows_f32", C.byref(a))
    return (out, mean) if return_mean else out


# --------------------------------------------------------- batched voice conversion (ragged rows, device lengths)
def reflect_pad_ragged(x, lengths, pad: int):
    """Row b of x [B, L] -> F.pad(x[b, :lengths[b]], (pad, pad), "reflect"), zero after lengths[b] + 2 pad:
    [B, L + 2 pad]."""
    assert x.dim() == 2
    return reflect_pad(x, pad, lengths)


def f0_convert_batch(f0_src, n_src, f0_trg, n_trg):
    """`f0_convert` per row in one launch: f0_src [B, N] with n_src [B] valid samples, f0_trg [B, Nt] (or [1, Nt]: one
    track shared by every row) with n_trg [B] -> [B, N], zero after n_src[b].  Row b equals f0_convert on that row's
    tracks bit for bit."""
    s, t = _c(f0_src), _c(f0_trg)
    B, N = s.shape
    assert t.dim() == 2 and t.shape[0] in (1, B)
    out = torch.empty(B, N, dtype=torch.float32, device=s.device)
    L.call("hsp_f0_convert_batch_f32", L.fptr(s), s.stride(0), L.ptr(_lengths(n_src)), L.fptr(t),
           0 if t.shape[0] == 1 else t.stride(0), L.ptr(_lengths(n_trg)), t.shape[1], L.fptr(out), out.stride(0), B, N)
    return out


def abs_max_rows(x, lengths=None):
    """max |x[b, :lengths[b]]| of every row of x [B, n] -> fp32 [B] on the device (no host read-back)."""
    assert x.dim() == 2 and x.stride(1) == 1
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    L.call("hsp_abs_max_rows_f32", L.fptr(x), x.stride(0), L.ptr(_lengths(lengths)), L.fptr(out), x.shape[0],
           x.shape[1])
    return out


def peak_int16(audio, lengths=None, gain=0.999):
    """[B, 1, n] / [B, n] fp32 -> int16 [B, n], every row scaled by its own peak (over ``lengths[b]`` samples) times
    ``gain``: a float for every row (hsp_peak_int16) or a device fp32 [B], one per row (hsp_peak_int16_gains).
    A silent row (peak 0) comes out as zeros, as the reference's ``(a / a.abs().max() ...).astype(int16)`` does."""
    a = _rows2d(audio)
    out = torch.empty(a.shape, dtype=torch.int16, device=a.device)
    if torch.is_tensor(gain):
        assert gain.shape == (a.shape[0],)
        name, g = "hsp_peak_int16_gains", L.fptr(_c(gain))
    else:
        name, g = "hsp_peak_int16", float(gain)
    L.call(name, L.fptr(a), a.stride(0), L.ptr(_lengths(lengths)), g, L.ptr(out), out.stride(0), a.shape[0], a.shape[1])
    return out


def peak_int16_gains(audio, lengths, gains):
    """`peak_int16` with a per-row device gain: gains fp32 [B]."""
    return peak_int16(audio, lengths, gains)


# ---------------------------------------------------------------- loudness (ITU-R BS.1770-4; scale_norm="lufs")
def loudness(audio, sample_rate: int, lengths=None):
    """Integrated loudness and peak of every row: [B, 1, n] / [B, n] fp32 (unit stride in time, any row stride) at
    ``sample_rate`` (a multiple of 8000 up to 48000), ``lengths`` int64 [B] valid samples (None = all n) ->
    (lufs fp32 [B], peak fp32 [B]) on the device, no host read-back.  A row under 400 ms is metered whole and ungated;
    a row with nothing above -70 LUFS reads -inf.  Row b equals the call on row b alone bit for bit."""
    a = _rows2d(audio)
    B, n = a.shape
    lib = L.lib()
    nbytes = lib.hsp_loudness_workspace_bytes(B, n)
    if nbytes < 0:
        raise L.HspError(f"hsp_loudness_workspace_bytes: no workspace for a batch of {B} rows x {n} samples")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=a.device)
    lufs = torch.empty(B, dtype=torch.float32, device=a.device)
    peak = torch.empty(B, dtype=torch.float32, device=a.device)
    L.call("hsp_loudness_f32", L.fptr(a), a.stride(0), L.ptr(_lengths(lengths)), B, n,
           int(sample_rate), L.ptr(ws), ws.numel() * 8, L.fptr(lufs), L.fptr(peak))
    return lufs, peak


def loudness_gains(lufs, peak, target_lufs: float = -23.0, ceiling: float = 0.999):
    """The per-row gain of `peak_int16_gains` that brings a row metered by `loudness` to ``target_lufs``:
    min(10^((target - lufs) / 20) * peak, ceiling) -> (gains fp32 [B], limited int32 [B]: 1 where the ceiling was
    taken; a silent row, lufs = -inf, takes it too)."""
    assert lufs.dim() == 1 and peak.shape == lufs.shape
    B = lufs.shape[0]
    gains = torch.empty(B, dtype=torch.float32, device=lufs.device)
    limited = torch.empty(B, dtype=torch.int32, device=lufs.device)
    L.call("hsp_loudness_gains_f32", L.fptr(_c(lufs)), L.fptr(_c(peak)), float(target_lufs), float(ceiling),
           L.fptr(gains), L.ptr(limited), B)
    return gains, limited


def lufs_int16(audio, lengths, sample_rate: int, target_lufs: float = -23.0, ceiling: float = 0.999):
    """The int16 stage of scale_norm="lufs": meter -> gains -> `peak_int16_gains`, three launches-only steps on the
    current stream.  [B, 1, n] / [B, n] fp32 -> int16 [B, n], row b at ``target_lufs`` over its lengths[b] samples
    unless its peak would pass ``ceiling`` of full scale."""
    a = _rows2d(audio)
    lufs, peak = loudness(a, sample_rate, lengths)
    gains, _ = loudness_gains(lufs, peak, target_lufs, ceiling)
    return peak_int16_gains(a, lengths, gains)


# ---------------------------------------------------------------- true peak and look-ahead limiter
TRUE_PEAK_RATE = 192000   # the interpolated rate: the standard's 4x at 48 kHz, held for the lower rates
TRUE_PEAK_Z = 6           # 2 Z taps per phase
TRUE_PEAK_BETA = 8.0
_TRUE_PEAK_BANKS = {}


def true_peak_bank_f64(fs: int):
    """The interpolator of include/hsp.h in float64: [F][2 Z], F = 192000 / fs, tap d = -(Z - 1) ... Z at index
    d + Z - 1, h_p[d] = sinc(d - p / F) * kaiser_8(|d - p / F| / Z); phase 0 is the unit impulse exactly."""
    import numpy as np
    fs = int(fs)
    if fs not in (16000, 24000, 48000):
        raise L.HspError(f"true peak: sample rate {fs} is not 16000, 24000 or 48000")
    F, Z = TRUE_PEAK_RATE // fs, TRUE_PEAK_Z
    t = np.arange(-(Z - 1), Z + 1, dtype=np.float64)[None, :] - np.arange(F, dtype=np.float64)[:, None] / F
    u = np.minimum(np.abs(t) / Z, 1.0)
    bank = np.sinc(t) * np.i0(TRUE_PEAK_BETA * np.sqrt(1.0 - u * u)) / np.i0(TRUE_PEAK_BETA)
    bank[0] = 0.0
    bank[0, Z - 1] = 1.0
    return bank


def true_peak_bank(fs: int, device=None):
    """-> (float64 bank [F][2 Z] on the host, the same bank as fp32 on ``device``), built once per (rate, device); a
    call inside a stream capture needs that upload done by an eager call first."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (int(fs), device)
    got = _TRUE_PEAK_BANKS.get(key)
    if got is None:
        hb = true_peak_bank_f64(fs)
        if torch.cuda.is_current_stream_capturing():
            raise L.HspError("true peak: the bank of this rate is not uploaded yet; make one eager call before "
                             "capturing the stream")
        got = (hb, torch.from_numpy(hb.astype("float32")).to(device))
        _TRUE_PEAK_BANKS[key] = got
    return got


def _rows_gains(audio, gains):
    a = _rows2d(audio)
    if gains is not None:
        assert gains.shape == (a.shape[0],)
        gains = _c(gains)
    return a, gains


def true_peak(audio, sample_rate: int, lengths=None, gains=None):
    """True peak of every row (hsp_true_peak_f32): [B, 1, n] / [B, n] fp32 at 16, 24 or 48 kHz, ``lengths`` int64 [B]
    (None = all n), ``gains`` device fp32 [B] applied first (None = 1) -> fp32 [B] (linear, 1 = full scale) on the
    device.  Never below the row's sample peak; 0 for an empty row."""
    a, gains = _rows_gains(audio, gains)
    B, n = a.shape
    _, bank = true_peak_bank(sample_rate, a.device)
    tp = torch.empty(B, dtype=torch.float32, device=a.device)
    L.call("hsp_true_peak_f32", L.fptr(a), a.stride(0), L.ptr(_lengths(lengths)), L.fptr(gains), B, n, L.fptr(bank),
           bank.shape[0], bank.shape[1] // 2, L.fptr(tp))
    return tp


def lookahead_samples(lookahead_ms: float, sample_rate: int) -> int:
    return int(round(float(lookahead_ms) * int(sample_rate) / 1000.0))


def limit(audio, sample_rate: int, ceiling: float, lookahead_ms: float = 1.5, lengths=None, gains=None,
          return_true_peak: bool = False):
    """The look-ahead true-peak limiter of include/hsp.h (hsp_limiter_f32) on gains[b] * row b: -> (z fp32 [B, n] with
    |z| <= ``ceiling`` on every sample and zeros from lengths[b] on, min_gain fp32 [B]: the smallest gain the limiter
    applied, 1 where it never engaged).  ``ceiling`` is linear (1 = full scale); the look-ahead is
    round(lookahead_ms * sample_rate / 1000) samples, 1 ... 480.  ``return_true_peak`` adds the true peak of the
    limiter's input (gains[b] * row b)."""
    a, gains = _rows_gains(audio, gains)
    B, n = a.shape
    _, bank = true_peak_bank(sample_rate, a.device)
    z = torch.empty(B, n, dtype=torch.float32, device=a.device)
    mg = torch.empty(B, dtype=torch.float32, device=a.device)
    tp = torch.empty(B, dtype=torch.float32, device=a.device) if return_true_peak else None
    lens = _lengths(lengths)
    args = L.LimiterArgs()
    args.x, args.x_bs, args.lengths, args.gains = L.fptr(a), a.stride(0), L.ptr(lens), L.fptr(gains)
    args.B, args.n = B, n
    args.bank, args.F, args.Z = L.fptr(bank), bank.shape[0], bank.shape[1] // 2
    args.W, args.ceiling = lookahead_samples(lookahead_ms, sample_rate), float(ceiling)
    args.y, args.y_bs, args.min_gain, args.tp = L.fptr(z), z.stride(0), L.fptr(mg), L.fptr(tp)
    L.call("hsp_limiter_f32", C.byref(args))
    return (z, mg, tp) if return_true_peak else (z, mg)


def gain_update(gains, lufs, target_lufs: float):
    """gains[b] * 10^((target_lufs - lufs[b]) / 20) -> fp32 [B] (hsp_gain_update_f32): a loudness that is not finite
    leaves the gain as it is.  ``gains`` None: the first gain of every row, from 1 -- 0 for a row without a loudness."""
    B = lufs.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=lufs.device)
    L.call("hsp_gain_update_f32", L.fptr(None if gains is None else _c(gains)), L.fptr(_c(lufs)), float(target_lufs),
           L.fptr(out), B)
    return out


def gain_int16(audio, lengths, gains):
    """int16(audio[b] * gains[b] * 32767) over lengths[b] samples, zeros after (hsp_gain_int16_f32): truncating and
    saturating like `peak_int16`, but with no peak normalisation."""
    a, gains = _rows_gains(audio, gains)
    out = torch.empty(a.shape, dtype=torch.int16, device=a.device)
    L.call("hsp_gain_int16_f32", L.fptr(a), a.stride(0), L.ptr(_lengths(lengths)), L.fptr(gains), L.ptr(out),
           out.stride(0), a.shape[0], a.shape[1])
    return out


def lufs_limit_int16(audio, lengths, sample_rate: int, target_lufs: float = -23.0, ceiling_db: float = -1.0,
                     lookahead_ms: float = 1.5, passes: int = 2):
    """The int16 stage of scale_norm="lufs" with the limiter: every row at ``target_lufs`` with its true peak at or
    under ``ceiling_db`` dBTP, also where the row's crest factor puts the plain gain of `lufs_int16` over full scale.
    A fixed chain of launches on the current stream, nothing read back:
      L_0 = meter(x), G_1 = 10^((target - L_0) / 20);  for k = 1 ... passes: z_k = limit(G_k x), L_k = meter(z_k),
      G_{k+1} = G_k 10^((target - L_k) / 20);  q = min(1, c / true_peak(z_K));  int16(z_K q 32767).
    -> (int16 [B, n], stats: dict of fp32 [B] device tensors ``achieved_lufs`` (L_K + 20 log10 q), ``true_peak``
    (linear, of z_K q) and ``min_gain`` (the smallest limiter gain of the last pass)).  A row without a loudness
    (silence, or empty) is zeros and reads -inf / 0 / 1."""
    passes = int(passes)
    if not 1 <= passes <= 4:
        raise L.HspError(f"lufs_limit_int16: passes = {passes} is not 1 ... 4")
    c = 10.0 ** (float(ceiling_db) / 20.0)
    a = _rows2d(audio)
    lufs, _ = loudness(a, sample_rate, lengths)
    g = gain_update(None, lufs, target_lufs)
    for k in range(passes):
        if k:
            g = gain_update(g, lufs, target_lufs)
        z, min_gain = limit(a, sample_rate, c, lookahead_ms, lengths, g)
        lufs, _ = loudness(z, sample_rate, lengths)
    q = torch.empty_like(lufs)
    achieved = torch.empty_like(lufs)
    tpk = torch.empty_like(lufs)
    L.call("hsp_limiter_stats_f32", L.fptr(lufs), L.fptr(true_peak(z, sample_rate, lengths)), c, L.fptr(q),
           L.fptr(achieved), L.fptr(tpk), lufs.shape[0])
    return gain_int16(z, lengths, q), {"achieved_lufs": achieved, "true_peak": tpk, "min_gain": min_gain}


# --------------------------------------------------------- sinc resampling (torchaudio 0.13.1 functional.resample)
KAISER_BETA = 14.769656459379492   # torchaudio's beta for resampling_method="kaiser_window", beta=None


class ResampleBank:
    """The filter bank of one rate pair, as torchaudio builds it (full) and as the kernel reads it (compacted)."""

    def __init__(self, o, n, width, full, bank, tap0):
        self.o, self.n, self.width = o, n, width
        self.K = 2 * width + o
        self.full = full            # float64 [n, K]: torchaudio's bank before its fp32 cast
        self.bank = bank            # float32 [n, n_taps]: taps tap0[p] ... tap0[p] + n_taps - 1 of phase p
        self.tap0 = tap0            # int32 [n]
        self.n_taps = bank.shape[1]

    def out_length(self, length: int) -> int:
        """torchaudio's target length ceil(n * length / o)."""
        return -(-self.n * int(length) // self.o)


def sinc_resample_bank(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                       resampling_method: str = "sinc_interpolation", beta: Optional[float] = None) -> ResampleBank:
    """torchaudio 0.13.1 _get_sinc_resample_kernel in float64 (phase / new_freq formed in fp32 first, as there), then
    compacted: per phase only the taps whose argument t was not clamped to +-lowpass_filter_width are kept (a clamped
    tap is sinc(+-lpw) * window(+-lpw), below 1e-15), padded with zeros to a common count n_taps."""
    import math
    import numpy as np
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    lpw = lowpass_filter_width
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    K = 2 * width + o
    idx = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    ph = (np.arange(0, -n, -1, dtype=np.int64).astype(np.float32) / np.float32(n)).astype(np.float64)[:, None]
    t_raw = (ph + idx) * base
    t = np.clip(t_raw, -lpw, lpw)
    if resampling_method == "sinc_interpolation":
        window = np.cos(t * math.pi / lpw / 2) ** 2
    elif resampling_method == "kaiser_window":
        b_ = KAISER_BETA if beta is None else float(beta)
        window = np.i0(b_ * np.sqrt(1 - (t / lpw) ** 2)) / np.i0(b_)
    else:
        raise L.HspError(f"unknown resampling_method {resampling_method!r} (sinc_interpolation or kaiser_window)")
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        full = np.where(t == 0, 1.0, np.sin(t) / t)
    full = full * window * (base / o)
    sig = np.abs(t_raw) < lpw                       # unclamped taps: one contiguous run per phase
    first = np.argmax(sig, axis=1)
    count = sig.sum(axis=1)
    n_taps = max(1, int(count.max()))
    tap0 = np.minimum(first, K - n_taps).astype(np.int32)
    cols = tap0[:, None] + np.arange(n_taps)[None, :]
    rows = np.arange(n)[:, None]
    bank = np.where(sig[rows, cols], full[rows, cols], 0.0).astype(np.float32)
    return ResampleBank(o, n, width, full, np.ascontiguousarray(bank), tap0)


_RESAMPLE_BANKS = {}


def resample(waveform, orig_freq, new_freq, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             resampling_method: str = "sinc_interpolation", beta: Optional[float] = None, lengths=None):
    """torchaudio.functional.resample (0.13.1; same signature and defaults) on the GPU: one hsp_resample_f32 launch.

    ``waveform`` [..., L] fp32 on the GPU -> [..., ceil(new * L / orig)] (gcd-reduced rates); the input tensor itself
    when the two rates are equal.  ``lengths`` int64 [B] (B = rows of ``waveform.reshape(-1, L)``, device tensor,
    each <= L) resamples a ragged batch: row b equals the call on ``waveform[b, :lengths[b]]`` alone, then zeros.
    The reference harnesses pass ``resampling_method="kaiser_window"``; the default stays torchaudio's Hann window.

    The bank is built on the host in float64 (``sinc_resample_bank``) and uploaded once per (rates, method, lpw,
    rolloff, beta, device); a call inside a stream capture needs that upload done by an eager call first.
    Pinned by the tests against a float64 restatement of torchaudio's formulas (max error 1e-5 at fp32) and against
    an analytic band-limited sine; it has not been compared with torchaudio itself (not in this image).  torchaudio's
    ``resample`` passes the waveform's dtype to its bank builder, so its own fp32 bank may be formed in fp32 arithmetic:
    any difference from this float64 build is at the fp32 rounding of the coefficients (~1e-7 relative), unmeasured."""
    for f in (orig_freq, new_freq):
        if not float(f).is_integer() or f <= 0:
            raise L.HspError(f"resample needs positive integer rates, got {orig_freq} -> {new_freq}")
    if resampling_method not in ("sinc_interpolation", "kaiser_window"):
        raise L.HspError(f"unknown resampling_method {resampling_method!r} (sinc_interpolation or kaiser_window)")
    if not waveform.is_cuda:
        raise L.HspError("resample runs on the GPU only (got a CPU tensor); there is no CPU fallback")
    if waveform.dtype != torch.float32:
        raise L.HspError(f"resample expects float32, got {waveform.dtype}")
    if int(orig_freq) == int(new_freq):
        return waveform
    key = (int(orig_freq), int(new_freq), resampling_method, int(lowpass_filter_width), float(rolloff),
           None if beta is None else float(beta), waveform.device)
    dev_bank = _RESAMPLE_BANKS.get(key)
    if dev_bank is None:
        if torch.cuda.is_current_stream_capturing():
            raise L.HspError("resample: the bank of this rate pair is not uploaded yet; make one eager call before "
                             "capturing the stream")
        hb = sinc_resample_bank(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
        dev_bank = (hb, torch.from_numpy(hb.bank).to(waveform.device), torch.from_numpy(hb.tap0).to(waveform.device))
        _RESAMPLE_BANKS[key] = dev_bank
    hb, bank, tap0 = dev_bank
    shp = waveform.shape
    Lx = shp[-1]
    x = _c(waveform.reshape(-1, Lx))
    B = x.shape[0]
    T_out = hb.out_length(Lx)
    y = torch.empty(B, T_out, dtype=torch.float32, device=x.device)
    lens = None
    if lengths is not None:
        lens = _c(lengths.reshape(-1).to(device=x.device, dtype=torch.int64))
        if lens.shape[0] != B:
            raise L.HspError(f"resample: lengths has {lens.shape[0]} entries for {B} rows")
    L.call("hsp_resample_f32", L.fptr(x), x.stride(0), L.ptr(lens), B, Lx, L.fptr(bank), L.ptr(tap0), hb.n_taps, hb.o,
           hb.n, hb.width, L.fptr(y), y.stride(0), T_out)
    return y.reshape(*shp[:-1], T_out)
