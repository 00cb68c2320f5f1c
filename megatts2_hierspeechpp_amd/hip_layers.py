"""Host-side layer objects over the libhsp C ABI.

``Conv1d`` / ``ConvTranspose1d`` / ``Linear`` keep the reference's parameter names
(``weight`` or ``weight_g``/``weight_v``, ``bias``) so reference checkpoints load
unchanged, and own a *packed* copy of the weight-norm-folded weights in the layout
the kernels read (``w[K][Cin][M]``).  Packing runs once on the GPU
(``hsp_fold_weight_norm_f32`` + ``hsp_gather_f32`` with a host-built index map); the
reference instead re-derives ``g*v/||v||`` on every forward.

All packed tensors of a model live in one contiguous fp32 arena so that a multi-GPU
job can ship them with a single RCCL broadcast.

Every launch of this module leaves through ``_bracket``, the one place that knows its measurement
hook (``LAUNCH_HOOK``).  A conv layer builds its launch (``prepare`` -> ``ConvLaunch``: the filled struct and the tensors
it points at) and then issues it (``ConvLaunch.run``); a caller of an entry point that takes several structs prepares them
itself for ``launch_group``.  The event bracket is ``_lib.timed``, which ``functional.act1d`` uses for ``ACT_HOOK`` too.
"""
from __future__ import annotations

import contextvars
import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import functional as Fh
from .synth import kaiser_sinc_filter12


# Optional measurement hook (bench.py): called as hook(kind, flops, bytes, ev_start, ev_end, args)
# with torch.cuda.Events recorded around the launch on the launch stream.
LAUNCH_HOOK = None
# hsp_conv1d_args.debug of every conv launch.  Always 0 in the product: the release libhsp.so refuses anything
# else.  tools/ set it programmatically together with HSP_LIB=.../libhsp_tune.so (kernel decomposition runs).
DEBUG_FLAGS = 0
# Folded columns (hsp_conv1d_args.fold_cols): Conv1d.prepare sets the field on the B > 1 launches whose kernel implements
# it (fold_cols_wanted).  Results are bit-identical either way; HSP_FOLD_COLS is the switch of a same-box A/B
# (tools/env_ab.py): "1" on, "0" off, "gemm" / "conv" the block token GEMM / the conv tiles alone.
FOLD_COLS = os.environ.get("HSP_FOLD_COLS", "1")


_ZEROS = {}


def _zeros(device) -> torch.Tensor:
    """64 zero floats per device: the source of out-of-range LDS-DMA lanes (hsp_conv1d_args.zeros)."""
    z = _ZEROS.get(device)
    if z is None:
        z = _ZEROS[device] = torch.zeros(64, dtype=torch.float32, device=device)
    return z


_DFT = {}


def _dft_tables(device):
    """(fwd, inv): the constant tables of csrc/hsp_dftseg.hip (include/hsp.h hsp_dftseg_tables_f32: the 64 x 64 matrix of
    the radix-2 half-length transform + the 128-point twiddles), filled by the library, once per device."""
    t = _DFT.get(device)
    if t is None:
        n = L.DFTSEG_TABLE_FLOATS
        f = np.zeros(n, dtype=np.float32)
        finv = np.zeros(n, dtype=np.float32)
        L.check(L.lib().hsp_dftseg_tables_f32(f.ctypes.data, finv.ctypes.data), "hsp_dftseg_tables_f32")
        t = _DFT[device] = (torch.from_numpy(f).to(device), torch.from_numpy(finv).to(device))
    return t


_TW = {}


def _wspec_twiddles(device):
    """256 float64 values in device memory, cos(2 pi n / 128) then sin, n < 128: the table of
    hsp_dftseg_weight_spectrum_f32 (include/hsp.h), generated here in float64."""
    t = _TW.get(device)
    if t is None:
        ang = 2.0 * np.pi * np.arange(128, dtype=np.float64) / 128.0
        t = _TW[device] = torch.from_numpy(np.concatenate([np.cos(ang), np.sin(ang)])).to(device)
    return t


# The channel product between the two transforms: "three" = hsp_cprod3_f32 (round 5: three real C x C products per bin,
# 6 C^2 flops per column and 3 C^2 weights per bin), "block" = round 4's [2C x 2C] real block matrix per bin on the conv
# kernel (hsp_conv1d_args.w_bs; 8 C^2 / 4 C^2) -- kept for A/B runs and for channel counts that are not multiples of 64.
FFT_PRODUCT = os.environ.get("HSP_FFT_PRODUCT", "three")


# ---------------------------------------------------------------- row-exact ragged batches
class RowLengths:
    """The valid length of every row of a ragged batch at each resolution of the vocoder: ``frames`` (device int64 [B])
    at the frame rate of the padded length ``T``; a tensor of L = f * T columns holds f * frames[b] valid ones.  Lengths
    and masks stay on the device (no host read-back, so a fixed shape captures as one hipGraph) and are built once per
    resolution: ``prepare(L)`` on the stream that later forks side streams, before the fork."""

    def __init__(self, frames: torch.Tensor, T: int):
        if frames.dtype != torch.int64 or frames.dim() != 1:
            raise L.HspError(f"row lengths must be int64 [B], got {frames.dtype} {tuple(frames.shape)}")
        self.frames, self.T = frames.contiguous(), int(T)
        self._lens: Dict[int, torch.Tensor] = {}
        self._masks: Dict[int, torch.Tensor] = {}

    def factor(self, L_: int) -> int:
        if L_ % self.T != 0:
            raise L.HspError(f"row_exact: a tensor of {L_} columns is not a whole multiple of the {self.T} frames")
        return L_ // self.T

    def at(self, L_: int) -> torch.Tensor:
        """int64 [B]: valid columns of every row of an L-column tensor."""
        t = self._lens.get(L_)
        if t is None:
            f = self.factor(L_)
            t = self._lens[L_] = self.frames if f == 1 else self.frames * f
        return t

    def mask(self, L_: int) -> torch.Tensor:
        """float [B, 1, L]: 1 over each row's valid columns, 0 after."""
        m = self._masks.get(L_)
        if m is None:
            m = self._masks[L_] = Fh.sequence_mask(self.at(L_), L_)
        return m

    def prepare(self, L_: int):
        self.at(L_)
        self.mask(L_)


# a context variable, not a module global: two threads (or asyncio tasks) driving models see only their own lengths
_ROWS: "contextvars.ContextVar[Optional[RowLengths]]" = contextvars.ContextVar("hsp_row_lengths", default=None)


class row_exact:
    """``with row_exact(RowLengths(...)):`` the vocoder layers run the ragged batch row-exactly: every Activation1d
    clamps its reads at its row's end and writes 0 past it, and the callers zero every tensor a conv reads directly past
    each row's end.  Nested use replaces the lengths for the inner block."""

    def __init__(self, rows: Optional[RowLengths]):
        self.rows = rows

    def __enter__(self):
        self._token = _ROWS.set(self.rows)
        return self.rows

    def __exit__(self, *exc):
        _ROWS.reset(self._token)
        return False


def row_lengths() -> Optional[RowLengths]:
    """The RowLengths of the enclosing ``row_exact`` block, or None (the default batched semantics)."""
    return _ROWS.get()


def fft_act_fusable(x) -> bool:
    """hsp_dftseg_args.act_*: the fused activation reads 16-B groups of every row (in a row-exact block its ragged form,
    hsp_dftseg_args.act_len)."""
    return (x.stride(2) == 1 and x.shape[2] % 4 == 0 and x.stride(0) % 4 == 0 and x.stride(1) % 4 == 0
            and x.data_ptr() % 16 == 0)


# SURVEY.md §8(b) names its minimum C ABI (hsp_conv1d_f32, hsp_convtr1d_f32, hsp_wn_layer_f32, hsp_layernorm_modulate_f32).
# Those entry points dispatch to the kernel-level ones this module calls by default; with SURVEY_ABI set (HSP_SURVEY_ABI=1)
# every launch goes through them instead - same kernels, same results (test_survey_abi_names_give_identical_results):
# ConvLaunch.run() swaps the entry point of a single conv; modules.WN / DiTConVBlock prepare a layer's launches for launch_group().
SURVEY_ABI = os.environ.get("HSP_SURVEY_ABI", "0") == "1"


def _bracket(kind: str, call, flops: int, nbytes: int, arg, soft: bool = False, span=None):
    """The measurement bracket of every launch of this module, and the only code that knows LAUNCH_HOOK: ``call()``
    performs the C call and returns its status; with a hook set it runs between two timing events on the launch stream
    (``_lib.timed``) and is reported as hook(kind, flops, nbytes, ev_start, ev_end, arg).  Without a hook no event is
    created.  ``soft``: a launch the library refuses with HSP_EINVAL reports nothing and its status is returned; every
    other failure raises.  ``call=None`` launches nothing: a summary record over ``span`` = (ev_start, ev_end) of
    earlier brackets.  Returns (status, ev_start, ev_end), the events None without a hook."""
    hook = LAUNCH_HOOK
    if call is None:
        rc, (e0, e1) = 0, span
    else:
        rc, e0, e1 = L.timed(hook, kind, call, soft)
    if hook is not None and e0 is not None:
        hook(kind, flops, nbytes, e0, e1, arg)
    return rc, e0, e1


class ConvLaunch:
    """One conv launch, built (Conv1d.prepare, ConvTranspose1d.prepare) and not yet issued: the entry point ``fn``, its
    ``kind`` for the hook, the filled hsp_conv1d_args ``args``, the algorithmic ``flops`` / ``nbytes``, the output ``out`` and
    ``refs``: every tensor the struct's raw device pointers address (a residual gathered while preparing included), which
    stays alive through them until the launch has been issued."""
    __slots__ = ("kind", "fn", "args", "flops", "nbytes", "out", "refs")

    def __init__(self, kind, fn, args, flops, nbytes, out, refs):
        self.kind = kind
        self.fn = fn
        self.args = args
        self.flops = flops
        self.nbytes = nbytes
        self.out = out
        self.refs = refs

    def run(self, soft: bool = False) -> int:
        """Issue the launch.  ``soft``: return the status instead of raising on HSP_EINVAL (a shape the requested
        fusion does not cover; the caller then issues the un-fused launches)."""
        a, fn = self.args, self.fn
        a.debug = DEBUG_FLAGS
        if SURVEY_ABI:
            fn = L.lib().hsp_convtr1d_f32 if a.rows == L.ROWS_SHUFFLE else L.lib().hsp_conv1d_f32
        return _bracket(self.kind, lambda: fn(C.byref(a), L.stream_ptr()), self.flops, self.nbytes, a, soft=soft)[0]


def launch_group(kind: str, fn, launches, *extra):
    """One call into an entry point taking several hsp_conv1d_args (``launches``: ConvLaunch objects, None = a NULL
    slot); one hook record with the summed flops / bytes and the first struct."""
    live = [p for p in launches if p is not None]
    for p in live:
        p.args.debug = DEBUG_FLAGS
    ptrs = [C.byref(p.args) if p is not None else None for p in launches]
    _bracket(kind, lambda: fn(*ptrs, *extra, L.stream_ptr()), sum(p.flops for p in live), sum(p.nbytes for p in live),
             launches[0].args)


def _set_fold_cols(a) -> None:
    """hsp_conv1d_args.fold_cols of a filled MFMA-path struct: asks the library which kernel the launch takes."""
    a.fold_cols = 0
    if FOLD_COLS != "0" and a.B > 1 and a.ncols % 4 == 0:
        a.debug = DEBUG_FLAGS
        plan = (C.c_int32 * 4)()
        gated = a.rows in (L.ROWS_GATE_WN, L.ROWS_GATE_GLU)
        if L.lib().hsp_conv1d_mfma_plan(C.byref(a), C.byref(plan)) == 0 and \
                FOLD_COLS in ("1", "gemm" if plan[2] == -2 else "conv") and \
                fold_cols_wanted(plan, a.B, a.ncols, gated=gated, halo=(a.K - 1) * a.dil, act1d=a.prologue == L.PRO_ACT1D):
            a.fold_cols = 1


def fold_cols_kernel(plan, gated: bool = False, halo: int = 0, act1d: bool = False) -> bool:
    """Does the kernel of a launch implement hsp_conv1d_args.fold_cols (any other refuses the field)?  ``plan``: the four
    numbers of hsp_conv1d_mfma_plan for the launch, (BM, BN, KC, LDS bytes); ``halo`` = (K - 1) dilation.  The block token
    GEMM (KC = -2; its 128 x 128 shape takes the field and keeps the per-utterance tiling) and the short-sequence conv
    tiles with the 64-column window slack, 64 x 64 on plain rows and 64 x 128 on gated rows (KC > 0; the same tile sizes
    with a halo beyond 61 columns, or 64 x 64 on gated rows, are other kernels), without the activation prologue."""
    bm, bn, kc = int(plan[0]), int(plan[1]), int(plan[2])
    if kc == -2:
        return True
    return kc > 0 and not act1d and halo + 3 <= 64 and (bm, bn) == ((64, 128) if gated else (64, 64))


def fold_cols_wanted(plan, B: int, ncols: int, gated: bool = False, halo: int = 0, act1d: bool = False) -> bool:
    """Does a launch of B utterances x ncols columns set the field?  Where its kernel implements the form and the form
    changes the tiling: more than one utterance, 16-B groups that never straddle two of them (ncols % 4 == 0), a padded
    last tile per utterance.  What else the conv tiles need (a "same" conv with a halo of at most 8, a window that fits
    the LDS pitch) the library checks itself: it keeps the per-utterance tiling, silently, where that does not hold."""
    if B < 2 or ncols % 4 != 0 or ncols % int(plan[1]) == 0 or (int(plan[2]) == -2 and int(plan[0]) != 64):
        return False
    return fold_cols_kernel(plan, gated, halo, act1d)


# ------------------------------------------------------------------ index maps (host logic)
# Activation epilogue (hsp_conv1d_args.act = HSP_ACT_ACT1D): the first conv of a low-channel AMP pair applies the
# pair's second Activation1d to its own output tile, so xt = c1(a1(x)) is never written and a2 is no launch.  Bit-identical
# to the two launches, and faster than them on both shapes that carry the form (profiles/epi_act_bench.txt).
# HSP_EPI_ACT=0 switches the form off (A/B runs, parity tests of both forms).
EPI_ACT = os.environ.get("HSP_EPI_ACT", "1") == "1"
EPI_ACT_TILES = ((32, 512), (64, 256))       # (BM, BN) of the two shapes whose kernels implement the form
EPI_ACT_FLOPS = 60                           # per output sample: 2 x 6-tap up-FIR, two snakes, 12-tap down-FIR


def epi_act_tiling(ncols: int, bn: int):
    """The overlapping column tiles of the form: [(first conv column, first stored column, stored columns)], tile t
    computing conv columns [t (bn - 16) - 8, t (bn - 16) + bn - 8) and storing from t (bn - 16) on."""
    seg = bn - 16
    return [(t * seg - 8, t * seg, min(seg, ncols - t * seg)) for t in range(-(-ncols // seg))]


def epi_act_plan_ok(plan) -> bool:
    """Does the PLAIN launch of the conv take one of the two shapes that carry the form (``plan``: the four numbers of
    hsp_conv1d_mfma_plan)?  Only then is the fused launch the same sum, in the same order, as the plain one."""
    return int(plan[2]) > 0 and (int(plan[0]), int(plan[1])) in EPI_ACT_TILES


def epi_act_eligible(cin: int, cout: int, L_: int, *, fft_first: bool, fft_second: bool, row_exact: bool, plan) -> bool:
    """amp_pair's rule for c2(c1(a1(x), epi_act=a2)): the form switched on, both convs direct, at most 64 channels, whole
    float4 rows, no row-exact batch (the ragged activation has no epilogue form), the plain launch of c1 on one of the
    form's shapes (epi_act_plan_ok).  No shape is excluded by measurement: the fused launch beat conv + activation on
    every one of profiles/epi_act_bench.txt."""
    if not EPI_ACT or fft_first or fft_second or row_exact:
        return False
    if cin > 64 or cout > 64 or L_ % 4 != 0:
        return False
    return plan is not None and epi_act_plan_ok(plan)


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def plain_rows(cout: int) -> np.ndarray:
    """packed row -> source output channel (-1 = zero padding); M multiple of 4."""
    m = _round_up(cout, 4)
    rows = np.full(m, -1, np.int64)
    rows[:cout] = np.arange(cout)
    return rows


def gated_rows(half: int) -> np.ndarray:
    """Row order of the GATE modes: 32-row blocks alternate between the 'a' half
    (tanh / linear) and the matching 'b' half (sigmoid) so that one wave holds both
    accumulators of an output channel (hsp_conv1d_mfma.hip epilogue)."""
    assert half % 32 == 0, "gated convs need a half-width that is a multiple of 32"
    m = np.arange(2 * half)
    return ((m >> 5) & 1) * half + (m >> 6) * 32 + (m & 31)


def conv_pack_map(cout: int, cin: int, k: int, rows: np.ndarray) -> np.ndarray:
    """index map src[Cout, Cin, K] -> dst[K][Cin][M]."""
    M = rows.shape[0]
    j = np.arange(k)[:, None, None]
    ci = np.arange(cin)[None, :, None]
    co = rows[None, None, :]
    idx = (co * cin + ci) * k + j
    idx = np.where(co >= 0, idx, -1)
    return np.ascontiguousarray(np.broadcast_to(idx, (k, cin, M))).astype(np.int32).reshape(-1)


def convtr_pack_map(cin: int, cout: int, k: int, up: int) -> Tuple[np.ndarray, int, int]:
    """ConvTranspose1d(stride=up) as a polyphase conv: returns (map, K', M).

    y[co, n] = sum_ci sum_i x[ci, i] * w[ci, co, n + p - up*i]; writing n + p = up*q + r
    gives, for packed row m = co*up + r and tap j' (input index q + j' - (K'-1)),
    the source tap r + (K'-1-j')*up (absent taps are zero).  src is w[Cin, Cout, K]."""
    kp = -(-k // up)
    M = _round_up(cout * up, 4)
    m = np.arange(M)
    co, r = m // up, m % up
    jp = np.arange(kp)[:, None, None]
    ci = np.arange(cin)[None, :, None]
    tap = r[None, None, :] + (kp - 1 - jp) * up
    idx = (ci * cout + co[None, None, :]) * k + tap
    ok = (tap < k) & (co[None, None, :] < cout)
    return np.where(ok, idx, -1).astype(np.int32).reshape(-1), kp, M


# ---------------------------------------------------------------------------- arena
class WeightArena:
    """One contiguous fp32 device buffer holding every packed tensor of a model."""

    ALIGN = 64  # floats (256 B): keeps float4 weight loads aligned

    def __init__(self):
        self.specs: List[Tuple[object, str, int]] = []
        self.buffer: Optional[torch.Tensor] = None
        self.views: Dict[Tuple[int, str], torch.Tensor] = {}
        self._offsets: List[int] = []
        self.total = 0

    def request(self, owner, name: str, numel: int):
        self._offsets.append(self.total)
        self.specs.append((owner, name, numel))
        self.total += _round_up(numel, self.ALIGN)

    def allocate(self, device):
        self.buffer = torch.zeros(max(self.total, 1), dtype=torch.float32, device=device)
        for (owner, name, numel), off in zip(self.specs, self._offsets):
            self.views[(id(owner), name)] = self.buffer[off:off + numel]

    def view(self, owner, name: str) -> torch.Tensor:
        return self.views[(id(owner), name)]


# Bumped whenever a HipLayer's parameters move (``.cuda()`` / ``.to(device)``) or are reloaded
# (``load_state_dict``): a top-level mirror compares its own stamp with this counter on every entry call -- one
# integer compare on the hot path -- and only walks its layers when something changed anywhere (ensure_ready()).
_EPOCH = 0


def _bump_epoch():
    global _EPOCH
    _EPOCH += 1


class HipLayer(nn.Module):
    """Base of modules that own packed device state.  ``_hsp_stale`` says the packed copy no longer matches the
    parameters (never packed, parameters moved to another device, or reloaded)."""

    _hsp_stale = True

    def hsp_requests(self) -> List[Tuple[str, int]]:
        return []

    def hsp_fill(self, arena: WeightArena, materialize: bool) -> None:
        pass

    def _apply(self, fn, *args, **kw):
        before = [(q.device, q.data_ptr()) for q in self._parameters.values() if q is not None]
        r = super()._apply(fn, *args, **kw)
        after = [(q.device, q.data_ptr()) for q in self._parameters.values() if q is not None]
        if before != after:
            self.__dict__["_hsp_stale"] = True
            _bump_epoch()
        return r

    def _load_from_state_dict(self, *args, **kw):
        r = super()._load_from_state_dict(*args, **kw)
        self.__dict__["_hsp_stale"] = True
        _bump_epoch()
        return r


def ensure_ready(model: nn.Module) -> None:
    """Drop-in behaviour of the reference's call sites (``Model(...).cuda()``, ``load_state_dict``, ``.eval()``,
    then inference methods: inference_plm.py:215-262): the first inference call after the parameters moved or
    changed folds / packs the weights on the device the parameters live on.  An explicit ``finalize(device)`` stays
    available (multi-GPU jobs lay the arena out without materialising it).  Raises on CPU: no CPU fallback."""
    if model.__dict__.get("_hsp_epoch") == _EPOCH:
        return
    if any(m._hsp_stale for m in model.modules() if isinstance(m, HipLayer)):
        p = next(model.parameters(), None)
        dev = p.device if p is not None else torch.device("cpu")
        if dev.type != "cuda":
            raise L.HspError(f"{type(model).__name__}: parameters are on {dev}; move the model to a ROCm device "
                             "(.cuda() / .to(device)) -- the product path has no CPU fallback")
        fin = getattr(model, "finalize", None)
        if fin is not None:
            fin(dev)
        else:
            finalize(model, dev)
    model.__dict__["_hsp_epoch"] = _EPOCH


def entry(fn):
    """Decorator of a mirror's public inference methods: pack the weights on first use (ensure_ready)."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *args, **kw):
        ensure_ready(self)
        return fn(self, *args, **kw)
    return wrapped


def _gather(src: torch.Tensor, idx_map: np.ndarray, dst: torch.Tensor):
    # the kernel walks dst.numel() consecutive floats and one int32 map entry for each of them
    assert dst.is_contiguous() and src.is_contiguous(), "hsp_gather_f32 reads and writes flat buffers"
    assert idx_map.dtype == np.int32 and idx_map.size == dst.numel() and idx_map.flags["C_CONTIGUOUS"]
    mp = torch.from_numpy(idx_map).to(src.device)
    L.call("hsp_gather_f32", L.fptr(src), L.ptr(mp), L.fptr(dst), dst.numel())
    # `mp` must outlive the asynchronous gather on the current stream
    torch.cuda.current_stream().synchronize()


def _fold(v: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    rows = v.shape[0]
    cols = v.numel() // rows
    # contiguous whatever v's strides are: the kernel writes rows of `cols` consecutive floats (empty_like would keep
    # the strides of a permuted v and the rows would land in the wrong places)
    w = torch.empty(v.shape, dtype=v.dtype, device=v.device)
    vc, gc = v.contiguous(), g.contiguous()          # named: a copy made here must live until the launch is issued
    assert gc.numel() == rows
    L.call("hsp_fold_weight_norm_f32", L.fptr(vc), L.fptr(gc), L.fptr(w), rows, cols)
    return w


def _spectrum(Cc: int, Np: int, device) -> torch.Tensor:
    """[64 bins][2 C][Np] spectrum buffer of a frequency-domain conv.  (Round 6 measured a padded plane stride -- 64 or 1088
    floats between the bins, so that the 128 scattered 128-B runs of a column do not share an address pattern modulo the HBM
    channel interleave: no effect on any transform kernel, 147.3 / 147.7 / 147.9 us per inverse launch,
    profiles/r06_plane_pad.txt; the knob is gone.)"""
    return torch.empty(64, 2 * Cc, Np, dtype=torch.float32, device=device)


class _ConvBase(HipLayer):
    def __init__(self, weight_shape, rows0: int, bias: bool, weight_norm: bool):
        super().__init__()
        if weight_norm:
            self.weight_g = nn.Parameter(torch.ones(rows0, 1, 1), requires_grad=False)
            self.weight_v = nn.Parameter(torch.zeros(*weight_shape), requires_grad=False)
        else:
            self.weight = nn.Parameter(torch.zeros(*weight_shape), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(bias), requires_grad=False) if bias else None
        self.has_bias = bool(bias)
        self.wn = weight_norm
        self._w: Optional[torch.Tensor] = None
        self._b: Optional[torch.Tensor] = None
        self._wf: Optional[torch.Tensor] = None     # per-bin matrices of the frequency-domain form (Conv1d.ensure_wf)

    def _folded(self) -> torch.Tensor:
        if self.wn:
            return _fold(self.weight_v.data, self.weight_g.data)
        return self.weight.data.contiguous()

    def _bias_src(self) -> torch.Tensor:
        return self.bias.data

    def _require_ready(self):
        if self._w is None:
            raise L.HspError(f"{type(self).__name__} used before finalize(): call model.finalize(device) after "
                             "loading weights")


class Conv1d(_ConvBase):
    """torch.nn.Conv1d (optionally weight-normed) with fused prologue/epilogue."""

    def __init__(self, cin, cout, k, stride=1, padding=0, dilation=1, bias=True, weight_norm=False,
                 rows=L.ROWS_PLAIN, weight_2d=False):
        super().__init__((cout, cin) if weight_2d else (cout, cin, k), cout, cout if bias else 0, weight_norm)
        self.cin, self.cout, self.k, self.stride, self.padding, self.dilation = cin, cout, k, stride, padding, dilation
        self.rows = rows
        self.trim_right = 0   # outputs dropped at the end (an even kernel with padding k // 2 yields one too many)
        if rows in (L.ROWS_GATE_WN, L.ROWS_GATE_GLU):
            self.row_map = gated_rows(cout // 2)
        else:
            self.row_map = plain_rows(cout)
        self.M = int(self.row_map.shape[0])
        # options (each set by the method named) and the buffers derived from them, all "off"
        self.packed = True                           # False: parameters only, the rows are packed into a StackedLinearCT
        self._pre_norm, self._c1 = None, None        # fuse_input_layernorm
        self._rowmajor, self._wt = False, None       # keep_rowmajor_weight
        self._flip_in = self._flip_out = False       # pack_flipped
        self._fft, self._wf_form = False, None       # enable_fft; the form `_wf` holds (ensure_wf)
        self._fft_ok: Dict[Tuple[int, int], bool] = {}     # fft_supported by (B, L): hierspeechpp_speechsynthesizer.fft_wins

    def fuse_input_layernorm(self, norm):
        """Run ``norm`` (an affine LayerNorm over the input channels: attributes ``weight``/``gamma``,
        ``bias``/``beta``, ``eps``) inside this 1x1 layer's GEMM: the packed weight becomes W diag(gamma), the
        bias W beta + b, and ``ln_c1`` the row sums of the packed weight (hsp_conv1d_args.ln_c1).  The layer is
        then called on the UN-normalised input."""
        assert self.k == 1 and self.rows == L.ROWS_PLAIN
        # past nn.Module.__setattr__, which would register the norm as a sub-module: it stays where the reference keeps
        # it, and a second registration would duplicate its state_dict keys under this layer's prefix
        self.__dict__["_pre_norm"] = norm

    def _ln_params(self):
        n = self._pre_norm
        g = (n.weight if hasattr(n, "weight") else n.gamma).data
        b = (n.bias if hasattr(n, "weight") else n.beta).data
        return g, b

    def keep_rowmajor_weight(self):
        """Also keep the folded weight as stored -- [cout][cin] row-major -- in the arena (``_wt``): the A operand of
        the projection inside hsp_mha_proj_f32 (attention + output projection in one launch)."""
        assert self.k == 1 and self.rows == L.ROWS_PLAIN
        self._rowmajor = True

    def pack_flipped(self, inputs: bool = False, outputs: bool = False):
        """Pack this layer for a tensor whose channel axis is stored REVERSED: ``inputs`` -- the input channels arrive in
        reverse order (the packed weight's input columns are reversed), ``outputs`` -- the output channels are to be
        written in reverse order (rows and bias reversed).  The parameters and their state-dict keys stay as the
        reference stores them; only the packed copy changes.  This is how modules.Flip (modules.py:270-277) between two
        coupling layers costs no launch: the layer after a Flip reads and writes the un-flipped tensor through a packed
        weight that has the permutation in it (modules.ResidualCouplingLayer_Transformer_simple.flipped)."""
        assert self.rows == L.ROWS_PLAIN and self._pre_norm is None and not self._rowmajor
        self._flip_in, self._flip_out = bool(inputs), bool(outputs)
        self.__dict__["_hsp_stale"] = True
        _bump_epoch()

    def hsp_requests(self):
        if not self.packed:
            return []
        fused = self._pre_norm is not None
        return [("w", self.k * self.cin * self.M)] + ([("b", self.cout)] if self.has_bias or fused else []) + \
            ([("c1", self.cout)] if fused else []) + \
            ([("wt", self.cout * self.cin)] if self._rowmajor else [])

    def enable_fft(self):
        """This same-length stride-1 conv may also run in its frequency-domain form (round 4, csrc/hsp_dftseg.hip):
        ``forward_fft`` computes it as forward DFT -> one batched channel product over the 64 bins -> inverse DFT, 1.7 (2.2
        in the block form) multiply-adds per output and channel pair instead of k.  The per-bin matrices of conj(rfft(w,
        128)) are DERIVED data: they are not part of the weight arena (what a multi-GPU job broadcasts) but
        a side buffer that ``ensure_wf`` fills from the packed taps on first use, on every rank, with
        hsp_dftseg_weight_spectrum_f32 -- a model that never meets a batch large enough for the form (fft_wins) never
        allocates them (201 MB per conv at 512 channels)."""
        assert self.stride == 1 and self.rows == L.ROWS_PLAIN and self.cin == self.cout and 2 <= self.k <= 64
        assert self.padding * 2 == (self.k - 1) * self.dilation, "same-length conv"
        self._fft = True

    def fft_form(self) -> str:
        return "three" if FFT_PRODUCT == "three" and self.cin % 64 == 0 else "block"

    def ensure_wf(self):
        """The per-bin matrices of this conv's channel product, derived on the device from the packed taps (``_w``:
        [k][C][M]) in float64 and rounded once: [64][3][C][C] = (a + b, a, b) of conj(W) = a + i b for hsp_cprod3_f32, or
        round 4's [64][2C][2C] block matrices.  Deterministic: every rank derives the same bits from the same taps."""
        if self._wf is not None and self._wf_form == self.fft_form():
            return self._wf
        self._require_ready()
        if torch.cuda.is_current_stream_capturing():
            raise L.HspError("ensure_wf() inside a stream capture: run one eager call first (or prepare_fft(model))")
        Cc, form = self.cin, self.fft_form()
        wf = torch.empty(64 * (3 if form == "three" else 4) * Cc * Cc, dtype=torch.float32, device=self._w.device)
        L.call("hsp_dftseg_weight_spectrum_f32", L.fptr(self._w), self.k, Cc, self.M,
               L.ptr(_wspec_twiddles(self._w.device)), L.fptr(wf), L.WSPEC_THREE if form == "three" else L.WSPEC_BLOCK)
        self._wf, self._wf_form = wf, form
        return wf

    def hsp_fill(self, arena, materialize):
        if not self.packed:
            return
        fused = self._pre_norm is not None
        self._w = arena.view(self, "w")
        self._b = arena.view(self, "b") if self.has_bias or fused else None
        self._c1 = arena.view(self, "c1") if fused else None
        self._wt = arena.view(self, "wt").view(self.cout, self.cin) if self._rowmajor else None
        self._wf = None                                   # derived from _w on first use (ensure_wf)
        if materialize:
            w = self._folded()
            if self._flip_in:
                w = w.flip(1).contiguous()
            if self._flip_out:
                w = w.flip(0).contiguous()
            if self._wt is not None:
                assert not fused
                self._wt.copy_(w.reshape(self.cout, self.cin))
            if fused:
                g, beta = self._ln_params()
                w2 = w.reshape(self.cout, self.cin).double()
                wg = w2 * g.double()[None, :]
                self._c1.copy_(wg.sum(1).float())
                c2 = w2 @ beta.double()
                if self.has_bias:
                    c2 = c2 + self._bias_src().double()
                self._b.copy_(c2.float())
                w = wg.float().reshape(w.shape).contiguous()
            _gather(w, conv_pack_map(self.cout, self.cin, self.k, self.row_map), self._w)
            if self._b is not None and not fused:
                self._b.copy_(self._bias_src().flip(0) if self._flip_out else self._bias_src())

    # The frequency-domain form in pieces (forward_fft strings them together; an AMP pair fuses the inverse of its first
    # conv with the forward transform of its second: forward_fft_pair)
    def _fft_args(self, B, Lx):
        """hsp_dftseg_args of this conv for a [B, C, Lx] tensor: geometry only, no pointers."""
        d, k = self.dilation, self.k
        hop = 129 - k
        nseg = -(-(-(-Lx // d)) // hop)
        da = L.DftSegArgs()
        da.B, da.C, da.L, da.k, da.dil, da.pad, da.nseg = B, self.cin, Lx, k, d, self.padding, nseg
        da.Np = _round_up(B * d * nseg, 4)
        da.post_scale = 1.0
        da.prod3 = int(self.fft_form() == "three")
        return da

    @staticmethod
    def _fft_point(da, xf, table):
        """Point hsp_dftseg_args at a spectrum buffer [64][2 C][Np] and a transform table."""
        da.xf, da.xf_bs, da.dft = L.fptr(xf), xf.stride(0), L.fptr(table)

    def _fft_probe(self, B, Lx, dummy=None):
        """What a *_supported predicate is asked with: geometry, a dense plane stride, ``dummy`` pointers (none is read)."""
        da = self._fft_args(B, Lx)
        da.xf_bs = 2 * self.cin * da.Np
        da.xf = da.dft = da.act_alpha_exp = da.act_beta_inv = da.act_filt = dummy
        return da

    def fft_supported(self, B, Lx) -> bool:
        """Do the transform kernels take this geometry (hsp_dftseg_supported: dilation <= 8, a spectrum below 4 GiB per
        launch, item counts within int)?  fft_wins asks before choosing the form; beyond it the direct conv runs."""
        return self._fft and bool(L.lib().hsp_dftseg_supported(C.byref(self._fft_probe(B, Lx))))

    @staticmethod
    def _fft_set_act(da, x_like, act1d):
        if act1d._ea is None:
            raise L.HspError("Activation1d used before finalize()")
        da.act_alpha_exp, da.act_beta_inv, da.act_filt = L.fptr(act1d._ea), L.fptr(act1d._binv), L.fptr(act1d._filt)
        rows = _ROWS.get()      # row-exact: the ragged activation (hsp_dftseg_args.act_len)
        if rows is not None:
            da.act_len = L.ptr(rows.at(x_like.shape[2]))

    def _fft_forward(self, x, act1d=None):
        """x [B, C, L] -> spectrum [64][2 C][Np] (hsp_dftseg_fwd_f32), the activation applied on the way if given."""
        B, Cc, Lx = x.shape
        assert Cc == self.cin and x.stride(2) == 1 and self._fft
        da = self._fft_args(B, Lx)
        xf = _spectrum(Cc, da.Np, x.device)
        da.x, da.x_bs, da.x_cs = L.fptr(x), x.stride(0), x.stride(1)
        self._fft_point(da, xf, _dft_tables(x.device)[0])
        if act1d is not None:
            if not fft_act_fusable(x):
                raise L.HspError("forward_fft(act1d=...) needs 16-B addressable rows")
            self._fft_set_act(da, x, act1d)
        _, e0, _ = _bracket("hsp_dftseg_fwd_f32", lambda: L.lib().hsp_dftseg_fwd_f32(C.byref(da), L.stream_ptr()),
                            2 * 2 * 64 * 64 * B * Cc * da.dil * da.nseg, 4 * (B * Cc * Lx + 128 * Cc * da.Np), None)
        return xf, e0

    def _fft_product(self, xf):
        """ONE batched launch over the 64 bins: yf[bin] = conj(W)[bin] xf[bin] -- three real C x C products per bin
        (hsp_cprod3_f32) or the [2C x 2C] block matrix [[Wr, Wi], [-Wi, Wr]] on the conv kernel."""
        Cc, Np = self.cin, xf.shape[2]
        wf = self.ensure_wf()
        yf = _spectrum(Cc, Np, xf.device)
        if self._wf_form == "three":
            pa = L.Cprod3Args()
            pa.xf, pa.yf, pa.w, pa.zeros = L.fptr(xf), L.fptr(yf), L.fptr(wf), L.fptr(_zeros(xf.device))
            pa.xf_bs, pa.yf_bs, pa.bins, pa.C, pa.Np, pa.debug = xf.stride(0), yf.stride(0), 64, Cc, Np, DEBUG_FLAGS
            _bracket("hsp_cprod3_f32", lambda: L.lib().hsp_cprod3_f32(C.byref(pa), L.stream_ptr()),
                     2 * 64 * 3 * Cc * Cc * Np, 4 * (64 * 2 * 2 * Cc * Np + 64 * 3 * Cc * Cc), None)
            return yf
        a = L.Conv1dArgs()
        _set_in(a, xf)                               # the 64 bins are the batch: [64][2 C][Np]
        a.w, a.K, a.dil, a.pad, a.stride = L.fptr(wf), 1, 1, 0, 1
        a.M, a.w_ld, a.w_bs = 2 * Cc, 2 * Cc, 4 * Cc * Cc
        _set_out(a, yf, 64, 2 * Cc, Np)
        a.ncols, a.rows, a.scale, a.post_scale = Np, L.ROWS_PLAIN, 1.0, 1.0
        ConvLaunch("hsp_conv1d_mfma_f32", L.lib().hsp_conv1d_mfma_f32, a, 2 * 64 * 4 * Cc * Cc * Np,
                   4 * (64 * 2 * 2 * Cc * Np + 64 * 4 * Cc * Cc), yf, (xf, yf, wf)).run()
        return yf

    def _fft_inverse_args(self, yf, B, Lx):
        da = self._fft_args(B, Lx)
        self._fft_point(da, yf, _dft_tables(yf.device)[1])
        da.bias = L.fptr(self._b) if self._b is not None else None
        return da

    def _fft_inverse(self, yf, B, Lx, *, res=None, out=None, accumulate=False, post_scale=1.0, before_inverse=None):
        Cc = self.cin
        if out is None:
            out = torch.empty(B, Cc, Lx, dtype=torch.float32, device=yf.device)
        assert out.shape == (B, Cc, Lx) and out.stride(2) == 1 and (res is None or (res.shape == out.shape and res.stride(2) == 1))
        if before_inverse is not None:
            torch.cuda.current_stream(yf.device).wait_event(before_inverse)
        da = self._fft_inverse_args(yf, B, Lx)
        da.y, da.y_bs, da.y_cs = L.fptr(out), out.stride(0), out.stride(1)
        if res is not None:
            da.res, da.res_bs, da.res_cs = L.fptr(res), res.stride(0), res.stride(1)
        da.accumulate, da.post_scale = int(bool(accumulate)), float(post_scale)
        _, _, e1 = _bracket("hsp_dftseg_inv_f32", lambda: L.lib().hsp_dftseg_inv_f32(C.byref(da), L.stream_ptr()),
                            2 * 2 * 64 * 64 * B * Cc * da.dil * da.nseg,
                            4 * (B * Cc * Lx * (self._fft_nio(res, accumulate) - 1) + 128 * Cc * da.Np), None)
        return out, e1

    @staticmethod
    def _fft_nio(res, accumulate) -> int:      # [B, C, L] tensors moved through HBM: in, out, residual, running sum twice
        return 2 + bool(res is not None) + 2 * bool(accumulate)

    def _fft_report(self, x, taps, res, accumulate, e_first, e_last, arg):
        """The summary record "hsp_fftconv": the launches of the form are booked with the flops / bytes they EXECUTE, the
        conv(s) they stand for once more as a whole -- algorithmic flops and bytes of the direct form with ``taps`` taps,
        from the first launch's start event to the last launch's end event."""
        B, Cc, Lx = x.shape
        _bracket("hsp_fftconv", None, 2 * B * Cc * Cc * taps * Lx,
                 4 * B * Cc * Lx * self._fft_nio(res, accumulate) + 4 * taps * Cc * Cc, arg, span=(e_first, e_last))

    def forward_fft(self, x, *, res=None, out=None, accumulate=False, post_scale=1.0, act1d=None, before_inverse=None):
        """The conv in its frequency-domain form (enable_fft()): three launches -- forward DFT of 128-sample segments,
        ONE 1x1 product over the 64 bins on the conv kernel (hsp_conv1d_args.w_bs), inverse DFT with the conv's epilogue
        (bias, residual, running sum, post_scale).  x [B, C, L] with unit time stride.  ``act1d``: the Activation1d in
        front of the conv, applied by the forward transform while it stages its input (needs 16-B addressable rows:
        fft_act_fusable).  ``before_inverse``: an event the stream waits on before the inverse transform, the only launch
        that touches ``out``."""
        self._require_ready()
        B, _, Lx = x.shape
        xf, e_first = self._fft_forward(x, act1d)
        yf = self._fft_product(xf)
        out, e_last = self._fft_inverse(yf, B, Lx, res=res, out=out, accumulate=accumulate, post_scale=post_scale,
                                        before_inverse=before_inverse)
        self._fft_report(x, self.k, res, accumulate, e_first, e_last, None)
        return out

    def fft_pair_ok(self, second, x) -> bool:
        """Can the inverse transform of this conv be fused with the activation and the forward transform of ``second``
        (hsp_dftseg_pair_f32) for an input like x?  Both unchunked and their two LDS stretches within one CU's 160 KB."""
        if not self._fft or not second._fft or second.cin != self.cin or x.shape[2] % 4:
            return False
        B, _, Lx = x.shape
        dummy = L.fptr(_zeros(x.device))
        ia, fa = self._fft_probe(B, Lx, dummy), second._fft_probe(B, Lx, dummy)
        return bool(L.lib().hsp_dftseg_pair_supported(C.byref(ia), C.byref(fa)))

    def _fft_pair_launch(self, second, yf, B, Lx, act_second, like):
        """ONE launch (hsp_dftseg_pair_f32): inverse transform of this conv's product ``yf`` + bias -> ``act_second`` ->
        forward transform for ``second``.  Returns second's spectrum."""
        Cc = self.cin
        ia = self._fft_inverse_args(yf, B, Lx)
        fa = second._fft_args(B, Lx)
        xf2 = _spectrum(Cc, fa.Np, yf.device)
        self._fft_point(fa, xf2, _dft_tables(yf.device)[0])
        self._fft_set_act(fa, like, act_second)
        _bracket("hsp_dftseg_pair_f32", lambda: L.lib().hsp_dftseg_pair_f32(C.byref(ia), C.byref(fa), L.stream_ptr()),
                 2 * 2 * 64 * 64 * B * Cc * (ia.dil * ia.nseg + fa.dil * fa.nseg), 4 * 128 * Cc * (ia.Np + fa.Np), None)
        return xf2

    def forward_fft_pair(self, second, x, *, act_first, act_second, res=None, out=None, accumulate=False, post_scale=1.0,
                         before_inverse=None):
        """second(act_second(self(act_first(x)))) [+ res ...] with both convs in the frequency domain and the tensor between
        them never in HBM: forward(x) -> product(self) -> [inverse + bias + act_second + forward] -> product(second) ->
        inverse with second's epilogue.  Five launches instead of six (eight with the activations)."""
        self._require_ready()
        second._require_ready()
        B, _, Lx = x.shape
        xf, e_first = self._fft_forward(x, act_first)
        yf = self._fft_product(xf)
        xf2 = self._fft_pair_launch(second, yf, B, Lx, act_second, x)
        yf2 = second._fft_product(xf2)
        out, e_last = second._fft_inverse(yf2, B, Lx, res=res, out=out, accumulate=accumulate, post_scale=post_scale,
                                          before_inverse=before_inverse)
        self._fft_report(x, self.k + second.k, res, accumulate, e_first, e_last, 2)   # (two convs)
        return out

    # ----------------------------------------------------------------------------
    def prepare(self, x, **kw) -> ConvLaunch:
        """The launch ``forward(x, **kw)`` would issue, built and not issued, for a caller of launch_group -- which takes
        plain GEMMs only: ``split_out`` and the fused input LayerNorm have launch protocols that are forward's alone."""
        if self._pre_norm is not None or "split_out" in kw:
            raise L.HspError("prepare(): split-row and fused-LayerNorm launches go through forward() only")
        return self._prepare(x, **kw)

    def _prepare(self, x, *, act1d=None, lrelu: Optional[float] = None, silu_in=False, act=L.ACT_NONE, cbias=None,
                mask=None, mask_mode=L.MASK_NONE, cscale=None, scale=1.0, res=None, out=None, accumulate=False,
                post_scale=1.0, force_direct=False, row_range=None, split_out=None, mask_mode2=L.MASK_NONE,
                epi_act=None) -> ConvLaunch:
        """The launch of this conv on x [B, Cin, L], built and not issued: geometry, the output (allocated when None),
        the filled struct, the direct-versus-MFMA choice.  ``row_range=(r0, r1)`` computes only output channels [r0, r1)
        (PLAIN rows, r0 % 4 == 0): the WN res/skip layer is one parameter set feeding two differently-fused launches.
        ``split_out=(split_row, out2, accumulate2)``: ONE launch for both halves of such a layer
        (hsp_conv1d_args.split_row): rows [0, split_row) -> the usual output with this call's epilogue, rows
        [split_row, cout) -> ``out2`` (+= if accumulate2; allocated when None); the launch's ``out`` is then (out, out2).
        ``epi_act=<Activation1d>``: the launch stores that activation of the conv's output (hsp_conv1d_args.act = HSP_ACT_ACT1D);
        the caller has checked the form's conditions (epi_act_eligible), the library refuses anything else."""
        self._require_ready()
        if act1d is not None and _ROWS.get() is not None:
            raise L.HspError("row_exact: the conv-prologue Activation1d (HSP_FUSE_ACT_MAX_C > 0) has no ragged form")
        B, Cin, Lin = x.shape
        assert Cin == self.cin, (Cin, self.cin)
        gated = self.rows in (L.ROWS_GATE_WN, L.ROWS_GATE_GLU)
        cout = self.cout // 2 if gated else self.cout
        r0 = 0
        if row_range is not None:
            r0, r1 = row_range
            assert not gated and r0 % 4 == 0 and 0 <= r0 < r1 <= self.cout
            cout = r1 - r0
        Lout = (Lin + 2 * self.padding - self.dilation * (self.k - 1) - 1) // self.stride + 1 - self.trim_right
        out2 = None
        if split_out is not None:
            split_row, out2, acc2 = split_out
            assert row_range is None and not gated and self.k == 1 and 0 < split_row < self.cout
            cout = split_row
            if out2 is None:
                assert not acc2
                out2 = torch.empty(B, self.cout - split_row, Lout, dtype=torch.float32, device=x.device)
        if out is None:
            out = torch.empty(B, cout, Lout, dtype=torch.float32, device=x.device)
        a = L.Conv1dArgs()
        _set_in(a, x)
        a.w, a.K, a.dil, a.pad, a.stride = L.fptr(self._w) + 4 * r0, self.k, self.dilation, self.padding, self.stride
        a.M = self.M if row_range is None else _round_up(cout, 4)
        a.w_ld = self.M
        _set_out(a, out, B, cout, Lout)
        a.ncols = Lout
        a.rows, a.gate_half = self.rows, (cout if gated else 0)
        a.bias = (L.fptr(self._b) + 4 * r0) if self._b is not None else None
        _set_epilogue(a, act, cbias, mask, mask_mode, cscale, scale, res, accumulate, post_scale, out)
        if act1d is not None:
            a.prologue = L.PRO_ACT1D
            a.alpha_exp, a.beta_inv, a.filt = L.fptr(act1d._ea), L.fptr(act1d._binv), L.fptr(act1d._filt)
        elif lrelu is not None:
            a.prologue, a.slope = L.PRO_LRELU, float(lrelu)
        elif silu_in:
            a.prologue = L.PRO_SILU
        if self._pre_norm is not None:
            a.ln_c1, a.ln_eps = L.fptr(self._c1), float(self._pre_norm.eps)
            assert not force_direct and row_range is None
        direct = _wants_direct(a, force_direct, silu_in)
        if direct and a.res_ts > 1:
            # the VALU kernel reads its residual at unit column stride (hsp_conv1d_args.res_ts is the register-path
            # token GEMM's): gather it first -- e.g. the PLM's last layer at B = 4, whose [D, 4] product is below the MFMA path
            res = Fh.copy_strided(res)
            a.res, a.res_bs, a.res_cs, a.res_ts = L.fptr(res), res.stride(0), res.stride(1), 0
        rows_full = cout * (2 if gated else 1)
        flops = 2 * B * rows_full * Cin * self.k * Lout
        # algorithmic traffic: input once, output once (+ residual / accumulate reads), weights once
        nbytes = 4 * (B * Cin * Lin + B * cout * Lout * (1 + (res is not None) + bool(accumulate))
                      + rows_full * Cin * self.k)
        if split_out is not None:                   # the split-row kernel is an MFMA one
            direct = False
            a.Cout = self.cout                      # rows [split_row, cout) go to the second output
            a.split_row, a.accumulate2, a.mask_mode2 = split_row, int(bool(acc2)), mask_mode2   # (the second output shares `mask`)
            a.y2, a.y2_bs, a.y2_cs = L.fptr(out2), out2.stride(0), out2.stride(1)
            flops = 2 * B * self.cout * Cin * Lout
            nbytes += 4 * B * (self.cout - split_row) * Lout * (1 + bool(acc2))
        if epi_act is not None:
            if direct or _ROWS.get() is not None:
                raise L.HspError("epi_act: the activation epilogue is the MFMA path's, and has no ragged form")
            if act != L.ACT_NONE or a.prologue != L.PRO_NONE:
                raise L.HspError("epi_act: no pointwise act and no prologue beside the activation epilogue")
            a.act = L.ACT_ACT1D                          # (alpha_exp / beta_inv / filt are the epilogue's then: per OUTPUT channel)
            a.alpha_exp, a.beta_inv, a.filt = L.fptr(epi_act._ea), L.fptr(epi_act._binv), L.fptr(epi_act._filt)
            flops += EPI_ACT_FLOPS * B * cout * Lout     # (nbytes as they are: input once, output once -- now the activated one)
        kind, fn = ("hsp_conv1d_direct_f32", L.lib().hsp_conv1d_direct_f32) if direct else \
            ("hsp_conv1d_mfma_f32", L.lib().hsp_conv1d_mfma_f32)
        if not direct:
            _set_fold_cols(a)
        return ConvLaunch(kind, fn, a, flops, nbytes, out if out2 is None else (out, out2),
                          (x, out, out2, res, cbias, mask, cscale, epi_act))

    def plain_plan(self, x):
        """(BM, BN, KC, LDS bytes) of the plain MFMA launch of this conv on x, or None where the library has none (or the
        VALU kernel takes it): what amp_pair asks before it fuses the next activation into the launch.  Cached per shape."""
        key = (tuple(x.shape), x.stride(), x.data_ptr() % 16)
        cache = self.__dict__.setdefault("_plain_plans", {})
        if key not in cache:
            p = self._prepare(x, out=x)          # (no launch: the output pointer only stands for an aligned buffer)
            plan = (C.c_int32 * 4)()
            p.args.debug = DEBUG_FLAGS
            ok = p.kind == "hsp_conv1d_mfma_f32" and L.lib().hsp_conv1d_mfma_plan(C.byref(p.args), C.byref(plan)) == 0
            cache[key] = tuple(plan) if ok else None
        return cache[key]

    def forward(self, x, **kw):
        """``_prepare`` (see there for the arguments) plus one of three launch protocols.  Returns the output; with ``split_out``
        (out, out2), or None when the library has no fused kernel for the shape (the caller then launches the halves)."""
        p = self._prepare(x, **kw)
        if kw.get("split_out") is not None:
            return None if p.run(soft=True) else p.out
        if self._pre_norm is None:
            p.run()
        elif p.run(soft=True):
            # fused input LayerNorm: token-GEMM shapes only (16-B addressable columns).  Anything else runs the
            # normalisation as its own launch -- WITHOUT the affine part, which is folded into the packed weights
            # (W diag(gamma), W beta + b) -- and then the same GEMM (an MFMA one: _wants_direct): identical arithmetic.
            xn = Fh.layernorm_mod(x, float(self._pre_norm.eps))
            _set_in(p.args, xn)
            p.args.ln_c1 = None
            _set_fold_cols(p.args)
            p.run()
        return p.out


class ConvTranspose1d(_ConvBase):
    """torch.nn.ConvTranspose1d (weight-normed) as a polyphase conv on the MFMA kernel."""

    def __init__(self, cin, cout, k, stride, padding=0, bias=True, weight_norm=False):
        super().__init__((cin, cout, k), cin, cout if bias else 0, weight_norm)
        self.cin, self.cout, self.k, self.up, self.padding = cin, cout, k, stride, padding
        self.pack_map, self.kp, self.M = convtr_pack_map(cin, cout, k, stride)

    def hsp_requests(self):
        return [("w", self.kp * self.cin * self.M)] + ([("b", self.cout)] if self.bias is not None else [])

    def hsp_fill(self, arena, materialize):
        self._w = arena.view(self, "w")
        self._b = arena.view(self, "b") if self.bias is not None else None
        if materialize:
            _gather(self._folded(), self.pack_map, self._w)
            if self._b is not None:
                self._b.copy_(self.bias.data)

    def prepare(self, x, *, res=None, out=None, lrelu: Optional[float] = None) -> ConvLaunch:
        self._require_ready()
        B, Cin, Lin = x.shape
        assert Cin == self.cin
        Lout = (Lin - 1) * self.up - 2 * self.padding + self.k
        if out is None:
            out = torch.empty(B, self.cout, Lout, dtype=torch.float32, device=x.device)
        a = L.Conv1dArgs()
        _set_in(a, x)
        a.w, a.K, a.M, a.dil, a.pad, a.stride = L.fptr(self._w), self.kp, self.M, 1, self.kp - 1, 1
        a.w_ld = self.M
        _set_out(a, out, B, self.cout, Lout)
        a.ncols = (Lout - 1 + self.padding) // self.up + 1
        a.rows, a.up, a.shuf_pad = L.ROWS_SHUFFLE, self.up, self.padding
        a.bias = L.fptr(self._b)
        _set_epilogue(a, L.ACT_NONE, None, None, L.MASK_NONE, None, 1.0, res, False, 1.0, out)
        if lrelu is not None:
            a.prologue, a.slope = L.PRO_LRELU, float(lrelu)
        flops = 2 * B * Cin * self.cout * self.k * Lin
        nbytes = 4 * (B * Cin * Lin + B * self.cout * Lout * (1 + (res is not None)) + Cin * self.cout * self.k)
        return ConvLaunch("hsp_conv1d_mfma_f32", L.lib().hsp_conv1d_mfma_f32, a, flops, nbytes, out, (x, out, res))

    def forward(self, x, **kw):
        p = self.prepare(x, **kw)
        p.run()
        return p.out


class _SubArena:
    """arena views of a layer that lives inside another HipLayer (not registered as a sub-module)"""

    def __init__(self, arena, owner, prefix):
        self.arena, self.owner, self.prefix = arena, owner, prefix

    def view(self, _layer, name):
        return self.arena.view(self.owner, self.prefix + name)


class PolyphaseConv1d(HipLayer):
    """nn.Conv1d(cin, cout, k, stride = s, padding = 0) on the unit-stride MFMA kernel: taps are grouped by phase
    p = j mod s, and phase p is a unit-stride conv with ceil((k - p) / s) taps over the strided view x[..., p::s]
    (hsp_conv1d_args.x_ts = s); the phases accumulate into one output.  Parameters keep nn.Conv1d's names and
    shapes (``weight`` [cout, cin, k], ``bias``): the feature-encoder layers of wav2vec2 (HF
    Wav2Vec2LayerNormConvLayer.conv: k 3 / stride 2 and k 2 / stride 2)."""

    def __init__(self, cin, cout, k, stride, bias=True):
        super().__init__()
        self.cin, self.cout, self.k, self.stride = cin, cout, k, stride
        self.weight = nn.Parameter(torch.zeros(cout, cin, k), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False) if bias else None
        ph = [Conv1d(cin, cout, len(range(p, k, stride)), bias=(bias and p == 0)) for p in range(min(stride, k))]
        self.__dict__["_phases"] = ph     # not registered: no duplicate state_dict keys

    def hsp_requests(self):
        return [(f"p{i}.{n}", numel) for i, ph in enumerate(self._phases) for n, numel in ph.hsp_requests()]

    def hsp_fill(self, arena, materialize):
        for i, ph in enumerate(self._phases):
            if materialize:
                ph.weight.data = self.weight.data[:, :, i::self.stride].contiguous()
                if ph.bias is not None:
                    ph.bias.data = self.bias.data
                ph.to(self.weight.device)
            ph.hsp_fill(_SubArena(arena, self, f"p{i}."), materialize)

    def forward(self, x, **kw):
        B, Cin, Lin = x.shape
        Lout = (Lin - self.k) // self.stride + 1
        out = torch.empty(B, self.cout, Lout, dtype=torch.float32, device=x.device)
        for i, ph in enumerate(self._phases):
            xp = x[:, :, i: i + self.stride * (Lout + ph.k - 1): self.stride]     # exactly Lout + K_p - 1 samples
            ph(xp, out=out, accumulate=i > 0, **(kw if i == len(self._phases) - 1 else {}))
        return out


class GroupedPosConv1d(HipLayer):
    """HF Wav2Vec2PositionalConvEmbedding.conv + SamePad + GELU + the residual add of the encoder:
    Conv1d(C, C, k = 128, padding = 64, groups = 16) with weight_norm over dim 2 (one gain per TAP: g [1, 1, k]), last
    output dropped (even kernel), y = x + gelu(conv(x)).  One group = two MFMA launches on channel-slice views, taps
    [0, 64) and [64, 128): the conv kernel stages all taps of a channel chunk at once, and 128 taps x 64 rows do not
    fit its LDS double buffer.  Parameter names: ``weight_g`` / ``weight_v`` (torch <= 2.0 checkpoints;
    ``parametrizations.weight.original0 / original1`` of newer ones are renamed on load by the owner) and ``bias``."""

    TAPS = 64

    def __init__(self, channels, k, groups):
        super().__init__()
        assert k % 2 == 0 and channels % groups == 0 and k % self.TAPS == 0
        self.channels, self.k, self.groups, self.cg = channels, k, groups, channels // groups
        self.weight_g = nn.Parameter(torch.ones(1, 1, k), requires_grad=False)
        self.weight_v = nn.Parameter(torch.zeros(channels, self.cg, k), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(channels), requires_grad=False)
        subs = []
        for _ in range(groups):
            for j0 in range(0, k, self.TAPS):
                # taps j0 .. j0 + 63 read x[t + j - k / 2]: a conv with padding k / 2 - j0 (negative = a shifted window;
                # the kernel bounds-checks every read) whose first L outputs are kept: natural length L + 2 pad - 63
                pad = k // 2 - j0
                c = Conv1d(self.cg, self.cg, self.TAPS, padding=pad, bias=(j0 == 0))
                c.trim_right = 2 * pad - (self.TAPS - 1)
                subs.append(c)
        self.__dict__["_subs"] = subs

    def hsp_requests(self):
        return [(f"s{i}.{n}", numel) for i, c in enumerate(self._subs) for n, numel in c.hsp_requests()]

    def hsp_fill(self, arena, materialize):
        w = None
        nb = self.k // self.TAPS
        if materialize:
            # weight_norm(dim = 2): w[:, :, j] = g[j] * v[:, :, j] / ||v[:, :, j]||_F  == the dim-0 fold of v laid out
            # [k][C * cg] (a permutation, no arithmetic); folded by the same kernel as every other weight-normed layer
            vp = self.weight_v.data.permute(2, 0, 1).contiguous().reshape(self.k, -1)
            w = _fold(vp, self.weight_g.data.reshape(self.k)).reshape(self.k, self.channels, self.cg).permute(1, 2, 0)
        for i, c in enumerate(self._subs):
            gi, bi = divmod(i, nb)
            if materialize:
                c.weight.data = w[gi * self.cg:(gi + 1) * self.cg, :, bi * self.TAPS:(bi + 1) * self.TAPS].contiguous()
                if c.bias is not None:
                    c.bias.data = self.bias.data[gi * self.cg:(gi + 1) * self.cg].contiguous()
            c.hsp_fill(_SubArena(arena, self, f"s{i}."), materialize)

    def forward(self, x):
        nb = self.k // self.TAPS
        conv = torch.empty_like(x)
        for i, c in enumerate(self._subs):
            gi, bi = divmod(i, nb)
            sl = slice(gi * self.cg, (gi + 1) * self.cg)
            c(x[:, sl], out=conv[:, sl], accumulate=bi > 0)
        return Fh.axpby(x, Fh.act(conv, L.ACT_GELU_ERF), 1.0, 1.0)


class Linear(Conv1d):
    """torch.nn.Linear on a (B, C) or (B, C, 1) style vector == 1x1 conv with L = 1.
    Parameters keep nn.Linear's 2-D ``weight`` shape for checkpoint compatibility."""

    def __init__(self, cin, cout, bias=True):
        super().__init__(cin, cout, 1, bias=bias, weight_2d=True)

    def forward(self, x, **kw):
        x3 = x.reshape(x.shape[0], self.cin, 1)
        return super().forward(x3, force_direct=True, **kw)


class LinearCT(Conv1d):
    """torch.nn.Linear applied along the channel axis of a channel-major [B, C, T] tensor (a 1x1
    conv on the MFMA path).  ``packed=False`` keeps only the parameters (nn.Linear names and
    shapes) for a layer whose rows are packed into a :class:`StackedLinearCT`."""

    def __init__(self, cin, cout, bias=True, packed=True):
        super().__init__(cin, cout, 1, bias=bias, weight_2d=True)
        self.packed = packed


class StackedLinearCT(Conv1d):
    """Several nn.Linear layers reading the same input, run as ONE GEMM with their output rows
    stacked (q/k/v projections of transformer_mega.MultiHeadAttention, ttv_v1/transformer_mega.py:54-56).
    Owns no parameters: the packed weight is gathered from the parts' ``weight`` / ``bias``."""

    def __init__(self, parts):
        super().__init__(parts[0].cin, sum(p.cout for p in parts), 1, bias=True, weight_2d=True)
        del self._parameters["weight"], self._parameters["bias"]
        self.__dict__["_parts"] = tuple(parts)  # not registered as sub-modules (no duplicate state_dict keys)

    def _folded(self):
        return torch.cat([p.weight.data for p in self._parts], 0).contiguous()

    def _bias_src(self):
        return torch.cat([p.bias.data for p in self._parts], 0)


def _set_in(a, x):
    """The input side of hsp_conv1d_args for x [B, Cin, Lin] at any strides."""
    a.B, a.Cin, a.Lin = x.shape
    a.x_bs, a.x_cs, a.x_ts = x.stride()            # (one call, not three: this runs once per launch)
    a.x = L.fptr(x)
    a.zeros = L.fptr(_zeros(x.device))


def _wants_direct(a, force_direct: bool, silu_in: bool) -> bool:
    """Does this launch take the VALU kernel (hsp_conv1d_direct_f32) instead of the MFMA one?  Shapes the MFMA kernels do
    not take: stride, degenerate channel / length counts, a SiLU prologue.  The same rule as wants_direct() in
    csrc/hsp_abi.hip, which decides again for a struct that arrives through hsp_conv1d_f32 (SURVEY_ABI) -- change the two
    together.  ``force_direct`` (a Linear's L = 1 products) is the host's alone.  Reads rows, prologue, ln_c1, stride,
    Cin, Cout and Lout of ``a`` as Conv1d.prepare has set them."""
    gated = a.rows in (L.ROWS_GATE_WN, L.ROWS_GATE_GLU)
    return (not gated and a.prologue != L.PRO_ACT1D and not a.ln_c1 and
            bool(force_direct or a.stride != 1 or a.Cin < 8 or a.Cout < 8 or a.Lout < 8 or silu_in))


def _set_out(a, out, B, cout, Lout):
    assert out.shape == (B, cout, Lout), (tuple(out.shape), (B, cout, Lout))
    a.y_bs, a.y_cs, ts = out.stride()
    assert ts == 1 or Lout == 1
    a.y = L.fptr(out)
    a.Cout, a.Lout = cout, Lout


def _set_epilogue(a, act, cbias, mask, mask_mode, cscale, scale, res, accumulate, post_scale, out):
    a.act = act
    if cbias is not None:
        assert cbias.dim() >= 2 and cbias.stride(1) == 1
        a.cbias, a.cbias_bs = L.fptr(cbias), cbias.stride(0)
    if mask is not None and mask_mode != L.MASK_NONE:
        assert mask.stride(-1) == 1
        a.mask, a.mask_bs, a.mask_mode = L.fptr(mask), mask.stride(0), mask_mode
    if cscale is not None:
        assert cscale.stride(1) == 1
        a.cscale, a.cscale_bs = L.fptr(cscale), cscale.stride(0)
    a.scale = float(scale)
    if res is not None:
        assert res.shape == out.shape
        a.res, a.res_bs, a.res_cs = L.fptr(res), res.stride(0), res.stride(1)
        if res.stride(2) != 1 and res.shape[2] != 1:
            if res.stride(2) < 1:         # a time-broadcast (.expand) residual: every kernel reads res_ts 0 as unit stride
                raise L.HspError("residual with time stride %d: materialise it (copy_strided) before the launch" % res.stride(2))
            a.res_ts = res.stride(2)      # hsp_conv1d_args.res_ts: the register-path token GEMM only (else HSP_EINVAL)
    a.accumulate = 1 if accumulate else 0
    a.post_scale = float(post_scale)


def prepare_fft(model: nn.Module) -> int:
    """Derive the per-bin matrices of every conv of ``model`` that carries the frequency-domain form now (Conv1d.ensure_wf
    does it on first use otherwise) -- before a hipGraph capture, or to pay the start-up cost at a chosen moment.  Returns
    the number of floats the side buffers hold."""
    n = 0
    for m in model.modules():
        if isinstance(m, Conv1d) and m._fft:
            n += m.ensure_wf().numel()
    return n


# ------------------------------------------------------------------ finalisation
def finalize(model: nn.Module, device, materialize: bool = True) -> WeightArena:
    """Pack every HipLayer of ``model`` into one arena on ``device``.

    ``materialize=False`` only lays the arena out (same offsets on every rank) so that
    the contents can arrive by broadcast (parallel.broadcast_weights)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise L.HspError("finalize() needs a ROCm device: the product path has no CPU fallback")
    L.lib()
    if materialize:
        model.to(device)
    arena = WeightArena()
    layers = [m for m in model.modules() if isinstance(m, HipLayer)]
    for m in layers:
        for name, numel in m.hsp_requests():
            arena.request(m, name, numel)
    with torch.cuda.device(device):
        arena.allocate(device)
        for m in layers:
            m.hsp_fill(arena, materialize)
            m.__dict__["_hsp_stale"] = False
        torch.cuda.current_stream().synchronize()
    model._hsp_arena = arena
    model.__dict__["_hsp_epoch"] = _EPOCH
    return arena
