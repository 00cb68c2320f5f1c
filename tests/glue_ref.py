"""Float64 restatements of the pointwise and glue operations of csrc/hsp_pointwise.hip, the four element-wise kernels
of csrc/hsp_denoiser.hip and hsp_copy_strided_f32, float32 restatements of the three STFT framing forms of
csrc/hsp_mel.hip, plus the seeded inputs and case tables the host and GPU tests share.

Every function is written from the formula in include/hsp.h and the kernel's header comment -- none calls the library
and none uses torch.  tests/test_glue_ref_host.py pins them against torch's CPU operations in float64 and asserts the
input conditions the GPU comparisons rely on; tests/test_gpu_glue_kernels.py and tests/test_gpu_framing_contract.py
compare the kernels with them.

Data movement (copy, flip, gather, mask, reflect pad), the single fp32 multiply of mask_mul and the one or two fp32
multiplies of framing are restated in float32, because their results must be bit-equal; everything else is float64 on
the fp32 inputs the kernel sees.
linear_interp is the one mixed case: its source position is DEFINED in fp32 (one rounding of scale * (t + 0.5) - 0.5,
SURVEY.md A15), so the position is formed in fp32 and the blend in float64.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
F64 = np.float64

# enum HSP_ACT_* of include/hsp.h
ACT_NONE, ACT_TANH, ACT_GELU_TANH, ACT_RELU, ACT_MISH, ACT_SILU, ACT_SOFTPLUS, ACT_GELU_ERF = range(8)
ACT_NAMES = ("none", "tanh", "gelu_tanh", "relu", "mish", "silu", "softplus", "gelu_erf")
ACT_EXACT = (ACT_NONE, ACT_RELU)          # identity and max(x, 0): bit for bit


def _f64(*a):
    return tuple(np.asarray(v, np.float32).astype(np.float64) for v in a)


# ------------------------------------------------------------------------------------------------ restatements
def layernorm(x, eps, mask=None, shift=None, scale=None, gamma=None, beta=None):
    """LayerNorm over C of [B, C, T] (biased variance), the per-channel affine gamma / beta [C], then * mask [B, T],
    then * (1 + scale) + shift with scale / shift [B, C] (modules.py:19-31, 346-347, 409-410)."""
    (x,) = _f64(x)
    mean = x.mean(1, keepdims=True)
    var = ((x - mean) ** 2).mean(1, keepdims=True)
    y = (x - mean) / np.sqrt(var + float(F32(eps)))
    if gamma is not None:
        g, b = _f64(gamma, beta)
        y = y * g[None, :, None] + b[None, :, None]
    if mask is not None:
        y = y * _f64(mask)[0][:, None, :]
    if scale is not None:
        sc, sh = _f64(scale, shift)
        y = y * (1.0 + sc[:, :, None]) + sh[:, :, None]
    return y


def softplus(x):
    """F.softplus with its default threshold: x above 20, log(1 + e^x) below."""
    x = np.asarray(x, np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0))


_erf = np.vectorize(math.erf, otypes=[np.float64])


def act(x, kind):
    """The pointwise functions HSP_ACT_* name (include/hsp.h), in float64."""
    (x,) = _f64(x)
    if kind == ACT_NONE:
        return x
    if kind == ACT_TANH:
        return np.tanh(x)
    if kind == ACT_GELU_TANH:
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    if kind == ACT_RELU:
        return np.maximum(x, 0.0)
    if kind == ACT_MISH:
        return x * np.tanh(np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0))
    if kind == ACT_SILU:
        return x / (1.0 + np.exp(-x))
    if kind == ACT_SOFTPLUS:
        return softplus(x)
    if kind == ACT_GELU_ERF:
        return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))
    raise ValueError(kind)


def interp_index(Lin, Lout):
    """Source position of output t as torch's CPU kernel forms it for fp32 data: scale = fp32(Lin) / fp32(Lout), then
    ONE rounding of scale * (t + 0.5) - 0.5 (the float64 product of two fp32 numbers and the subtraction of 0.5 are
    exact at these sizes, so the cast below is that single rounding), clamped at 0.  -> (i0, i1, lambda1 as float64)."""
    assert Lin < 2 ** 20 and Lout < 2 ** 20
    scale = F32(Lin) / F32(Lout)
    t = np.arange(Lout, dtype=np.float32) + F32(0.5)
    src = (np.float64(scale) * t.astype(np.float64) - 0.5).astype(np.float32)
    src = np.maximum(src, F32(0.0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < Lin - 1)
    return i0, i1, src.astype(np.float64) - i0


def linear_interp(x, Lout):
    """F.interpolate(x, Lout, mode='linear', align_corners=False) along the last axis of [B, C, Lin]."""
    (x,) = _f64(x)
    i0, i1, l1 = interp_index(x.shape[-1], Lout)
    return (1.0 - l1) * x[..., i0] + l1 * x[..., i1]


def linear_interp_ragged(x, Lout, lens_in, lens_out):
    """Row b = linear_interp of its first lens_in[b] samples to lens_out[b] outputs, zeros after."""
    B, C, _ = x.shape
    y = np.zeros((B, C, Lout), np.float64)
    for b in range(B):
        y[b, :, :lens_out[b]] = linear_interp(x[b:b + 1, :, :lens_in[b]], int(lens_out[b]))[0]
    return y


def fold_weight_norm(v, g):
    """w[r] = g[r] v[r] / ||v[r]||_2 : torch.nn.utils.weight_norm over dim 0 of [rows, cols]."""
    v, g = _f64(v, g)
    return g[:, None] * v / np.sqrt((v * v).sum(1, keepdims=True))


def masked_mean(x, mask):
    """out[b, c] = sum over ALL t of x[b, c, t] / sum_t mask[b, t]: the padded frames are summed too, as the
    reference's temporal_avg_pool does (styleencoder.py:83-91)."""
    x, mask = _f64(x, mask)
    return x.sum(2) / mask.sum(1)[:, None]


def masked_sum_mean(x, mask):
    """What masked_mean is NOT: the mean over the valid frames only."""
    x, mask = _f64(x, mask)
    return (x * mask[:, None, :]).sum(2) / mask.sum(1)[:, None]


def snake_consts(alpha_log, beta_log):
    """exp(alpha), 1 / (exp(beta) + 1e-9): activations.py:113-117."""
    a, b = _f64(alpha_log, beta_log)
    return np.exp(a), 1.0 / (np.exp(b) + 1e-9)


def sample_prior(stats, noise, mask, noise_scale):
    """z = (m + noise * exp(logs) * noise_scale) * mask with stats = [B, 2C, T] (m then logs), mask [B, T]."""
    stats, noise, mask = _f64(stats, noise, mask)
    C = stats.shape[1] // 2
    return (stats[:, :C] + noise * np.exp(stats[:, C:]) * float(F32(noise_scale))) * mask[:, None, :]


def axpby(x, z, a, b):
    x, z = _f64(x, z)
    return float(F32(a)) * x + float(F32(b)) * z


def mask_mul(x, mask):
    """One fp32 multiply per element: exact."""
    return (np.asarray(x, np.float32) * np.asarray(mask, np.float32)[:, None, :]).astype(np.float32)


def gather(src, index_map):
    m = np.asarray(index_map)
    return np.where(m >= 0, np.asarray(src, np.float32)[np.maximum(m, 0)], F32(0.0)).astype(np.float32)


def sequence_mask(lengths, T):
    return (np.arange(T)[None, :] < np.asarray(lengths, np.int64)[:, None]).astype(np.float32)


def flip_channels(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)[:, ::-1])


def reflect_pad(x, pad):
    return np.pad(np.asarray(x, np.float32), ((0, 0), (pad, pad)), mode="reflect")


def reflect_pad_ragged(x, lengths, pad):
    """Row b = reflect_pad of its first lengths[b] samples, zeros after: [B, L + 2 pad]."""
    x = np.asarray(x, np.float32)
    y = np.zeros((x.shape[0], x.shape[1] + 2 * pad), np.float32)
    for b, n in enumerate(lengths):
        y[b, :n + 2 * pad] = reflect_pad(x[b:b + 1, :n], pad)[0]
    return y


def reflect_index(i, n):
    """Sample i of a row of n samples under torch's "reflect" padding (the edge sample is not repeated), -n < i < 2n - 1."""
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def stft_frames(x, window, hop, scale=None):
    """The frames torch.stft(center=True, pad_mode="reflect") multiplies by its DFT matrix, [n_fft, T] with
    T = 1 + len(x) // hop: frames[n, t] = w[n] * x[reflect(t hop + n - n_fft / 2)], one fp32 multiply; with ``scale``
    the sample is scaled first, w[n] * (x * scale): two fp32 multiplies in that order."""
    x, w = np.asarray(x, np.float32), np.asarray(window, np.float32)
    n_fft, T = len(w), 1 + len(x) // hop
    v = x[reflect_index(np.arange(T)[None, :] * hop + np.arange(n_fft)[:, None] - n_fft // 2, len(x))]
    if scale is not None:
        v = v * F32(scale)
    assert v.dtype == np.float32
    return w[:, None] * v


def stft_frames_ragged(x, lengths, window, hop, f_ld):
    """[B, n_fft, f_ld]: row b holds stft_frames of its first lengths[b] samples, zeros on the columns after them."""
    out = np.zeros((len(lengths), len(window), f_ld), np.float32)
    for b, n in enumerate(lengths):
        fr = stft_frames(x[b, :n], window, hop)
        out[b, :, :fr.shape[1]] = fr
    return out


def stft_frames_packed(x, lengths, window, hop, first, f_ld, scale=None):
    """ONE [n_fft, f_ld] matrix: the frames of row b (times scale[b]) at columns [first[b], first[b] + T_b), zeros on
    every other column."""
    out = np.zeros((len(window), f_ld), np.float32)
    for b, n in enumerate(lengths):
        fr = stft_frames(x[b, :n], window, hop, None if scale is None else scale[b])
        out[:, first[b]:first[b] + fr.shape[1]] = fr
    return out


def mag_pha(re, im, compress):
    """|z|^compress and angle(z) of z = re + i im, [n_freqs, T]; the imaginary part of the first and the last bin is
    taken as +0, as a real FFT returns it (denoiser/infer.py:12-24)."""
    re, im = _f64(re, im)
    im = im.copy()
    im[0] = 0.0
    im[-1] = 0.0
    return np.hypot(re, im) ** float(F32(compress)), np.arctan2(im, re)


def atan2(y, x):
    y, x = _f64(y, x)
    return np.arctan2(y, x)


def polar(mag, pha, power):
    mag, pha = _f64(mag, pha)
    m = mag ** float(F32(power))
    return m * np.cos(pha), m * np.sin(pha)


def lsigmoid_mul(m, slope, beta, mag):
    """out[t, f] = mag[t, f] * beta * sigmoid(slope[f] * m[t, f]) (denoiser/utils.py:44-53, generator.py:140)."""
    m, slope, mag = _f64(m, slope, mag)
    with np.errstate(over="ignore"):
        return mag * float(F32(beta)) / (1.0 + np.exp(-slope[None, :] * m))


# ------------------------------------------------------------------------------------------------ seeded cases
def ragged_lengths(B, T, short_row=True):
    """Row 0 full, row 1 of length 1 (``short_row``), the others in between."""
    lens = [T, 1 if short_row else max(1, T // 2), max(1, (2 * T) // 3), max(1, T // 3)]
    if B == 1:
        lens = [max(1, (2 * T) // 3)]
    return np.array(lens[:B], np.int64)


# ---- LayerNorm.  The launcher takes the register kernel (16 columns x 16 channel groups) up to C = 512 and the loop
# kernel (64 columns x 4 waves) above.  Every C with two T values, every T with both kernels; "ops" is the operand set:
# "" none, "m" mask, "a" gamma + beta, "s" shift + scale (columns of wider buffers, mod_bs = C + 5), "mas" all.
LN_REG_MAX_C = 512
LN_EPS = 1e-5
LN_MIN_STD = 0.5
LN_CASES = [
    # register kernel
    dict(C=1, T=1, B=1, ops=""), dict(C=1, T=17, B=3, ops="mas"),
    dict(C=15, T=15, B=3, ops="m"), dict(C=15, T=65, B=1, ops="s"),
    dict(C=16, T=17, B=1, ops="a"), dict(C=16, T=130, B=3, ops=""),
    dict(C=17, T=1, B=3, ops="s"), dict(C=17, T=63, B=3, ops="mas"),
    dict(C=276, T=15, B=3, ops="mas"), dict(C=276, T=130, B=3, ops="m"),
    dict(C=511, T=63, B=1, ops="a"), dict(C=511, T=65, B=3, ops="mas"),
    dict(C=512, T=17, B=3, ops="s"), dict(C=512, T=65, B=1, ops=""),
    # loop kernel
    dict(C=513, T=1, B=3, ops="mas"), dict(C=513, T=17, B=1, ops=""), dict(C=513, T=65, B=3, ops="m"),
    dict(C=515, T=15, B=1, ops="a"), dict(C=515, T=63, B=3, ops="s"), dict(C=515, T=130, B=3, ops="mas"),
    dict(C=1024, T=1, B=1, ops="s"), dict(C=1024, T=65, B=1, ops="a"), dict(C=1024, T=130, B=3, ops="m"),
    dict(C=1024, T=17, B=3, ops="mas"),
    # one per kernel with a common offset of 100 and no affine or modulation
    dict(C=511, T=17, B=3, ops="", offset=100.0), dict(C=1024, T=63, B=3, ops="", offset=100.0),
]
for _i, _c in enumerate(LN_CASES):
    _c.setdefault("offset", None)
    _c["seed"] = 1000 + _i
LN_PAIR = dict(C=LN_REG_MAX_C + 1, T=65, B=3, ops="mas", offset=None, seed=1100)


def ln_id(c):
    return f"c{c['C']}_t{c['T']}_b{c['B']}_{c['ops'] or 'plain'}" + ("_off100" if c["offset"] else "")


def ln_case(C, T, B, ops, offset, seed):
    """x: every (b, t) column is a draw of C normals scaled to unit standard deviation (C = 1: the column is its
    offset alone) plus a per-column offset in [-10, 10] (or the common ``offset``).  gamma and 1 + scale in [-2, 2],
    beta and shift in [-1, 1]."""
    r = np.random.default_rng(seed)
    z = r.standard_normal((B, C, T))
    if C > 1:
        z = (z - z.mean(1, keepdims=True)) / z.std(1, keepdims=True)
    else:
        z = np.zeros_like(z)
    off = r.uniform(-10.0, 10.0, (B, 1, T)) if offset is None else np.full((B, 1, T), float(offset))
    out = dict(x=(z + off).astype(np.float32), C=C, T=T, B=B, ops=ops, offset=offset, eps=LN_EPS,
               mask=None, gamma=None, beta=None, shift=None, scale=None)
    gamma, beta = r.uniform(-2.0, 2.0, C), r.uniform(-1.0, 1.0, C)
    scale, shift = r.uniform(-3.0, 1.0, (B, C)), r.uniform(-1.0, 1.0, (B, C))
    if "m" in ops:
        out["mask"] = sequence_mask(ragged_lengths(B, T), T)
    if "a" in ops:
        out["gamma"], out["beta"] = gamma.astype(np.float32), beta.astype(np.float32)
    if "s" in ops:
        out["scale"], out["shift"] = scale.astype(np.float32), shift.astype(np.float32)
    return out


def ln_pair_cases():
    """The first width of the loop kernel (513) and the last of the register kernel (512) on the same numbers: the
    narrower case is the first 512 channels of the wider one."""
    wide = ln_case(**LN_PAIR)
    C = LN_REG_MAX_C
    cut = dict(wide, C=C, x=np.ascontiguousarray(wide["x"][:, :C]))
    for k in ("gamma", "beta"):
        cut[k] = wide[k][:C].copy()
    for k in ("scale", "shift"):
        cut[k] = np.ascontiguousarray(wide[k][:, :C])
    return cut, wide


def ln_reference(c):
    return layernorm(c["x"], c["eps"], c["mask"], c["shift"], c["scale"], c["gamma"], c["beta"])


# ---- wave-per-row reductions: 4 rows per workgroup, 64 lanes per row
MM_SHAPES = ((1, 1), (3, 5), (2, 64))
MM_TS = (1, 63, 64, 65, 1000)


def masked_mean_case(B, C, T):
    """x = 2 + N(0, 1/16) in EVERY frame, the padded ones included; lengths T, T/2, T/3 (at least 1)."""
    r = np.random.default_rng(2000 + 97 * B + 7 * C + T)
    x = (2.0 + 0.25 * r.standard_normal((B, C, T))).astype(np.float32)
    lens = np.array([T, max(1, T // 2), max(1, T // 3)][:B], np.int64)
    return x, sequence_mask(lens, T), lens


FOLD_ROWS = (1, 3, 4, 5, 130)
FOLD_COLS = (1, 7, 63, 64, 65, 200 * 11)


def fold_case(rows, cols):
    r = np.random.default_rng(2100 + 13 * rows + cols)
    v = r.standard_normal((rows, cols)).astype(np.float32)
    if cols == 1:
        v = np.where(np.abs(v) < 0.1, F32(0.5), v)           # a one-element row is its own norm: keep it off zero
    return v, r.uniform(0.2, 3.0, rows).astype(np.float32) * np.where(r.random(rows) < 0.3, -1, 1).astype(np.float32)


SNAKE_CS = (1, 255, 257)


def snake_case(C):
    r = np.random.default_rng(2200 + C)
    return r.uniform(-3.0, 3.0, C).astype(np.float32), r.uniform(-3.0, 3.0, C).astype(np.float32)


# ---- exact data movement
COPY_BIG = (3, 9, 38839)          # 1 048 576 + 77 elements: the 4096 x 256 grid takes a second trip
assert int(np.prod(COPY_BIG)) == 4096 * 256 + 77


def copy_views(shape, seed):
    """(name, base array, view of it with logical shape ``shape``) for the layouts the denoiser hands to
    hsp_copy_strided_f32 -- permute(1, 0, 2), (2, 0, 1), (2, 1, 0), a .t() view -- and a sliced view.  Built with numpy
    so that the same strides (in elements) can be taken on the device copy of the base array."""
    B, C, T = shape
    r = np.random.default_rng(seed)
    new = lambda *s: r.standard_normal(s).astype(np.float32)
    out = []
    a = new(C, B, T)
    out.append(("permute(1,0,2)", a, a.transpose(1, 0, 2)))
    a = new(C, T, B)
    out.append(("permute(2,0,1)", a, a.transpose(2, 0, 1)))
    a = new(T, C, B)
    out.append(("permute(2,1,0)", a, a.transpose(2, 1, 0)))
    a = new(B, T, C)
    out.append(("t()", a, a.transpose(0, 2, 1)))
    a = new(B + 1, C + 2, T + 3)
    out.append(("slice", a, a[1:, 1:C + 1, 2:T + 2]))
    return out


def elem_strides(view):
    return tuple(s // view.itemsize for s in view.strides)


def elem_offset(base, view):
    return (view.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // base.itemsize


GATHER_NS = (1, 257, 70001)


def gather_case(n, nsrc=1000):
    """About a fifth of the map is negative (-> 0), the rest points into 1000 sources: every source is read often."""
    r = np.random.default_rng(2300 + n)
    m = r.integers(-nsrc // 4, nsrc, n).astype(np.int32)
    m[0] = -1 if n > 1 else 7
    m[-1] = nsrc - 1
    return (1.0 + r.random(nsrc)).astype(np.float32), m          # sources in [1, 2): never 0


def seqmask_lengths(T):
    return np.array([0, 1, T, T + 3, -2, max(1, T // 2)], np.int64)


# ---- element-wise float
AXPBY_NS = (1, 255, 70001)
AXPBY_AB = ((1.0, 1.0), (math.sqrt(256.0), 0.0), (0.3, 0.7))
PRIOR_SHAPES = ((1, 1, 1), (2, 3, 65), (3, 96, 17))
PRIOR_SCALES = (0.0, 0.333, 1.0)


def prior_case(B, C, T):
    """m in N(0, 1), logs uniform in [-6, 3], both non-zero under the mask; ragged 0/1 mask."""
    r = np.random.default_rng(2400 + B * 1000 + C + T)
    stats = np.concatenate([r.standard_normal((B, C, T)), r.uniform(-6.0, 3.0, (B, C, T))], 1).astype(np.float32)
    noise = r.standard_normal((B, C, T)).astype(np.float32)
    lens = ragged_lengths(B, T, short_row=False) if B > 1 else np.array([T], np.int64)
    return stats, noise, sequence_mask(lens, T)


ACT_SPECIAL = (0.0, 1e-6, 20.0, 20.001, 88.0, 104.0)      # +-: zero, tiny, the softplus / mish switch, exp overflow


def act_points():
    """4001 points on [-30, 30] and the special values with both signs (-0.0 included)."""
    sp = np.array(ACT_SPECIAL, np.float32)
    return np.concatenate([np.linspace(-30.0, 30.0, 4001).astype(np.float32), sp, -sp])


# magnitude bands in which the activation outputs are compared, each against the bar of its own reference values
ACT_BANDS = ((0.0, 1.0), (1.0, 8.0), (8.0, 30.0), (30.0, 200.0))

# ---- framing and reflect padding: exact operations
# n_fft = 320, hop = 5.  L = 347: T = 70 frames -- a second, part-filled 64-frame tile; 320 window positions -- a second
# 256-position block whose one 64-position group is whole (a third and fourth are empty); L = 161 = n_fft / 2 + 1: the
# shortest legal row, both edges reflect inside one frame.  Ragged and packed forms: rows of 347, 161 and 200 samples.
FRAME_N_FFT, FRAME_HOP = 320, 5
FRAME_LS = (347, 161)
FRAME_RAGGED = (347, 161, 200)
FRAME_GAP = 3                                # columns between packed segments
FRAME_SCALE = (0.5, 3.0, 1.25)
PAD_SHAPES = ((300, 37), (2, 1))             # (L, pad)


def frame_window(n_fft=FRAME_N_FFT):
    """The periodic Hann window in fp32 from float64 (torch.hann_window's values are not needed: any fp32 window does)."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)


def frame_rows(B, L, seed):
    """B rows of L normals; no sample is 0, so a frame element is 0 only where the window is."""
    x = np.random.default_rng(seed).standard_normal((B, L)).astype(np.float32)
    return np.where(x == 0, F32(1.0), x)


def frame_ld(T):
    return (T + 3) & ~3


def packed_table(lengths, hop=FRAME_HOP, gap=FRAME_GAP):
    """(first column, frames) of every row laid end to end with ``gap`` columns between neighbours, and T_tot."""
    frames = [1 + n // hop for n in lengths]
    first, t = [], 0
    for n in frames:
        first.append(t)
        t += n + gap
    return first, frames, t - gap


# ---- linear interpolation
INTERP_PLAIN = ((1, 1), (1, 9), (9, 1), (7, 14), (50, 21), (33, 100), (100, 33))
INTERP_CS = (1, 3)
INTERP_RAGGED = tuple((lin, ratio) for lin in (40, 41) for ratio in (2, 3))


def interp_case(B, C, Lin, seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, (B, C, Lin)).astype(np.float32)     # never 0


def interp_ragged_lens(Lin, ratio):
    lin = np.array([Lin, Lin - 1, 1, 17], np.int64)
    return lin, lin * ratio


# ---- denoiser element-wise
DN_FREQS = (5, 201)
DN_TS = (1, 7, 130)
DN_COMPRESS = (1.0, 0.3)
CUT_CLEARANCE = 1e-3


def off_branch_cut(re, im):
    """Move every point with re < 0 and |im| < 0.01 to |im| = 0.01 (sign kept, +0 counted positive)."""
    near = (re < 0) & (np.abs(im) < 0.01)
    return np.where(near, np.where(np.signbit(im), F32(-0.01), F32(0.01)), im).astype(np.float32)


def cut_distance(re, im):
    """Smallest |im| over the points with re < 0 (inf when there is none)."""
    d = np.abs(im[re < 0])
    return float(d.min()) if d.size else math.inf


def mag_pha_case(nf, T):
    """spec rows [0, nf) real and [nf, 2 nf) imaginary.  The imaginary rows of bins 0 and nf - 1 hold noise of both
    signs and their real part is negative in every other column; bin 1 (and bin 0, column 0 when T > 2) is exactly zero
    in the even columns."""
    r = np.random.default_rng(2500 + nf + T)
    re = r.standard_normal((nf, T)).astype(np.float32)
    im = r.standard_normal((nf, T)).astype(np.float32)
    for f in (0, nf - 1):
        re[f] = np.abs(re[f]) + F32(0.1)
        re[f, ::2] *= F32(-1.0)
        im[f] = (1e-6 * r.standard_normal(T)).astype(np.float32)
        im[f, ::2] = -np.abs(im[f, ::2]) - F32(1e-9)                   # the noise that would give -pi
    if T > 1:
        im[nf - 1, 1] = F32(3e-7)
    im[1:nf - 1] = off_branch_cut(re[1:nf - 1], im[1:nf - 1])
    zero = np.zeros((nf, T), bool)
    zero[1, ::2] = True
    if T > 2:
        zero[0, 2] = True
    re[zero] = 0.0
    im[zero] = 0.0
    return re, im, zero


def atan2_axis_case():
    """Both axes and the origin with every combination of signed zeros."""
    z, o = F32(0.0), F32(1.5)
    y = np.array([z, -z, z, -z, o, o, -o, -o, z, -z, z, -z], np.float32)
    x = np.array([o, o, -o, -o, z, -z, z, -z, z, z, -z, -z], np.float32)
    return y, x


def atan2_random_case(n, seed):
    """All four quadrants, magnitudes over six decades, clear of the branch cut."""
    r = np.random.default_rng(seed)
    x = (r.standard_normal(n) * 10.0 ** r.uniform(-3, 3, n)).astype(np.float32)
    y = (r.standard_normal(n) * 10.0 ** r.uniform(-3, 3, n)).astype(np.float32)
    return off_branch_cut(x, y), x


def polar_case(nf, T):
    """mag >= 0 with exact zeros, pha uniform on [-pi, pi] with +-fp32(pi), +-0 and +-pi/2 planted."""
    r = np.random.default_rng(2600 + nf + T)
    mag = np.abs(r.standard_normal((nf, T))).astype(np.float32) * F32(1.5)
    mag[r.random((nf, T)) < 0.1] = 0.0
    pha = r.uniform(-math.pi, math.pi, (nf, T)).astype(np.float32)
    pha = np.clip(pha, -F32(math.pi), F32(math.pi))
    plant = np.array([math.pi, -math.pi, 0.0, -0.0, math.pi / 2, -math.pi / 2], np.float32)
    flat = pha.reshape(-1)
    n = min(len(plant), flat.size - 1)
    flat[:n] = plant[:n]
    mag.reshape(-1)[:n] = np.maximum(mag.reshape(-1)[:n], F32(0.5))
    mag.reshape(-1)[-1] = 0.0
    return mag, pha


LSIG = ((1, 5), (7, 201))


def lsigmoid_case(T, F):
    """slope[f] distinct per column; slope * m reaches +200 in column 0 and -200 in column 1 of the last row."""
    r = np.random.default_rng(2700 + T + F)
    m = (3.0 * r.standard_normal((T, F))).astype(np.float32)
    slope = r.uniform(0.5, 2.0, F).astype(np.float32)
    slope[0], slope[1] = 2.0, 4.0
    m[-1, 0], m[-1, 1] = 100.0, -50.0
    mag = (0.5 + r.random((T, F))).astype(np.float32)
    return m, slope, mag
