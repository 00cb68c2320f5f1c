"""Float64 restatements of the text front-end's glue operations, and the seeded inputs the GPU tests feed them.

Every function here is written from the formula in the kernel's header comment (include/hsp.h, csrc/hsp_frontend.hip)
and the reference lines it cites -- none calls the library.  tests/test_frontend_ref_host.py pins them against the
oracle and torch on a CPU and checks the conditions the GPU tests rely on (distance of a duration from an integer,
margin of a nearest code, fp32-vs-float64 headroom) for the exact seeds the case builders below use;
tests/test_gpu_frontend_kernels.py compares the kernels with them.

Integer-valued and "exact" operations (embedding sum, bias add, threshold, max-pool, int16 peak normalisation) are
restated in float32 in the kernel's operation order, because their results must be bit-equal; everything else is
float64.
"""
from __future__ import annotations

import math

import numpy as np
import torch

F32 = np.float32
LOG_2PI = math.log(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------ restatements
def gaussian_upsample(x, dur, rng, lengths, frames, T):
    """GaussianUpsampling.forward (ttv_v1/Gaussian.py:35-69) with the range clamp min(range, 2 dur), max(., 1e-5)
    (ttv_v1/t2w2v_transformer.py:961-963), per row, in float64: x [B, C, N], dur / rng [B, N], lengths int [B] (phones
    n >= lengths[b] carry no weight), frames [B] (output frames t >= frames[b] are zero) -> [B, C, T]."""
    x, dur, rng = (np.asarray(a, np.float64) for a in (x, dur, rng))
    B, C, N = x.shape
    out = np.zeros((B, C, T), np.float64)
    for b in range(B):
        L = int(min(N, max(0, int(lengths[b]))))
        Tb = int(min(T, max(0, math.ceil(float(frames[b])))))      # t < frames[b] for integer t
        if L == 0 or Tb == 0:
            continue
        d = dur[b]
        c = (np.cumsum(d) - 0.5 * d)[:L]
        v = np.maximum(np.minimum(rng[b], 2.0 * d), 1e-5)[:L]
        t = np.arange(Tb, dtype=np.float64)
        w = -0.5 * (LOG_2PI + np.log(v)[:, None] + (t[None, :] - c[:, None]) ** 2 / v[:, None])   # [L, Tb]
        w = np.exp(w - w.max(0, keepdims=True))
        w /= w.sum(0, keepdims=True)
        out[b, :, :Tb] = x[b, :, :L] @ w
    return out


def duration_exact(logw, lengths, length_scale):
    """ceil(exp(logw) * length_scale) (ttv_v1/t2w2v_transformer.py:955-957) in float64 on the fp32 inputs the kernel
    sees; zero from lengths[b] on.  -> (dur float64 [B, N], frames int64 [B], value float64 [B, N] before the ceil)."""
    lw = np.asarray(logw, np.float32).astype(np.float64)
    val = np.exp(lw) * float(np.float32(length_scale))
    B, N = lw.shape
    valid = np.arange(N)[None, :] < np.clip(np.asarray(lengths, np.int64), 0, N)[:, None]
    dur = np.where(valid, np.ceil(val), 0.0)
    return dur, dur.sum(1).astype(np.int64), val


def duration_keep(dur, lengths):
    """The kernel's second mode: caller-supplied durations kept bit for bit, padding cleared, rows summed."""
    dur = np.asarray(dur, np.float32)
    N = dur.shape[1]
    valid = np.arange(N)[None, :] < np.clip(np.asarray(lengths, np.int64), 0, N)[:, None]
    out = np.where(valid, dur, F32(0.0)).astype(np.float32)
    return out, out.astype(np.float64).sum(1)


def embedding_sum(ids, tables, scale):
    """out[b, :, t] = ((tab0[id0] * s + tab1[id1] * s) + tab2[id2] * s) in float32, each term scaled first
    (TextEncoder.forward, ttv_v1/t2w2v_transformer.py:127-131): ids list of int [B, T], tables list of [rows, C]."""
    s = F32(scale)
    acc = None
    for i, tab in zip(ids, tables):
        term = (np.asarray(tab, np.float32)[np.asarray(i)] * s).astype(np.float32)        # [B, T, C]
        acc = term if acc is None else (acc + term).astype(np.float32)
    return np.ascontiguousarray(acc.transpose(0, 2, 1))


def add_cbias(x, cb):
    """y[b, c, t] = x[b, c, t] + cb[b, c]: one float32 add."""
    return (np.asarray(x, np.float32) + np.asarray(cb, np.float32)[:, :, None]).astype(np.float32)


def zero_below(x, thr):
    """torch's ``x[x < thr] = 0`` (inference_plm.py:166): NaN, -inf < thr, and x == thr follow the comparison."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x < F32(thr), F32(0.0), x).astype(np.float32)


def maxpool1d(x, k):
    """nn.MaxPool1d(kernel_size = stride = k), floor mode: [B, C, L] -> [B, C, L // k]."""
    x = np.asarray(x, np.float32)
    B, C, L = x.shape
    Lo = L // k
    return x[:, :, :Lo * k].reshape(B, C, Lo, k).max(-1)


def vq_sqdist(x, embed):
    """Squared distances in float64: x [B, D, T], embed [bins, D] -> [B, T, bins]."""
    x, e = np.asarray(x, np.float64), np.asarray(embed, np.float64)
    xt = x.transpose(0, 2, 1)                                                       # [B, T, D]
    return ((xt[:, :, None, :] - e[None, None, :, :]) ** 2).sum(-1)


def vq_nearest(x, embed, rep=1, Tout=None):
    """EuclideanCodebook.quantize (ttv_v1/core_vq.py:175-183): the nearest code in float64, the first index on ties,
    every code held ``rep`` times and cut to Tout (ttv_v1/t2w2v_transformer.py:1051-1052).
    -> (codes int64 [B, Tout], margin float64 [B, T] = second-smallest distance minus smallest over DISTINCT distances
    of a column, i.e. what separates the winner from a different answer)."""
    d = vq_sqdist(x, embed)
    codes = d.argmin(-1)                                                            # first minimum
    best = d.min(-1, keepdims=True)
    other = np.where(d > best, d, np.inf).min(-1)
    margin = other - best[..., 0]
    codes = np.repeat(codes, rep, axis=1)
    return codes[:, :(Tout if Tout is not None else codes.shape[1])].astype(np.int64), margin


def peak_int16(x, lengths, gains):
    """``audio / max(abs(audio)) * 32767.0 * gain`` then numpy's truncating ``astype(int16)`` (inference_plm.py:183-190)
    per row over its first lengths[b] samples, float32 in that operation order; samples past lengths[b] are 0.  Values
    beyond the int16 range saturate (the kernel's documented behaviour for prompt-peak gains above 1).  A row whose peak
    is 0 is 0 / 0 = NaN in the reference expression, which ``astype(int16)`` turns into 0: silence stays silence."""
    x = np.asarray(x, np.float32)
    B, n = x.shape
    out = np.zeros((B, n), np.int16)
    for b in range(B):
        L = n if lengths is None else int(min(n, max(0, int(lengths[b]))))
        if L == 0:
            continue
        row = x[b, :L]
        mx = np.abs(row).max()
        if not mx > 0:
            continue
        v = (((row / mx).astype(np.float32) * F32(32767.0)).astype(np.float32) * F32(gains[b])).astype(np.float32)
        out[b, :L] = np.trunc(np.clip(v, F32(-32768.0), F32(32767.0))).astype(np.int16)
    return out


def lstm_packed_f64(state_dict, x, lengths, input_size, hidden, layers):
    """torch.nn.LSTM (bidirectional, batch_first) in float64 on packed sequences: x [B, N, In], lengths [B] >= 1 ->
    [B, N, 2H] with zeros after each row's length."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    ref = torch.nn.LSTM(input_size, hidden, num_layers=layers, bidirectional=True, batch_first=True).double().eval()
    ref.load_state_dict({k: v.double() for k, v in state_dict.items()})
    with torch.no_grad():
        y, _ = ref(pack_padded_sequence(x.double(), lengths.cpu(), batch_first=True, enforce_sorted=False))
        y, _ = pad_packed_sequence(y, batch_first=True, total_length=x.shape[1])
    return y


# ------------------------------------------------------------------------------------------------ seeded cases
# (N, T, C) of the Gaussian cases: N across the 8-group stride (1, 7, 8, 9, 33) up to the launcher's limit (438), T on
# both sides of the 32-frame tile and in the thousands, C across the 8-sub-channel / 32-channel passes.
GAUSS_CASES = [
    dict(seed=11, N=1, C=1, T=31), dict(seed=12, N=7, C=8, T=32), dict(seed=13, N=8, C=31, T=33),
    dict(seed=14, N=9, C=32, T=None), dict(seed=15, N=33, C=33, T=None), dict(seed=16, N=150, C=256, T=None),
    dict(seed=17, N=438, C=8, T=None), dict(seed=18, N=438, C=256, T=4536),
]
GAUSS_N_LIMIT = 438      # 140 N bytes of LDS <= 60 KB


def softplus(a):
    return np.log1p(np.exp(-np.abs(a))) + np.maximum(a, 0.0)


def gauss_case(seed, N, C, T=None, B=3):
    """B ragged rows: row 0 is full, rows 1.. are shorter in phones and frames.  Durations 1..20 with about 10 % exact
    zeros, softplus ranges scaled so that about half exceed the 2 dur clamp; x is a channel slice of a buffer with one
    extra row (the product's 257-row layout).  ``T`` pins the longest row's frame count (durations are drawn until the
    sum fits); None takes what the draw gives."""
    r = np.random.default_rng(seed)
    lens = np.array([N] + [max(1, (N * k) // (B + 1)) for k in range(B - 1, 0, -1)], np.int64)[:B]
    dur = np.zeros((B, N), np.float32)
    for b in range(B):
        d = r.integers(1, 21, lens[b]).astype(np.float32)
        d[r.random(lens[b]) < 0.1] = 0.0
        if lens[b] == 1:
            d[:] = max(d[0], 1.0)
        dur[b, :lens[b]] = d
    if T is not None:     # rescale row b to sum exactly to its share of T (keeps the zeros; values stay small integers)
        for b, Tb in enumerate([T, max(1, 2 * T // 3 - 1), max(1, T // 3)][:B]):
            d = dur[b, :lens[b]]
            nz = np.flatnonzero(d > 0)
            assert 0 < len(nz) <= Tb
            d[nz] = np.maximum(1, np.floor(d[nz] * (Tb / d.sum())))
            i = 0
            while d.sum() != Tb:
                j = nz[i % len(nz)]
                if d.sum() < Tb:
                    d[j] += 1
                elif d[j] > 1:
                    d[j] -= 1
                i += 1
    frames = dur.sum(1).astype(np.float32)
    Tmax = int(frames.max())
    # ranges: softplus of a normal, times the duration scale, so that values fall on both sides of 2 dur
    rng = (softplus(r.standard_normal((B, N))) * (1.0 + 2.0 * np.maximum(dur, 1.0) * r.random((B, N)))).astype(np.float32)
    xbuf = r.standard_normal((B, C + 1, N)).astype(np.float32)
    return dict(xbuf=xbuf, dur=dur, rng=rng, lens=lens, frames=frames, T=Tmax, B=B, C=C, N=N)


DUR_NS = (1, 255, 256, 257, 700)
DUR_SCALES = (0.5, 1.0, 1.3, 2.0)
DUR_MIN_DIST = 1e-3


def duration_case(seed, N, scale, B=4):
    """logw built backwards from targets k + u, k in 0..39, u in [2e-3, 1 - 2e-3]: logw = fp32(log((k + u) / scale)).
    Lengths: 0, inside the row, N, and beyond N."""
    r = np.random.default_rng(seed)
    k = r.integers(0, 40, (B, N)).astype(np.float64)
    u = 2e-3 + (1.0 - 4e-3) * r.random((B, N))
    logw = np.log((k + u) / float(np.float32(scale))).astype(np.float32)
    lens = np.array([0, max(1, N // 2), N, N + 5], np.int64)[:B]
    return logw, lens


VQ_CASES = [dict(seed=21, B=1, T=63, rep=1, cut=0), dict(seed=22, B=1, T=64, rep=8, cut=0),
            dict(seed=23, B=1, T=65, rep=8, cut=3), dict(seed=24, B=3, T=43, rep=8, cut=7),
            dict(seed=25, B=2, T=500, rep=1, cut=1)]
VQ_MIN_MARGIN = 1e-4


def vq_case(seed, B, T, D=20, bins=1024, **_):
    r = np.random.default_rng(seed)
    embed = r.standard_normal((bins, D)).astype(np.float32)
    xbuf = r.standard_normal((B, D + 3, T + 2)).astype(np.float32)       # x = xbuf[:, 1:D + 1, :T]: strided rows
    return xbuf, embed


def vq_tie_case(seed=26, B=2, T=70, D=20, bins=1024):
    """Codebook rows duplicated (e -> e + 512 for the first 300 rows, plus a triple), inputs placed exactly on codebook
    rows: both copies are at distance exactly 0 in any arithmetic, so the first index must win."""
    r = np.random.default_rng(seed)
    embed = r.standard_normal((bins, D)).astype(np.float32)
    embed[512:812] = embed[:300]
    embed[1000] = embed[5]
    pick = r.integers(0, bins, (B, T))
    pick[0, :4] = [5, 517, 1000, 299]
    x = np.ascontiguousarray(embed[pick].transpose(0, 2, 1))
    return x, embed


def peak_case(seed, n):
    """Rows: plain; negative peak; short; length 0; all zeros with a positive length; plain (for a gain > 1)."""
    r = np.random.default_rng(seed)
    x = (r.standard_normal((6, n)) * 0.3).astype(np.float32)
    x[1, n // 3] = -2.5                                  # the peak is a negative sample
    x[4] = 0.0
    lens = np.array([n, n, max(1, n // 2 - 1), 0, n, n - 1], np.int64)
    gains = np.array([0.999, 1.0, 0.999, 0.999, 0.999, 1.37], np.float32)
    return x, lens, gains
