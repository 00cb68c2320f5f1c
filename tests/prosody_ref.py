"""Float64 restatement of hsp_prosody_encode_f32 (include/hsp.h) and the seeded inputs its tests share.

Written from the header comment and the reference lines it cites (ttv_v1/t2w2v_transformer.py:912-929); nothing here
calls the library.  tests/test_prosody_ref_host.py pins it against the oracle, torch and the reference fixtures of
tests/golden/prosody/ on a CPU and checks the condition the exact-code comparisons rely on (the float64 margin of every
pooled frame); tests/test_gpu_prosody.py compares the kernel and the model layer with it.
"""
from __future__ import annotations

import os
import re

import numpy as np

from megatts2_hierspeechpp_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "prosody")
D, BINS, K, POOL = 20, 1024, 5, 8
CONVS = ("plm_conv1.conv1", "plm_conv1.conv2", "plm_conv2.conv1", "plm_conv2.conv2")
EMBED = "quantizer.vq.layers.0._codebook.embed"
MIN_MARGIN = 1e-3          # float64 distance between the best and the second-best code that an exact comparison needs


def tile_frames() -> int:
    """PE_P of csrc/hsp_prosody.hip: the pooled frames one workgroup handles."""
    src = open(os.path.join(ROOT, "megatts2_hierspeechpp_amd", "csrc", "hsp_prosody.hip")).read()
    return int(re.search(r"constexpr int PE_P = (\d+);", src).group(1))


def weights(seed: int = 7) -> dict:
    """The synthetic PLMConv taps / biases (torch layout [Cout, Cin, K]) and the codebook, keyed as the state dict."""
    w = {}
    for c in CONVS:
        w[c + ".weight"] = synth.synth_tensor(c + ".weight", (D, D, K), seed)
        w[c + ".bias"] = synth.synth_tensor(c + ".bias", (D,), seed)
    w[EMBED] = synth.synth_tensor(EMBED, (BINS, D), seed)
    return w


def pack_taps(w, ld: int = D) -> np.ndarray:
    """[Cout, Cin, K] -> the packed [K][Cin][ld] layout of hsp_conv1d_args.w (rows past Cout are zero)."""
    out = np.zeros((w.shape[2], w.shape[1], ld), np.float32)
    out[:, :, :w.shape[0]] = np.asarray(w, np.float32).transpose(2, 1, 0)
    return out


def conv5(x, w, b):
    """Conv1d(k = 5, padding = 2) in float64: x [C, T], w [Cout, C, 5], b [Cout] or None."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    T = x.shape[1]
    xp = np.pad(x, ((0, 0), (2, 2)))
    y = np.zeros((w.shape[0], T))
    for k in range(K):
        y += w[:, :, k] @ xp[:, k:k + T]
    return y if b is None else y + np.asarray(b, np.float64)[:, None]


def plm_conv(x, m, w, name):
    h = conv5(x * m, w[name + ".conv1.weight"], w.get(name + ".conv1.bias")) * m
    return conv5(h, w[name + ".conv2.weight"], w.get(name + ".conv2.bias")) * m


def encode_row(x, n, w):
    """One row of the header's semantics.  x [D, T], n its length -> (code [Tp], margin [Tp], q [D, Tp], h [D, T]);
    margin = second-smallest minus smallest DISTINCT float64 squared distance, NaN at pooled frames >= ceil(n / 8)."""
    x = np.asarray(x, np.float64)
    T = x.shape[1]
    n = int(min(max(n, 0), T))
    Tp, npool = -(-T // POOL), -(-n // POOL)
    m = (np.arange(T) < n).astype(np.float64)[None]
    h = plm_conv(x, m, w, "plm_conv1")
    hp = np.pad(h, ((0, 0), (0, POOL * Tp - T)))                      # frames >= T count as zeros
    p = hp.reshape(x.shape[0], Tp, POOL).max(-1)
    mp = (np.arange(Tp) < npool).astype(np.float64)[None]
    q = plm_conv(p, mp, w, "plm_conv2")
    e = np.asarray(w[EMBED], np.float64)
    d = ((q.T[:, None, :] - e[None]) ** 2).sum(-1)                    # [Tp, bins]; argmin = first maximum of -d
    code = d.argmin(-1)
    best = d.min(-1, keepdims=True)
    margin = np.where(d > best, d, np.inf).min(-1) - best[:, 0]
    margin[npool:] = np.nan
    return code.astype(np.int64), margin, q, h


def encode(x, lengths, w):
    """x [B, D, T] (any strides), lengths [B] -> dict(codes int64 [B, T], pooled int64 [B, Tp], margin [B, Tp])."""
    B, _, T = x.shape
    Tp = -(-T // POOL)
    codes, pooled, margin = np.zeros((B, T), np.int64), np.zeros((B, Tp), np.int64), np.full((B, Tp), np.nan)
    for b in range(B):
        n = int(min(max(int(lengths[b]), 0), T))
        c, mg, _, _ = encode_row(x[b], n, w)
        pooled[b, :-(-n // POOL)] = c[:-(-n // POOL)]
        codes[b, :n] = np.repeat(c, POOL)[:n]
        margin[b] = mg
    return dict(codes=codes, pooled=pooled, margin=margin)


def compared_margin(margin, lengths):
    """The margins of every pooled frame a comparison looks at (j < ceil(n / 8)), flat; none is left out."""
    out = [margin[b, :-(-int(n) // POOL)] for b, n in enumerate(lengths)]
    return np.concatenate(out) if out else np.zeros(0)


# ---------------------------------------------------------------------------------------------------------- cases
def mel_case(lengths, T, seed, channels: int = 80):
    """A padded ragged mel batch [B, channels, T]: row b holds synth_inputs' mel on its first lengths[b] frames and
    OTHER finite values after them (a kernel that reads past a row's length shows)."""
    B = len(lengths)
    mel = np.clip(np.random.default_rng(seed + 1000).normal(-4.0, 2.0, (B, channels, T)), -6.9, 3.0).astype(np.float32)
    for b, n in enumerate(lengths):
        n = min(int(n), T)
        if n > 0:
            mel[b, :, :n] = synth.synth_inputs(1, n, seed=seed + b)["mel"][0, :channels]
    return mel


RAGGED = (200, 131, 41, 9, 1, 8, 7)


def cases():
    """name -> (mel [B, 80, T], lengths): the shapes of tests/test_gpu_prosody.py, built once."""
    P = tile_frames()
    Tb = POOL * (2 * P + 1)
    return {
        "ragged": (mel_case(RAGGED, 200, 7100), np.array(RAGGED, np.int64)),
        "tile_edge": (mel_case((POOL * P - 1, POOL * P, POOL * P + 1, Tb), Tb, 7200),
                      np.array((POOL * P - 1, POOL * P, POOL * P + 1, Tb), np.int64)),
        "t43": (mel_case((43, 30), 43, 7300), np.array((43, 30), np.int64)),
        "len0": (mel_case((0, 24), 24, 7400), np.array((0, 24), np.int64)),
    }


def tie_case(seed: int = 7):
    """Two identical codebook rows: the code the first row of the "t43" case chooses at pooled frame 0 is copied to a
    LOWER and to a HIGHER index (overwriting two codes that no frame of the case chooses, nor would choose next).  The
    two copies are at the same distance in any arithmetic, so every frame that chose the original must now report the
    lowest of the three indices."""
    mel, lengths = cases()["t43"]
    w = weights(seed)
    base = encode(mel[:, :D], lengths, w)
    used = set(base["pooled"].ravel().tolist())
    win = int(base["pooled"][0, 0])
    lo = next(i for i in range(win) if i not in used) if any(i not in used for i in range(win)) else None
    hi = next(i for i in range(BINS - 1, win, -1) if i not in used)
    e = w[EMBED].copy()
    e[hi] = e[win]
    if lo is not None:
        e[lo] = e[win]
    w2 = dict(w)
    w2[EMBED] = e
    return mel, lengths, w2, win, lo, hi


def negative_tail_case(seed: int = 7):
    """The padding-zero maximum with nothing left to chance: the first PLMConv's second conv has zero taps and a bias
    of -1 - c / 32, so h is that negative constant on every valid frame of every channel and 0 on the masked ones.  A
    window that straddles a row's end (lengths 13 and 21: 5 valid frames + 3 zeros) must pool to exactly 0 in all 20
    channels, a full window to the negative bias; a kernel that skips the masked frames pools the bias instead and,
    with the second PLMConv's taps, lands on another code (checked by the host test)."""
    w = weights(seed)
    w["plm_conv1.conv2.weight"] = np.zeros((D, D, K), np.float32)
    w["plm_conv1.conv2.bias"] = (-1.0 - np.arange(D) / 32.0).astype(np.float32)
    lengths = np.array((13, 21, 24), np.int64)
    return mel_case(lengths, 24, 7500), lengths, w


def fit_codes(codes, ls, lt, width):
    """fit_prosody_codes as a loop: target frame t < Lt takes source index ((2 t + 1) Ls) // (2 Lt); zeros after."""
    codes = np.asarray(codes)
    out = np.zeros((codes.shape[0], width), np.int64)
    for b in range(codes.shape[0]):
        for t in range(min(int(lt[b]), width)):
            out[b, t] = codes[b, ((2 * t + 1) * int(ls[b])) // (2 * int(lt[b]))]
    return out
