"""Float64 restatement of the true-peak meter, the look-ahead limiter and the lufs_limit_int16 chain as include/hsp.h
defines them, the yardstick of the limiter tests, and the seeded signals those tests run.  Nothing
here imports the package; the BS.1770 meter is loudness_ref.integrated_loudness."""
import functools

import numpy as np

import loudness_ref as LR

RATE = 192000
Z = 6
BETA = 8.0
TILE = 2048          # samples of a row per workgroup (csrc/hsp_limiter.hip): the row lengths of the tests straddle it


def bank(fs):
    """[F][2 Z] float64: h_p[d] = sinc(d - p / F) kaiser_8(|d - p / F| / Z), d = -(Z - 1) ... Z at index d + Z - 1;
    phase 0 is the unit impulse exactly."""
    F = RATE // fs
    assert F * fs == RATE and F in (4, 8, 12)
    h = np.zeros((F, 2 * Z))
    for p in range(F):
        for k, d in enumerate(range(-(Z - 1), Z + 1)):
            t = d - p / F
            u = min(abs(t) / Z, 1.0)
            h[p, k] = np.sinc(t) * np.i0(BETA * np.sqrt(1.0 - u * u)) / np.i0(BETA)
    h[0] = 0.0
    h[0, Z - 1] = 1.0
    return h


def lam(fs):
    """max_p sum_d |h_p[d]|: the most the interpolator amplifies a bounded signal"""
    return float(np.abs(bank(fs)).sum(axis=1).max())


def interpolated(y, fs):
    """u[i, p] = sum_d h_p[d] y[i + d], y = 0 outside the row -> [n, F]"""
    y = np.asarray(y, np.float64)
    n = len(y)
    yp = np.concatenate([np.zeros(Z - 1), y, np.zeros(Z)])
    win = np.lib.stride_tricks.sliding_window_view(yp, 2 * Z) if n else np.zeros((0, 2 * Z))
    return win @ bank(fs).T


def peaks(y, fs):
    """P[i] = max_p |u[i, p]|"""
    return np.abs(interpolated(y, fs)).max(axis=1) if len(y) else np.zeros(0)


def true_peak(y, fs):
    return float(peaks(y, fs).max()) if len(y) else 0.0


def weights(W):
    j = np.arange(-W, W + 1)
    w = 1.0 + np.cos(np.pi * j / (W + 1))
    return w / w.sum()


def limiter_curves(y, fs, c, W):
    """-> (r, s) over the row: r[i] = min(1, c / max(P[i - 1], P[i])), m[k] = min_{|j| <= W} r[k + j] on every integer k
    with r = 1 outside the row, s[i] = min(r[i], 1 - sum_j w[j] (1 - m[i + j]))."""
    y = np.asarray(y, np.float64)
    n = len(y)
    if n == 0:
        return np.zeros(0), np.zeros(0)
    P = peaks(y, fs)
    p2 = np.maximum(P, np.concatenate([[0.0], P[:-1]]))
    with np.errstate(divide="ignore"):
        r = np.where(p2 > 0, np.minimum(1.0, c / np.where(p2 > 0, p2, 1.0)), 1.0)
    rp = np.concatenate([np.ones(2 * W), r, np.ones(2 * W)])                  # r on [-2W, n + 2W)
    m = np.lib.stride_tricks.sliding_window_view(rp, 2 * W + 1).min(axis=1)   # m on [-W, n + W)
    mean = 1.0 - np.lib.stride_tricks.sliding_window_view(1.0 - m, 2 * W + 1) @ weights(W)
    return r, np.minimum(r, mean)


def limit(y, fs, c, W):
    """-> (z, min_gain)"""
    _, s = limiter_curves(y, fs, c, W)
    return s * np.asarray(y, np.float64), (float(s.min()) if len(s) else 1.0)


def lookahead_samples(lookahead_ms, fs):
    return int(round(lookahead_ms * fs / 1000.0))


def chain(x, fs, target, ceiling_db=-1.0, lookahead_ms=1.5, passes=2):
    """The chain of functional.lufs_limit_int16 in float64 -> dict: wav (int16), z (z_K q, float64), achieved_lufs,
    true_peak, min_gain, lufs (L_0 ... L_K)."""
    x = np.asarray(x, np.float64)
    c = 10.0 ** (ceiling_db / 20.0)
    W = lookahead_samples(lookahead_ms, fs)
    L = [LR.lufs(x, fs)]
    if not np.isfinite(L[0]):
        return dict(wav=np.zeros(len(x), np.int16), z=np.zeros(len(x)), achieved_lufs=-np.inf, true_peak=0.0, min_gain=1.0,
                    lufs=L)
    G = 10.0 ** ((target - L[0]) / 20.0)
    for k in range(passes):
        if k and np.isfinite(L[-1]):
            G *= 10.0 ** ((target - L[-1]) / 20.0)
        z, mg = limit(G * x, fs, c, W)
        L.append(LR.lufs(z, fs))
    t = true_peak(z, fs)
    q = min(1.0, c / t) if t > 0 else 1.0
    zq = z * q
    wav = np.clip(np.trunc(zq * 32767.0), -32768, 32767).astype(np.int16)
    return dict(wav=wav, z=zq, achieved_lufs=L[-1] + 20.0 * np.log10(q), true_peak=t * q, min_gain=mg, lufs=L)


# ---------------------------------------------------------------------------------------------- seeded signals
def bursty(n, seed, fs=16000):
    """high crest factor: speech at level 0.08 plus 4 ms decaying noise bursts of amplitude 0.9 every 0.31 s"""
    r = np.random.default_rng(1000 + seed)
    x = LR.speech(n, seed, fs, level=0.08).astype(np.float64)
    nb = int(0.004 * fs)
    env = np.exp(-4.0 * np.arange(nb) / nb)
    for start in range(int(0.05 * fs), n - nb, int(0.31 * fs)):
        b = r.standard_normal(nb) * env
        x[start:start + nb] += 0.9 * b / np.abs(b).max()
    return x.astype(np.float32)


def tone(n, fs, freq, phase=0.0, amp=1.0):
    return (amp * np.sin(2 * np.pi * freq * np.arange(n) / fs + phase)).astype(np.float32)


def row_lengths(W):
    """every edge the kernel has, and a row of about a second"""
    return (1, 5, W, 2 * W + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + Z, 16011)


@functools.lru_cache(maxsize=None)
def rows(W):
    """The ragged rows of the kernel tests: bursty / speech signals cut to `row_lengths`, scaled so that max |y|
    reaches about 4 on some and stays under the ceiling on others.  float32, shared and left unchanged."""
    out = []
    for k, n in enumerate(row_lengths(W)):
        x = bursty(max(n, 4000), 7 + k)[-n:] if k % 2 == 0 else LR.speech(max(n, 64), 30 + k)[:n]
        scale = (4.0, 1.3, 0.4, 2.5)[k % 4]
        x = np.ascontiguousarray(x, np.float32)
        out.append((x / max(np.abs(x).max(), 1e-9) * scale).astype(np.float32))
    return tuple(out)
