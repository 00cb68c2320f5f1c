"""Float64 restatement of ITU-R BS.1770-4 integrated loudness (mono), the yardstick of the loudness tests, and the
seeded signals those tests meter.  scipy.signal.lfilter runs the K-weighting; nothing here imports the package."""
import functools

import numpy as np
from scipy.signal import lfilter

# BS.1770-4, table 1 and 2 (48 kHz): stage 1 b0 b1 b2 a1 a2, stage 2 b0 b1 b2 a1 a2
TABLE_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)
ABS_GATE = -70.0
REL_GATE = -10.0


def kweight_coefs(fs):
    """The analytic design behind the standard's table: high shelf, then high-pass (numerator 1, -2, 1) -> the 10
    coefficients in TABLE_48K's order."""
    K = np.tan(np.pi * 1681.974450955533 / fs)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
          2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K = np.tan(np.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    s2 = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return tuple(s1 + s2)


def kweight(x, fs):
    c = kweight_coefs(fs)
    y = lfilter(c[0:3], [1.0, c[3], c[4]], np.asarray(x, np.float64))
    return lfilter(c[5:8], [1.0, c[8], c[9]], y)


def block_loudness(x, fs):
    """Loudness of every 400 ms block (hop 100 ms) lying wholly inside x; -inf for a block of zero power."""
    y2 = kweight(x, fs) ** 2
    hop = fs // 10
    nblk = max(len(y2) // hop - 3, 0)
    z = np.array([y2[j * hop:j * hop + 4 * hop].sum() / (4 * hop) for j in range(nblk)], np.float64)
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z), z


def integrated_loudness(x, fs):
    """-> (LUFS, margin): margin = the smallest distance in LU of any block from either gate (inf without blocks).
    Under 400 ms: the whole length as one block, ungated.  No block above -70 LUFS: -inf."""
    x = np.asarray(x, np.float64)
    l, z = block_loudness(x, fs)
    with np.errstate(divide="ignore"):
        if len(z) == 0:
            if len(x) == 0:
                return -np.inf, np.inf
            return float(-0.691 + 10.0 * np.log10(np.mean(kweight(x, fs) ** 2))), np.inf
        margin = float(np.min(np.abs(l - ABS_GATE)))
        keep = l > ABS_GATE
        if not keep.any():
            return -np.inf, margin
        rel = -0.691 + 10.0 * np.log10(np.mean(z[keep])) + REL_GATE
        margin = min(margin, float(np.min(np.abs(l - rel))))
        keep &= l > rel
        return float(-0.691 + 10.0 * np.log10(np.mean(z[keep]))), margin


def lufs(x, fs):
    return integrated_loudness(x, fs)[0]


# ---------------------------------------------------------------------------------------------- seeded signals
def speech(n, seed, fs=16000, level=0.5):
    """harmonics of a gliding pitch under a slow envelope + a noise floor; peak = level"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / fs
    ph = 2 * np.pi * np.cumsum(110.0 + 30.0 * np.sin(2 * np.pi * 0.9 * t + seed)) / fs
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.7 * t + seed) ** 2)
    x = 0.3 * x + 0.02 * r.standard_normal(n)
    return (level * x / np.abs(x).max()).astype(np.float32)


def two_level(seed=31, fs=16000):
    """3 s: 1 s loud, 1 s 25 dB quieter, 1 s of digital silence -- the absolute gate drops the silent blocks, the
    relative gate the quiet ones."""
    loud = speech(fs, seed, fs, 0.5)
    quiet = speech(fs, seed + 1, fs, 0.5 * 10.0 ** (-25.0 / 20.0))
    return np.concatenate([loud, quiet, np.zeros(fs, np.float32)])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (sample rate, float32 signal): the rows the GPU meter is held to (tests/test_gpu_loudness.py); their
    conditioning -- no block within 0.1 LU of a gate -- is asserted in tests/test_loudness_host.py."""
    out = {}
    for i, n in enumerate((799, 800, 801, 1599, 6400, 19680)):     # chunk / hop edges, one block, a ragged block tail
        out[f"16k_{n}"] = (16000, speech(n, 10 + i))
    out["16k_two_level"] = (16000, two_level())
    out["24k_2s"] = (24000, speech(48000, 20, 24000))
    out["48k_2s"] = (48000, speech(96000, 21, 48000))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (LUFS, margin, peak) of a case in float64, computed once."""
    fs, x = cases()[name]
    l, margin = integrated_loudness(x, fs)
    return l, margin, float(np.abs(x).max())
