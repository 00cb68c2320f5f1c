"""float64 numpy restatement of the seeded prior noise (include/hsp.h "seeded prior noise"), built on the Philox of
tests/plm_sampling_ref.py: the reference of tests/test_prior_noise_host.py and tests/test_gpu_prior_noise.py."""
import numpy as np

from plm_sampling_ref import philox4x32_10

STREAM = 1                      # the last counter word of this stream (the PLM draws use 0)
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))      # sqrt(-2 ln 2^-24) = 5.768: the largest |n| the stream can give

# the known answers of the contract: (seed, channel, first frame) -> values, from a float64 evaluation
KNOWN = {
    (1000, 0, 0): [-1.819521210688301, 0.4685280562411677, 0.7035363122575036, 0.984648160397131,
                   0.39148994292624123, 0.1361556961679569],
    (1000, 2, 4): [-0.5225558302847337, -0.12913841629986805],
    (-1, 0, 0): [0.4897898724091717, 1.6242049205926896, 0.8821279789020379, -2.918026960546835,
                 1.4345491095309184, -0.35873011982242986],
    (-1, 2, 4): [-0.1586133989102504, -0.4652295006993956],
    (2 ** 40 + 5, 0, 0): [0.11434612240971377, -0.6371950068416106, -1.3107262544793503, 1.006429109291443,
                          -0.9519717800969502, 0.11977474607183766],
    (2 ** 40 + 5, 2, 4): [0.012306109456026402, 0.6535437695915555],
}


def key_of(seed: int):
    """(low, high) 32 bits of the int64 seed in two's complement."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def counters(C: int, g0: int, g1: int) -> np.ndarray:
    """The counters (t >> 2, c, 0, STREAM) of channels [0, C) and frame groups [g0, g1) -> uint64 [C, g1 - g0, 4]."""
    g, c = np.meshgrid(np.arange(g0, g1, dtype=np.uint64), np.arange(C, dtype=np.uint64))
    return np.stack([g, c, np.zeros_like(g), np.full_like(g, STREAM)], -1)


def randn_row(seed: int, C: int, T: int, t0: int = 0) -> np.ndarray:
    """Frames [t0, T) of the row of ``seed`` -> float64 [C, T - t0]."""
    g0, g1 = t0 // 4, (T + 3) // 4
    ctr = counters(C, g0, g1)
    key = np.broadcast_to(np.array(key_of(seed), np.uint64), ctr.shape[:-1] + (2,))
    w = philox4x32_10(ctr, key).astype(np.uint64)                       # [C, G, 4]
    out = np.empty((C, 4 * (g1 - g0)), np.float64)
    for p in range(2):
        u1 = ((w[..., 2 * p] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        u2 = (w[..., 2 * p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * p::4] = r * np.cos(2.0 * np.pi * u2)
        out[:, 2 * p + 1::4] = r * np.sin(2.0 * np.pi * u2)
    return out[:, t0 - 4 * g0:T - 4 * g0]


def randn_rows(seeds, C: int, T: int, t0: int = 0) -> np.ndarray:
    """n[b, c, t] for t in [t0, T) -> float64 [B, C, T - t0]."""
    return np.stack([randn_row(int(s), C, T, t0) for s in seeds])
