"""Case table and tile bookkeeping of the conv kernel's activation epilogue (hsp_conv1d_args.act = HSP_ACT_ACT1D), shared by
tests/test_epi_act_host.py (CPU) and tests/test_gpu_epi_act_contract.py (GPU).  Nothing here calls the library.

The shapes are the smallest that reach every seam of the overlapping column tiles (BN - 16 stored columns per tile: 496
on the 32 x 512 shape, 240 on the 64 x 256 one): rows shorter than the 8-column halo, so that both replicate pads fall
into one tile (L = 4, 8, 12); one tile that ends one float4 short of the boundary, exactly on it, and one float4 past
it (492 / 496 / 500 and 236 / 240 / 244); two full tiles plus a tail (1000 and 484)."""
from __future__ import annotations

import itertools

import numpy as np

B = 2
GUARD = 64                    # sentinel floats on either side of the output tensor
SENT = 1234.5

SHAPES = [(32, L, k, d) for L, k, d in itertools.product((4, 8, 12, 492, 496, 500, 1000), (3, 7, 11), (1, 5))] + \
         [(64, L, k, d) for L, k, d in itertools.product((236, 240, 244, 484), (3, 7), (1, 3))]
IDS = [f"c{c}_L{L}_k{k}_d{d}" for c, L, k, d in SHAPES]
TILE_OF = {32: (32, 512), 64: (64, 256)}       # channels -> (BM, BN) of the shape that carries the form


def tiling(ncols: int, bn: int):
    """Pure-Python model of the kernel's column tiles: (first conv column, first stored column, stored columns)."""
    out, t, seg = [], 0, bn - 16
    while t * seg < ncols:
        out.append((t * seg - 8, t * seg, min(seg, ncols - t * seg)))
        t += 1
    return out


def eligible_model(cin, cout, L, fft_first, fft_second, row_exact, plan, enabled=True):
    """amp_pair's rule: both convs direct, at most 64 channels, L % 4 == 0, no row-exact mode, the plan of the plain
    launch is a conv tile that carries the form: 32 x 512 or 64 x 256."""
    if not enabled or fft_first or fft_second or row_exact or cin > 64 or cout > 64 or L % 4:
        return False
    return plan is not None and plan[2] > 0 and tuple(plan[:2]) in ((32, 512), (64, 256))


def reference_batch(L: int) -> int:
    """Utterances of the REFERENCE conv launch.  The dispatcher sends a launch of at most 128 tiles of 128 x 128 to the
    short-sequence shapes, which walk K in another chunk order; amp_pair fuses only where the plain launch takes the
    form's own shape, so the reference launch carries the case's two utterances plus enough zero ones to be such a launch
    (an utterance's result does not depend on its neighbours)."""
    return max(B, 128 // -(-L // 128) + 1)


def operands(c: int, L: int, k: int, d: int):
    """Seeded per-channel random operands of a case: x [B, c, L], W [c, c, k], bias, alpha_exp, beta_inv."""
    r = np.random.default_rng(1000003 * c + 10007 * L + 101 * k + d)
    x = r.standard_normal((B, c, L)).astype(np.float32)
    W = (r.standard_normal((c, c, k)) / np.sqrt(c * k)).astype(np.float32)
    bias = (0.1 * r.standard_normal(c)).astype(np.float32)
    alpha_exp = np.exp(r.uniform(-1.0, 1.5, c)).astype(np.float32)
    beta_inv = (1.0 / (np.exp(r.uniform(-1.0, 1.5, c)) + 1e-9)).astype(np.float32)
    return x, W, bias, alpha_exp, beta_inv
