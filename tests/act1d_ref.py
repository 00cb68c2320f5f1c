"""The stand-alone Activation1d launches (hsp_act1d_snakebeta_f32 / hsp_act1d_snakebeta_ragged_f32, include/hsp.h,
"anti-aliased activation") in numpy float64, the seeded case table that tests/test_act1d_ref_host.py (CPU) and
tests/test_gpu_act1d_contract.py (GPU) both walk, and the restated predicates that say which kernel and which branch of
csrc/hsp_pointwise.hip a case reaches.

Nothing here calls the library.  The plain reference is conv_ref.act1d as it is (tests/test_conv_ref_host.py pins it to
the oracle's closed form); the ragged one is that function on every row cut to clip(lens[b], 1, L), +0.0 from there on.

An operand is a flat float32 buffer with GUARD sentinel floats in front of and behind the tensor; `x_shift` / `y_shift`
move the tensor that many floats off the buffer's 16-byte alignment (both tests assert the buffers themselves are 16-byte
aligned), which is what sends an L % 4 == 0 call to the workgroup-tile kernel.
"""
from __future__ import annotations

import math

import numpy as np

from conv_ref import F32, F64, SENT, act1d

GUARD = 64             # sentinel floats on either side of x and of y
ACT_TILE = 1024        # csrc/hsp_pointwise.hip: outputs per workgroup of act1d_kernel
SEG, WAVES, ITEMS = 496, 4, 4   # ACT2_SEG, ACT2_WAVES, ACT2_ITEMS of act1d_seg_kernel
# |argument| in revolutions up to which the ISA manual defines v_cos_f32 without the v_fract_f32 reduction.  (Measured on an
# MI355X: the instruction reduces larger arguments itself -- the library built without the fract gave the same bits up to
# 2^23 revolutions -- so on that part the `big` cases guard the scaling and the rounding of the argument, not the fract.)
REV_LIMIT = 256.0
# "v_cos_f32 is accurate to ~1e-6 absolute on [0, 1)" (csrc/hsp_device.h): a claim nobody here has measured.  It enters
# `estimate` only -- never a bar.
COS_ABS_ERR = 1e-6
U = 2.0 ** -24


def filt24():
    from megatts2_hierspeechpp_amd.synth import kaiser_sinc_filter12
    h = kaiser_sinc_filter12()
    return np.concatenate([h, h]).astype(F32)


# ------------------------------------------------------------------------------------------------ references
def clip_lens(lens, L):
    return np.clip(np.asarray(lens, np.int64), 1, L)


def act1d_ragged(x, lens, alpha_exp, beta_inv, filt):
    """Row b over [0, n_b), n_b = clip(lens[b], 1, L), is act1d of the row cut to n_b; +0.0 from n_b on.  Nothing at
    t >= n_b is read."""
    B, C, L = x.shape
    y = np.zeros((B, C, L), F64)
    for b, n in enumerate(clip_lens(lens, L)):
        y[b, :, :n] = act1d(x[b:b + 1, :, :n], alpha_exp, beta_inv, filt)[0]
    return y


def upsampled(x, filt):
    """(up, sum of |terms| of up) of act1d's first stage: up[m] = 2 sum_i x[.] fu[.] on replicate-padded rows."""
    x = np.asarray(x, F64)
    L = x.shape[-1]
    fu = np.asarray(filt[:12], F32).astype(F64)
    q = np.arange(L)
    up, mag = np.empty(x.shape[:-1] + (2 * L,), F64), np.empty(x.shape[:-1] + (2 * L,), F64)
    for par, (o, t0) in enumerate(((3, 11), (2, 10))):
        terms = [x[..., np.clip(q - o + i, 0, L - 1)] * fu[t0 - 2 * i] * 2.0 for i in range(6)]
        up[..., par::2], mag[..., par::2] = sum(terms), sum(np.abs(t) for t in terms)
    return up, mag


def revolutions(x, alpha_exp, filt):
    """|up| alpha_exp / pi: the argument of the hardware cosine, in revolutions, before its reduction."""
    up, _ = upsampled(x, filt)
    return np.abs(up) * np.asarray(alpha_exp, F32).astype(F64)[None, :, None] / math.pi


def _estimate_rows(x, alpha_exp, beta_inv, filt):
    L = x.shape[-1]
    up, mag = upsampled(x, filt)
    ea = np.asarray(alpha_exp, F32).astype(F64)[None, :, None]
    bi = np.asarray(beta_inv, F32).astype(F64)[None, :, None]
    R = np.abs(up) * ea / math.pi
    e = bi * math.pi * R * U + 0.5 * bi * COS_ABS_ERR + bi * ea * 7.0 * U * mag
    fd = np.asarray(filt[12:], F32).astype(F64)
    q = np.arange(L)
    win = np.stack([e[..., np.clip(2 * q + k - 5, 0, 2 * L - 1)] for k in range(12)]).max(0)
    return float(np.abs(fd).sum()) * win


def estimate(case):
    """A-priori fp32 error of every output element: sum|fd| times, at the worst 2x-rate sample under the output's taps,
         beta_inv pi R 2^-24                    the fract reduction at R = |up| alpha_exp / pi revolutions (one rounding of
                                                the product up * kf, seen through the phase slope 2 pi of cos),
       + beta_inv / 2 * COS_ABS_ERR             the cosine's own absolute error (see COS_ABS_ERR),
       + beta_inv alpha_exp 7 2^-24 sum|x fu|   the rounding of `up` (six fmas and the gain) through the slope of sin^2.
    An estimate for the printed error / estimate ratio and for sizing the large-argument cases; never a bar."""
    x, L = case["x"], case["L"]
    if case["lens"] is None:
        return _estimate_rows(x, case["alpha_exp"], case["beta_inv"], case["filt"])
    est = np.zeros(x.shape, F64)
    for b, n in enumerate(clip_lens(case["lens"], L)):
        est[b, :, :n] = _estimate_rows(x[b:b + 1, :, :n], case["alpha_exp"], case["beta_inv"], case["filt"])[0]
    return est


def reference(case):
    if case["lens"] is None:
        return act1d(case["x"], case["alpha_exp"], case["beta_inv"], case["filt"])
    return act1d_ragged(case["x"], case["lens"], case["alpha_exp"], case["beta_inv"], case["filt"])


# ------------------------------------------------------------------------------------------------ predicates (restated)
def seg_rows(L, x_byte_off, y_byte_off):
    """act1d_seg_rows of csrc/hsp_pointwise.hip, from L and the byte offsets of x and y against 16-byte alignment."""
    return L % 4 == 0 and (x_byte_off | y_byte_off) % 16 == 0


def kernel_of(case):
    """'seg' (act1d_seg_kernel) or 'tile' (act1d_kernel) for a plain case; the ragged entry point refuses 'tile'."""
    return "seg" if seg_rows(case["L"], 4 * (GUARD + case["x_shift"]), 4 * (GUARD + case["y_shift"])) else "tile"


def tile_branches(L):
    """Per ACT_TILE tile of act1d_kernel: True where the paired interior branch runs (mlo >= 0 && mlo + a2w <= 2 L)."""
    out = []
    for tile in range(-(-L // ACT_TILE)):
        p0 = tile * ACT_TILE
        n_out = min(ACT_TILE, L - p0)
        a2w, mlo = 2 * n_out + 10, 2 * p0 - 5
        out.append(mlo >= 0 and mlo + a2w <= 2 * L)
    return out


def seg_items(B, C, L):
    """The work split of act1d_seg_kernel: per wave of the launch (WAVES per block, ITEMS consecutive items each) the
    number of items, whether its items span two channels' constants and whether they span two batch rows; `tail4`: the
    row's last item holds exactly four outputs."""
    nseg = -(-L // SEG)
    nwork = nseg * B * C
    blocks = -(-nwork // (WAVES * ITEMS))
    items, chan, row = [], [], []
    for g in range(blocks * WAVES):
        w = range(min(g * ITEMS, nwork), min(g * ITEMS + ITEMS, nwork))
        rows = sorted({i // nseg for i in w})
        items.append(len(w))
        chan.append(len(rows) > 1)
        row.append(len({r // C for r in rows}) > 1)
    return dict(nseg=nseg, nwork=nwork, blocks=blocks, items=items, cross_channel=chan, cross_row=row,
                empty=[g for g, n in enumerate(items) if n == 0], tail4=L - (nseg - 1) * SEG == 4)


# ------------------------------------------------------------------------------------------------ the case table
def _p(id, B, C, L, **kw):
    return dict(dict(id=id, B=B, C=C, L=L, x_shift=0, y_shift=0, lens=None, big=False), **kw)


RAGGED_LENS = (-3, 0, 1, 2, 3, 4, 5, 493, 494, 495, 496, 497, 498, 499, 992, 1487, 1488, 1495)
BIG_ALPHA, BIG_BETA_INV, BIG_SCALE = 300.0, 0.1, 1.5     # the large-argument channel (channel 0 of the `big` cases)

SPECS = [
    # ---- wave-per-segment kernel
    _p("seg_L4_both_pads_in_one_item", 1, 1, 4),
    _p("seg_L8_two_channels_one_wave", 1, 2, 8),
    _p("seg_L496_c5_two_empty_waves", 1, 5, 496),
    _p("seg_L500_tail4", 2, 3, 500),
    _p("seg_L992_short_wave", 1, 3, 992),
    _p("seg_L1988_30_items", 2, 3, 1988),
    # ---- workgroup-tile kernel
    _p("tile_L1", 1, 1, 1), _p("tile_L2", 1, 2, 2), _p("tile_L3", 1, 3, 3), _p("tile_L5", 2, 1, 5),
    _p("tile_L37", 1, 3, 37), _p("tile_L1023", 1, 2, 1023), _p("tile_L1025", 1, 2, 1025),
    _p("tile_L2050_no_interior", 1, 2, 2050),
    _p("tile_L2051_first_interior", 1, 2, 2051),
    _p("tile_L3077_two_interior", 1, 3, 3077),
    _p("tile_L2052_y_off1", 1, 2, 2052, y_shift=1),
    _p("tile_L2052_x_off1", 1, 2, 2052, x_shift=1),
    # ---- arguments of hundreds of revolutions on channel 0
    _p("seg_L1488_big_argument", 1, 2, 1488, big=True),
    _p("tile_L2051_big_argument", 1, 2, 2051, big=True),
    # ---- ragged: one launch, one row per length
    _p("ragged_L1488_18_rows", len(RAGGED_LENS), 2, 1488, lens=RAGGED_LENS),
]
for _i, _s in enumerate(SPECS):
    _s["seed"] = 8100 + _i
IDS = [s["id"] for s in SPECS]
assert len(set(IDS)) == len(IDS)
PLAIN_IDS = [s["id"] for s in SPECS if s["lens"] is None]
BATCH_ROWS_ID = "seg_L1988_30_items"


def spec_of(id):
    return SPECS[IDS.index(id)]


def build(spec):
    """x = 1.5 randn, constants distinct per channel: alpha_exp in [0.5, 4], beta_inv in [0.3, 1.5]; channel 0 of a `big`
    case takes BIG_ALPHA / BIG_BETA_INV.  Ragged rows hold NaN at odd and +Inf at even t >= clip(lens[b], 1, L)."""
    r = np.random.default_rng(spec["seed"])
    B, C, L = spec["B"], spec["C"], spec["L"]
    x = (1.5 * r.standard_normal((B, C, L))).astype(F32)
    ea, bi = r.uniform(0.5, 4.0, C).astype(F32), r.uniform(0.3, 1.5, C).astype(F32)
    if spec["big"]:
        x[:, 0] = (BIG_SCALE * r.standard_normal((B, L))).astype(F32)
        ea[0], bi[0] = BIG_ALPHA, BIG_BETA_INV
    lens = None
    if spec["lens"] is not None:
        lens = np.asarray(spec["lens"], np.int64)
        t = np.arange(L)
        for b, n in enumerate(clip_lens(lens, L)):
            x[b, :, (t >= n) & (t % 2 == 1)] = np.nan
            x[b, :, (t >= n) & (t % 2 == 0)] = np.inf
    return dict(id=spec["id"], B=B, C=C, L=L, x=x, alpha_exp=ea, beta_inv=bi, filt=filt24(), lens=lens,
                x_shift=spec["x_shift"], y_shift=spec["y_shift"], big=spec["big"])


def x_buffer(case):
    """(flat float32 buffer holding x between two guard bands, element offset of x)."""
    off = GUARD + case["x_shift"]
    n = case["x"].size
    buf = np.full(off + n + GUARD, SENT, F32)
    buf[off:off + n] = case["x"].reshape(-1)
    return buf, off


def y_buffer(case):
    """(sentinel-filled flat float32 buffer, element offset of y)."""
    off = GUARD + case["y_shift"]
    return np.full(off + case["x"].size + GUARD, SENT, F32), off


_CACHE = {}


def case(id):
    """(case, float64 reference [B, C, L], estimate [B, C, L]) -- computed once per process, never modified."""
    if id not in _CACHE:
        c = build(spec_of(id))
        ref, est = reference(c), estimate(c)
        for a in (c["x"], ref, est):
            a.setflags(write=False)
        _CACHE[id] = (c, ref, est)
    return _CACHE[id]
