"""The contract of hsp_cprod3_args (include/hsp.h, "channel product in three real products per bin") in numpy float64 on
the operands the entry point sees -- [bins][2 C][Np] planes addressed by xf_bs / yf_bs, w [bins][3][C][C] stored [input
channel][output row] -- the seeded case table that tests/test_cprod3_ref_host.py (CPU) and
tests/test_gpu_cprod3_contract.py (GPU) both walk, and the restated role every consumer wave of
csrc/hsp_cprod3.hip takes in a case.

Nothing here calls the library.  With A_j = w[bin][j] transposed to [output row][input channel]:
    k1 = A1 Xr,  k2 = A2 (Xi - Xr),  k3 = A3 (Xr + Xi);   Yr = k1 - k3 (rows [0, C)),  Yi = k1 + k2 (rows [C, 2 C)).
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
SENT = 1234.5          # canary of the output buffer
GUARD = 64             # floats in front of and behind xf (NaN) and yf (sentinel)
BM, BN, KC = 64, 128, 16           # CP_BM, CP_BN, CP_KC of csrc/hsp_cprod3.hip
ROLES = ("two_full", "two_masked", "one_full", "one_masked", "barrier_only")


# ------------------------------------------------------------------------------------------------ predicates (restated)
def wave_role(Np, nt, wn):
    """The role of the consumer waves (*, wn) of column tile nt, from left = Np - (n0 + 64 wn) as cprod3_kernel decides
    it: two 32-column blocks when left > 32 (every column present when left >= 64), one when 0 < left <= 32 (every
    column present when left == 32), none -- the wave only keeps the barrier count -- when left <= 0."""
    left = Np - (nt * BN + 64 * wn)
    if left > 32:
        return "two_full" if left >= 64 else "two_masked"
    if left > 0:
        return "one_full" if left == 32 else "one_masked"
    return "barrier_only"


def roles(Np):
    """{(column tile, wn): role} of a launch."""
    return {(nt, wn): wave_role(Np, nt, wn) for nt in range(-(-Np // BN)) for wn in (0, 1)}


def block_order(bins):
    """'xcd' (every tile of a bin on one XCD: bins % 8 == 0) or 'plain'."""
    return "xcd" if bins % 8 == 0 else "plain"


def block_tiles(bins, C, Np):
    """(row tile, column tile, bin) of every block index of a launch, as cprod3_kernel decodes blockIdx.x."""
    n_mt, n_nt = C // BM, -(-Np // BN)
    T = n_mt * n_nt
    out = []
    for bid in range(bins * T):
        if bins % 8 == 0:
            q, t = bid >> 3, (bid >> 3) % T
            out.append((t % n_mt, t // n_mt, (q // T) * 8 + (bid & 7)))
        else:
            out.append((bid % n_mt, (bid // n_mt) % n_nt, bid // T))
    return out


# ------------------------------------------------------------------------------------------------ the case table
def _c(bins, C, Np, strided=False):
    return dict(id=f"bins{bins}_C{C}_Np{Np}" + ("_strided" if strided else ""), bins=bins, C=C, Np=Np, strided=strided)


SPECS = [
    _c(1, 64, 4),                       # one masked block beside a barrier-only wave
    _c(8, 64, 96),                      # two full + one full (left == 32) in the only tile
    _c(9, 64, 132, strided=True),
    _c(1, 128, 160),                    # second tile: one full block, one barrier-only wave
    _c(8, 128, 164, strided=True),      # second tile: the two-block masked consumer (left == 36)
    _c(9, 64, 196),                     # second tile: two full + one masked
    _c(16, 64, 224),                    # the production tail 128 + 96
    _c(1, 320, 224, strided=True),      # five row tiles, twenty chunks
    _c(8, 64, 256),
    _c(1, 320, 164),
    _c(16, 128, 132, strided=True),
    _c(9, 128, 4),
]
for _i, _s in enumerate(SPECS):
    _s["seed"] = 8300 + _i
IDS = [s["id"] for s in SPECS]
assert len(set(IDS)) == len(IDS)
ORDER_ID = "bins8_C128_Np164_strided"      # the launch compared with eight bins = 1 launches


def spec_of(id):
    return SPECS[IDS.index(id)]


def build(spec):
    """xf: randn planes, the slack between planes and both guard bands NaN (none of it may be read).  yf: all sentinel.
    w: randn / sqrt(C).  Strided cases: xf_bs = 2 C Np + 4, yf_bs = 2 C Np + 64."""
    r = np.random.default_rng(spec["seed"])
    bins, C, Np = spec["bins"], spec["C"], spec["Np"]
    plane = 2 * C * Np
    xf_bs, yf_bs = (plane + 4, plane + 64) if spec["strided"] else (plane, plane)
    xf = np.full(GUARD + bins * xf_bs + GUARD, np.nan, F32)
    for j in range(bins):
        xf[GUARD + j * xf_bs:GUARD + j * xf_bs + plane] = r.standard_normal(plane).astype(F32)
    w = (r.standard_normal((bins, 3, C, C)) / np.sqrt(C)).astype(F32)
    yf = np.full(GUARD + bins * yf_bs + GUARD, SENT, F32)
    return dict(id=spec["id"], bins=bins, C=C, Np=Np, xf=xf, xf_off=GUARD, xf_bs=xf_bs, yf=yf, yf_off=GUARD, yf_bs=yf_bs,
                w=w.reshape(-1))


def planes(buf, off, bs, bins, C, Np):
    """[bins][2 C][Np] view-copy of a plane buffer."""
    return np.stack([buf[off + j * bs:off + j * bs + 2 * C * Np].reshape(2 * C, Np) for j in range(bins)])


def written(a):
    """Which elements of the yf buffer the contract writes: 2 C Np floats from the start of every plane."""
    m = np.zeros(a["yf"].size, bool)
    for j in range(a["bins"]):
        m[a["yf_off"] + j * a["yf_bs"]:a["yf_off"] + j * a["yf_bs"] + 2 * a["C"] * a["Np"]] = True
    return m


def product(xr, xi, A):
    """The header's three products on float64 [bins][C][Np] planes and A [bins][3][row][input channel]."""
    k1, k2, k3 = A[:, 0] @ xr, A[:, 1] @ (xi - xr), A[:, 2] @ (xr + xi)
    return np.concatenate([k1 - k3, k1 + k2], axis=1)


def _operands(a):
    bins, C, Np = a["bins"], a["C"], a["Np"]
    X = planes(a["xf"], a["xf_off"], a["xf_bs"], bins, C, Np).astype(F64)
    A = a["w"].reshape(bins, 3, C, C).astype(F64).transpose(0, 1, 3, 2)
    return X[:, :C], X[:, C:], A


def reference(a):
    """[bins][2 C][Np] float64."""
    return product(*_operands(a))


def derived_bound(a):
    """Per element 2 (C + 8) 2^-24 (|A1| |Xr| + (|A2| + |A3|) (|Xr| + |Xi|)): the forward error of fp32 sums of C products
    in any order with a factor 2, the form of conv_ref.derived_bound; the fp32 rounding of the fragment sums Xi - Xr and
    Xr + Xi and the two epilogue additions are inside the + 8.  Each row half gets the bound of both (an upper bound)."""
    xr, xi, A = _operands(a)
    axr, axi, aA = np.abs(xr), np.abs(xi), np.abs(A)
    half = aA[:, 0] @ axr + (aA[:, 1] + aA[:, 2]) @ (axr + axi)
    return 2.0 * (a["C"] + 8) * 2.0 ** -24 * np.concatenate([half, half], axis=1)


_CACHE = {}


def case(id):
    """(args, float64 reference planes, bound planes) -- computed once per process, never modified."""
    if id not in _CACHE:
        a = build(spec_of(id))
        ref, bound = reference(a), derived_bound(a)
        for v in (a["xf"], a["w"], a["yf"], ref, bound):
            v.setflags(write=False)
        _CACHE[id] = (a, ref, bound)
    return _CACHE[id]


def to_struct(a, base, bin0=0, bins=None):
    """hsp_cprod3_args of a case.  ``base``: operand name -> address of its buffer's first element ('zeros' included).
    ``bin0`` / ``bins``: the sub-launch over the planes [bin0, bin0 + bins)."""
    from megatts2_hierspeechpp_amd import _lib as L
    s = L.Cprod3Args()
    C = a["C"]
    s.xf = base["xf"] + 4 * (a["xf_off"] + bin0 * a["xf_bs"])
    s.yf = base["yf"] + 4 * (a["yf_off"] + bin0 * a["yf_bs"])
    s.w = base["w"] + 4 * bin0 * 3 * C * C
    s.zeros = base["zeros"]
    s.xf_bs, s.yf_bs = a["xf_bs"], a["yf_bs"]
    s.bins, s.C, s.Np, s.debug = (a["bins"] if bins is None else bins), C, a["Np"], 0
    return s


def fake_base():
    return dict(xf=0x100000, yf=0x4000000, w=0x8000000, zeros=0xc000000)
