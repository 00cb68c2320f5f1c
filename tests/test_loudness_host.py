"""CPU: the float64 restatement of BS.1770-4 (tests/loudness_ref.py) against the standard's own numbers, the
conditioning of the signals the GPU meter is held to, the chunked-scan identity the kernels rest on, the agreement of
header and binding on the new names, and the argument checks of the new entry points (they reject before any HIP call,
so they run here on dummy pointers)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import loudness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hsp_loudness_workspace_bytes", "hsp_loudness_coefs_f64", "hsp_loudness_f32", "hsp_loudness_gains_f32")
RATES = (8000, 16000, 24000, 32000, 40000, 48000)


def test_restatement_reproduces_the_48k_table():
    got = R.kweight_coefs(48000)
    assert max(abs(a - b) for a, b in zip(got, R.TABLE_48K)) <= 1e-6


def test_library_coefficients_match_the_design_and_the_table():
    from megatts2_hierspeechpp_amd import _lib
    lib = _lib.lib()
    out = (C.c_double * 10)()
    for fs in RATES:
        assert lib.hsp_loudness_coefs_f64(fs, out) == 0
        assert max(abs(a - b) for a, b in zip(out, R.kweight_coefs(fs))) <= 1e-12, fs
    assert lib.hsp_loudness_coefs_f64(48000, out) == 0 and tuple(out) == R.TABLE_48K     # the table wins at 48 kHz


def test_997_hz_full_scale_sine_reads_minus_3_01():
    """The calibration point of BS.1770: a 0 dBFS 997 Hz sine in one channel reads -3.01 LUFS."""
    t = np.arange(5 * 48000) / 48000.0
    assert abs(R.lufs(np.sin(2 * np.pi * 997.0 * t), 48000) - (-3.01)) <= 0.1


def test_edge_rules_short_and_silent():
    fs = 16000
    x = R.speech(6399, 3)                                              # one sample short of a block
    assert len(R.block_loudness(x, fs)[1]) == 0
    want = -0.691 + 10 * np.log10(np.mean(R.kweight(x, fs) ** 2))      # its whole length as one block
    l, margin = R.integrated_loudness(x, fs)
    assert l == want and margin == np.inf
    quiet = x * 10.0 ** (-80.0 / 20.0)                                 # about -94 LUFS: ungated, so still reported
    assert abs(R.lufs(quiet, fs) - (want - 80.0)) < 1e-6
    assert R.lufs(np.zeros(100), fs) == -np.inf and R.lufs(np.zeros(0), fs) == -np.inf
    assert R.lufs(np.zeros(3 * fs), fs) == -np.inf                     # blocks, none above -70
    assert R.lufs(R.speech(3 * fs, 4) * 1e-4, fs) == -np.inf           # about -94 LUFS in every block: all gated
    assert len(R.block_loudness(R.speech(6400, 3), fs)[1]) == 1


def test_gpu_inputs_are_well_conditioned():
    """No block of any signal the GPU meter is held to lies within 0.1 LU of either gate in float64: a gate flipped by
    fp32 / fp64 rounding can neither fail nor mask a kernel test.  A condition on the inputs, not a tolerance."""
    for name in R.cases():
        l, margin, peak = R.reference(name)
        assert margin > 0.1, (name, margin)
        assert np.isfinite(l) and 0 < peak < 1
    fs, x = R.cases()["16k_two_level"]
    bl, z = R.block_loudness(x, fs)
    absg = bl > R.ABS_GATE
    rel = -0.691 + 10 * np.log10(z[absg].mean()) + R.REL_GATE
    assert 0 < (~absg).sum() and 0 < (absg & (bl <= rel)).sum() and 0 < (absg & (bl > rel)).sum()   # both gates act
    for n in (799, 800, 801, 1599):
        assert len(R.block_loudness(R.cases()[f"16k_{n}"][1], 16000)[1]) == 0                       # the fallback rule


def _step(c, x, s):
    """one sample through both biquads, transposed direct form II (csrc/hsp_loudness.hip: kw_step)"""
    y1 = c[0] * x + s[0]
    s[0] = c[1] * x - c[3] * y1 + s[1]
    s[1] = c[2] * x - c[4] * y1
    y2 = y1 + s[2]
    s[2] = -2.0 * y1 - c[8] * y2 + s[3]
    s[3] = y1 - c[9] * y2
    return y2


@pytest.mark.parametrize("fs", [16000, 48000])
def test_chunked_scan_equals_the_sequential_filter(fs):
    """The kernels' algorithm in float64 numpy: chunks of 800 from a zero state, the carry s[c + 1] = M^800 s[c] + z[c],
    then every chunk again from its true state -- the chunk sums equal those of the plain recurrence (lfilter)."""
    x = R.speech(800 * 5 + 123, 9, fs).astype(np.float64)
    c = R.kweight_coefs(fs)
    chunks = [x[i:i + 800] for i in range(0, len(x), 800)]
    P = np.zeros((4, 4))
    for j in range(4):
        s = [0.0] * 4
        s[j] = 1.0
        for _ in range(800):
            _step(c, 0.0, s)
        P[:, j] = s
    z = []
    for ch in chunks:
        s = [0.0] * 4
        for v in ch:
            _step(c, v, s)
        z.append(np.array(s))
    start = [np.zeros(4)]
    for k in range(len(chunks) - 1):
        start.append(P @ start[k] + z[k])
    want = R.kweight(x, fs) ** 2
    for k, ch in enumerate(chunks):
        s = list(start[k])
        got = sum(_step(c, v, s) ** 2 for v in ch)
        ref = want[800 * k:800 * k + len(ch)].sum()
        assert abs(got - ref) <= 1e-9 * ref, (k, got, ref)


def test_hop_is_a_whole_number_of_chunks_at_every_rate():
    for fs in RATES:
        assert fs % 10 == 0 and (fs // 10) % 800 == 0 and (fs // 10) // 800 == fs // 8000


def test_header_and_binding_agree_on_the_new_names():
    from megatts2_hierspeechpp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hsp.h")).read()
    declared = set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert _lib.SIGNATURES["hsp_loudness_workspace_bytes"][0] is C.c_int64
    assert lib.hsp_version() == 104                                    # additive: the ABI number stays


def test_new_entry_points_reject_bad_arguments():
    from megatts2_hierspeechpp_amd import _lib
    lib = _lib.lib()
    p = 16                                     # a dummy non-NULL, 8-B aligned pointer: every call fails its checks first
    E = _lib.EINVAL
    B, n = 3, 5000
    ws = lib.hsp_loudness_workspace_bytes(B, n)
    assert ws == B * 7 * 44                                            # 7 chunks of 800: 4 + 1 doubles and a float each
    assert lib.hsp_loudness_workspace_bytes(1, 800) == 44 and lib.hsp_loudness_workspace_bytes(1, 801) == 88
    for bad in ((0, n), (65536, n), (B, 0), (B, -1)):
        assert lib.hsp_loudness_workspace_bytes(*bad) == E, bad
    ok = dict(x=p, x_bs=n, lengths=None, B=B, n=n, sr=16000, ws=p, ws_bytes=ws, lufs=p, peak=p)

    def meter(**kw):
        a = dict(ok, **kw)
        return lib.hsp_loudness_f32(a["x"], a["x_bs"], a["lengths"], a["B"], a["n"], a["sr"], a["ws"], a["ws_bytes"],
                                    a["lufs"], a["peak"], None)

    for kw in (dict(x=None), dict(ws=None), dict(lufs=None), dict(peak=None),            # null pointers
               dict(x_bs=n - 1), dict(B=0), dict(B=65536), dict(n=0),                    # x_bs too short, empty batch
               dict(sr=44100), dict(sr=22050), dict(sr=0), dict(sr=56000), dict(sr=-16000),   # unsupported rates
               dict(ws_bytes=ws - 1), dict(ws=12)):                                      # small / misaligned workspace
        assert meter(**kw) == E, kw

    def gains(lufs=p, peak=p, target=-23.0, ceiling=0.999, out=p, limited=p, B=B):
        return lib.hsp_loudness_gains_f32(lufs, peak, target, ceiling, out, limited, B, None)

    for kw in (dict(lufs=None), dict(peak=None), dict(out=None), dict(limited=None), dict(B=0),
               dict(target=float("nan")), dict(target=float("-inf")), dict(ceiling=0.0), dict(ceiling=-1.0),
               dict(ceiling=float("inf")), dict(ceiling=float("nan"))):
        assert gains(**kw) == E, kw
    out = (C.c_double * 10)()
    assert lib.hsp_loudness_coefs_f64(48000, None) == E
    for sr in (44100, 4000, 96000, 0):
        assert lib.hsp_loudness_coefs_f64(sr, out) == E, sr


def test_unknown_scale_norm_still_raises():
    from megatts2_hierspeechpp_amd import _lib, inference_plm as IP
    from megatts2_hierspeechpp_amd.inference_speechsr import super_resolution
    assert IP.SCALE_NORMS == ("max", "prompt", "lufs")
    assert IP.output_gain("max", None) == 0.999 and IP.output_gain("lufs", None) == 0.999
    with pytest.raises(_lib.HspError, match="unknown scale_norm 'rms'"):
        IP.output_gain("rms", None)
    with pytest.raises(_lib.HspError, match="unknown scale_norm 'prompt'"):
        super_resolution(None, None, 16000, scale_norm="prompt")
