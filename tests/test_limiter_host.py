"""CPU: properties of the float64 restatement of the true-peak meter and limiter (tests/limiter_ref.py), the host-built
bank of the package against it, the argument checks of the new entry points (they reject before any HIP call, so they
run here on dummy pointers), the agreement of header, binding and struct layout, and the keyword checks of the
harnesses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import limiter_ref as M
import loudness_ref as LR
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hsp_true_peak_f32", "hsp_limiter_f32", "hsp_gain_update_f32", "hsp_limiter_stats_f32", "hsp_gain_int16_f32")
RIPPLE_DB = 0.0005


def test_phase_0_is_the_impulse_and_the_package_builds_the_same_bank():
    from megatts2_hierspeechpp_amd import functional as Fh
    for fs in (16000, 24000, 48000):
        h = M.bank(fs)
        assert h.shape == (192000 // fs, 12)
        assert h[0].tolist() == [0.0] * 5 + [1.0] + [0.0] * 6
        assert np.array_equal(h.astype(np.float32)[0], h[0])
        got = Fh.true_peak_bank_f64(fs)
        assert got.shape == h.shape and np.abs(got - h).max() <= 1e-15 and np.array_equal(got[0], h[0])
        x = LR.speech(3000, 5, fs)
        assert (M.peaks(x, fs) >= np.abs(x.astype(np.float64))).all()      # a true peak is never below the sample peak
    from megatts2_hierspeechpp_amd import _lib
    with pytest.raises(_lib.HspError, match="sample rate 44100"):
        Fh.true_peak_bank_f64(44100)


@pytest.mark.parametrize("fs", [16000, 24000, 48000])
def test_quarter_rate_sine_reads_its_true_peak(fs):
    """A full-scale sine at fs / 4 with phase 45 degrees has the sample peak -3.01 dB and the true peak 0 dB.  The bank
    samples the waveform every 1 / F of a sample, so at the worst phase it misses the crest by half a step, pi 0.25 / F
    of phase at this frequency: the reading lies between 20 log10 cos(pi 0.25 / F) and 0 dB, up to the bank's own
    ripple.  Measured from the bank at fs / 4: every phase's gain lies in [-0.00035, +0.00017] dB at all three rates
    (RIPPLE_DB = 0.0005 covers it); over 37 sine phases the reading spans [-0.0086, +0.0002] dB at F = 12,
    [-0.0335, 0] at F = 8, [-0.1333, 0] at F = 4, against the bounds -0.0186 / -0.0419 / -0.1685 dB."""
    F = 192000 // fs
    h = M.bank(fs)
    gain = np.abs((h * np.exp(1j * np.pi / 2 * np.arange(-5, 7))[None, :]).sum(axis=1))
    assert np.abs(20 * np.log10(gain)).max() <= RIPPLE_DB
    lo = 20 * np.log10(np.cos(np.pi * 0.25 / F)) - RIPPLE_DB
    for ph in np.linspace(0.0, np.pi / 2, 37):
        s = M.tone(4000, fs, fs / 4, ph)
        tp = 20 * np.log10(M.peaks(s, fs)[100:-100].max())
        assert lo <= tp <= RIPPLE_DB, (fs, ph, tp)
    s = M.tone(4000, fs, fs / 4, np.pi / 4)
    assert abs(20 * np.log10(np.abs(s).max()) + 3.0103) <= 1e-3
    assert abs(20 * np.log10(M.peaks(s, fs)[100:-100].max())) <= RIPPLE_DB      # the crest lies on phase F / 2


@pytest.mark.parametrize("W", [1, 24, 80])
def test_gain_curve_never_exceeds_r(W):
    """s <= r on every sample, the last W of a row included (m is defined on every integer, not padded), so |z| <= c."""
    c = 10.0 ** (-1.0 / 20.0)
    for y in M.rows(24) + (np.zeros(50, np.float32), 4.0 * M.tone(300, 16000, 4000.0, 0.7)):
        r, s = M.limiter_curves(y, 16000, c, W)
        assert (s <= r).all() and (s > 0).all() and (r <= 1).all()
        assert (s[-W:] <= r[-W:]).all()
        z, mg = M.limit(y, 16000, c, W)
        assert np.abs(z).max() <= c * (1 + 1e-15) and mg == s.min()
    z, mg = M.limit(0.5 * LR.speech(5000, 3), 16000, c, W)
    assert mg == 1.0 and np.array_equal(z, 0.5 * LR.speech(5000, 3).astype(np.float64))     # never engaged
    assert M.limit(np.zeros(0), 16000, c, W)[1] == 1.0 and M.true_peak(np.zeros(0), 16000) == 0.0
    assert abs(M.weights(W).sum() - 1.0) <= 1e-15
    # the weights as the kernel forms them: (1 + cos(pi j / (W + 1))) / (2 W + 2)
    j = np.arange(-W, W + 1)
    assert np.abs(M.weights(W) - (1 + np.cos(np.pi * j / (W + 1))) / (2 * W + 2)).max() <= 1e-15


def test_reference_chain_reaches_what_the_capped_gain_cannot():
    """2 s of bursty, seed 3, 16 kHz, W = 24 (L_0 = -27.32 LUFS, sample peak 0.974): the capped gain of lufs_int16 leaves
    the row at -27.10 LUFS at every target; the float64 chain reads -25.30 / -23.60 (pass 1 / 2) at -23, -19.61 / -16.25
    at -16, -17.77 / -14.18 at -14, true peak at the ceiling."""
    x = M.bursty(32000, 3)
    l0, pk = LR.lufs(x, 16000), float(np.abs(x).max())
    for target, want in ((-23.0, (-25.30, -23.60)), (-16.0, (-19.61, -16.25)), (-14.0, (-17.77, -14.18))):
        capped = LR.lufs(min(10.0 ** ((target - l0) / 20.0), 0.999 / pk) * x.astype(np.float64), 16000)
        assert capped < target - 1.0
        for passes in (1, 2):
            ch = M.chain(x, 16000, target, passes=passes)
            assert abs(ch["achieved_lufs"] - want[passes - 1]) <= 0.01, (target, passes, ch["achieved_lufs"])
            assert ch["true_peak"] <= 10.0 ** (-1.0 / 20.0) * (1 + 1e-12) and ch["min_gain"] < 0.5
            assert M.true_peak(ch["wav"] / 32767.0, 16000) <= 10.0 ** (-1.0 / 20.0) + M.lam(16000) / 32767.0
        assert abs(ch["achieved_lufs"] - target) < abs(capped - target) - 3.0
    silent = M.chain(np.zeros(8000), 16000, -16.0)
    assert not silent["wav"].any() and silent["achieved_lufs"] == -np.inf and silent["true_peak"] == 0.0 \
        and silent["min_gain"] == 1.0


def test_header_binding_and_struct_layout_agree(tmp_path):
    from megatts2_hierspeechpp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hsp.h")).read()
    declared = set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert _lib.SIGNATURES["hsp_limiter_f32"][1][0] is C.POINTER(_lib.LimiterArgs)
    assert lib.hsp_version() == 104                                    # additive: the ABI number stays
    src = open(os.path.join(ROOT, "megatts2_hierspeechpp_amd", "csrc", "hsp_limiter.hip")).read()
    assert int(re.search(r"constexpr int TILE = (\d+);", src).group(1)) == M.TILE     # the row lengths straddle this tile
    assert int(re.search(r"constexpr int WMAX = (\d+);", src).group(1)) == 480
    helpers.assert_struct_layouts(tmp_path, {"hsp_limiter_args": _lib.LimiterArgs})


def test_new_entry_points_reject_bad_arguments():
    from megatts2_hierspeechpp_amd import _lib
    lib = _lib.lib()
    p = 16                                     # a dummy non-NULL pointer: every call fails its checks first
    E = _lib.EINVAL
    B, n = 3, 5000
    inf, nan = float("inf"), float("nan")

    def tp(x=p, x_bs=n, lengths=None, gains=None, B=B, n=n, bank=p, F=12, Z=6, out=p):
        return lib.hsp_true_peak_f32(x, x_bs, lengths, gains, B, n, bank, F, Z, out, None)

    for kw in (dict(x=None), dict(bank=None), dict(out=None), dict(B=0), dict(B=65536), dict(n=0), dict(n=-4),
               dict(x_bs=n - 1), dict(F=0), dict(F=6), dict(F=16), dict(F=-4), dict(Z=5), dict(Z=0), dict(Z=12)):
        assert tp(**kw) == E, kw

    def lim(null=False, **kw):
        a = _lib.LimiterArgs()
        a.x, a.x_bs, a.B, a.n, a.bank, a.F, a.Z, a.W, a.ceiling = p, n, B, n, p, 8, 6, 24, 0.891
        a.y, a.y_bs, a.min_gain = p, n, p
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.hsp_limiter_f32(None if null else C.byref(a), None)

    assert lim(null=True) == E
    for kw in (dict(x=None), dict(bank=None), dict(y=None), dict(min_gain=None), dict(B=0), dict(B=65536), dict(n=0),
               dict(x_bs=n - 1), dict(y_bs=n - 1), dict(F=5), dict(F=24), dict(Z=4), dict(W=0), dict(W=-1), dict(W=481),
               dict(ceiling=0.0), dict(ceiling=-0.5), dict(ceiling=inf), dict(ceiling=nan)):
        assert lim(**kw) == E, kw

    def upd(gin=None, lufs=p, target=-16.0, out=p, B=B):
        return lib.hsp_gain_update_f32(gin, lufs, target, out, B, None)

    for kw in (dict(lufs=None), dict(out=None), dict(B=0), dict(target=nan), dict(target=inf), dict(target=-inf)):
        assert upd(**kw) == E, kw

    def stats(lufs=p, t=p, c=0.891, q=p, ach=p, peak=p, B=B):
        return lib.hsp_limiter_stats_f32(lufs, t, c, q, ach, peak, B, None)

    for kw in (dict(lufs=None), dict(t=None), dict(q=None), dict(ach=None), dict(peak=None), dict(B=0), dict(c=0.0),
               dict(c=-1.0), dict(c=inf), dict(c=nan)):
        assert stats(**kw) == E, kw

    def i16(x=p, x_bs=n, lengths=None, gains=p, out=p, o_bs=n, B=B, n=n):
        return lib.hsp_gain_int16_f32(x, x_bs, lengths, gains, out, o_bs, B, n, None)

    for kw in (dict(x=None), dict(gains=None), dict(out=None), dict(B=0), dict(B=65536), dict(n=0), dict(x_bs=n - 1),
               dict(o_bs=n - 1)):
        assert i16(**kw) == E, kw


def test_limiter_needs_scale_norm_lufs():
    from megatts2_hierspeechpp_amd import _lib, inference_plm as IP, inference_vc as IV, functional as Fh
    from megatts2_hierspeechpp_amd.inference_speechsr import super_resolution
    with pytest.raises(_lib.HspError, match="limiter=True needs scale_norm='lufs'"):
        super_resolution(None, None, 16000, scale_norm="max", limiter=True)
    with pytest.raises(_lib.HspError, match="limiter=True needs scale_norm='lufs'"):
        IV.vc(None, None, None, None, None, None, scale_norm="max", limiter=True)
    with pytest.raises(_lib.HspError, match="limiter=True needs scale_norm='lufs'"):
        IP.tts_from_prompt(None, None, None, None, None, None, scale_norm="max", limiter=True)
    with pytest.raises(_lib.HspError, match="limiter=True needs scale_norm='lufs'"):
        IP.tts_from_codes(None, None, None, None, None, None, None, None, scale_norm="prompt", limiter=True)
    with pytest.raises(_lib.HspError, match="limiter=True needs scale_norm='lufs'"):
        IP.tts(None, None, None, None, None, None, None, None, None, limiter=True)
    with pytest.raises(_lib.HspError, match="return_stats=True needs limiter=True"):
        super_resolution(None, None, 16000, scale_norm="lufs", return_stats=True)
    IP.check_limiter("lufs", True, True)
    assert Fh.lookahead_samples(1.5, 16000) == 24 and Fh.lookahead_samples(1.5, 48000) == 72
    for name in ("tts", "tts_from_codes", "tts_from_prompt"):
        import inspect
        ps = inspect.signature(getattr(IP, name)).parameters
        assert [ps[k].default for k in ("limiter", "ceiling_db", "lookahead_ms", "limiter_passes", "return_stats")] == \
            [False, -1.0, 1.5, 2, False], name
