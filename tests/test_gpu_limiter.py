"""GPU (-m gpu): the true-peak meter and look-ahead limiter of csrc/hsp_limiter.hip against the float64 restatement
(tests/limiter_ref.py), ragged batches against solo rows, the chain functional.lufs_limit_int16 end to end and under
graph capture, and limiter=True of the harnesses.

Bars, all computed from the inputs (Z = 6, Lambda = max_p sum_d |h_p[d]| of the bank, about 1.76):
  true peak  2 (2Z + 1) 2^-24 Lambda max|y|: the fp32 rounding of the 2Z coefficients and of the 2Z fma steps of one
             output; the factor 2 allows for summation-order freedom.
  gain s     eps_r + (2W + 4) 2^-24 with eps_r = 2 ((2Z + 1) 2^-24 Lambda max|y| / c + 2^-23): r = c / p2 carries the
             relative error of p2 (at most that of the true peak over c, since p2 >= c wherever r < 1) and its own
             rounding and one-float step down; min and convex combinations are 1-Lipschitz in the sup norm, and the
             2W + 1 fma steps of the weighted mean, the rounding of the weights and of 1 - m add (2W + 4) 2^-24.
             z = fl(s y) adds one rounding of the product: |z - s_ref y| <= (bar_s + 2^-24) |y|.
  loudness   TOL = 0.1 LU (EBU Tech 3341) and the int16 allowance of tests/test_gpu_loudness.py, restated here.

What the float64 chain reaches (2 s of bursty, seed 3, 16 kHz, W = 24; L_0 = -27.32 LUFS): the capped gain of
lufs_int16 leaves -27.10 LUFS at every target; the chain reads -25.30 / -23.60 (passes 1 / 2) at -23, -19.61 / -16.25 at
-16 and -17.77 / -14.18 at -14 (asserted in tests/test_limiter_host.py).  The GPU is held to those readings within TOL,
not to the target."""
import math

import numpy as np
import pytest
import torch

import helpers as H
import limiter_ref as M
import loudness_ref as R

pytestmark = pytest.mark.gpu

TOL = 0.1
C_DB = -1.0
C32 = float(np.float32(10.0 ** (C_DB / 20.0)))
EPS = 2.0 ** -24
RATES = [(16000, 24), (16000, 80), (24000, 36), (48000, 72)]       # (rate, look-ahead W): 1.5 / 5 / 1.5 / 1.5 ms
GAINS = (1.0, 0.5, 1.0, 0.9, 0.25, 1.6, 1.0, 1.0, 1.0)             # rows 2 and 6 (peak 0.4) stay under the ceiling


def int16_allowance(target):
    return 20.0 * np.log10(1.0 + 10.0 ** (4.0 / 20.0) / 32767.0 / 10.0 ** ((target - 10.0 + 0.691) / 20.0))


def bar_tp(fs, ymax):
    return 2.0 * (2 * M.Z + 1) * EPS * M.lam(fs) * ymax


def bar_s(fs, W, ymax, c=C32):
    return 2.0 * ((2 * M.Z + 1) * EPS * M.lam(fs) * ymax / c + 2.0 ** -23) + (2 * W + 4) * EPS


def _batch(W, device, extra=29, tail=3):
    """The rows of limiter_ref.rows(W) in one [B, n] view of a [B, n + extra] buffer, NaN outside every row; their
    lengths, their gains, and y = fl32(gain x) per row on the host."""
    xs = M.rows(W)
    lens = [len(x) for x in xs]
    n = max(lens) + tail
    buf = torch.full((len(xs), n + extra), float("nan"), dtype=torch.float32)
    for b, x in enumerate(xs):
        buf[b, :lens[b]] = torch.from_numpy(x)
    g = np.asarray(GAINS, np.float32)
    ys = [(g[b] * x).astype(np.float32) for b, x in enumerate(xs)]
    return (buf.to(device)[:, :n], torch.tensor(lens, dtype=torch.int64, device=device),
            torch.from_numpy(g).to(device), ys)


@pytest.mark.parametrize("fs,W", RATES)
def test_true_peak_matches_float64_and_batch_rows_equal_solo_rows(fs, W, device):
    from megatts2_hierspeechpp_amd import functional as Fh
    x, lens, g, ys = _batch(W, device)
    assert x.stride(0) > x.shape[1] and torch.isnan(x).any()
    tp = Fh.true_peak(x, fs, lens, g)
    assert torch.isfinite(tp).all()
    for b, y in enumerate(ys):
        want, ymax = M.true_peak(y, fs), float(np.abs(y).max())
        dev = abs(float(tp[b]) - want)
        print(f"fs {fs} row {b} (n = {len(y)}): tp gpu {float(tp[b]):.7f} float64 {want:.7f} |diff| {dev:.2e} bar {bar_tp(fs, ymax):.2e}")
        assert dev <= bar_tp(fs, ymax), (b, float(tp[b]), want)
        assert float(tp[b]) >= ymax                                            # phase 0 is the impulse
        solo = Fh.true_peak(x[b:b + 1, :len(y)].contiguous(), fs, None, g[b:b + 1])
        assert torch.equal(solo, tp[b:b + 1]), b
    assert torch.equal(Fh.true_peak(x[3:8], fs, lens[3:8], g[3:8]), tp[3:8])   # a different batch around the same rows
    plain = Fh.true_peak(x[:, :5], fs)                                         # no lengths, no gains
    assert abs(float(plain[7]) - M.true_peak(M.rows(W)[7][:5], fs)) <= bar_tp(fs, 4.0)
    assert float(Fh.true_peak(x, fs, torch.zeros_like(lens))[0]) == 0.0        # empty rows


@pytest.mark.parametrize("fs,W", RATES)
def test_limiter_matches_float64_and_holds_the_ceiling(fs, W, device):
    from megatts2_hierspeechpp_amd import functional as Fh
    x, lens, g, ys = _batch(W, device)
    ms = W * 1000.0 / fs
    assert Fh.lookahead_samples(ms, fs) == W
    z, mg, tp = Fh.limit(x, fs, C32, ms, lens, g, return_true_peak=True)
    assert torch.equal(tp, Fh.true_peak(x, fs, lens, g))                       # the P the limiter computes anyway
    assert torch.isfinite(z).all() and float(z.abs().max()) <= C32             # |z| <= c on every sample, exactly
    zh, mgh = z.cpu().numpy(), mg.cpu().numpy()
    engaged = 0
    for b, y in enumerate(ys):
        nb, ymax = len(y), float(np.abs(y).max())
        zr, mgr = M.limit(y, fs, C32, W)
        bar = bar_s(fs, W, ymax)
        dev = np.abs(zh[b, :nb] - zr) - (bar + EPS) * np.abs(y)
        print(f"fs {fs} W {W} row {b} (n = {nb}, max|y| {ymax:.2f}): min_gain gpu {mgh[b]:.7f} float64 {mgr:.7f}, "
              f"max |z - z_ref| {np.abs(zh[b, :nb] - zr).max():.2e}, bar_s {bar:.2e}")
        assert dev.max() <= 0.0, (b, dev.max())
        assert abs(float(mgh[b]) - mgr) <= bar, (b, mgh[b], mgr)
        assert not zh[b, nb:].any()
        if mgr == 1.0:                                                         # never engaged: s = 1 exactly, z = y bitwise
            assert mgh[b] == 1.0 and np.array_equal(zh[b, :nb], y), b
        else:
            engaged += mgr < 0.5
        z1, m1 = Fh.limit(x[b:b + 1, :nb].contiguous(), fs, C32, ms, None, g[b:b + 1])
        assert torch.equal(z1[0], z[b, :nb]) and torch.equal(m1, mg[b:b + 1]), b
    assert engaged >= 3 and mgh[2] == 1.0 and mgh[6] == 1.0                    # it works hard, and idles on rows 2 and 6
    z2, m2 = Fh.limit(x[3:8], fs, C32, ms, lens[3:8], g[3:8])                  # a different batch around the same rows
    assert torch.equal(z2, z[3:8]) and torch.equal(m2, mg[3:8])


def test_int16_gain_and_gain_update_ops(device):
    from megatts2_hierspeechpp_amd import functional as Fh
    r = np.random.default_rng(11)
    x = r.uniform(-1.2, 1.2, (3, 700)).astype(np.float32)
    g = np.array([0.999, 1.0, 0.37], np.float32)
    lens = [700, 0, 333]
    buf = torch.full((3, 720), float("nan"))
    for b in range(3):
        buf[b, :lens[b]] = torch.from_numpy(x[b, :lens[b]])
    out = Fh.gain_int16(buf.to(device)[:, :705], torch.tensor(lens, device=device), torch.from_numpy(g).to(device)).cpu()
    for b in range(3):
        v = (x[b, :lens[b]] * g[b]).astype(np.float32) * np.float32(32767.0)
        want = np.clip(np.trunc(v), -32768, 32767).astype(np.int16)
        assert np.array_equal(out[b, :lens[b]].numpy(), want) and not out[b, lens[b]:].any()
    assert int(out[0].max()) == 32767 and int(out[0].min()) == -32768            # saturating, not wrapping
    lufs = np.array([-27.3, -np.inf, -16.0, np.nan], np.float32)
    g0 = Fh.gain_update(None, torch.from_numpy(lufs).to(device), -16.0).cpu().numpy()
    want = (10.0 ** ((-16.0 - lufs[[0, 2]].astype(np.float64)) / 20.0)).astype(np.float32)
    np.testing.assert_allclose(g0[[0, 2]], want, rtol=2.0 ** -23, atol=0)
    assert g0[1] == 0.0 and g0[3] == 0.0                                       # no loudness: the row stays silent
    g1 = Fh.gain_update(torch.from_numpy(g0).to(device), torch.from_numpy(lufs).to(device), -14.0).cpu().numpy()
    np.testing.assert_allclose(g1[[0, 2]], (g0[[0, 2]].astype(np.float64) * 10.0 ** ((-14.0 - lufs[[0, 2]].astype(np.float64)) / 20.0)),
                               rtol=2.0 ** -23, atol=0)
    assert g1[1] == 0.0 and g1[3] == 0.0


# ---------------------------------------------------------------------------------------------- the chain
def _bursty_rows(device):
    xs = [M.bursty(32000, 3), M.bursty(24000, 4)]
    buf = torch.full((2, 32000 + 40), float("nan"), dtype=torch.float32)
    for b, x in enumerate(xs):
        buf[b, :len(x)] = torch.from_numpy(x)
    return xs, buf.to(device)[:, :32005], torch.tensor([32000, 24000], dtype=torch.int64, device=device)


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("target", [-23.0, -16.0, -14.0])
def test_chain_reads_what_the_float64_chain_reads(target, passes, device):
    """High-crest rows that today's capped gain leaves more than 1 LU under the target come out of the chain as close
    to it as the float64 chain gets (the figures are in the module docstring), true peak at or under the ceiling."""
    from megatts2_hierspeechpp_amd import functional as Fh
    fs, W = 16000, 24
    xs, x, lens = _bursty_rows(device)
    wav, stats = Fh.lufs_limit_int16(x, lens, fs, target, C_DB, 1.5, passes)
    assert wav.dtype == torch.int16 and wav.shape == x.shape
    lufs0, peak0 = Fh.loudness(x, fs, lens)
    _, limited = Fh.loudness_gains(lufs0, peak0, target)
    old = Fh.lufs_int16(x, lens, fs, target).to(torch.float32) / 32767.0
    old_l, _ = Fh.loudness(old, fs, lens)
    c = 10.0 ** (C_DB / 20.0)
    bar16 = TOL + int16_allowance(target)
    for b, xb in enumerate(xs):
        nb = len(xb)
        ref = M.chain(xb, fs, target, C_DB, 1.5, passes)
        got = {k: float(v[b]) for k, v in stats.items()}
        w = wav[b, :nb].cpu().numpy()
        remeter = R.lufs(w / 32767.0, fs)
        tp16 = M.true_peak(w / 32767.0, fs)
        g_ref = 10.0 ** (sum(target - l for l in ref["lufs"][:passes]) / 20.0)
        y = g_ref * xb.astype(np.float64)
        lsb = 1 + np.ceil(bar_s(fs, W, float(np.abs(y).max())) * np.abs(y) * 32767.0)
        off = np.abs(w.astype(np.int64) - ref["wav"].astype(np.int64))
        print(f"target {target} passes {passes} row {b}: capped gain reads {float(old_l[b]):.3f}; chain gpu "
              f"{got['achieved_lufs']:.4f} float64 {ref['achieved_lufs']:.4f} int16 re-metered {remeter:.4f}; true peak gpu "
              f"{got['true_peak']:.6f} float64 {ref['true_peak']:.6f} int16 {tp16:.6f}; min_gain gpu {got['min_gain']:.5f} "
              f"float64 {ref['min_gain']:.5f}; int16 max |diff| {off.max()} LSB (bar up to {int(lsb.max())})")
        assert int(limited[b]) == 1 and float(old_l[b]) < target - 1.0             # today's rule: capped, under the target
        assert abs(got["achieved_lufs"] - ref["achieved_lufs"]) <= TOL
        assert abs(remeter - ref["achieved_lufs"]) <= bar16
        assert abs(got["achieved_lufs"] - target) < abs(float(old_l[b]) - target)
        assert (off <= lsb).all(), (b, int(off.max()))
        assert got["true_peak"] <= C32 and tp16 <= c + M.lam(fs) / 32767.0
        # the two chains' gains G_K may differ by the meter tolerance per pass; min_gain scales with 1 / G_K at the most
        assert abs(got["min_gain"] - ref["min_gain"]) <= bar_s(fs, W, float(np.abs(y).max())) + \
            ref["min_gain"] * (10.0 ** (passes * TOL / 20.0) - 1.0)
        assert not wav[b, nb:].any()
    with pytest.raises(Exception, match="passes"):
        Fh.lufs_limit_int16(x, lens, fs, target, passes=5)


def test_chain_edge_rows_silent_and_empty(device):
    from megatts2_hierspeechpp_amd import functional as Fh
    x = torch.zeros(3, 9000, device=device)
    x[1] = float("nan")
    x[2, :8000] = torch.from_numpy(M.bursty(8000, 5)).to(device)
    lens = torch.tensor([9000, 0, 8000], dtype=torch.int64, device=device)     # silent; empty; a live row beside them
    wav, st = Fh.lufs_limit_int16(x, lens, 16000, -16.0)
    assert not wav[:2].any() and wav[2, :8000].any() and not wav[2, 8000:].any()
    assert torch.isneginf(st["achieved_lufs"][:2]).all() and torch.isfinite(st["achieved_lufs"][2])
    assert st["true_peak"][:2].tolist() == [0.0, 0.0] and st["min_gain"][:2].tolist() == [1.0, 1.0]
    assert 0 < float(st["true_peak"][2]) <= C32 and float(st["min_gain"][2]) < 1.0


def test_chain_capture_replays_equal_eager(device):
    """The whole chain is launches and memset nodes on one stream (no read-back): captured and replayed twice, it gives
    the eager result bit for bit."""
    from megatts2_hierspeechpp_amd import functional as Fh
    _, x, lens = _bursty_rows(device)

    def run():
        wav, st = Fh.lufs_limit_int16(x, lens, 16000, -16.0)
        return wav, st["achieved_lufs"], st["true_peak"], st["min_gain"]

    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed = run()
    for _ in range(2):
        for t in graphed:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for e, r in zip(eager, graphed):
            assert torch.equal(e, r)


# ---------------------------------------------------------------------------------------------- the output stage
@pytest.mark.parametrize("fs,lens", [(16000, (9600, 7000, 3000, 0)), (48000, (24000, 20000))])
def test_output_stage_int16_equals_the_functional_chains(fs, lens, device):
    """OutputStage.int16 is a dispatch and nothing else: every norm gives the bits of the functional chain it names.
    Row 0 (bursty) is over full scale at the target's plain gain, so the capped gain of 'lufs' and the limiter both
    work on it; row 1 (speech at 0.9) needs neither; at 16 kHz row 2 is under 400 ms (the ungated meter) and row 3
    is empty."""
    from megatts2_hierspeechpp_amd import functional as Fh
    from megatts2_hierspeechpp_amd.output import OutputStage
    target, n = -16.0, max(lens)
    sig = [M.bursty(n, 3, fs), R.speech(lens[1], 5, fs, level=0.9)]
    buf = torch.full((len(lens), n), float("nan"), dtype=torch.float32)
    for b, nb in enumerate(lens):
        buf[b, :nb] = torch.from_numpy(sig[b % 2][:nb])
    x, nv = buf.to(device), torch.tensor(lens, dtype=torch.int64, device=device)
    row_gains = torch.tensor([0.5, 0.7, 0.9, 0.3][:len(lens)], dtype=torch.float32, device=device)

    def equal(got, want):
        (w, s), (w_ref, s_ref) = got, want
        assert w.dtype == torch.int16 and w.shape == x.shape and torch.equal(w, w_ref)
        assert (s is None) == (s_ref is None)
        for k in ("achieved_lufs", "true_peak", "min_gain") if s is not None else ():
            assert torch.equal(s[k], s_ref[k]), k

    w_max = Fh.peak_int16(x, nv, 0.999)
    equal(OutputStage(scale_norm="max").int16(x, nv, fs, 0.999), (w_max, None))
    equal(OutputStage().int16(x, nv, fs), (w_max, None))
    equal(OutputStage(scale_norm="max").int16(x, nv, fs, torch.full_like(row_gains, 0.999)), (w_max, None))
    equal(OutputStage(scale_norm="prompt").int16(x, nv, fs, row_gains), (Fh.peak_int16_gains(x, nv, row_gains), None))
    lufs = OutputStage(scale_norm="lufs", target_lufs=target)
    equal(lufs.int16(x, nv, fs), (Fh.lufs_int16(x, nv, fs, target), None))
    equal(lufs.int16(x.unsqueeze(1), nv, fs, row_gains), (Fh.lufs_int16(x, nv, fs, target), None))   # no gain in 'lufs'
    wav, stats = OutputStage(scale_norm="lufs", target_lufs=target, limiter=True, return_stats=True).int16(x, nv, fs)
    equal((wav, stats), Fh.lufs_limit_int16(x, nv, fs, target, -1.0, 1.5, 2))
    equal(OutputStage(scale_norm="lufs", target_lufs=target, limiter=True, ceiling_db=-2.0, lookahead_ms=5.0,
                      limiter_passes=1).int16(x, nv, fs), Fh.lufs_limit_int16(x, nv, fs, target, -2.0, 5.0, 1))
    # not vacuous: the limiter engages on row 0 and idles on row 1, and 'lufs' alone caps row 0 and not row 1
    l0, p0 = Fh.loudness(x, fs, nv)
    gains, limited = Fh.loudness_gains(l0, p0, target)
    print(f"fs {fs}: plain gain x peak {(10.0 ** ((target - l0[:2].double()) / 20.0) * p0[:2]).tolist()}, capped gains "
          f"{gains.tolist()}, limited {limited.tolist()}, min_gain {stats['min_gain'].tolist()}")
    assert float(stats["min_gain"][0]) < 1.0 and float(stats["min_gain"][1]) == 1.0
    assert limited[:2].tolist() == [1, 0]
    w_lufs = Fh.lufs_int16(x, nv, fs, target)
    assert not torch.equal(wav, w_lufs) and not torch.equal(w_max, w_lufs)    # three norms, three different results
    for b, nb in enumerate(lens):
        assert not wav[b, nb:].any() and not w_max[b, nb:].any()


# ---------------------------------------------------------------------------------------------- harnesses
def _mel_fn(device):
    from megatts2_hierspeechpp_amd.Mels_preprocess import MelSpectrogramFixed
    return MelSpectrogramFixed(sample_rate=16000, n_fft=1280, win_length=1280, hop_length=320, f_min=0, f_max=8000,
                               n_mels=80, window_fn=torch.hann_window).finalize(device)


def _track(n, seed, lo=90.0, hi=300.0):
    r = np.random.default_rng(seed)
    return np.where(r.random(n) < 0.3, 0, r.uniform(lo, hi, n)).astype(np.float32)


def _stats_equal_the_chain(stats, wav_rows, audio_rows, fs, target):
    """every row's stats and int16 samples equal lufs_limit_int16 on that row's float audio alone"""
    from megatts2_hierspeechpp_amd import functional as Fh
    for b, (w, a) in enumerate(zip(wav_rows, audio_rows)):
        w1, s1 = Fh.lufs_limit_int16(a.reshape(1, -1).contiguous(), None, fs, target)
        assert torch.equal(w1.reshape(-1), w.reshape(-1)), b
        for k in ("achieved_lufs", "true_peak", "min_gain"):
            assert torch.equal(stats[k][b:b + 1], s1[k]), (b, k)
        print(f"row {b}: achieved {float(s1['achieved_lufs'][0]):.3f} LUFS, true peak {float(s1['true_peak'][0]):.4f}, "
              f"min_gain {float(s1['min_gain'][0]):.4f}")
        assert float(s1["true_peak"][0]) <= C32


def _equals_the_chain(wav, stats, audio, n_valid, fs, target):
    """what a harness returned equals lufs_limit_int16 on the float audio it returned, the whole batch in one call"""
    from megatts2_hierspeechpp_amd import functional as Fh
    w, s = Fh.lufs_limit_int16(audio, n_valid, fs, target)
    assert torch.equal(w, wav)
    for k in ("achieved_lufs", "true_peak", "min_gain"):
        assert torch.equal(s[k], stats[k]), k


def test_vc_batch_limiter(device):
    from megatts2_hierspeechpp_amd import inference_vc as IV, synth
    from oracle.hsp_oracle import default_config
    models = IV.VcModels(default_config())
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 2))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = _mel_fn(device)
    srcs = [IV.pad_source(torch.from_numpy(R.speech(n, 50 + b, level=0.9)).to(device).reshape(1, -1))
            for b, n in enumerate((12000, 30000))]
    f0s = [torch.from_numpy(_track(s.shape[-1] // 80 + 1, 60 + b)).to(device) for b, s in enumerate(srcs)]
    prompt = torch.from_numpy(R.speech(24000, 70, level=0.9)).to(device).reshape(1, -1)
    f0t = torch.from_numpy(_track(24000 // 80, 71, 150.0, 350.0)).to(device)
    T = max(s.shape[-1] for s in srcs) // 320
    noise = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 192, T)).astype(np.float32)).to(device)
    kw = dict(noise=noise, return_float=True, scale_norm="lufs", target_lufs=-16)
    w0, n0, a0 = IV.vc_batch(models, mel_fn, srcs, f0s, prompt, f0t, **kw)
    w1, n1, a1 = IV.vc_batch(models, mel_fn, srcs, f0s, prompt, f0t, limiter=False, **kw)
    assert torch.equal(w0, w1) and torch.equal(a0, a1)                         # off: today's call, bit for bit
    wav, n_out, audio, stats = IV.vc_batch(models, mel_fn, srcs, f0s, prompt, f0t, limiter=True, return_stats=True, **kw)
    assert torch.equal(audio, a0) and torch.equal(n_out, n0)
    lens = n_out.tolist()
    _stats_equal_the_chain(stats, [wav[b, :n] for b, n in enumerate(lens)], [audio[b, 0, :n] for b, n in enumerate(lens)],
                           16000, -16.0)
    for b, n in enumerate(lens):
        assert not wav[b, n:].any()
    _equals_the_chain(wav, stats, audio, n_out, 16000, -16.0)                  # the ragged batch as one chain call
    w1, a1, s1 = IV.vc(models, mel_fn, srcs[1], f0s[1].reshape(1, -1), prompt, f0t.reshape(1, -1), noise=noise[1:2],
                       return_float=True, scale_norm="lufs", target_lufs=-16, limiter=True, return_stats=True)
    assert w1.dtype == torch.int16 and s1["achieved_lufs"].shape == (1,) and float(s1["true_peak"][0]) <= C32
    _equals_the_chain(w1.reshape(1, -1), s1, a1, None, 16000, -16.0)


def test_tts_from_prompt_limiter_and_takes(device):
    from megatts2_hierspeechpp_amd import inference_plm as IP, synth
    from megatts2_hierspeechpp_amd.ttv_v1.t2w2v_transformer import PlmSampling
    from oracle.hsp_oracle import default_config
    models = IP.TtsModels(default_config(), H.TTV_MODEL)
    models.load_state_dict({k: torch.from_numpy(synth.synth_tensor(k, tuple(v.shape), 7))
                            for k, v in models.state_dict().items()})
    models.finalize(device)
    mel_fn = _mel_fn(device)
    r = np.random.default_rng(5)
    N = 7
    ids = torch.from_numpy(r.integers(12, 113, (1, N))).to(device)
    tone = torch.from_numpy(r.integers(0, 11, (1, N))).to(device)
    lang = torch.where(ids < 74, 1, 2)
    kw = dict(dur=torch.full((1, N), 4.0, device=device), return_float=True, scale_norm="lufs", target_lufs=-16.0,
              noise=torch.from_numpy(r.standard_normal((1, 192, N * 2)).astype(np.float32)).to(device))
    prompt = torch.from_numpy(R.speech(20000, 80, level=0.9)).reshape(1, -1).to(device)
    w0, a0 = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, **kw)
    w1, a1 = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, limiter=False, **kw)
    assert torch.equal(w0, w1) and torch.equal(a0, a1)                         # off: today's call, bit for bit
    wav, audio, stats = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, limiter=True, return_stats=True, **kw)
    assert wav.dtype == torch.int16 and wav.shape == w0.shape and torch.equal(audio, a0)
    _stats_equal_the_chain(stats, [wav], [audio[0]], 16000, -16.0)
    _equals_the_chain(wav.reshape(1, -1), stats, audio, None, 16000, -16.0)
    sp = PlmSampling(temperature=1.1, top_k=40, top_p=0.95, repetition_penalty=1.2)
    wav2, audio2, stats2 = IP.tts_from_prompt(models, mel_fn, ids, tone, lang, prompt, limiter=True, return_stats=True,
                                              plm_sampling=sp, seed=3, takes=2, **kw)
    assert wav2.shape == (2, wav.shape[0]) and stats2["min_gain"].shape == (2,)
    _stats_equal_the_chain(stats2, [wav2[0], wav2[1]], [audio2[0], audio2[1]], 16000, -16.0)
    _equals_the_chain(wav2, stats2, audio2, None, 16000, -16.0)                # both takes as one chain call


def test_super_resolution_limiter(device):
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    from megatts2_hierspeechpp_amd.inference_speechsr import super_resolution
    from megatts2_hierspeechpp_amd.speechsr48k.speechsr import SynthesizerTrn as SpeechSR
    sr = SpeechSR(128, 30, "0", [3, 7, 11], [[1, 3, 5]] * 3, [3], 32, [3])
    sr.load_state_dict({k: torch.from_numpy(synth.synth_tensor("sr." + k, tuple(v.shape), 0)) for k, v in sr.state_dict().items()})
    finalize(sr, device)
    x = torch.from_numpy(R.speech(16000, 90, level=0.9)).reshape(1, -1).to(device)
    w0 = super_resolution(sr, x, 16000, scale_norm="lufs", target_lufs=-16.0)
    assert torch.equal(w0, super_resolution(sr, x, 16000, scale_norm="lufs", target_lufs=-16.0, limiter=False))
    wav, stats = super_resolution(sr, x, 16000, scale_norm="lufs", target_lufs=-16.0, limiter=True, return_stats=True)
    assert wav.shape == (48000,) and wav.dtype == torch.int16
    _stats_equal_the_chain(stats, [wav], [sr(x.unsqueeze(1)).reshape(-1)], 48000, -16.0)
    _equals_the_chain(wav.reshape(1, -1), stats, sr(x.unsqueeze(1)), None, 48000, -16.0)
